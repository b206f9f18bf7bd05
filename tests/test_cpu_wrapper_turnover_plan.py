"""The tap-table bookkeeping of rate changes inside a binding with clocks per stream (beatrice-vst_amd/csrc/wrapper_turnover_plan.h;
BeatriceBatch_SetStreamRateInFlight / RestartStreamInFlight) without a GPU.  The header is plain C++17 without HIP: a stand-alone program
with its own main is compiled against it and wrapper_plan.h with g++ under the address and undefined-behaviour sanitizers and run directly.

It walks seeded sequences of rate changes, calls and drains the way the batch does (batch_wrappers.hip.h rbr_place / rbr_restart /
rbr_step): a model of the device buffer that a copy writes when it is enqueued -- launches and copies share one stream, so enqueue order
is execution order --, a record per call and stream that names its class's two tables by offset, the input half launched with the call,
the output half `delay` calls later or at a drain, each with the buffer that is the batch's THEN.  At every launch the record's offsets
must lie inside that buffer and address exactly the taps of the rate the call was planned with; the held places never overlap; after
every reap the number of held classes is within live_bound().  A run with the arena told a delay of 0 under a real delay of 6 must trip
the taps check: the walk does see a place that is written too early."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <random>
#include <vector>
#include "wrapper_plan.h"
#include "wrapper_turnover_plan.h"

static const double kPool[] = {8000, 11025, 16000, 22050, 24000, 32000, 37800, 44056, 44100, 47952, 48000, 50000, 64000, 88200, 96000, 176400, 192000};
static std::map<double, wrapn::RateClass> g_cls;
static const wrapn::RateClass& cls_of(double rate) {
  auto it = g_cls.find(rate);
  if (it == g_cls.end()) {
    wrapn::RateClass c;
    if (!c.configure(rate)) { std::printf("rate %g refused\n", rate); std::exit(3); }
    it = g_cls.emplace(rate, c).first;
  }
  return it->second;
}
#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

struct Rec { double rate; int off_down, off_up; };
struct Job { long long call; std::vector<Rec> rs; };

int main(int argc, char** argv) {
  if (argc != 6) return 2;
  const unsigned seed = (unsigned)std::atoi(argv[1]);
  const int B = std::atoi(argv[2]), delay = std::atoi(argv[3]), calls = std::atoi(argv[4]), told_delay = std::atoi(argv[5]);
  std::mt19937 rng(seed);
  auto pick = [&](int n) { return (int)(rng() % (unsigned)n); };
  const int n_pool = (int)(sizeof(kPool) / sizeof(kPool[0]));

  // the binding: the classes of the streams' first rates, laid out one after the other in a buffer of exactly their length
  wturn::TapArena ar;
  ar.start(B, told_delay);
  std::vector<int> cls(B);
  for (int s = 0; s < B; ++s) {
    const double rate = kPool[pick(n_pool)];
    int c = ar.find(rate);
    if (c < 0) c = ar.add_initial(rate, (int)cls_of(rate).taps_down.size(), (int)cls_of(rate).taps_up.size(), 0);
    ar.join(c, 0);
    cls[s] = c;
  }
  std::vector<float> dev((size_t)ar.capacity);
  auto put = [&](std::vector<float>& buf, const wturn::Slot& sl) {
    const wrapn::RateClass& k = cls_of(sl.rate);
    CHECK(sl.off >= 0 && (size_t)sl.off + sl.floats <= buf.size() && sl.floats == (int)(k.taps_down.size() + k.taps_up.size()), "place %d + %d in %zu", sl.off, sl.floats, buf.size());
    std::memcpy(buf.data() + sl.off_down(), k.taps_down.data(), sizeof(float) * k.taps_down.size());
    std::memcpy(buf.data() + sl.off_up(), k.taps_up.data(), sizeof(float) * k.taps_up.size());
  };
  for (const wturn::Slot& sl : ar.slots) put(dev, sl);

  long long n_calls = 0, grown = 0, reused = 0, lingering_rejoined = 0, most_held = 0;
  std::deque<Job> jobs;
  auto launch = [&](const Job& j, const char* half) {   // a kernel reads the record's tables in the buffer that is the batch's now
    for (int s = 0; s < B; ++s) {
      const Rec& r = j.rs[s];
      const wrapn::RateClass& k = cls_of(r.rate);
      CHECK(r.off_down >= 0 && (size_t)r.off_down + k.taps_down.size() <= dev.size() && r.off_up >= 0 && (size_t)r.off_up + k.taps_up.size() <= dev.size(),
            "%s half of call %lld at call %lld, stream %d: out of the buffer", half, j.call, n_calls, s);
      CHECK(!std::memcmp(dev.data() + r.off_down, k.taps_down.data(), sizeof(float) * k.taps_down.size()) &&
            !std::memcmp(dev.data() + r.off_up, k.taps_up.data(), sizeof(float) * k.taps_up.size()),
            "%s half of call %lld at call %lld, stream %d (%g Hz): not the taps it was planned with", half, j.call, n_calls, s, r.rate);
    }
  };
  auto invariants = [&]() {
    ar.reap(n_calls);
    int held = 0;
    for (size_t i = 0; i < ar.slots.size(); ++i) {
      const wturn::Slot& a = ar.slots[i];
      if (!a.held) continue;
      ++held;
      CHECK(a.off >= 0 && a.off + a.floats <= ar.capacity && (size_t)ar.capacity <= dev.size(), "slot %zu outside the capacity", i);
      for (size_t j = i + 1; j < ar.slots.size(); ++j) {
        const wturn::Slot& c = ar.slots[j];
        CHECK(!c.held || a.off + a.floats <= c.off || c.off + c.floats <= a.off, "slots %zu and %zu overlap", i, j);
        CHECK(!c.held || c.rate != a.rate, "two held classes of %g Hz", a.rate);
      }
    }
    most_held = std::max<long long>(most_held, held);
    CHECK(held <= ar.live_bound(), "%d classes held, bound %d", held, ar.live_bound());
    int users = 0;
    for (const wturn::Slot& a : ar.slots) { CHECK(a.users >= 0 && (a.held || a.users == 0), "users of a released class"); users += a.users; }
    CHECK(users == B, "%d users", users);
  };
  auto set_rate = [&](int s, double rate) {   // rbr_restart + rbr_place
    int c = ar.find(rate);
    if (c >= 0 && c != cls[s] && ar.slots[c].users == 0) ++lingering_rejoined;
    if (c < 0) {
      const wrapn::RateClass& k = cls_of(rate);
      ar.reap(n_calls);
      const wturn::Place p = ar.plan((int)(k.taps_down.size() + k.taps_up.size()));
      CHECK(p.index >= 0 && p.capacity >= ar.capacity && p.off + (int)(k.taps_down.size() + k.taps_up.size()) <= p.capacity, "plan");
      if (p.grows) {
        std::vector<float> longer((size_t)p.capacity, -1.0f);
        for (const wturn::Slot& sl : ar.slots) if (sl.held) put(longer, sl);
        dev.swap(longer);   // (the launches enqueued so far have run on the old one: one stream)
        ++grown;
      } else {
        ++reused;
      }
      ar.commit(p, rate, (int)k.taps_down.size(), (int)k.taps_up.size());
      put(dev, ar.slots[p.index]);
      c = p.index;
    }
    if (c != cls[s]) { ar.join(c, n_calls); ar.leave(cls[s], n_calls); cls[s] = c; }
  };

  for (; n_calls < calls;) {
    // between two calls: nothing, a few rate changes, or a burst on one stream (classes no call is issued under)
    const int what = pick(10);
    const int changes = what < 4 ? 0 : what < 8 ? 1 + pick(3) : 12 + pick(12);
    const int burst_stream = pick(B);
    for (int i = 0; i < changes; ++i) set_rate(changes >= 12 ? burst_stream : pick(B), kPool[pick(n_pool)]);
    invariants();
    // the call: records, input half now, output halves that are due behind it (rbr_step)
    Job j{n_calls, std::vector<Rec>(B)};
    for (int s = 0; s < B; ++s) j.rs[s] = Rec{ar.slots[cls[s]].rate, ar.slots[cls[s]].off_down(), ar.slots[cls[s]].off_up()};
    launch(j, "input");
    jobs.push_back(j);
    ++n_calls;
    while (!jobs.empty() && jobs.front().call + delay <= n_calls - 1) { launch(jobs.front(), "output"); jobs.pop_front(); }
    if (pick(40) == 0) while (!jobs.empty()) { launch(jobs.front(), "output (drain)"); jobs.pop_front(); }   // BeatriceBatch_Synchronize
  }
  while (!jobs.empty()) { launch(jobs.front(), "output (unbind)"); jobs.pop_front(); }
  std::printf("ok calls %lld grown %lld reused %lld rejoined %lld held_max %lld bound %d capacity %d\n", n_calls, grown, reused, lingering_rejoined, most_held,
              ar.live_bound(), ar.capacity);
  return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("wrapper_turnover_plan")
    src = d / "wrapper_turnover_plan_driver.cc"
    src.write_text(DRIVER)
    exe = d / "wrapper_turnover_plan_driver"
    # (the sanitizers' runtimes linked statically: the program carries them itself)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(REPO, "beatrice-vst_amd", "csrc"),
                    "-o", str(exe), str(src)], check=True)

    def run(seed, B, delay, calls, told_delay=None):
        return subprocess.run([str(exe), str(seed), str(B), str(delay), str(calls), str(delay if told_delay is None else told_delay)],
                              capture_output=True, text=True)
    return run


@pytest.mark.parametrize("seed,B,delay", [(1, 5, 27), (2, 5, 3), (3, 1, 6), (4, 16, 11), (5, 3, 1), (6, 7, 27)])
def test_every_launch_reads_the_taps_its_call_was_planned_with(driver, seed, B, delay):
    r = driver(seed, B, delay, 600)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    words = r.stdout.split()
    got = {words[i]: int(words[i + 1]) for i in range(1, len(words), 2)}
    # not vacuous: buffers were outgrown, freed places were written again, classes nobody was on were taken up again while still held
    assert got["calls"] == 600 and got["grown"] >= 1 and got["reused"] >= 1 and got["rejoined"] >= 1, got
    assert got["held_max"] <= got["bound"] == B * (delay + 2), got


def test_the_walk_sees_a_place_that_is_written_too_early(driver):
    """the arena is told a delay of 0, the output halves run 6 calls late: some place is released and written while a record still names it"""
    r = driver(1, 5, 6, 600, told_delay=0)
    assert r.returncode == 1 and "not the taps it was planned with" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
