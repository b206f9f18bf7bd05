"""When an entry of the speaker tables is free (beatrice-vst_amd/csrc/speaker_entry_plan.h; BeatriceBatch_SpeakerEntryBusy and the -3 of
BeatriceBatch_MorphSpeakersInFlight / InstallSpeakersInFlight) without a GPU.  The header is plain C++17 without HIP: a stand-alone program
with its own main is compiled against it with g++ under the address and undefined-behaviour sanitizers and run as a child process.

The program walks seeded scripts of what a batch does in the modes in which the two calls leave the tick pipeline running -- D, E, F (one
feeding tick per call, sit-outs in D and F, idle ticks, drains), P (a call launches 0 to 3 feeding ticks, an idle one if none; streams sit
steps out, one of them over long stretches) and G (a call fires 0 to 2 hops; at 2 or 4 hops per step a step fills over several calls and is
fed when its last hop fires; drains, flushes that drop a hop fired beyond the last full step, unbind and re-bind) -- 12 streams on 6
entries, 400 calls per seed.  Setters move streams between calls the way BeatriceBatch_SetTargetSpeaker[s] / MorphSpeakerStaged /
FlushSpeaker do (at once, or one key/value block per hop after a four-hop wait), the feed installs blocks and draws codebooks the way
advance_kv / draw_codebooks do, and every change goes to the plan where batch.hip sends it.

Against the plan stands a brute-force model that keeps every fed step with the set of entries it read for `stages` ticks, and for G the step
still filling with every entry named since its first hop fired -- across drained points, too.
  1. Whenever the plan answers "free", no stream names the entry, no step inside the pipeline read it and the filling step does not.
  2. Whenever the plan answers "busy" for an entry no stream names, the header's safe-side bound has not passed: fewer than `stages` ticks
     since the base it states (the last feed; the feed in progress for a per-hop install at several hops per step; the feed of the filling
     step, still to come) -- so a plan that always answered busy is caught.
A plan told one stage fewer, and one that is not told about the filling step, must be caught by 1."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "speaker_entry_plan.h"

using namespace bhip;
#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

static const int kB = 12, kS = 6, kNamed = 7, kCalls = 400;
struct Stream { int target = 0, add = 0, cb = 0, kv[4] = {0, 0, 0, 0}, count = 4, delay = 0; };
struct Step { int left; unsigned read; };   // brute force: a step inside the pipeline, the stages it has still to run, the entries it read
struct Totals { long long free_seen = 0, busy_named = 0, busy_step = 0, waited = 0, drains = 0, feeds = 0, idle = 0, sat_out = 0, dropped = 0, zero_tick_calls = 0, multi_tick_calls = 0; };

static void walk(char mode_c, int H, unsigned seed, int stages, int told_stages, bool tell_filling, Totals& tot) {
  const modes::Mode mode = mode_c == 'D' ? modes::Mode::D : mode_c == 'E' ? modes::Mode::E : mode_c == 'F' ? modes::Mode::F : mode_c == 'G' ? modes::Mode::G : modes::Mode::P;
  std::mt19937 rng(seed);
  auto pick = [&](int n) { return (int)(rng() % (unsigned)n); };
  // the batch as far as the rule reads it (tick::State, BeatriceBatch::ResidentBlocks)
  long long tick = 0, last_feed_tick = -1000, hops_fired = 0;
  std::vector<Stream> cfg((size_t)kB);
  sentry::Plan plan;
  plan.start(kB, kS, kNamed);
  // the model
  std::vector<Step> inside;
  bool fill_active = false;
  unsigned fill_read = 0;
  const long long kPending = -1, kNone = -2;
  std::vector<long long> base((size_t)kS, kNone);   // property 2: the base the header states for the entry's stamp
  std::vector<long long> floor_at((size_t)kS, -1000);   // ... and the last feed that replaced a key/value block naming the entry

  auto names = [&](int s, int* now) {
    const Stream& c = cfg[(size_t)s];
    const int v[kNamed] = {c.target, c.add, c.cb, c.kv[0], c.kv[1], c.kv[2], c.kv[3]};
    for (int i = 0; i < kNamed; ++i) now[i] = v[i];
  };
  auto read_of = [&](int s) { int now[kNamed]; names(s, now); unsigned m = 0; for (int v : now) m |= 1u << v; return m; };
  auto named_now = [&]() { unsigned m = 0; for (int s = 0; s < kB; ++s) m |= read_of(s); return m; };
  bool step_open = false;   // (BeatriceBatch::ResidentBlocks::step_open, kept the way rb_step keeps it)
  auto filling_flag = [&]() { return step_open; };
  auto clock = [&]() { return sentry::Clock{tick, last_feed_tick, told_stages, tell_filling && filling_flag()}; };
  // a change of stream s's settings has been made: to the plan (recount), and to the model
  auto changed = [&](int s, unsigned named_before, bool next_step_too) {
    int now[kNamed];
    names(s, now);
    plan.name(s, now, clock(), next_step_too);
    const unsigned after = named_now(), gone = named_before & ~after;
    if (fill_active) fill_read |= after;
    for (int e = 0; e < kS; ++e)
      if (gone >> e & 1) base[(size_t)e] = next_step_too ? tick : filling_flag() ? kPending : std::max(last_feed_tick, floor_at[(size_t)e]);
  };
  auto set_target = [&](int s, int e, int delay) {
    const unsigned before = named_now();
    Stream& c = cfg[(size_t)s];
    c.target = c.add = e; c.count = 0; c.delay = delay;
    if (delay == 0) c.cb = e;   // (the staged morph's streams draw their codebook at the feed)
    changed(s, before, false);
  };
  auto flush = [&](int s) {
    const unsigned before = named_now();
    Stream& c = cfg[(size_t)s];
    for (; c.count < 4; ++c.count) c.kv[c.count] = c.target;
    c.delay = 0;
    changed(s, before, false);
  };
  auto compare = [&](const char* when) {
    const unsigned named = named_now();
    unsigned read = fill_active ? fill_read : 0u;
    for (const Step& st : inside) read |= st.read;
    for (int e = 0; e < kS; ++e) {
      const bool busy = plan.busy(e, tick, mode);
      const bool is_named = named >> e & 1, is_read = read >> e & 1;
      CHECK(plan.named_now(e) == is_named, "%s, tick %lld, entry %d: the plan counts names %d, the streams' settings say %d", when, tick, e, (int)plan.named_now(e), (int)is_named);
      if (!busy) {
        CHECK(!is_named && !is_read, "%s, tick %lld, entry %d: the plan says free, named %d, read by a step inside or filling %d", when, tick, e, (int)is_named, (int)is_read);
        ++tot.free_seen;
      } else if (is_named) {
        ++tot.busy_named;
      } else {
        const long long b0 = base[(size_t)e];
        CHECK(b0 != kNone, "%s, tick %lld, entry %d: busy, and its last name never went", when, tick, e);
        CHECK(b0 == kPending || tick < b0 + stages, "%s, tick %lld, entry %d: still busy, the bound was tick %lld", when, tick, e, b0 + stages);
        ++tot.busy_step;
        if (b0 == kPending) ++tot.waited;
      }
    }
  };
  auto launch = [&]() {   // every step inside runs one stage; a step that has run its last one is out
    size_t keep = 0;
    for (Step& st : inside) if (--st.left > 0) inside[keep++] = st;
    inside.resize(keep);
    tick += 1;
  };
  auto feed = [&](const std::vector<char>& out) {   // tick_run(feeding): advance_kv, draw_codebooks, the launch
    unsigned read = 0;
    for (int s = 0; s < kB; ++s) {
      if (out[(size_t)s]) { ++tot.sat_out; continue; }   // an absent row: every body skips it, advance_kv and the draw too
      Stream& c = cfg[(size_t)s];
      unsigned before = named_now(), rows = 0, kv_before = 0;
      for (int v : c.kv) kv_before |= 1u << v;
      bool installed = false;
      for (int hh = 0; hh < H; ++hh) {   // each hop is preceded by one block install and runs on the blocks installed by then
        if (c.delay > 0) --c.delay;
        else if (c.count < 4) { c.kv[c.count++] = c.target; installed = true; }
        for (int v : c.kv) rows |= 1u << v;
      }
      if (H > 1) read |= rows;
      if (installed && H > 1)            // (the bound: a block this feed replaced counts as read by the step being fed)
        for (int e = 0; e < kS; ++e) if ((rows | kv_before) >> e & 1) floor_at[(size_t)e] = tick;
      if (installed) changed(s, before, H > 1);
      if (c.cb != c.target || pick(16) == 0) {   // the lottery: a codebook of its own per step (the target's, mostly)
        before = named_now();
        c.cb = pick(8) == 0 ? pick(3) : c.target;
        changed(s, before, false);
      }
      read |= read_of(s);
    }
    if (fill_active) { read |= fill_read; fill_active = false; fill_read = 0; }
    inside.push_back(Step{stages, read});
    last_feed_tick = tick;
    plan.fed(tick, told_stages);
    for (long long& b0 : base) if (b0 == kPending) b0 = tick;
    launch();
    ++tot.feeds;
  };
  auto drop_filling = [&]() {
    plan.filling_dropped(last_feed_tick, told_stages);
    for (long long& b0 : base) if (b0 == kPending) b0 = last_feed_tick;
    fill_active = false; fill_read = 0; hops_fired = 0; step_open = false;
    ++tot.dropped;
  };
  auto drain = [&]() {
    while (tick <= last_feed_tick + stages - 1) launch();
    CHECK(inside.empty(), "drained and %zu steps inside", inside.size());
    ++tot.drains;
  };
  const std::vector<char> nobody((size_t)kB, 0);
  auto some_out = [&](int always_out) {
    std::vector<char> out((size_t)kB, 0);
    for (int s = 0; s < kB; ++s) out[(size_t)s] = s == always_out || pick(4) == 0;
    return out;
  };
  auto fire = [&](int k) {   // rb_step: the hops are counted first, then the full steps go in
    const long long first = hops_fired;
    hops_fired += k;
    int fed = 0;
    for (long long h = first + 1; h <= first + k; ++h) {
      // (a step this call both starts and completes is never seen filling by a caller: it takes the settings of its feed)
      if (H > 1 && (h - 1) % H == 0 && first + k < h - 1 + H) { fill_active = true; fill_read = named_now(); }
      if (h % H == 0) {
        step_open = sentry::step_open_during_feed(first, H, fed);
        feed(nobody);
        ++fed;
        compare("after a step of G went in");
      }
    }
    step_open = sentry::step_open_after_call(hops_fired, H);
    if (fed == 0 && H == 1) { launch(); ++tot.idle; }
  };

  int long_absent = -1, absent_left = 0;
  for (int call = 0; call < kCalls; ++call) {
    // between two calls: settings move
    for (int i = pick(3); i > 0; --i) {
      const int s = pick(kB);
      if (pick(5) == 0) flush(s);
      else set_target(s, pick(10) < 7 ? pick(3) : 3 + pick(3), pick(2) ? 0 : 4);
      compare("after a setter");
    }
    if (pick(9) == 0) {   // an entry's streams all leave it at once
      const int e = 3 + pick(3);
      for (int s = 0; s < kB; ++s) if (read_of(s) >> e & 1) { set_target(s, pick(3), 0); if (pick(2)) flush(s); }
      compare("after an entry was left");
    }
    if (absent_left == 0 && pick(12) == 0) { long_absent = pick(kB); absent_left = stages + pick(6); }
    const bool sit_outs = mode == modes::Mode::D || mode == modes::Mode::F || mode == modes::Mode::P;
    const int away = sit_outs && absent_left > 0 ? long_absent : -1;
    if (absent_left > 0) --absent_left;
    // the call
    if (mode == modes::Mode::G) {
      fire(pick(3));
    } else if (mode == modes::Mode::P) {
      const int n = pick(4);
      for (int i = 0; i < n; ++i) { feed(some_out(away)); compare("after a tick of P"); }
      if (n == 0) { launch(); ++tot.idle; ++tot.zero_tick_calls; }
      if (n > 1) ++tot.multi_tick_calls;
    } else {
      if (pick(8) == 0) { launch(); ++tot.idle; }
      else feed(sit_outs && (away >= 0 || pick(3) == 0) ? some_out(away) : nobody);
    }
    compare("after a call");
    // now and then: a drained point; in G a flush or a new binding
    const int what = pick(60);
    if (what < 3) {
      drain();
      compare("after a drain");
    } else if (what == 3 && mode == modes::Mode::G) {   // BeatriceBatch_FlushResidentBlocks: made-up calls fill the step, a hop beyond it is dropped
      drain();
      if (H > 1 && fill_active) {
        while (fill_active) fire(1);
        drain();
        if (pick(2)) fire(1);
      }
      drop_filling();
      compare("after a flush");
    } else if (what == 4 && mode == modes::Mode::G) {   // unbind and bind again: tick mode goes and comes, the tick counter starts over
      drain();
      drop_filling();
      tick = 0; last_feed_tick = -1000;
      plan.clear_at_drained_point();
      for (long long& f : floor_at) f = -1000;
      for (long long& b0 : base) if (b0 != kNone) b0 = -1000;
      compare("after a re-bind");
    }
  }
}

int main(int argc, char** argv) {
  if (argc != 8) return 2;
  const char mode = argv[1][0];
  const int H = std::atoi(argv[2]), seed0 = std::atoi(argv[3]), seeds = std::atoi(argv[4]), stages = std::atoi(argv[5]), told = std::atoi(argv[6]);
  const bool tell_filling = std::atoi(argv[7]) != 0;
  Totals t;
  for (int i = 0; i < seeds; ++i) walk(mode, H, (unsigned)(seed0 + i), stages, told, tell_filling, t);
  std::printf("ok free %lld busy_named %lld busy_step %lld waited %lld drains %lld feeds %lld idle %lld sat_out %lld dropped %lld zero_tick_calls %lld multi_tick_calls %lld\n",
              t.free_seen, t.busy_named, t.busy_step, t.waited, t.drains, t.feeds, t.idle, t.sat_out, t.dropped, t.zero_tick_calls, t.multi_tick_calls);
  return 0;
}
"""

SEEDS = 50
CASES = [("D", 1), ("D", 2), ("D", 4), ("E", 1), ("E", 4), ("F", 1), ("F", 2), ("F", 4), ("P", 1), ("G", 1), ("G", 2), ("G", 4)]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("speaker_entry_plan")
    src = d / "speaker_entry_plan_driver.cc"
    src.write_text(DRIVER)
    exe = d / "speaker_entry_plan_driver"
    # (the sanitizers' runtimes linked statically: the program carries them itself)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I", os.path.join(REPO, "beatrice-vst_amd", "csrc"), "-o", str(exe), str(src)],
                   check=True)

    def run(mode, H, stages, seed0=1, seeds=SEEDS, told_stages=None, tell_filling=True):
        r = subprocess.run([str(exe), mode, str(H), str(seed0), str(seeds), str(stages), str(stages if told_stages is None else told_stages),
                            "1" if tell_filling else "0"], capture_output=True, text=True)
        words = r.stdout.split()
        got = {words[i]: int(words[i + 1]) for i in range(1, len(words) - 1, 2)} if r.stdout.startswith("ok ") else {}
        return r, got
    return run


@pytest.mark.parametrize("stages", [5, 28])
@pytest.mark.parametrize("mode,H", CASES)
def test_free_means_nothing_reads_and_busy_ends_at_the_bound(driver, mode, H, stages):
    r, got = driver(mode, H, stages)
    assert r.returncode == 0 and got, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    # not vacuous: entries were free, busy by a name, busy by a step alone; the pipeline drained; steps went in
    assert got["free"] >= 1000 and got["busy_named"] >= 1000 and got["busy_step"] >= 1000 and got["drains"] >= SEEDS and got["feeds"] >= 100 * SEEDS, got
    if mode in "DFP":
        assert got["sat_out"] >= 1000, got
    if mode == "P":
        assert got["zero_tick_calls"] >= SEEDS and got["multi_tick_calls"] >= SEEDS, got
    if mode == "G":
        assert got["dropped"] >= SEEDS, got
        assert (got["waited"] >= 100) == (H > 1), got     # entries waited for a filling step exactly where steps fill over several calls


@pytest.mark.parametrize("mode,H", CASES)
def test_a_plan_told_one_stage_fewer_is_caught(driver, mode, H):
    r, _ = driver(mode, H, 5, told_stages=4)
    assert r.returncode == 1 and "the plan says free" in r.stdout and "read by a step inside or filling 1" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


@pytest.mark.parametrize("H", [2, 4])
def test_a_plan_not_told_about_the_filling_step_is_caught(driver, H):
    r, _ = driver("G", H, 5, tell_filling=False)
    assert r.returncode == 1 and "the plan says free" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
