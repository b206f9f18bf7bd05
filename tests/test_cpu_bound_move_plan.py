"""The host-side rules of a stream's move between two bindings with clocks per stream (beatrice-vst_amd/csrc/bound_move_plan.h;
BeatriceBatch_BoundStreamQuiescent / MoveBoundStreamsInFlight / ExportBoundStreamsInFlight / ImportBoundStreamsInFlight) without a GPU.
The header is plain C++17 without HIP: a stand-alone program with its own main is compiled against it with g++ under the address and
undefined-behaviour sanitizers and run directly.

It walks seeded sequences of calls the way rbr_step makes them -- every stream hands in a block or sits the call out, a call feeds one
tick per FIFO piece in which some stream fires (the streams that fire are present in that step) and at least one tick, pushes its job and
launches the jobs that are `delay` calls old -- with drained points in between, and marks the tracker where rbr_step and tick_run mark it.
Against it stands a brute-force model: the list of the steps inside the tick pipeline, each with the stages it has still to run and the
streams present, and the list of jobs still owed, each with the streams that were active in its call.  A stream is at rest when neither
list names it.  After every call and every drained point the header's verdict and the model agree for every stream, and the header's
statement "at rest once call c + delay has been made" is held against the model for delay = stages - 1, the binding's.  The refusal
order is asked on the way.  Whenever a stream is at rest it is moved by hand into a second binding with a hop numbering, a slot ring and
a slot map of its own, through the header's items (every one checked against the geometry it indexes) and, every other time, through the
in-order FIFO form; the destination's output half, restated from wrapr_post_kernel, must then read for every 48 kHz sample what the
source's would have read, across the hops the stream fires afterwards."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <random>
#include <vector>
#include "bound_move_plan.h"

using namespace bhip;
#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

struct Step { int left; std::vector<char> present; };
struct Owed { long long call; std::vector<char> active; };

// one binding's wrapper bookkeeping for ONE stream row, as far as the output half reads it: hop g's 240 samples are "labels" g * 1000 + j
struct Bound {
  int B, io_slots, map_ring, io_host = 0;
  std::vector<float> out24;      // [io_slots][B][240]
  std::vector<int> slot_map;     // [B][map_ring]
  std::vector<long long> t48, hops_s, hop_base;
  std::vector<int> fill;
  std::vector<std::vector<float>> fifo;   // [B][480] bound form: places below fill are the stream's own
  Bound(int B_, int io_slots_, int ring) : B(B_), io_slots(io_slots_), map_ring(ring), out24((size_t)io_slots_ * B_ * 240, -7.0f),
      slot_map((size_t)B_ * ring, -1), t48((size_t)B_, 0), hops_s((size_t)B_, 0), hop_base((size_t)B_, 0), fill((size_t)B_, 0),
      fifo((size_t)B_, std::vector<float>(480, -9.0f)) {}
  // the stream takes m inner samples whose values are `next_sample` on; a hop fires at every 480th and rides in the slot the step takes
  void feed(int s, int m, float& next_sample, float& next_hop_label) {
    for (int i = 0; i < m; ++i) {
      fifo[(size_t)s][(size_t)fill[(size_t)s]] = next_sample; next_sample += 1.0f;
      ++t48[(size_t)s];
      if (++fill[(size_t)s] == 480) {
        fill[(size_t)s] = 0;
        const int slot = io_host; io_host = (io_host + 1) % io_slots;
        slot_map[(size_t)s * map_ring + (size_t)(hops_s[(size_t)s] % map_ring)] = slot;   // wrapr_fifo_body
        for (int j = 0; j < 240; ++j) out24[((size_t)slot * B + s) * 240 + j] = next_hop_label + j;
        next_hop_label += 1000.0f;
        ++hops_s[(size_t)s];
      }
    }
  }
  void others_step() { io_host = (io_host + 1) % io_slots; }   // a step the stream is absent from: its row is skipped
  // wrapr_post_kernel's gather for sample t of the stream
  float read(int s, long long t) const {
    const long long k = t / 480 - 1;
    const int off = (int)(t % 480);
    if (k < 0 || (off & 1)) return 0.0f;
    const long long e = (hop_base[(size_t)s] + k) % map_ring;
    CHECK(e >= 0 && e < map_ring, "slot-map index %lld", e);
    const int slot = slot_map[(size_t)s * map_ring + (size_t)e];
    CHECK(slot >= 0 && slot < io_slots, "slot %d", slot);
    return out24[((size_t)slot * B + s) * 240 + (size_t)(off >> 1)];
  }
};

int main(int argc, char** argv) {
  if (argc != 7) return 2;
  const unsigned seed = (unsigned)std::atoi(argv[1]);
  const int B = std::atoi(argv[2]), delay = std::atoi(argv[3]), hops = std::atoi(argv[4]), calls_to_walk = std::atoi(argv[5]), told_delay = std::atoi(argv[6]);
  const int stages = delay + 1;   // the binding's: delay = TickStages() - 1
  std::mt19937 rng(seed);
  auto pick = [&](int n) { return (int)(rng() % (unsigned)n); };

  long long tick = 0, calls = 0;
  smove::Presence seen; seen.start(B);
  bmove::Marks marks; marks.start(B);
  std::deque<long long> jobs;            // the product's queue: call numbers
  std::vector<Step> inside;              // brute force
  std::vector<Owed> owed;
  std::vector<unsigned char> reset_pending((size_t)B, 0), restart_pending((size_t)B, 0);
  std::vector<long long> last_active((size_t)B, -1);
  long long at_rest_seen = 0, busy_seen = 0, drains = 0, boundary = 0, refusals = 0, moves = 0, via_fifo = 0, no_hop = 0;

  auto run_tick = [&](bool feeding, const std::vector<char>& present) {
    for (Step& st : inside) --st.left;
    for (size_t i = 0; i < inside.size();) if (inside[i].left <= 0) inside.erase(inside.begin() + (long)i); else ++i;
    if (feeding) {
      // (the step fed by tick T runs stage s in tick T + s: `stages` launches, this one included)
      Step st{stages - 1, present};
      for (int s = 0; s < B; ++s) if (present[(size_t)s]) seen.fed(s, tick);
      if (st.left > 0) inside.push_back(st);
    }
    ++tick;
  };
  auto call = [&](const std::vector<char>& active) {   // rbr_step
    const long long c = calls;
    for (int s = 0; s < B; ++s) if (active[(size_t)s]) { marks.active(s, c); restart_pending[(size_t)s] = 0; last_active[(size_t)s] = c; }
    int ticks = 0;
    for (int piece = 0; piece < hops; ++piece) {
      std::vector<char> fires((size_t)B, 0);
      bool any = false;
      for (int s = 0; s < B; ++s) { fires[(size_t)s] = active[(size_t)s] && pick(2); any = any || fires[(size_t)s]; }
      if (!any) continue;
      run_tick(true, fires);
      for (int s = 0; s < B; ++s) if (fires[(size_t)s]) reset_pending[(size_t)s] = 0;
      ++ticks;
    }
    if (ticks == 0) run_tick(false, std::vector<char>((size_t)B, 0));
    jobs.push_back(c); owed.push_back(Owed{c, active});
    calls = c + 1;
    while (!jobs.empty() && jobs.front() + delay <= c) { jobs.pop_front(); owed.erase(owed.begin()); }
  };
  auto drain = [&]() {   // tick_drain
    while (!inside.empty()) run_tick(false, std::vector<char>((size_t)B, 0));
    jobs.clear(); owed.clear();
    seen.drained();
    ++drains;
  };
  auto rest_of = [&](bool is_source) {
    bmove::Rest r;
    r.seen = &seen; r.ticks = tick; r.stages = stages; r.marks = &marks;
    r.oldest_owed = jobs.empty() ? calls : jobs.front();
    if (told_delay != delay && !jobs.empty()) r.oldest_owed = jobs.front() + (delay - told_delay);   // (the tracker that is told a shorter delay)
    if (is_source) { r.reset_pending = reset_pending.data(); r.restart_pending = restart_pending.data(); }
    return r;
  };
  auto truly_at_rest = [&](int s) {
    for (const Step& st : inside) if (st.present[(size_t)s]) return false;
    for (const Owed& o : owed) if (o.active[(size_t)s]) return false;
    return true;
  };
  auto compare = [&](const char* where) {
    const bmove::Rest r = rest_of(false);
    for (int s = 0; s < B; ++s) {
      const bool want = truly_at_rest(s), got = bmove::quiescent(r, s);
      CHECK(want == got, "%s: call %lld tick %lld stream %d: the plan says %d, the steps and jobs inside say %d", where, calls, tick, s, (int)got, (int)want);
      if (want) ++at_rest_seen; else ++busy_seen;
      // the header's statement: once call c + delay has been made the stream is at rest, and (without a drain) not a call before
      if (last_active[(size_t)s] >= 0 && calls - 1 >= bmove::rule_b_call(last_active[(size_t)s], delay)) CHECK(want, "%s: stream %d busy behind call c + delay", where, s);
      if (last_active[(size_t)s] >= 0 && calls - 1 == bmove::rule_b_call(last_active[(size_t)s], delay)) ++boundary;
    }
  };
  auto ask_refusals = [&]() {
    int a = pick(B), b2 = pick(B);
    const int two[2] = {a, b2};
    const int n = a == b2 ? 1 : 2;
    bmove::Side side; side.bound_ragged = true; side.B = B; side.n = n; side.streams = two; side.pointers_ok = true;
    CHECK(bmove::args(side) == bmove::kGo, "args");
    bmove::Side bad = side; bad.bound_ragged = false;
    CHECK(bmove::args(bad) == bmove::kRefused, "outside P");
    bad = side; bad.pointers_ok = false;
    CHECK(bmove::args(bad) == bmove::kRefused, "a NULL pointer");
    const int twice[2] = {a, a}, outside[1] = {B};
    bad = side; bad.n = 2; bad.streams = twice;
    CHECK(bmove::args(bad) == bmove::kRefused, "named twice");
    bad = side; bad.n = 1; bad.streams = outside;
    CHECK(bmove::args(bad) == bmove::kRefused, "out of range");
    bool rest = true, pending = false;
    for (int i = 0; i < n; ++i) { rest = rest && truly_at_rest(two[i]); pending = pending || reset_pending[(size_t)two[i]] || restart_pending[(size_t)two[i]]; }
    CHECK((bmove::at_rest(side, rest_of(false)) == bmove::kGo) == rest, "a destination: pending flags do not refuse");
    CHECK((bmove::at_rest(side, rest_of(true)) == bmove::kGo) == (rest && !pending), "a source: pending flags refuse");
    // -1 before -3 before the work, whatever else is wrong
    const bool rest_ok = bmove::at_rest(side, rest_of(true)) == bmove::kGo;
    for (int m = 0; m < 16; ++m) {
      const bool ar = m & 1, bl = m & 2, pa = m & 4, ra = m & 8;
      const bmove::Verdict v = bmove::verdict(ar, bl, pa, ra, rest_ok);
      CHECK(v == (!(ar && bl && pa && ra) ? bmove::kRefused : rest_ok ? bmove::kGo : bmove::kBusy), "order %d", m);
    }
    ++refusals;
  };
  // a stream at rest carries its wrapper state into another binding, by hand through the header
  auto move_by_hand = [&]() {
    const int Bs = 1 + pick(3), Bd = 1 + pick(3), s = pick(Bs), t = pick(Bd);
    Bound src(Bs, 3 + pick(40), 3 + pick(40)), dst(Bd, 3 + pick(40), 3 + pick(40));
    float smp = 1.0f, lab = 100000.0f, dsmp = -1.0f, dlab = -100000.0f;
    src.io_host = pick(src.io_slots); dst.io_host = pick(dst.io_slots);
    // the destination slot's first user, then the stream itself in the source (also: not one hop yet)
    dst.feed(t, pick(3000), dsmp, dlab);
    src.hops_s[(size_t)s] = pick(100); src.hop_base[(size_t)s] = src.hops_s[(size_t)s];   // (restarted once: hop numbers do not start at 0)
    src.feed(s, pick(4) == 0 ? pick(480) : pick(5000), smp, lab);
    for (int i = pick(src.io_slots - 1); i > 0; --i) src.others_step();   // (the sit-out: fewer steps than slots)
    for (int i = pick(dst.io_slots - 1); i > 0; --i) dst.others_step();
    const long long t48 = src.t48[(size_t)s];
    CHECK(bmove::fill_of(t48) == src.fill[(size_t)s], "fill");
    if (!bmove::has_hop(t48)) ++no_hop;
    const bmove::Item from = bmove::source_item(s, src.hops_s[(size_t)s], t48, src.fill[(size_t)s], src.map_ring);
    const bmove::Item to = bmove::dest_item(t, dst.hops_s[(size_t)t], from.fill, dst.io_host, dst.io_slots, dst.map_ring);
    CHECK(bmove::item_ok(bmove::Geometry{src.B, src.io_slots, src.map_ring}, from), "source item");
    CHECK(bmove::item_ok(bmove::Geometry{dst.B, dst.io_slots, dst.map_ring}, to), "destination item");
    // what the source's output half would read from here on, for the samples that need the carried hop
    std::vector<float> want;
    for (long long u = t48; u < (t48 / 480 + 1) * 480; ++u) want.push_back(src.read(s, u));
    const float* hop = nullptr;
    if (from.has_hop) {
      const int slot = src.slot_map[(size_t)from.stream * src.map_ring + (size_t)from.entry];
      CHECK(slot >= 0 && slot < src.io_slots, "the source's map names slot %d", slot);
      hop = &src.out24[((size_t)slot * src.B + from.stream) * 240];
    }
    float* cell = &dst.out24[((size_t)to.slot * dst.B + to.stream) * 240];
    long long t48_dst = t48;
    if (pick(2)) {   // through the in-order FIFO form (the wrapper blob)
      std::vector<float> blob(480);
      for (int i = 0; i < 480; ++i) blob[(size_t)i] = bmove::fifo_place(i, from.fill, src.fifo[(size_t)s].data(), hop);
      for (int i = from.fill; i < 480; ++i) CHECK(blob[(size_t)i] == src.read(s, t48 - from.fill + i), "the in-order form at place %d", i);
      for (int j = 0; j < 240; ++j) cell[j] = bmove::hop_place(j, to.fill, blob.data());
      dst.fifo[(size_t)t] = blob;
      t48_dst = bmove::t48_of_blob(to.fill);
      ++via_fifo;
    } else {
      for (int j = 0; j < 240; ++j) cell[j] = hop ? hop[j] : 0.0f;
      dst.fifo[(size_t)t] = src.fifo[(size_t)s];
    }
    dst.slot_map[(size_t)to.stream * dst.map_ring + (size_t)to.entry] = to.slot;
    dst.hop_base[(size_t)t] = bmove::hop_base(dst.hops_s[(size_t)t], t48_dst, dst.map_ring);
    CHECK(dst.hop_base[(size_t)t] >= 0 && dst.hop_base[(size_t)t] < dst.map_ring, "hop_base");
    dst.t48[(size_t)t] = t48_dst; dst.fill[(size_t)t] = to.fill;
    for (size_t i = 0; i < want.size(); ++i) CHECK(dst.read(t, t48_dst + (long long)i) == want[i], "sample %zu behind the move", i);
    for (int i = 0; i < to.fill; ++i) CHECK(dst.fifo[(size_t)t][(size_t)i] == src.fifo[(size_t)s][(size_t)i], "FIFO place %d", i);
    // the stream goes on in both: the same samples in, the same hops out (few enough that no slot comes round), read through both maps
    const int more = pick(480 * (std::min(std::min(src.io_slots, dst.io_slots), std::min(src.map_ring, dst.map_ring)) - 2));
    float smp2 = smp, lab2 = lab;
    src.feed(s, more, smp, lab);
    dst.feed(t, more, smp2, lab2);
    for (long long i = 0; i < more; i += 1 + pick(7)) {
      const long long back = std::min<long long>(i, 479 + src.fill[(size_t)s]);   // (only the last hop and the one before are still wanted)
      CHECK(dst.read(t, dst.t48[(size_t)t] - 1 - back) == src.read(s, src.t48[(size_t)s] - 1 - back), "sample %lld behind the move", more - back);
    }
    ++moves;
  };

  while (calls < calls_to_walk) {
    const int what = pick(24);
    if (what == 0) {
      drain();
      std::fill(last_active.begin(), last_active.end(), -1);
      compare("after a drain");
    } else if (what <= 6) {   // one stream sits a run of calls out while the others go on: long enough to come to rest
      const int s = pick(B), run = delay - 1 + pick(4);
      for (int i = 0; i < run; ++i) {
        std::vector<char> active((size_t)B, 0);
        for (int u = 0; u < B; ++u) active[(size_t)u] = u != s && pick(4) != 0;
        call(active);
        compare("inside a sit-out");
      }
    } else {
      std::vector<char> active((size_t)B, 0);
      for (int u = 0; u < B; ++u) active[(size_t)u] = pick(3) != 0;
      call(active);
    }
    compare("after a call");
    if (pick(4) == 0) { (pick(2) ? reset_pending : restart_pending)[(size_t)pick(B)] ^= 1; }
    if (pick(3) == 0) ask_refusals();
    if (pick(8) == 0) move_by_hand();
  }
  drain();
  compare("at the end");
  // a rate on the destination: the binding's own cap passes, one hop fewer does not
  CHECK(bmove::rate_fits(48000.0, 480, wrapn::most_hops(480, 48000.0)) && !bmove::rate_fits(16000.0, 480, wrapn::most_hops(480, 48000.0)), "rate_fits");
  CHECK(!bmove::rate_fits(0.0, 480, 99) && !bmove::rate_fits(-1.0, 480, 99) && !bmove::rate_fits(1e9, 480, 99), "rates no class takes");
  std::printf("ok calls %lld drains %lld at_rest %lld busy %lld boundary %lld refusals %lld moves %lld via_fifo %lld no_hop %lld\n", calls, drains, at_rest_seen, busy_seen,
              boundary, refusals, moves, via_fifo, no_hop);
  return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("bound_move_plan")
    src = d / "bound_move_plan_driver.cc"
    src.write_text(DRIVER)
    exe = d / "bound_move_plan_driver"
    # (the sanitizers' runtimes linked statically: the program carries them itself)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I", os.path.join(REPO, "beatrice-vst_amd", "csrc"), "-o", str(exe), str(src)],
                   check=True)

    def run(seed, B, delay, hops, calls, told_delay=None):
        return subprocess.run([str(exe), str(seed), str(B), str(delay), str(hops), str(calls), str(delay if told_delay is None else told_delay)],
                              capture_output=True, text=True)
    return run


@pytest.mark.parametrize("seed,B,delay,hops", [(1, 3, 1, 1), (2, 5, 2, 3), (3, 2, 16, 2), (4, 1, 5, 1), (5, 8, 13, 3), (6, 3, 7, 2), (7, 4, 16, 1)])
def test_the_verdict_agrees_with_the_steps_and_jobs_inside(driver, seed, B, delay, hops):
    r = driver(seed, B, delay, hops, 3000)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    words = r.stdout.split()
    got = {words[i]: int(words[i + 1]) for i in range(1, len(words), 2)}
    # not vacuous: drains, streams at rest while others were busy, the boundary call itself, refusals asked, moves both ways
    assert got["calls"] >= 3000 and got["drains"] >= 1 and got["at_rest"] >= 100 and got["busy"] >= 100 and got["boundary"] >= 20, got
    assert got["refusals"] >= 100 and got["moves"] >= 50 and got["via_fifo"] >= 10 and got["no_hop"] >= 1, got


@pytest.mark.parametrize("delay", [2, 5, 16])
def test_a_tracker_told_one_call_fewer_is_caught(driver, delay):
    r = driver(1, 4, delay, 2, 3000, told_delay=delay - 1)
    assert r.returncode == 1 and "the steps and jobs inside say 0" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
