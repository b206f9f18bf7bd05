"""The host-side rules of a stream's move between two ticking batches (beatrice-vst_amd/csrc/stream_move_plan.h;
BeatriceBatch_StreamQuiescent / ExportStreamsInFlight / ImportStreamsInFlight / MoveStreamsInFlight) without a GPU.  The header is plain
C++17 without HIP: a stand-alone program with its own main is compiled against it and stream_blob.h with g++ under the address and
undefined-behaviour sanitizers and run directly.

It walks seeded sequences of what a batch in plain tick mode does -- steps every stream takes part in, steps some streams sit out (from the
first of which the batch is ragged and every stream has its own counter), ticks that feed nothing, drained points (the idle ticks that
empty the pipeline, then one counter again) -- the way tick_run / tick_drain / tick_relevel do, and marks the tracker where they mark it.
Against it stands a brute-force model that keeps the list of the steps inside the pipeline, each with the stages it still has to run and
the streams that took part: a stream is at rest when no step in the list names it.  After every tick and every drained point the two must
agree for every stream.  Whenever two streams are at rest, one's labelled rings (slot counter % m holds the label of the step that wrote
it) are taken at its own counter and turned into the other's, and the result is held against rotating by hand: the label written k steps
ago must sit k slots behind the destination's own counter, for every ring size, also when the counters lie on either side of the wrap.
The order of the refusals is asked on the way.  A tracker told one stage fewer than the pipeline has must be caught."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "stream_blob.h"
#include "stream_move_plan.h"

using namespace bhip;
#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

static const int kM[] = {1, 2, 3, 4, 6, 17};   // slot counts; the walk's wrap is a multiple of each, as the step counter's is
static const int kWrap = 2 * 3 * 4 * 17;
static const int kNM = (int)(sizeof(kM) / sizeof(kM[0]));

struct Step { int left; std::vector<char> present; };   // brute force: a step inside the pipeline and the stages it has still to run

int main(int argc, char** argv) {
  if (argc != 6) return 2;
  const unsigned seed = (unsigned)std::atoi(argv[1]);
  const int B = std::atoi(argv[2]), stages = std::atoi(argv[3]), ticks_to_walk = std::atoi(argv[4]), told_stages = std::atoi(argv[5]);
  std::mt19937 rng(seed);
  auto pick = [&](int n) { return (int)(rng() % (unsigned)n); };

  // the batch (tick::State and BeatriceBatch as far as the move's rules read them)
  long long tick = 0, last_feed_tick = -1000;
  int hop_host = kWrap - 25 + pick(20);   // (the walk crosses the wrap early and then again and again)
  bool ragged = false;
  std::vector<int> hop_s((size_t)B, hop_host);
  std::vector<unsigned char> reset_pending((size_t)B, 0);
  smove::Presence seen;
  seen.start(B);
  std::vector<Step> inside;
  // labelled rings: ring[s][i][slot]
  std::vector<std::vector<std::vector<long long>>> ring((size_t)B);
  for (int s = 0; s < B; ++s) for (int i = 0; i < kNM; ++i) ring[(size_t)s].push_back(std::vector<long long>((size_t)kM[i], -1 - s));
  long long label = 0, asked = 0, at_rest_seen = 0, busy_seen = 0, turns = 0, across_wrap = 0, drains = 0, sat_out = 0;
  auto hop_next = [&](int c) { return c + 1 == kWrap ? 0 : c + 1; };

  auto run_tick = [&](bool feeding, const std::vector<char>& out) {   // tick_run
    if (feeding) {
      bool any_out = false;
      for (char o : out) any_out = any_out || o;
      if (!ragged && any_out) { hop_s.assign((size_t)B, hop_host); ragged = true; }
      Step st{stages, std::vector<char>((size_t)B, 0)};
      for (int s = 0; s < B; ++s) {
        const bool present = !(ragged && out[(size_t)s]);
        st.present[(size_t)s] = present;
        if (!present) { ++sat_out; continue; }
        const int c = smove::own_counter(ragged, hop_s, s, hop_host);
        for (int i = 0; i < kNM; ++i) ring[(size_t)s][(size_t)i][(size_t)(c % kM[i])] = label;
        ++label;
        if (ragged) { hop_s[(size_t)s] = hop_next(hop_s[(size_t)s]); seen.fed(s, tick); }
      }
      if (!ragged) seen.fed_all(tick);
      inside.push_back(st);
      hop_host = hop_next(hop_host);
      last_feed_tick = tick;
    }
    // the launch: every step inside runs one stage; a step that has run its last one is out
    size_t keep = 0;
    for (Step& st : inside) if (--st.left > 0) inside[keep++] = st;
    inside.resize(keep);
    tick += 1;
  };
  auto drain = [&]() {   // tick_drain + tick_relevel
    const std::vector<char> nobody((size_t)B, 0);
    while (tick <= last_feed_tick + stages - 1) run_tick(false, nobody);
    CHECK(inside.empty(), "drained and %zu steps inside", inside.size());
    if (ragged) {   // every stream that lags is rotated forward to the batch's counter
      for (int s = 0; s < B; ++s) {
        const int d = sblob::counter_shift(hop_host, hop_s[(size_t)s], kWrap);
        for (int i = 0; i < kNM; ++i) {
          std::vector<long long>& r = ring[(size_t)s][(size_t)i];
          std::vector<long long> turned(r.size());
          for (size_t j = 0; j < r.size(); ++j) turned[(j + (size_t)sblob::turn(d, kM[i])) % r.size()] = r[j];
          r = turned;
        }
      }
      hop_s.assign((size_t)B, hop_host);
      ragged = false;
    }
    seen.drained();
    ++drains;
  };
  auto compare = [&](const char* when) {
    for (int s = 0; s < B; ++s) {
      bool brute = true;
      for (const Step& st : inside) brute = brute && !st.present[(size_t)s];
      const bool got = seen.quiescent(s, tick, told_stages);
      CHECK(got == brute, "%s, tick %lld, stream %d: the tracker says %d, the steps inside the pipeline say %d", when, tick, s, (int)got, (int)brute);
      (brute ? at_rest_seen : busy_seen) += 1;
    }
  };
  auto refusals = [&]() {   // the order: every -1 before any -3
    std::vector<int> all((size_t)B);
    for (int s = 0; s < B; ++s) all[(size_t)s] = s;
    smove::Side side;
    side.plain_tick = true; side.B = B; side.n = B; side.streams = all.data(); side.pointers_ok = true;
    bool all_rest = true, any_reset = false;
    for (int s = 0; s < B; ++s) { all_rest = all_rest && seen.quiescent(s, tick, told_stages); any_reset = any_reset || reset_pending[(size_t)s]; }
    CHECK(smove::args(side) == smove::kGo, "a good call refused");
    CHECK((smove::at_rest(side, seen, tick, told_stages, nullptr) == smove::kGo) == all_rest, "at_rest without flags");
    CHECK((smove::at_rest(side, seen, tick, told_stages, reset_pending.data()) == smove::kGo) == (all_rest && !any_reset), "at_rest with flags");
    smove::Side bad = side;
    bad.plain_tick = false;
    CHECK(smove::args(bad) == smove::kRefused, "another mode");
    bad = side; bad.pointers_ok = false;
    CHECK(smove::args(bad) == smove::kRefused, "a NULL pointer");
    bad = side; bad.n = 0;
    CHECK(smove::args(bad) == smove::kRefused, "n = 0");
    bad = side; bad.n = B + 1;
    CHECK(smove::args(bad) == smove::kRefused, "n = B + 1");
    bad = side; bad.streams = nullptr;
    CHECK(smove::args(bad) == smove::kRefused, "no streams");
    std::vector<int> twice = all;
    if (B > 1) { twice[1] = twice[0]; bad = side; bad.streams = twice.data(); CHECK(smove::args(bad) == smove::kRefused, "named twice"); }
    twice = all; twice[0] = B; bad = side; bad.streams = twice.data();
    CHECK(smove::args(bad) == smove::kRefused, "out of range");
    twice[0] = -1;
    CHECK(smove::args(bad) == smove::kRefused, "negative");
    ++asked;
  };
  auto import_by_hand = [&]() {   // a stream at rest is taken at its own counter and turned into another one at rest
    std::vector<int> rest;
    for (int s = 0; s < B; ++s) if (seen.quiescent(s, tick, told_stages)) rest.push_back(s);
    if (rest.empty()) return;
    const int from = rest[(size_t)pick((int)rest.size())], to = rest[(size_t)pick((int)rest.size())];
    const int c = smove::own_counter(ragged, hop_s, from, hop_host), d = smove::own_counter(ragged, hop_s, to, hop_host);
    // ... and a destination anywhere on the counter's circle, the other side of the wrap included
    const int d_far = pick(kWrap);
    for (const int dst_counter : {d, d_far}) {
      const int shift = smove::import_shift(dst_counter, c, kWrap);
      CHECK(shift >= 0 && shift < kWrap, "shift %d", shift);
      for (int i = 0; i < kNM; ++i) {
        const int m = kM[i];
        const std::vector<long long>& blob = ring[(size_t)from][(size_t)i];   // slot order
        std::vector<long long> dst((size_t)m, -99);
        for (int j = 0; j < m; ++j) dst[(size_t)((j + sblob::turn(shift, m)) % m)] = blob[(size_t)j];
        for (int k = 1; k <= m; ++k) {   // by hand: what the source wrote k steps ago is k slots behind the destination's counter
          const int src_slot = ((c - k) % m + m) % m, dst_slot = ((dst_counter - k) % m + m) % m;
          CHECK(dst[(size_t)dst_slot] == blob[(size_t)src_slot], "ring of %d slots, counters %d -> %d, %d steps back", m, c, dst_counter, k);
        }
        ++turns;
      }
      if ((c > kWrap / 2) != (dst_counter > kWrap / 2)) ++across_wrap;
    }
  };

  const std::vector<char> nobody((size_t)B, 0);
  while (tick < ticks_to_walk) {
    const int what = pick(20);
    if (what == 0) {
      drain();
      compare("after a drain");
    } else if (what <= 2) {
      run_tick(false, nobody);   // a tick that feeds nothing
    } else if (what <= 5) {
      run_tick(true, nobody);    // every stream takes part
    } else if (what <= 8) {      // one stream sits a run of steps out while the others go on: long enough to come to rest
      const int s = pick(B), run = stages - 2 + pick(4);
      std::vector<char> out((size_t)B, 0);
      out[(size_t)s] = 1;
      for (int i = 0; i < run; ++i) { run_tick(true, out); compare("inside a run of sat-out steps"); }
    } else {
      std::vector<char> out((size_t)B, 0);
      for (int s = 0; s < B; ++s) out[(size_t)s] = pick(3) == 0;
      run_tick(true, out);
    }
    compare("after a tick");
    if (pick(4) == 0) { reset_pending[(size_t)pick(B)] ^= 1; refusals(); }
    if (pick(3) == 0) import_by_hand();
  }
  drain();
  compare("at the end");
  std::printf("ok ticks %lld drains %lld sat_out %lld at_rest %lld busy %lld turns %lld across_wrap %lld asked %lld\n", tick, drains, sat_out, at_rest_seen,
              busy_seen, turns, across_wrap, asked);
  return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("stream_move_plan")
    src = d / "stream_move_plan_driver.cc"
    src.write_text(DRIVER)
    exe = d / "stream_move_plan_driver"
    # (the sanitizers' runtimes linked statically: the program carries them itself)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I", os.path.join(REPO, "beatrice-vst_amd", "csrc"), "-o", str(exe), str(src)],
                   check=True)

    def run(seed, B, stages, ticks, told_stages=None):
        return subprocess.run([str(exe), str(seed), str(B), str(stages), str(ticks), str(stages if told_stages is None else told_stages)],
                              capture_output=True, text=True)
    return run


@pytest.mark.parametrize("seed,B,stages", [(1, 3, 2), (2, 8, 5), (3, 5, 28), (4, 1, 5), (5, 8, 28), (6, 2, 2)])
def test_the_tracker_agrees_with_the_steps_inside_the_pipeline(driver, seed, B, stages):
    r = driver(seed, B, stages, 4000)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    words = r.stdout.split()
    got = {words[i]: int(words[i + 1]) for i in range(1, len(words), 2)}
    # not vacuous: streams sat out, came to rest while the pipeline was busy, were busy, rings were turned on both sides of the wrap
    assert got["ticks"] >= 4000 and got["drains"] >= 1 and got["sat_out"] >= 1 and got["asked"] >= 1, got
    assert got["at_rest"] >= 100 and got["busy"] >= 100 and got["turns"] >= 100 and got["across_wrap"] >= 1, got


@pytest.mark.parametrize("stages", [2, 5, 28])
def test_a_tracker_told_one_stage_fewer_is_caught(driver, stages):
    r = driver(1, 5, stages, 4000, told_stages=stages - 1)
    assert r.returncode == 1 and "the steps inside the pipeline say 0" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
