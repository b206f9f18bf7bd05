"""The quiescence rule of a batch around resident 48 kHz blocks (mode F; beatrice-vst_amd/csrc/stream_move_plan.h kRuleAround48k;
BeatriceBatch_Stream48kQuiescent / ExportStreams48kInFlight / ImportStreams48kInFlight / MoveStreams48kInFlight) without a GPU.  The
header is plain C++17 without HIP: a stand-alone program with its own main is compiled against it with g++ under the address and
undefined-behaviour sanitizers and run directly.

It walks seeded sequences of what such a batch does -- steps every stream takes part in, steps some streams sit out, ticks that feed
nothing, drains -- the way tick_run / tick_drain do, and marks the tracker where they mark it.  Against it stands a brute-force model of
the pipeline WITH the wrapper around it: the steps inside the ticks, each with the stages it has still to run, and the one step whose
output half is still owed (it runs in the wrapper launch in front of the next tick, or in the flush launch of a drain).  Every launch is
recorded with the streams whose state it touches -- a tick launch the rings of the streams of every step inside, a wrapper launch the
input-half state of the streams of the step being fed and the output-half state of the streams of the step owed.
  * Whenever the rule says "at rest", no launch from then on may touch the stream until it is fed again (checked at every launch).
  * Whenever it says "busy", a launch that touches the stream must still be to come without any feed (a step inside, or the owed one).
  * So one launch earlier than "at rest" it says busy; a tracker told one stage fewer, and the plain rule of mode D asked of this
    pipeline, are both caught saying "at rest" one launch too early.
The order of the refusals is asked on the way: every -1 before any -3, a D batch asked by the 48k calls and the reverse among them."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "stream_move_plan.h"

using namespace bhip;
#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

struct Step { int left; std::vector<char> present; };   // a step inside the ticks and the stages it has still to run

int main(int argc, char** argv) {
  if (argc != 7) return 2;
  const unsigned seed = (unsigned)std::atoi(argv[1]);
  const int B = std::atoi(argv[2]), stages = std::atoi(argv[3]), ticks_to_walk = std::atoi(argv[4]), told_stages = std::atoi(argv[5]);
  const smove::Rule rule = std::atoi(argv[6]) ? smove::kRuleAround48k : smove::kRulePlain;
  std::mt19937 rng(seed);
  auto pick = [&](int n) { return (int)(rng() % (unsigned)n); };

  long long tick = 0, last_feed_tick = -1000, launches = 0;
  bool ragged = false;
  std::vector<unsigned char> reset_pending((size_t)B, 0);
  smove::Presence seen;
  seen.start(B);
  std::vector<Step> inside;
  bool owed = false;                 // Resident48::deferred_slot >= 0
  std::vector<char> owed_present;    // ... and who took part in that step
  std::vector<long long> said_at_rest((size_t)B, -1);   // the launch count at which the rule said "at rest" and the stream has not been fed since
  long long asked = 0, at_rest_seen = 0, busy_seen = 0, drains = 0, sat_out = 0, flushes = 0, wrapper_launches = 0, owed_alone = 0;

  // a launch and the streams whose state it touches: nobody the rule has declared at rest
  auto launch = [&](const char* what, const std::vector<char>& touched) {
    for (int s = 0; s < B; ++s)
      CHECK(!(touched[(size_t)s] && said_at_rest[(size_t)s] >= 0), "%s (launch %lld, tick %lld) touches stream %d, which the rule declared at rest at launch %lld",
            what, launches, tick, s, said_at_rest[(size_t)s]);
    ++launches;
  };
  auto run_tick = [&](bool feeding, const std::vector<char>& out) {   // tick_run
    std::vector<char> present((size_t)B, 0);
    if (feeding) {
      bool any_out = false;
      for (char o : out) any_out = any_out || o;
      if (!ragged && any_out) ragged = true;
      for (int s = 0; s < B; ++s) {
        present[(size_t)s] = !(ragged && out[(size_t)s]);
        if (!present[(size_t)s]) { ++sat_out; continue; }
        said_at_rest[(size_t)s] = -1;   // fed again
        if (ragged) seen.fed(s, tick);
      }
      if (!ragged) seen.fed_all(tick);
      inside.push_back(Step{stages, present});
      last_feed_tick = tick;
    }
    if (feeding || owed) {   // the wrapper launch: the input half of the step being fed, the output half of the step owed
      std::vector<char> touched = present;
      if (owed) for (int s = 0; s < B; ++s) touched[(size_t)s] = touched[(size_t)s] || owed_present[(size_t)s];
      launch("the wrapper launch", touched);
      owed = false;
      ++wrapper_launches;
    }
    {   // the tick launch: every step inside runs one stage; the step that runs its last one owes its output half
      std::vector<char> touched((size_t)B, 0);
      for (const Step& st : inside) for (int s = 0; s < B; ++s) touched[(size_t)s] = touched[(size_t)s] || st.present[(size_t)s];
      launch("the tick launch", touched);
      size_t keep = 0;
      for (Step& st : inside) {
        if (--st.left > 0) { inside[keep++] = st; continue; }
        CHECK(!owed, "two steps left the ticks in one launch");
        owed = true; owed_present = st.present;
      }
      inside.resize(keep);
    }
    tick += 1;
  };
  auto drain = [&]() {   // tick_drain: idle ticks, the flush launch, one counter again, the marks cleared
    const std::vector<char> nobody((size_t)B, 0);
    while (tick <= last_feed_tick + stages - 1) run_tick(false, nobody);
    CHECK(inside.empty(), "drained and %zu steps inside", inside.size());
    if (owed) { launch("the flush launch", owed_present); owed = false; ++flushes; }
    ragged = false;
    seen.drained();
    ++drains;
  };
  auto compare = [&](const char* when) {
    bool only_owed = false;
    for (int s = 0; s < B; ++s) {
      bool to_come = owed && owed_present[(size_t)s];   // without a feed: the stages the steps inside still run, and the output half owed
      const bool in_ticks = [&] { for (const Step& st : inside) if (st.present[(size_t)s]) return true; return false; }();
      only_owed = only_owed || (to_come && !in_ticks);
      to_come = to_come || in_ticks;
      const bool got = smove::quiescent(seen, rule, s, tick, told_stages);
      CHECK(got == !to_come, "%s, tick %lld, stream %d: the rule says %d, the launches still to come say %d", when, tick, s, (int)got, (int)!to_come);
      if (got && said_at_rest[(size_t)s] < 0) said_at_rest[(size_t)s] = launches;
      (got ? at_rest_seen : busy_seen) += 1;
    }
    if (only_owed) ++owed_alone;   // (the launch the plain rule does not know about)
  };
  auto refusals = [&]() {   // the order: every -1 before any -3
    std::vector<int> all((size_t)B);
    for (int s = 0; s < B; ++s) all[(size_t)s] = s;
    smove::Side side;
    side.around48k = true; side.rule = smove::kRuleAround48k; side.B = B; side.n = B; side.streams = all.data(); side.pointers_ok = true;
    bool all_rest = true, any_reset = false;
    for (int s = 0; s < B; ++s) { all_rest = all_rest && smove::quiescent(seen, smove::kRuleAround48k, s, tick, stages); any_reset = any_reset || reset_pending[(size_t)s]; }
    CHECK(smove::args(side) == smove::kGo, "a good call refused");
    CHECK((smove::at_rest(side, seen, tick, stages, nullptr) == smove::kGo) == all_rest, "at_rest without flags");
    CHECK((smove::at_rest(side, seen, tick, stages, reset_pending.data()) == smove::kGo) == (all_rest && !any_reset), "at_rest with flags");
    smove::Side bad = side;
    bad.around48k = false; bad.plain_tick = true;    // a D batch asked by the 48k calls
    CHECK(smove::args(bad) == smove::kRefused, "the 48k calls on a batch in plain tick mode");
    bad = side; bad.rule = smove::kRulePlain;        // an F batch asked by the plain calls
    CHECK(smove::args(bad) == smove::kRefused, "the plain calls on a batch around 48 kHz blocks");
    bad.plain_tick = true;
    CHECK(smove::args(bad) == smove::kGo, "the plain calls on a batch in plain tick mode");
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
    // a call that is wrong AND names a busy stream is refused for being wrong: args() is asked first and never looks at the pipeline
    ++asked;
  };

  const std::vector<char> nobody((size_t)B, 0);
  while (tick < ticks_to_walk) {
    const int what = pick(20);
    if (what == 0) {
      drain();
      compare("after a drain");
    } else if (what <= 5) {
      run_tick(true, nobody);    // every stream takes part
    } else if (what <= 9) {      // one stream sits a run of steps out while the others go on: long enough to come to rest, or one short of it
      const int s = pick(B), run = stages - 1 + pick(4);
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
  }
  drain();
  compare("at the end");
  std::printf("ok ticks %lld drains %lld sat_out %lld at_rest %lld busy %lld launches %lld wrapper_launches %lld flushes %lld owed_alone %lld asked %lld\n", tick, drains,
              sat_out, at_rest_seen, busy_seen, launches, wrapper_launches, flushes, owed_alone, asked);
  return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("stream_move48k_plan")
    src = d / "stream_move48k_plan_driver.cc"
    src.write_text(DRIVER)
    exe = d / "stream_move48k_plan_driver"
    # (the sanitizers' runtimes linked statically: the program carries them itself)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I", os.path.join(REPO, "beatrice-vst_amd", "csrc"), "-o", str(exe), str(src)],
                   check=True)

    def run(seed, B, stages, ticks, told_stages=None, rule48k=True):
        return subprocess.run([str(exe), str(seed), str(B), str(stages), str(ticks), str(stages if told_stages is None else told_stages),
                               "1" if rule48k else "0"], capture_output=True, text=True)
    return run


@pytest.mark.parametrize("seed,B,stages", [(1, 3, 3), (2, 8, 5), (3, 5, 28), (4, 1, 5), (5, 8, 30), (6, 2, 3), (7, 8, 17)])
def test_the_rule_agrees_with_the_launches_still_to_come(driver, seed, B, stages):
    r = driver(seed, B, stages, 4000)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    words = r.stdout.split()
    got = {words[i]: int(words[i + 1]) for i in range(1, len(words), 2)}
    # not vacuous: streams sat out, came to rest while the pipeline was busy, were busy with nothing but the owed output half to come
    assert got["ticks"] >= 4000 and got["drains"] >= 1 and got["sat_out"] >= 1 and got["asked"] >= 1 and got["flushes"] >= 1, got
    assert got["at_rest"] >= 100 and got["busy"] >= 100 and got["owed_alone"] >= 10 and got["wrapper_launches"] >= 1000, got


@pytest.mark.parametrize("stages", [3, 5, 28])
def test_a_rule_told_one_stage_fewer_is_caught(driver, stages):
    r = driver(1, 5, stages, 4000, told_stages=stages - 1)
    assert r.returncode == 1 and "the launches still to come say 0" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


@pytest.mark.parametrize("stages", [3, 5, 28])
def test_the_plain_rule_is_one_launch_too_early_for_this_pipeline(driver, stages):
    """what mode D asks -- the step has left the last stage -- says "at rest" while the step's output half is still owed"""
    r = driver(1, 5, stages, 4000, rule48k=False)
    assert r.returncode == 1 and "the rule says 1, the launches still to come say 0" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
