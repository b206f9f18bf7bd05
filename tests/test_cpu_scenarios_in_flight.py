"""The generator and the model of tests/scenario_in_flight.py are what they claim, and the scenarios can tell (no GPU).

* the same seed gives the same scenario, and it survives json;
* COVERAGE IS A CONDITION: over the committed list every named interaction is reached by at least three scenarios, and in a D step at every
  H of 1, 2, 4 (the rule of tests/test_cpu_scenarios.py::test_every_interaction_is_reached); D cells that cannot exist are listed with their
  reason and are seen to be empty (a move as its drained fall-back is defined for A steps);
* the list has the shapes the family was planned with, few enough oracle legs and hops, a reference for every stream, and between 10 % and
  40 % of its planned in-flight calls are predicted to be refused with -3;
* THE PYTHON QUIESCENCE MODEL IS THE HEADER: a stand-alone program that includes csrc/stream_move_plan.h (compiled alone, as
  tests/test_cpu_scenarios.py compiles batch_modes.h) is given each scenario's fed, drained and present marks and prints
  smove::Presence::quiescent() per (batch, step, slot): the output equals the model's table;
* THE SCENARIOS DISCRIMINATE: seven deliberately wrong variants of the oracle's script, one per family, each differ from the unmutated leg
  within 8 steps of the first place their scripts part, on some scenario of the list (cheapest first)."""
import json
import os
import subprocess

import numpy as np
import pytest

import scenario_in_flight as si

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IN_FLIGHT = ("reset", "install", "move")


@pytest.fixture(scope="module")
def scns():
    return si.scenarios()


@pytest.fixture(scope="module")
def reps(scns):
    return [si.replay(s) for s in scns]


def test_same_seed_same_scenario(scns):
    args = si.SEEDS[5]
    one, two = si.make_scenario(*args), si.make_scenario(*args)
    assert json.dumps(one) == json.dumps(two)
    back = json.loads(json.dumps(one))
    assert json.dumps(back) == json.dumps(one), "a scenario is plain data: it survives json unchanged"
    assert si.interactions(back) == si.interactions(one)
    other = si.make_scenario(args[0] + 100, *args[1:])
    assert json.dumps(other["events"]) != json.dumps(one["events"])
    assert len({json.dumps(s["events"]) for s in scns}) == len(scns)


def test_every_interaction_is_reached(scns, reps):
    cells, per_name = {}, {name: set() for name in si.INTERACTIONS}
    for s, r in zip(scns, reps):
        for name, hits in r["world"].hits.items():
            for h in hits:
                cells.setdefault((name, h["mode"], h["H"]), set()).add(s["seed"])
                per_name[name].add(s["seed"])
    cols = [(m, H) for m in "ADE" for H in (1, 2, 4)]
    print("\nscenarios that reach an interaction, per (mode of the step, hops per step); over %d scenarios" % len(scns))
    print("%-48s %s  total" % ("", " ".join("%s%d" % c for c in cols)))
    for name in si.INTERACTIONS:
        print("%-48s %s  %5d  %s" % (name, " ".join("%2d" % len(cells.get((name, m, H), ())) for m, H in cols), len(per_name[name]), sorted(per_name[name])))
    for (name, H), why in si.UNREACHABLE.items():
        print("unreachable: %s at H = %d -- %s" % (name, H, why))
        assert not cells.get((name, "D", H)), "%s at H = %d is listed as unreachable in a D step and was reached there" % (name, H)
    missing = [name for name in si.INTERACTIONS if len(per_name[name]) < 3]
    assert not missing, "reached by fewer than three scenarios: %s" % missing
    holes = [(name, H) for name in si.INTERACTIONS for H in (1, 2, 4) if (name, H) not in si.UNREACHABLE and not cells.get((name, "D", H))]
    assert not holes, "not reached in a D step: %s" % holes


def test_the_list_has_the_shapes_the_family_was_planned_with(scns, reps):
    assert 12 <= len(scns) <= 16
    assert {(s["B"]["X"], s["B"]["Y"]) for s in scns} == {(1, 1), (5, 3), (24, 5), (37, 24), (37, 37), (256, 37)}
    assert {s["H"] for s in scns} == {1, 2, 4}
    assert [(s["B"]["X"], s["H"]) for s in scns if s["B"]["X"] == 256] == [(256, 4)]
    assert {s["seed"] for s in scns} >= set(si.ACROSS_THE_WRAP) and len(si.ACROSS_THE_WRAP) == 4
    planned = refused = 0
    for s, r in zip(scns, reps):
        w = r["world"]
        steps = len(s["events"])
        assert 40 <= steps <= 70 and 1 <= len(s["phases"]) <= 3, si.scenario_id(s)
        assert len(s["legs"]) <= 10 and si.oracle_hops(s, w) <= 2800, si.scenario_id(s)
        # every stream of both batches has a reference: the oracle for the logical streams an event touches, that sit out or that move
        # (and whatever is fed in a slot they leave), the product's in-order chain for the streams that start in a slot and never leave it,
        # never sit out and see no call but a reset of every stream
        legs, rest = set(s["legs"]), si.untouched(s, w)
        for L, ops in w.timeline.items():
            home = {(what[2], what[3]) for what in ops if what[0] == "hop"}
            if L not in legs:
                assert len(home) == 1 and L < s["B"]["X"] + s["B"]["Y"], "logical stream %d has no reference" % L
                (b, slot), = home
                assert slot in rest[b] and si.w_initial(b, s["B"], slot) == L
                assert sum(1 for what in ops if what[0] == "hop") == steps, "a stream compared with the in-order chain never sits out"
                assert all(what[0] in ("hop", "reset") for what in ops[3:])
        for b in "XY":
            assert all(slot not in rest[b] for ab in s["absent"][b] for slot in ab)
            if s["bystanders"][b] is not None:
                assert si.w_initial(b, s["B"], s["bystanders"][b]) in legs
        calls = [(ev, rc) for k in range(steps) for ev, rc in s["events"][k] + s["after"][k] if ev[0] in IN_FLIGHT]
        assert all(rc in (0, -3) for _, rc in calls)
        assert all(rc == 0 for k in range(steps) for ev, rc in s["events"][k] + s["after"][k] if ev[0] not in IN_FLIGHT)
        planned += len(calls)
        refused += sum(1 for _, rc in calls if rc == -3)
        at, _ = si._phase_table(s["phases"])
        for k in range(steps):      # moves where both batches are in D; in E reset and install only
            for ev, rc in s["events"][k]:
                assert ev[0] != "move" or at[k][1] in "DA"
                assert at[k][1] != "E" or ev[0] in ("reset", "install", "set", "refeed")
    print("\n%d planned in-flight calls, %d predicted -3 (%.0f %%)" % (planned, refused, 100.0 * refused / planned))
    assert 0.10 <= refused / planned <= 0.40
    corners = {(b, slot) for s in scns for b in "XY" if s["B"][b] >= 24 for slot in s["actors"][b]}
    assert {slot for _, slot in corners} & {15, 16, 31, 32}


def test_the_wrap_falls_inside_the_four_scenarios_with_a_move_between(bv, scns):
    Bv = bv
    for s in scns:
        if s["seed"] not in si.ACROSS_THE_WRAP:
            continue
        start = si.wrap_starts(Bv, s)
        kx, ky = Bv.STEP_WRAP - start["X"], Bv.STEP_WRAP - start["Y"]      # the step at which each batch's counter is 0 again
        assert 0 < kx < ky < len(s["events"])
        between = [k for k in range(kx, ky + 1) for ev, rc in s["events"][k] if ev[0] == "move" and rc == 0]
        assert between, "%s: no move between X's wrap (step %d) and Y's (step %d)" % (si.scenario_id(s), kx, ky)


DUMPER = """
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "stream_move_plan.h"
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  bhip::smove::Presence p;
  int B = 0;
  char line[1 << 16];
  while (std::fgets(line, sizeof(line), f)) {
    char* tok = std::strtok(line, " \\n");
    if (!tok) continue;
    const char c = tok[0];
    if (c == 'S') { B = std::atoi(std::strtok(nullptr, " \\n")); p.start(B); }
    else if (c == 'D') p.drained();
    else if (c == 'F') p.fed_all(std::atoll(std::strtok(nullptr, " \\n")));
    else if (c == 'P') {
      const long long t = std::atoll(std::strtok(nullptr, " \\n"));
      while ((tok = std::strtok(nullptr, " \\n"))) p.fed(std::atoi(tok), t);
    } else if (c == 'A') {
      const long long ticks = std::atoll(std::strtok(nullptr, " \\n"));
      const int stages = std::atoi(std::strtok(nullptr, " \\n"));
      for (int s = 0; s < B; ++s) std::putchar(p.quiescent(s, ticks, stages) ? '1' : '0');
      std::putchar('\\n');
    }
  }
  std::fclose(f);
  return 0;
}
"""


def test_the_quiescence_model_is_the_header(scns, reps, tmp_path):
    """from csrc/stream_move_plan.h itself (compiled alone), not from a second hand-written copy of the rule"""
    src = tmp_path / "ask_presence.cc"
    src.write_text(DUMPER)
    exe = tmp_path / "ask_presence"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "beatrice-vst_amd", "csrc"), "-o", str(exe), str(src)], check=True)
    asked = 0
    for s, r in zip(scns, reps):
        for b in "XY":
            m = r["world"].M[b]
            lines, want = [], []
            for mark in m.trace:
                if mark[0] == "start":
                    lines.append("S %d" % m.B)
                elif mark[0] == "drained":
                    lines.append("D")
                elif mark[0] == "step":
                    _, tick, absent = mark
                    lines.append("F %d" % tick if absent is None else "P %d %s" % (tick, " ".join(str(x) for x in range(m.B) if x not in absent)))
                else:
                    _, tick, k = mark
                    lines.append("A %d %d" % (tick, si.STAGES))
                    want.append("".join(str(q) for q in r["probes"][k][b][0]))
            path = tmp_path / ("marks_%d_%s.txt" % (s["seed"], b))
            path.write_text("\n".join(lines) + "\n")
            got = subprocess.run([str(exe), str(path)], check=True, capture_output=True, text=True).stdout.split()
            assert len(got) == len(want) > 0
            for i, (g, wnt) in enumerate(zip(got, want)):
                assert g == wnt, "%s batch %s, %d-th D step: the header says %s, the model %s" % (si.scenario_id(s), b, i, g, wnt)
            asked += len(want)
            assert any("0" in x for x in want) and any("1" in x for x in want)
    print("\n%d rows of quiescence answers equal the header's" % asked)


MUTANTS = ["reset_at_call", "reset_restores_defaults", "reset_survives_import", "pending_flushed", "pitch_context_lost", "previous_voice",
           "refeed_from_zeros"]
HORIZON, TRIES = 8, 4


def _first_parting(good, bad):
    """(index of the first op that differs, the step of the next compared hop of the unmutated script from there) or None"""
    for i in range(max(len(good), len(bad))):
        if i >= len(good) or i >= len(bad) or good[i] != bad[i]:
            nxt = [what[1] for what in good[i:] if what[0] == "hop"]
            return (i, nxt[0]) if nxt else None
    return None


@pytest.mark.parametrize("mutant", MUTANTS)
def test_a_wrong_reference_is_told_apart(bv, oracle, scns, reps, tmp_path_factory, mutant):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_model
    d = str(tmp_path_factory.mktemp("model8s"))
    make_model.make_model(d, n_speakers=si.REAL)
    env = si.Env(bv, oracle, None, d)
    occurrences = []
    for s, r in zip(scns, reps):
        bad = si.replay(s, mutant=mutant, check=False)["world"]
        for L in s["legs"]:
            at = _first_parting(r["world"].timeline[L], bad.timeline.get(L, []))
            if at is not None:
                occurrences.append(((at[1] + HORIZON) * s["H"], s["seed"], L, at[1], s, r["world"].timeline[L], bad.timeline[L], r["world"].audio_of[L]))
    occurrences.sort(key=lambda o: o[:4])
    assert occurrences, "no scenario's script changes under %s" % mutant
    om = si.oracle_models(env)
    try:
        for cost, seed, L, step, s, good, bad, who in occurrences[:TRIES]:
            xs = si.audio(bv, s, who, len(s["events"]))
            y, _ = si.run_leg(env, s, om, good, xs, stop_after=step + HORIZON)
            z, _ = si.run_leg(env, s, om, bad, xs, stop_after=step + HORIZON)
            for (k, _, _, p), (k2, _, _, q) in zip(y, z):
                assert k == k2
                if not np.array_equal(p, q):
                    assert step <= k <= step + HORIZON
                    print("\nmutant %s told apart: %s, logical stream %d, step %d (the scripts part before step %d), max-abs %g"
                          % (mutant, si.scenario_id(s), L, k, step, float(np.abs(p - q).max())))
                    return
    finally:
        om.close()
    pytest.fail("%s equals the unmutated leg within %d steps on the %d cheapest occurrences" % (mutant, HORIZON, min(TRIES, len(occurrences))))
