"""The scenario generator of tests/scenario.py is what it claims, and its scenarios can tell (no GPU).

* the same seed gives the same scenario, another seed another one;
* every entry point of the mode table that the product runner calls for a scenario of the committed list is allowed by
  beatrice-vst_amd/csrc/batch_modes.h in the mode the batch is in at that call (the header compiled alone, as tests/test_cpu_mode_table.py does);
* COVERAGE IS A CONDITION: over the committed list every named interaction is reached by at least three scenarios, and in a tick phase at
  every H of 1, 2, 4 -- the cells that cannot exist are listed with the reason (scenario.UNREACHABLE) and are seen to be empty;
* THE SCENARIOS DISCRIMINATE: OracleBatch with one small deliberate deviation of the reference protocol each ("mutants") gives, for the
  stream the deviation touches, samples that differ from the unmutated leg in some scenario of the list.  An oracle hop costs milliseconds,
  so each mutant runs on one stream of the cheapest scenarios that hold its interaction, beside the unmutated stream, and stops at the
  first step that differs."""
import json
import os
import subprocess

import numpy as np
import pytest

import scenario as sc
from oracle_batch import OracleBatch, _Calls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def scns():
    return sc.scenarios()


def test_same_seed_same_scenario(scns):
    seed, B, H, phases = sc.SEEDS[4]
    one, two = sc.make_scenario(seed, B, H, phases), sc.make_scenario(seed, B, H, phases)
    assert json.dumps(one) == json.dumps(two)
    assert json.loads(json.dumps(one)) == one, "a scenario is plain data: it survives json unchanged"
    other = sc.make_scenario(seed + 1, B, H, phases)
    assert json.dumps(other["events"]) != json.dumps(one["events"]) and other["absent"] != one["absent"]
    assert len({json.dumps(s["events"]) for s in scns}) == len(scns)
    assert sc.interactions(one) == sc.interactions(two)


def test_the_list_has_the_shapes_the_issue_names(scns):
    assert 20 <= len(scns) <= 30
    assert {s["B"] for s in scns} == {1, 5, 24, 37, 256} and {s["H"] for s in scns} == {1, 2, 4}
    assert sum(1 for s in scns if s["B"] == 256) <= 4
    for s in scns:
        steps = len(s["events"])
        assert 2 <= len(s["phases"]) <= 4 and (40 <= steps <= 90 or steps >= 330), sc.scenario_id(s)
        assert s["B"] == 1 or s["B"] % 16 != 0 or s["B"] == 256, "the last 16-row tile is ragged"
    assert any(len(s["events"]) >= 330 and s["H"] == 4 and len(s["sample"]) <= 4 for s in scns), "one long scenario at four hops per step"
    # every stream has a reference: the oracle for the sampled ones, the product's in-order chain for those that never sit a step out
    for s in scns:
        away = {x for ab in s["absent"] for x in ab}
        assert len(away) <= 8 and len(s["sample"]) <= 12 and away <= set(s["sample"]), sc.scenario_id(s)
        assert set(s["sample"]) | set(sc.never_absent(s)) == set(range(s["B"]))
        assert set(s["actors"]) <= set(s["sample"])
        for ev in s["initial"] + [e for evs in s["events"] for e in evs]:
            assert ev[0] in sc.VOCABULARY and (ev[1] >= -1 or ev[0] == "SetTargetSpeakers")
    # tile corners are among the streams the oracle follows
    corners = {x for s in scns if s["B"] >= 37 for x in s["sample"]}
    assert {0, 15, 16, 31, 32} <= corners and any(s["B"] - 1 in s["sample"] for s in scns if s["B"] >= 24)


def test_the_bench_default_shape_class_is_in_the_list(scns):
    """tests/test_cpu_bench_defaults_are_tested.py stays as it is; here: tick mode at the bench's default hops per step in at least three
    scenarios, one of them at the bench's default number of streams"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_for_scenarios", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    H = bench.DEFAULT_HOPS_PER_STEP_TICK
    hits = [s for s in scns if s["H"] == H and any(m == "D" for m, _ in s["phases"])]
    assert len(hits) >= 3
    assert any(s["B"] == bench.DEFAULT_STREAMS[bench.DEFAULT_CONFIG] for s in hits)


DUMPER = """
#include <cstdio>
#include <cstring>
#include "batch_modes.h"
using namespace bhip::modes;
static void ask(int id, const char* name, Flags f) {
  for (int e = 0; e < kEntries; ++e)
    if (!std::strcmp(kTable[e].name, name)) { std::printf("%d %d %c\\n", id, allowed((Entry)e, f) ? 1 : 0, "ABCDEFGPS"[(int)mode_of(f)]); return; }
  std::printf("%d unknown\\n", id);
}
int main() {
QUERIES  return 0;
}
"""


def test_every_call_of_the_runner_is_allowed_by_the_mode_table(scns, tmp_path):
    """from the header itself (compiled alone), not from a second hand-written copy of the table"""
    queries = []
    for s in scns:
        for entry, flags, letter in sc.calls_of(s):
            q = (entry, tuple(sorted(flags.items())), letter)
            if q not in queries:
                queries.append(q)
    body = ""
    for i, (entry, flags, letter) in enumerate(queries):
        body += "  { Flags f; %s ask(%d, \"%s\", f); }\n" % (" ".join("f.%s = %s;" % (k, str(v).lower()) for k, v in flags), i, entry)
    src = tmp_path / "ask_modes.cc"
    src.write_text(DUMPER.replace("QUERIES", body))
    exe = tmp_path / "ask_modes"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "beatrice-vst_amd", "csrc"), "-o", str(exe), str(src)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == len(queries) > 10
    for ln, (entry, flags, letter) in zip(lines, queries):
        _, ok, mode = ln.split()
        assert ok == "1", "%s with %s is refused by the table (mode %s)" % (entry, dict(flags), mode)
        assert letter is None or mode == letter, "%s with %s: the flags derive to mode %s, the phase is %s" % (entry, dict(flags), mode, letter)
    assert {"SetSilentStreams", "StreamFrames", "EnablePipelining(2)", "EnableTickPipeline(0)", "EnableSilentBlockRule(0)"} <= {q[0] for q in queries}
    # sit-outs exist in tick phases only (in order the flags are cleared for any step that is not a 48 kHz block)
    for s in scns:
        at, _ = sc._phase_table(s["phases"])
        assert all(at[k][1] == "D" for k, ab in enumerate(s["absent"]) if ab)


def test_every_interaction_is_reached(scns):
    cells = {}      # (name, mode, H) -> scenarios
    per_name = {name: set() for name in sc.INTERACTIONS}
    for s in scns:
        for name, hits in sc.interactions_detail(s).items():
            for h in hits:
                cells.setdefault((name, h["mode"], h["H"]), set()).add(s["seed"])
                per_name[name].add(s["seed"])
        assert set(sc.interactions(s)) == {n for n, hits in sc.interactions_detail(s).items() if hits}
    cols = [(m, H) for m in "ABCDE" for H in (1, 2, 4)]
    print("\nscenarios that reach an interaction, per (mode of the step, hops per step); over %d scenarios" % len(scns))
    print("%-36s %s  total" % ("", " ".join("%s%d" % c for c in cols)))
    for name in sc.INTERACTIONS:
        print("%-36s %s  %5d" % (name, " ".join("%2d" % len(cells.get((name, m, H), ())) for m, H in cols), len(per_name[name])))
    for (name, H), why in sc.UNREACHABLE.items():
        print("unreachable: %s at H = %d -- %s" % (name, H, why))
        assert not any(cells.get((name, m, H)) for m in "ABCDE"), "%s at H = %d is listed as unreachable and was reached" % (name, H)
    missing = [name for name in sc.INTERACTIONS if len(per_name[name]) < 3]
    assert not missing, "reached by fewer than three scenarios: %s" % missing
    holes = [(name, H) for name in sc.INTERACTIONS for H in (1, 2, 4) if (name, H) not in sc.UNREACHABLE and not cells.get((name, "D", H))]
    assert not holes, "not reached in a tick phase: %s" % holes


def test_a_failure_can_be_told_as_one_streams_story(scns):
    """what a failing comparison prints: the stream's own events with its pending-install count, its present / absent history, the
    interactions that touch it"""
    s = scns[4]
    hit = sc.interactions_detail(s)["switch_then_sitout_while_pending"][0]
    story = sc.stream_story(s, hit["stream"], hit["step"] + 3)
    print("\n" + story)
    assert "seed %d, B = %d, H = %d" % (s["seed"], s["B"], s["H"]) in story and str(s["phases"]) in story
    assert "step %3d [D] ABSENT" % hit["step"] in story and "(pending " in story and "-> pending" in story
    assert "switch_then_sitout_while_pending at steps" in story and "mode per step" in story


# ---- mutants of the reference ----------------------------------------------------------------------------------------------------------
def _calls(**methods):
    return type("MutantCalls", (_Calls,), {"BeatriceBatch_" + k: v for k, v in methods.items()})


def _switch_keeps_count(self, h, stream, speaker):
    def f(c):
        before = c["s1"].kv_count
        c["speaker"] = speaker
        c["s1"].set_target_speaker(speaker)
        if before < 4:
            c["s1"].kv_count = before       # WRONG: the second switch carries on where the first one's installs stood
    return self._each(stream, f)


def _switch_remembering(self, h, stream, speaker):
    def f(c):
        if c["s1"].kv_count == 4:
            c["settled"] = c["speaker"]     # (the speaker whose four blocks are installed)
        c["speaker"] = speaker
        c["s1"].set_target_speaker(speaker)
    return self._each(stream, f)


def _reset_leaves_blocks_pending(self, h, stream):
    def f(c):
        n, bv = c["s1"].kv_count, self.o.bv
        self.o._fresh(c)
        if n < 4:                           # WRONG: the blocks the switch had not installed yet stay the old speaker's and follow one per hop
            s1 = c["s1"]
            s1.a.RegisterKeyValueSpeakerEmbedding(s1.m.embed, bv.fptr(s1.m.tables.kv[c.get("settled", 0)]), s1.ec)
            for blk in range(n, 4):
                s1.a.SetKeyValueSpeakerEmbedding(s1.m.embed, blk, s1.ec, s1.wc)
            s1.a.RegisterKeyValueSpeakerEmbedding(s1.m.embed, bv.fptr(s1.m.tables.kv[c["speaker"]]), s1.ec)
            s1.kv_count = n
    return self._each(stream, f)


def _flush_installs_three(self, h, stream):
    def f(c):
        while c["s1"].kv_count < 3:
            c["s1"].set_kv_block()
        c["s1"].kv_count = 4                # WRONG: the fourth block is never installed
    return self._each(stream, f)


def _reset_keeps_pitch_context(self, h, stream):
    def f(c):
        old = c["s1"]
        c["s1"] = None
        self.o._fresh(c)
        new = c["s1"]
        new.a.DestroyPitchContext1(new.tc)
        new.tc = old.tc                     # WRONG: the pitch estimator's context (its previous bin, its history) survives the reset
        old.a.DestroyPhoneContext1(old.pc)
        old.a.DestroyWaveformContext1(old.wc)
        old.a.DestroyEmbeddingContext(old.ec)
    return self._each(stream, f)


def _dropped_while_absent(name):
    base = getattr(_Calls, "BeatriceBatch_" + name)

    def call(self, h, stream, *args):
        if stream in self.o.st and self.o.st[stream]["absent"]:
            return 0                        # WRONG: a setting made while the stream sits out is lost
        return base(self, h, stream, *args)
    return call


def _knn_late(self, h, stream, k):
    c = self.o.st.get(stream)
    if c is not None and c["absent"]:
        c["late_k"] = k                     # WRONG: applied after the stream's next step instead of before it
        return 0
    return _Calls.BeatriceBatch_SetVQNumNeighbors(self, h, stream, k)


class SecondSwitchKeepsCount(OracleBatch):
    calls_class = _calls(SetTargetSpeaker=_switch_keeps_count)


class ResetLeavesBlocksPending(OracleBatch):
    calls_class = _calls(SetTargetSpeaker=_switch_remembering, ResetStream=_reset_leaves_blocks_pending)


class SitOutConsumesInstalls(OracleBatch):
    def sit_out(self, s):
        for _ in range(self.H):             # WRONG: one pending block per hop that was never made
            self.st[s]["s1"].set_kv_block()


class SettingWhileAbsentDropped(OracleBatch):
    calls_class = _calls(**{name: _dropped_while_absent(name) for name in sc.SETTERS})


class FlushInstallsThree(OracleBatch):
    calls_class = _calls(FlushSpeaker=_flush_installs_three)


class ResetKeepsPitchContext(OracleBatch):
    calls_class = _calls(ResetStream=_reset_keeps_pitch_context)


class KnnOfAbsentStreamOneStepLate(OracleBatch):
    calls_class = _calls(SetVQNumNeighbors=_knn_late)

    def step_stream(self, s, xs):
        y = super().step_stream(s, xs)
        c = self.st[s]
        if "late_k" in c:
            _Calls.BeatriceBatch_SetVQNumNeighbors(self.a, None, s, c.pop("late_k"))
        return y


MUTANTS = [("a", SecondSwitchKeepsCount, "switch_while_pending"), ("b", ResetLeavesBlocksPending, "reset_while_pending"),
           ("c", SitOutConsumesInstalls, "switch_then_sitout_while_pending"), ("d", SettingWhileAbsentDropped, "setting_while_absent"),
           ("e", FlushInstallsThree, "flush_while_pending"), ("f", ResetKeepsPitchContext, "reset_on_return"),
           ("g", KnnOfAbsentStreamOneStepLate, "knn_change_while_absent")]
TRIES = 4        # occurrences tried per mutant, cheapest first (a deviation can be masked: the switch went to the speaker already installed ...)
HORIZON = 8      # steps after the interaction within which the samples must differ


@pytest.mark.parametrize("letter,mutant,interaction", MUTANTS, ids=[m[1].__name__ for m in MUTANTS])
def test_a_wrong_reference_is_told_apart(bv, oracle, model_dir, scns, letter, mutant, interaction):
    occurrences = []
    for s in scns:
        for h in sc.interactions_detail(s)[interaction]:
            if h["stream"] in s["sample"]:
                occurrences.append(((h["step"] + HORIZON) * s["H"], s["seed"], h["step"], h["stream"], s))
    occurrences.sort(key=lambda o: o[:4])
    assert occurrences, "no scenario holds %s on a sampled stream" % interaction
    models = bv.Models(oracle, model_dir)
    hops = 0
    try:
        seen = set()
        for cost, seed, step, stream, s in occurrences:
            if (seed, stream) in seen or len(seen) >= TRIES:
                continue
            seen.add((seed, stream))
            good = OracleBatch(bv, oracle, model_dir, s["B"], sample=[stream], models=models, hops_per_step=s["H"])
            bad = mutant(bv, oracle, model_dir, s["B"], sample=[stream], models=models, hops_per_step=s["H"])
            xs = sc.stream_input(bv, s, stream)
            try:
                for (k, y), (_, z) in zip(sc.stream_timeline(good, s, stream, xs), sc.stream_timeline(bad, s, stream, xs)):
                    hops += 2 * s["H"] if y is not None else 0
                    assert (y is None) == (z is None)
                    if y is not None and not np.array_equal(y, z):
                        print("\nmutant (%s) %s told apart: %s, stream %d, step %d (first %s at step %d), max-abs %g at rms %g; %d oracle hops"
                              % (letter, mutant.__name__, sc.scenario_id(s), stream, k, interaction, step, float(np.abs(y - z).max()),
                                 float(np.sqrt(np.mean(y * y))), hops))
                        return
                    if k >= step + HORIZON:
                        break
            finally:
                good.close()
                bad.close()
    finally:
        models.close()
    raise AssertionError("mutant %s gives the unmutated samples in %s" % (mutant.__name__, sorted(seen)))
