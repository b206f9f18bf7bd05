"""Seeded scenarios for the batch's per-stream state machine (test plumbing: generator, bookkeeping, runners; no pytest in here).

The -m gpu tests drive the batched library with hand-written scripts, each written to show one feature.  What decides, per stream and per
hop, WHICH table row, key/value slot, step counter and ring position the kernels read is host-side state (csrc/batch.hip advance_kv,
BeatriceBatch_ResetStream, SetVQNumNeighbors' stage that comes and goes, the ragged steps of batch_tick.hip.h), and its pieces interact.
A scenario is a generated script that PLANTS those interactions -- a second switch while blocks of the first are pending, a reset inside a
sit-out run, a switch whose installs straddle a drain ... -- at random streams (tile corners: oracle_batch.pick_streams) and steps, fills
the rest with independent random events, and walks the batch through several modes with its state carried over:

  make_scenario(seed, B, H, phases)  plain data (dicts / lists / ints, json-able), from np.random.default_rng(seed) only
  interactions(scn)                  the named interactions the scenario really contains, from a replay of the bookkeeping in plain Python
  run_oracle(env, scn, sample)       reference: one independent Stream1 per sampled stream on the CPU oracle (oracle_batch.OracleBatch),
                                     a step a stream sits out is H hops never made
  run_in_order(env, scn)             the product's in-order chain, one hop per step, nobody sits out: reference for the streams that
                                     never sit a step out (in order the flags of SetSilentStreams only exist for 48 kHz blocks)
  run_product(env, scn)              the product, ONE batch of H hops per step walked through the phases

Phase modes are the letters of include/beatrice_batch.h's mode table: A in order, B stage pipelining (host buffers), C resident I/O (fed in
chunks without waiting; with stage pipelining of depth 2 or 3 underneath in some), D tick mode (with the silent-block rule when the phase
has sit-outs), E host streaming.  Every phase is entered from A and left to A, along cells the table allows
(every mode-changing call is asserted to return 0; tests/test_cpu_scenarios.py holds `calls_of()` against csrc/batch_modes.h).  The wrapper
modes F / G / P and S at 48 kHz are NOT covered here: their reference is the wrapper oracle, another leg: tests/wrapper_walk.py walks one batch across
the transitions between those modes (tests/test_cpu_wrapper_walk.py, tests/test_gpu_wrapper_walk.py).  Morph slots and the codebook
lottery are out as well (OracleBatch has no model of them).  The calls that change a stream's state while the ticks keep running
(reset, install, export / import / move in flight) have a family of their own: tests/scenario_in_flight.py.

Replay one scenario of the list:  python tests/scenario.py --seed N [--B .. --H .. --phases D:40,A:6] [--dump scenario.json] [--gpu]
(without --gpu it prints the scenario and its interactions; with --gpu it runs the comparison of tests/test_gpu_scenarios.py for it)."""
import argparse
import ctypes as C
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle_batch import OracleBatch, pick_streams  # noqa: E402

MODE_NAMES = {"A": "in order", "B": "stage pipelining", "C": "resident I/O", "D": "tick", "E": "host streaming"}
DRAINED = "CD"           # phases fed in chunks with a drain (BeatriceBatch_Synchronize) between them
N_SPEAKERS = 3           # the model fixture of tests/conftest.py
SETTERS = ["SetFormantShift", "SetVQNumNeighbors", "SetMinSourcePitch", "SetMaxSourcePitch", "SetPitchShift", "SetAverageSourcePitch",
           "SetIntonationIntensity", "SetPitchCorrection", "SetPitchCorrectionType"]
VOCABULARY = ["SetTargetSpeaker", "SetTargetSpeakers", "FlushSpeaker", "ResetStream"] + SETTERS

INTERACTIONS = ["switch_while_pending", "reset_while_pending", "flush_while_pending", "switch_then_sitout_while_pending", "reset_while_absent",
                "reset_on_return", "setting_while_absent", "knn_change_while_absent", "sitout_after_install_step", "switch_straddles_step", "switch_straddles_drain",
                "knn_stage_appears", "knn_stage_vanishes", "knn_change_while_others_pending", "all_streams_setter_in_tick", "reset_all_in_tick",
                "stream_absent_from_first_step", "stream_absent_at_drain", "whole_batch_absent_step", "pending_across_mode_change",
                "absent_history_across_mode_change"]
# (interaction, H) cells that cannot exist, and why -- tests/test_cpu_scenarios.py prints them instead of passing silently
UNREACHABLE = {("sitout_after_install_step", 1): "defined for H > 1: only there the rows of a step's early hops hold key/value entries the later hops have replaced",
               ("switch_straddles_step", 1): "one install per step at one hop per step: the name is defined for H > 1",
               ("switch_straddles_step", 4): "a step of four hops installs all four blocks (a delayed install exists for morph slots only, which are out)"}

# the committed list: (seed, B, H, phases).  B: 1, a ragged single tile (5, 24), 37 = two 16-row tiles + a ragged third, 256; tick phases (D) at
# every H; 3040 is the long one (rings and resident slots wrap many times under sit-outs); bench.py's default shape class (tick mode, H = 4)
# is in 3004, 3013, 3014, 3022, 3023, 3040 ...
SEEDS = [
    (3001, 1, 1, [("D", 44), ("A", 6), ("E", 16)]),
    (3002, 1, 2, [("A", 6), ("D", 40), ("A", 4)]),
    (3003, 1, 4, [("D", 40), ("C", 8)]),
    (3004, 5, 4, [("D", 36), ("A", 4), ("D", 12)]),
    (3005, 5, 1, [("A", 8), ("D", 50), ("B", 8)]),
    (3006, 5, 2, [("D", 40), ("E", 12), ("A", 4)]),
    (3007, 24, 1, [("C", 14), ("D", 46), ("A", 6)]),
    (3008, 24, 2, [("D", 42), ("A", 4), ("D", 14)]),
    (3009, 24, 4, [("A", 4), ("D", 40)]),
    (3010, 37, 1, [("D", 60), ("A", 8)]),
    (3011, 37, 2, [("B", 8), ("D", 40), ("C", 10)]),
    (3012, 37, 4, [("D", 40), ("E", 8)]),
    (3013, 37, 4, [("E", 10), ("A", 3), ("D", 36)]),
    (3014, 256, 4, [("D", 40), ("A", 4)]),
    (3015, 256, 1, [("A", 6), ("D", 54)]),
    (3016, 37, 1, [("E", 24), ("A", 4), ("D", 40), ("C", 12)]),
    (3017, 24, 2, [("A", 10), ("B", 10), ("D", 30), ("E", 12)]),
    (3018, 5, 1, [("D", 30), ("C", 12), ("D", 30)]),
    (3019, 1, 1, [("A", 10), ("D", 50)]),
    (3020, 37, 2, [("D", 50), ("A", 6)]),
    (3021, 256, 2, [("C", 10), ("D", 36)]),
    (3022, 5, 4, [("A", 4), ("D", 40), ("E", 8)]),
    (3023, 24, 4, [("D", 44), ("B", 6)]),
    (3024, 1, 4, [("E", 10), ("D", 40)]),
    (3040, 37, 4, [("D", 300), ("A", 4), ("D", 30)]),
]


def scenarios():
    return [make_scenario(seed, B, H, phases) for seed, B, H, phases in SEEDS]


def scenario_id(scn):
    return "seed%d-B%d-H%d" % (scn["seed"], scn["B"], scn["H"])


# ------------------------------------------------------------------------------------------------------------------------------ generator
def _phase_table(phases):
    """per step: (phase index, mode letter); per phase: first step"""
    at, starts, k = [], [], 0
    for i, (mode, n) in enumerate(phases):
        starts.append(k)
        at += [(i, mode)] * n
        k += n
    return at, starts


def _setter_args(rng, name):
    if name == "SetFormantShift":
        return [float(rng.integers(-4, 5)) / 2.0]
    if name == "SetVQNumNeighbors":
        return [int(rng.integers(0, 9))]
    if name == "SetMinSourcePitch":
        return [float(rng.integers(33, 50))]
    if name == "SetMaxSourcePitch":
        return [float(rng.integers(62, 81))]
    if name == "SetPitchShift":
        return [float(rng.integers(-12, 13))]
    if name == "SetAverageSourcePitch":
        return [float(rng.integers(40, 70))]
    if name == "SetIntonationIntensity":
        return [float(rng.integers(0, 9)) / 4.0]
    if name == "SetPitchCorrection":
        return [float(rng.integers(0, 5)) / 4.0]
    if name == "SetPitchCorrectionType":
        return [int(rng.integers(0, 2))]
    raise AssertionError(name)


def make_scenario(seed, B, H, phases):
    rng = np.random.default_rng(seed)
    phases = [[str(m), int(n)] for m, n in phases]
    assert all(m in MODE_NAMES and n > 0 for m, n in phases) and H in (1, 2, 4) and B >= 1
    at, starts = _phase_table(phases)
    steps = len(at)
    chunks = []
    for mode, n in phases:
        sizes, left = [], n
        while mode in DRAINED and left > 0:
            sizes.append(min(left, int(rng.integers(3, 14))))
            left -= sizes[-1]
        chunks.append(sizes)
    drain_after = _drain_steps(phases, chunks)
    # who acts: the planted interactions (and every sit-out) happen on a few streams at the corners of the row tilings; all of them are in the
    # oracle sample (its size is what the oracle leg costs: hops = sample x steps x H)
    n_act = {1: 4, 2: 3, 4: 2}[H] if steps < 200 else 2
    pool = pick_streams(B, 8)      # first / last rows of the 16- and 32-row tiles, the ragged last tile (all streams of a small batch)
    actors = sorted(int(s) for s in rng.choice(pool, size=min(n_act, len(pool)), replace=False))
    rest = [s for s in pool if s not in actors]
    sample = sorted(set(actors) | set(range(B) if B <= 5 else rest[:1]))
    events = [[] for _ in range(steps)]
    absent = [set() for _ in range(steps)]
    planted = []
    speaker = [s % N_SPEAKERS for s in range(B)]     # what the generator believes each stream's target is (only to pick a DIFFERENT one)

    def other_speaker(s):
        speaker[s] = int((speaker[s] + 1 + rng.integers(0, N_SPEAKERS - 1)) % N_SPEAKERS)
        return speaker[s]

    def ev(k, name, stream, *args):
        if 0 <= k < steps:
            events[k].append([name, int(stream), list(args)])

    def sit(s, k0, n):
        """stream s sits steps k0 .. k0 + n - 1 out, as far as they lie in the tick phase of k0"""
        for k in range(k0, min(k0 + n, steps)):
            if at[k] == at[k0] and at[k][1] == "D":
                absent[k].add(s)

    knn_initial = bool(rng.random() < 0.25)
    initial = [["SetTargetSpeakers", -2, [list(range(B)), [s % N_SPEAKERS for s in range(B)]]]]
    if knn_initial:
        initial += [["SetVQNumNeighbors", s, [s % 3]] for s in range(B)]
    initial.append(["FlushSpeaker", -1, []])

    # ---- planted at the scenario's own landmarks: phase starts and ends, drains
    for i, (mode, n) in enumerate(phases):
        first, last = starts[i], starts[i] + n - 1
        s = int(rng.choice(actors))
        if i + 1 < len(phases):      # a switch whose installs are still pending when the mode changes
            if mode == "D" and (H == 4 or rng.random() < 0.5):
                ev(last, "SetTargetSpeaker", s, other_speaker(s))
                sit(s, last - int(rng.integers(0, 3)), 3)
            elif H < 4:
                ev(last - (int(rng.integers(0, 3)) if H == 1 else 0), "SetTargetSpeaker", s, other_speaker(s))
            planted.append(["pending_at_mode_change", s, last])
        if mode == "D":
            if rng.random() < 0.6:
                s = int(rng.choice(actors))
                sit(s, first, int(rng.integers(1, 4)))
                planted.append(["absent_from_first_step", s, first])
            ends = [k for k in drain_after if first <= k < last]
            for k in [int(x) for x in rng.choice(ends, size=min(2, len(ends)), replace=False)] if ends else []:
                s = int(rng.choice(actors))
                if rng.random() < 0.5:     # a switch whose installs straddle the drain (at H = 4: made in a step the stream sits out)
                    ev(k - (int(rng.integers(0, 3)) if H == 1 else 0), "SetTargetSpeaker", s, other_speaker(s))
                    if H == 4:
                        sit(s, k, 1)
                    planted.append(["switch_over_drain", s, k])
                else:
                    sit(s, k - int(rng.integers(0, 2)), int(rng.integers(2, 4)))
                    planted.append(["absent_at_drain", s, k])
            if set(sample) == set(range(B)) and n > 12:   # a step nobody takes part in (every stream of such a batch is in the oracle sample)
                k = int(rng.integers(first + 2, last - 2))
                for s in range(B):
                    absent[k].add(s)
                planted.append(["whole_batch_absent", -1, k])

    # ---- planted in windows of eight steps per actor: every recipe once before any comes twice
    def double(k, s, second, tick):
        """a switch, then `second` while blocks of the switch are pending"""
        ev(k, "SetTargetSpeaker", s, other_speaker(s))
        if tick and (H == 4 or rng.random() < 0.4):      # pending because the stream sits out in between
            d = int(rng.integers(1, 4))
            sit(s, k if H == 4 else k + 1, d)
            k2 = k + d + (0 if H == 4 else 1) - int(rng.integers(0, 2))      # inside the run, or on return
        else:
            k2 = k + (int(rng.integers(1, 4)) if H == 1 else (1 if H == 2 else 0))
        k2 = min(max(k2, k), steps - 1)
        if second == "SetTargetSpeaker":
            ev(k2, second, s, other_speaker(s))
        else:
            ev(k2, second, s)

    def r_switch_switch(k, s, tick):
        double(k, s, "SetTargetSpeaker", tick)

    def r_switch_reset(k, s, tick):
        double(k, s, "ResetStream", tick)

    def r_switch_flush(k, s, tick):
        double(k, s, "FlushSpeaker", tick)

    def r_switch_sitout(k, s, tick):
        """the stream sits out with installs pending: from the step after the switch, or at H = 4 (where a step it takes part in installs all
        four) from the switch's own step on"""
        ev(k, "SetTargetSpeaker", s, other_speaker(s))
        sit(s, k if H == 4 else k + 1, int(rng.integers(1, 7)))

    def r_reset_in_sitout(k, s, tick):
        n = int(rng.integers(2, 6))
        sit(s, k, n)
        ev(k + int(rng.integers(0, n)), "ResetStream", s)

    def r_reset_on_return(k, s, tick):
        n = int(rng.integers(1, 5))
        sit(s, k, n)
        ev(k + n, "ResetStream", s)

    def r_setting_in_sitout(k, s, tick):
        n = int(rng.integers(2, 6))
        sit(s, k, n)
        ev(k + int(rng.integers(0, n)), "SetVQNumNeighbors", s, int(rng.integers(2, 6)))
        name = ["SetFormantShift", "SetPitchShift"][int(rng.integers(0, 2))]
        ev(k + int(rng.integers(0, n)), name, s, [1.5, -7.0][name == "SetPitchShift"] * (1 if rng.random() < 0.5 else -1))

    def r_knn_pulse(k, s, tick):
        """k-NN 0 -> k -> 0 for the only stream that uses it (the stage appears and vanishes) while another stream's installs are pending"""
        o = int((s + 1 + rng.integers(0, max(B - 1, 1))) % B)
        ev(k, "SetVQNumNeighbors", -1, 0)
        if o != s:
            ev(k + 1, "SetTargetSpeaker", o, other_speaker(o))
        ev(k + 1, "SetVQNumNeighbors", s, int(rng.integers(1, 9)))
        d = int(rng.integers(2, 5))
        if o != s:
            ev(k + d, "SetTargetSpeakers", -2, [o], [other_speaker(o)])
        ev(k + d, "SetVQNumNeighbors", s, 0)

    def r_all_streams(k, s, tick):
        name = SETTERS[int(rng.integers(0, len(SETTERS)))]
        if name == "SetVQNumNeighbors":
            name = "SetPitchShift"
        ev(k, name, -1, *_setter_args(rng, name))
        if rng.random() < 0.5:
            ev(k + int(rng.integers(1, 5)), "ResetStream", -1)
        else:
            ev(k + int(rng.integers(1, 5)), "SetTargetSpeaker", -1, int(rng.integers(0, N_SPEAKERS)))

    anywhere = [r_switch_switch, r_switch_reset, r_switch_flush, r_knn_pulse, r_all_streams]
    tick_only = [r_switch_sitout, r_reset_in_sitout, r_reset_on_return, r_setting_in_sitout]
    windows = [(k, s) for s in actors for k in range(1, steps - 8, 8) if at[k] == at[k + 7]]
    order = [int(i) for i in rng.permutation(len(windows))]
    queue = {True: [], False: []}
    for i in order:
        k, s = windows[i]
        tick = at[k][1] == "D"
        if steps >= 200 and rng.random() < 0.5:      # the long scenario is mostly plain running under sit-outs
            if tick:
                sit(s, k + int(rng.integers(0, 4)), int(rng.integers(1, 5)))
            continue
        if not queue[tick]:
            recipes = anywhere + (tick_only + tick_only if tick else [])
            queue[tick] = [recipes[int(j)] for j in rng.permutation(len(recipes))]
        recipe = queue[tick].pop()
        recipe(k + int(rng.integers(0, 3)), s, tick)
        planted.append([recipe.__name__[2:], s, k])

    # ---- the rest: independent random events on any stream
    for k in range(steps):
        if rng.random() < 0.2:
            name = VOCABULARY[int(rng.integers(0, len(VOCABULARY)))]
            s = -1 if rng.random() < 0.08 else int(rng.integers(0, B))
            if name == "SetVQNumNeighbors" and rng.random() < 0.7:
                name = "SetPitchShift"          # (a k-NN user somewhere keeps the stage from ever vanishing: keep those rare)
            if name == "ResetStream" and s < 0 and rng.random() < 0.5:
                s = int(rng.integers(0, B))
            if name == "SetTargetSpeaker":
                ev(k, name, s, int(rng.integers(0, N_SPEAKERS)))
            elif name == "SetTargetSpeakers":
                n = int(rng.integers(1, min(B, 6) + 1))
                ss = sorted(int(x) for x in rng.choice(B, size=n, replace=False))
                ev(k, name, -2, ss, [int(x) for x in rng.integers(0, N_SPEAKERS, size=n)])
            elif name in ("FlushSpeaker", "ResetStream"):
                ev(k, name, s)
            else:
                ev(k, name, s, *_setter_args(rng, name))

    # resident I/O phases run with stage pipelining underneath (depth 2 or 3: stage s of step t + 1 overlaps stage s + 1 of step t) or without
    depths = [int(rng.choice([0, 2, 3])) if mode == "C" else 0 for mode, _ in phases]
    return {"seed": int(seed), "B": int(B), "H": int(H), "phases": phases, "chunks": chunks, "depths": depths, "actors": actors, "sample": sample,
            "initial": initial, "events": events, "absent": [sorted(a) for a in absent], "planted": planted}


def _drain_steps(phases, chunks):
    """the steps after which the pipeline is drained inside a phase (ends of the chunks of the C and D phases)"""
    out, k = set(), 0
    for (mode, n), sizes in zip(phases, chunks):
        j = k
        for c in sizes:
            j += c
            out.add(j - 1)
        k += n
    return out


# ---------------------------------------------------------------------------------------------------------------------------- bookkeeping
def expand(event, B):
    """an event as the (name, stream, args) calls of single streams it stands for"""
    name, stream, args = event
    if name == "SetTargetSpeakers":
        return [("SetTargetSpeaker", s, [sp]) for s, sp in zip(args[0], args[1])]
    return [(name, s, args) for s in (range(B) if stream < 0 else [stream])]


def replay(scn):
    """Replays the bookkeeping of the scenario in plain Python: yields per step k a dict with the mode, the calls of single streams with the
    stream's pending-install count at the call, who sits the step out and every stream's pending installs after the step's hops;
    collects the interactions on the way (the generator's return value)."""
    B, H = scn["B"], scn["H"]
    at, starts = _phase_table(scn["phases"])
    drains = _drain_steps(scn["phases"], scn["chunks"])
    pend, knn = [0] * B, [0] * B
    found = {name: [] for name in INTERACTIONS}
    missed = [0] * B          # steps sat out in the current phase
    for ev in scn["initial"]:
        for name, s, args in expand(ev, B):
            if name == "SetTargetSpeaker":
                pend[s] = 4
            elif name in ("FlushSpeaker", "ResetStream"):
                pend[s] = 0
            elif name == "SetVQNumNeighbors":
                knn[s] = args[0]
    prev_absent, installed = set(), set()
    for k in range(len(at)):
        phase, mode = at[k]
        ab = set(scn["absent"][k])
        assert not ab or mode == "D", "a stream can sit a step out in tick mode only"

        def hit(name, s, cell=mode):
            found[name].append({"step": k, "stream": s, "mode": cell, "H": H})
        if k == starts[phase] and k > 0:
            cell = "D" if "D" in (at[k - 1][1], mode) else mode
            for s in range(B):
                if pend[s] > 0:
                    hit("pending_across_mode_change", s, cell)
                if missed[s] > 0:
                    hit("absent_history_across_mode_change", s, cell)
            missed = [0] * B
        users = sum(1 for v in knn if v > 0)
        calls = []
        for ev in scn["events"][k]:
            if ev[1] == -1 and mode == "D":
                hit("reset_all_in_tick" if ev[0] == "ResetStream" else "all_streams_setter_in_tick", -1)
            for name, s, args in expand(ev, B):
                calls.append((name, s, args, pend[s]))
                if name == "SetTargetSpeaker":
                    if pend[s] > 0:
                        hit("switch_while_pending", s)
                    pend[s] = 4
                elif name == "ResetStream":
                    if pend[s] > 0:
                        hit("reset_while_pending", s)
                    if s in ab:
                        hit("reset_while_absent", s)
                    elif s in prev_absent:
                        hit("reset_on_return", s)
                    pend[s] = 0
                elif name == "FlushSpeaker":
                    if pend[s] > 0:
                        hit("flush_while_pending", s)
                    pend[s] = 0
                else:
                    if s in ab:
                        hit("setting_while_absent", s)
                    if name == "SetVQNumNeighbors":
                        if s in ab and args[0] != knn[s]:
                            hit("knn_change_while_absent", s)
                        if args[0] != knn[s] and any(pend[o] > 0 for o in range(B) if o != s):
                            hit("knn_change_while_others_pending", s)
                        knn[s] = args[0]
        users_now = sum(1 for v in knn if v > 0)
        if users == 0 and users_now > 0:
            hit("knn_stage_appears", -1)
        if users > 0 and users_now == 0:
            hit("knn_stage_vanishes", -1)
        for s in sorted(ab):
            missed[s] += 1
            if H > 1 and s in installed:
                hit("sitout_after_install_step", s)
            if pend[s] > 0:
                hit("switch_then_sitout_while_pending", s)
            if k == starts[phase]:
                hit("stream_absent_from_first_step", s)
            if k in drains:
                hit("stream_absent_at_drain", s)
        if len(ab) == B:
            hit("whole_batch_absent_step", -1)
        installed = set()         # streams whose installs moved in this step
        for s in range(B):
            if s not in ab and pend[s] > 0:
                before, pend[s] = pend[s], max(0, pend[s] - H)
                installed.add(s)
                if H > 1 and pend[s] > 0 and before > pend[s]:
                    hit("switch_straddles_step", s)
        if k in drains:
            for s in range(B):
                if pend[s] > 0:
                    hit("switch_straddles_drain", s)
        prev_absent = ab
        yield {"step": k, "mode": mode, "calls": calls, "absent": ab, "pending": list(pend)}
    return found


def interactions_detail(scn):
    """{name: [{step, stream (-1: the whole batch), mode, H}, ...]} -- every occurrence"""
    gen = replay(scn)
    while True:
        try:
            next(gen)
        except StopIteration as stop:
            return stop.value


def interactions(scn):
    """the set of named interactions the scenario actually contains"""
    return {name for name, hits in interactions_detail(scn).items() if hits}


def never_absent(scn):
    out = set(s for ab in scn["absent"] for s in ab)
    return [s for s in range(scn["B"]) if s not in out]


def stream_story(scn, stream, upto):
    """One stream's own events up to step `upto` with its pending-install count and present / absent history, and the interactions
    that touch it: what a failing comparison prints."""
    lines = ["seed %d, B = %d, H = %d, phases %s: stream %d up to step %d" % (scn["seed"], scn["B"], scn["H"], scn["phases"], stream, upto)]
    lines.append("  before step 0: %s" % [e for e in scn["initial"] if any(s == stream for _, s, _ in expand(e, scn["B"]))])
    history = ""
    for st in replay(scn):
        k = st["step"]
        if k > upto:
            break
        history += "-" if stream in st["absent"] else st["mode"]
        mine = ["%s%s (pending %d)" % (name, tuple(args), p) for name, s, args, p in st["calls"] if s == stream]
        if mine or stream in st["absent"]:
            lines.append("  step %3d [%s]%s %s -> pending %d" % (k, st["mode"], " ABSENT" if stream in st["absent"] else "", "; ".join(mine), st["pending"][stream]))
    lines.append("  mode per step (-: sat out): %s" % history)
    lines.append("  drains after steps %s" % sorted(d for d in _drain_steps(scn["phases"], scn["chunks"]) if d <= upto))
    for name, hits in interactions_detail(scn).items():
        mine = [h["step"] for h in hits if h["stream"] in (stream, -1) and h["step"] <= upto]
        if mine:
            lines.append("  %s at steps %s" % (name, mine))
    return "\n".join(lines)


# ------------------------------------------------------------------------------------------------------------------------- mode transitions
def calls_of(scn):
    """The entry points of the mode table the product runner calls, in call order, as (entry as csrc/batch_modes.h names it, the flags of
    bhip::modes::Flags the batch has at the call, the mode letter the flags must derive to or None) -- tests/test_cpu_scenarios.py asks
    allowed() and mode_of() for each."""
    H = scn["H"]
    at, starts = _phase_table(scn["phases"])
    out = []
    for i, (mode, n) in enumerate(scn["phases"]):
        rule = any(scn["absent"][k] for k in range(starts[i], starts[i] + n))
        f = {"H": H}

        def call(entry, letter=None):
            out.append((entry, dict(f), letter))
        if mode == "A":
            call("ConvertFrames", "A")
        elif mode == "B":
            call("EnablePipelining(2)")
            f["pipelined"] = True
            call("ConvertFrames", "B")
        elif mode in "CD":
            call("BindResidentIO(bind)")
            f["io"] = True
            if mode == "D":
                call("EnableTickPipeline(1)")
                f["tk"] = True
                if rule:
                    call("EnableSilentBlockRule(1)")
                    f["silent"] = True
                    call("SetSilentStreams", "D")
            if scn["depths"][i]:
                call("EnablePipelining(2)")      # (the table's row for any depth >= 1)
                f["pipelined"] = True
            call("ConvertFramesDevice(NULL)", mode)
            f.pop("pipelined", None)
            if mode == "D":
                call("EnableTickPipeline(0)")
                del f["tk"]
            call("BindResidentIO(unbind)")
            del f["io"]
            if rule:
                call("EnableSilentBlockRule(0)")
        elif mode == "E":
            call("EnableHostStreaming(1)")
            f.update(tk=True, hs=True, io=True)
            call("StreamFrames", "E")
    return out


# -------------------------------------------------------------------------------------------------------------------------------- runners
class Env:
    """what the runners need from the fixtures of tests/conftest.py"""

    def __init__(self, bv, oracle, product, model_dir):
        self.bv, self.oracle, self.model_dir = bv, oracle, model_dir
        self.product = bv.bind_batch(product) if product is not None else None


def stream_input(bv, scn, s):
    """[steps][H * 160]: stream s's own signal"""
    steps = sum(n for _, n in scn["phases"])
    return bv.synth_audio(160 * scn["H"] * steps, seed=6000 + 37 * (scn["seed"] % 1000) + s).reshape(steps, scn["H"] * 160)


def inputs(bv, scn):
    return np.stack([stream_input(bv, scn, s) for s in range(scn["B"])])


def apply_event(target, event):
    """one event on anything that looks like bv.Batch (`.a`, `.h`); every call must return 0"""
    name, stream, args = event
    if name == "SetTargetSpeakers":
        n = len(args[0])
        rc = target.a.BeatriceBatch_SetTargetSpeakers(target.h, n, (C.c_int * n)(*args[0]), (C.c_int * n)(*args[1]))
    else:
        rc = getattr(target.a, "BeatriceBatch_" + name)(target.h, stream, *args)
    assert rc == 0, "%s returned %d" % (event, rc)


def stream_timeline(ob, scn, s, xs):
    """Sampled stream s of an OracleBatch through the whole scenario: the events that address it, each as a call on s alone, before the step
    they precede; a step the stream sits out is H hops never made.  Yields (step, samples [H * 240] or None when it sat the step out)."""
    B = scn["B"]

    def mine(event):
        return [[name, s, args] for name, t, args in expand(event, B) if t == s]
    for event in scn["initial"]:
        for e in mine(event):
            apply_event(ob, e)
    for k in range(len(scn["events"])):
        away = s in scn["absent"][k]
        ob.begin_step(s, away)
        for event in scn["events"][k]:
            for e in mine(event):
                apply_event(ob, e)
        if away:
            ob.sit_out(s)
            yield k, None
        else:
            yield k, ob.step_stream(s, xs[k])


def run_oracle(env, scn, sample):
    """{stream: [steps][H * 240]} for the sampled streams (rows of the steps a stream sits out stay zero): one oracle stream each.  The
    streams are independent, so each runs its whole timeline on a thread of its own (the oracle's C calls release the interpreter)."""
    H = scn["H"]
    sample = sorted(sample)
    ob = OracleBatch(env.bv, env.oracle, env.model_dir, scn["B"], sample=sample, hops_per_step=H)

    def timeline(s):
        out = np.zeros((len(scn["events"]), H * 240), np.float32)
        for k, y in stream_timeline(ob, scn, s, stream_input(env.bv, scn, s)):
            if y is not None:
                out[k] = y
        return out

    try:
        with ThreadPoolExecutor(max_workers=min(8, max(1, len(sample)))) as pool:
            return dict(zip(sample, pool.map(timeline, sample)))
    finally:
        ob.close()


def run_in_order(env, scn):
    """([steps][B][H * 240], raw pitch bins [B] of the last hop, the set of raw bins seen at the end of every step) from the product's
    in-order chain at ONE hop per step; nobody sits out."""
    bv, B, H = env.bv, scn["B"], scn["H"]
    steps = sum(n for _, n in scn["phases"])
    x = inputs(bv, scn)
    m = bv.Models(env.product, env.model_dir)
    batch = bv.Batch(m, B)
    try:
        for event in scn["initial"]:
            apply_event(batch, event)
        out = np.zeros((steps, B, H * 240), np.float32)
        bins = set()
        for k in range(steps):
            for event in scn["events"][k]:
                apply_event(batch, event)
            for hh in range(H):
                out[k, :, hh * 240:(hh + 1) * 240] = batch.convert(np.ascontiguousarray(x[:, k, hh * 160:(hh + 1) * 160]))
            q = batch.intermediates()[1].copy()
            bins.update(int(v) for v in q)
    finally:
        batch.close()
        m.close()
    return out, q, bins


def run_product(env, scn, start_counter=None):
    """([steps][B][H * 240], raw pitch bins [B] of the last hop) from ONE batch of H hops per step walked through the scenario's phases,
    state carried from phase to phase.  Every mode-changing call is asserted to return 0.  start_counter: the new batch's step counter
    (BeatriceBatch_SetStepCounter; the counter wraps at bv.STEP_WRAP) -- a fresh batch computes the same samples wherever it starts, so
    the in-order reference and the oracle know nothing of it; the run must then end at (start_counter + steps) mod the wrap."""
    from tick_driver import Resident
    bv, B, H = env.bv, scn["B"], scn["H"]
    at, starts = _phase_table(scn["phases"])
    x = inputs(bv, scn)
    m = bv.Models(env.product, env.model_dir)
    batch = bv.Batch(m, B, hops_per_step=H, start_counter=start_counter)
    a, h = batch.a, batch.h
    out = np.zeros((len(at), B, H * 240), np.float32)

    def before(k, rule):
        for event in scn["events"][k]:
            apply_event(batch, event)
        if scn["absent"][k]:
            assert rule
            assert a.BeatriceBatch_SetSilentStreams(h, bytes(1 if s in scn["absent"][k] else 0 for s in range(B))) == 0

    try:
        for event in scn["initial"]:
            apply_event(batch, event)
        for i, (mode, n) in enumerate(scn["phases"]):
            k0 = starts[i]
            rule = any(scn["absent"][k] for k in range(k0, k0 + n))
            if mode in "AB":
                if mode == "B":
                    assert a.BeatriceBatch_EnablePipelining(h, 2) == 0
                for k in range(k0, k0 + n):
                    before(k, False)
                    out[k] = batch.convert(np.ascontiguousarray(x[:, k]))
                if mode == "B":
                    assert a.BeatriceBatch_EnablePipelining(h, 0) == 0
            elif mode in "CD":
                r = Resident(bv, batch, tick=mode == "D")
                try:
                    if rule:      # (tick mode is on by now: the rule is enabled inside it)
                        assert a.BeatriceBatch_EnableSilentBlockRule(h, 1) == 0
                    if scn["depths"][i]:
                        assert a.BeatriceBatch_EnablePipelining(h, scn["depths"][i]) == 0
                    k = k0
                    for c in scn["chunks"][i]:
                        out[k:k + c] = r.feed([x[:, j] for j in range(k, k + c)], lambda j, k=k: before(k + j, rule))
                        k += c
                    assert k == k0 + n
                    if scn["depths"][i]:
                        assert a.BeatriceBatch_EnablePipelining(h, 0) == 0
                    r.leave()
                    if rule:
                        assert a.BeatriceBatch_EnableSilentBlockRule(h, 0) == 0
                finally:
                    r.free()
            elif mode == "E":
                assert a.BeatriceBatch_EnableHostStreaming(h, 1) == 0
                y = np.zeros((B, H * 240), np.float32)
                done = k0
                for k in range(k0, k0 + n):
                    before(k, False)
                    rc = a.BeatriceBatch_StreamFrames(h, bv.fptr(np.ascontiguousarray(x[:, k])), bv.fptr(y))
                    assert rc in (0, 1)
                    if rc == 1:
                        out[done] = y
                        done += 1
                while a.BeatriceBatch_StreamFlush(h, bv.fptr(y)) == 1:
                    assert done < k0 + n
                    out[done] = y
                    done += 1
                assert done == k0 + n
                assert a.BeatriceBatch_EnableHostStreaming(h, 0) == 0
        q = batch.intermediates()[1].reshape(B, H)[:, H - 1].copy()
        if start_counter is not None:
            end = batch.step_counter()
            print("%s: step counter %d before, %d after %d steps" % (scenario_id(scn), start_counter, end, len(at)))
            assert end == (start_counter + len(at)) % bv.STEP_WRAP
    finally:
        batch.close()
        m.close()
    return out, q


def compare(env, scn, say=print, start_counter=None, references=None):
    """The comparison of tests/test_gpu_scenarios.py for one scenario; returns the list of failures (strings, empty = fine).
    start_counter: see run_product (the product through the phases only).  references: a dict in which the scenario's in-order and oracle
    legs are kept for a second comparison of the same scenario."""
    got, q = run_product(env, scn, start_counter)
    key = scenario_id(scn)
    if references is None or key not in references:
        legs = run_in_order(env, scn) + (run_oracle(env, scn, scn["sample"]),)
        if references is not None:
            references[key] = legs
    else:
        legs = references[key]
    ref, ref_q, bins, want = legs
    steps, B = got.shape[0], scn["B"]
    present = [[s not in scn["absent"][k] for s in range(B)] for k in range(steps)]
    stay = never_absent(scn)
    problems = []

    def first_bad(reference, streams, what):
        for k in range(steps):
            for s in streams:
                if present[k][s] and not np.array_equal(got[k, s], reference(k, s)):
                    d = float(np.abs(got[k, s] - reference(k, s)).max())
                    problems.append("%s: first differing (step, stream, max-abs) = (%d, %d, %g)\n%s" % (what, k, s, d, stream_story(scn, s, k)))
                    return
    first_bad(lambda k, s: ref[k, s], stay, "product through the phases vs its in-order chain")
    first_bad(lambda k, s: want[s][k], sorted(want), "product through the phases vs the oracle")
    if not np.array_equal(q[stay], ref_q[stay]):
        problems.append("raw pitch bins at the end differ from the in-order chain's: streams %s" % [s for s in stay if q[s] != ref_q[s]][:12])
    loud = max(float(np.abs(w).max()) for w in want.values())
    if not loud > 0.05:
        problems.append("the oracle leg is silence (max-abs %g)" % loud)
    if len(bins) < 2:
        problems.append("fewer than two distinct raw pitch bins over the whole run: %s" % sorted(bins))
    if not problems:
        say("%s: bit-identical to in-order (%d streams) and to the oracle (%d sampled: %s); interactions: %s"
            % (scenario_id(scn), len(stay), len(want), sorted(want), ", ".join(sorted(interactions(scn)))))
    return problems


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--seed", type=int, required=True)
    ap.add_argument("--B", type=int)
    ap.add_argument("--H", type=int)
    ap.add_argument("--phases", help="e.g. D:40,A:6 (default: as in the committed list for that seed)")
    ap.add_argument("--dump", help="write the scenario as json")
    ap.add_argument("--gpu", action="store_true", help="run the product against its in-order chain and the oracle")
    ap.add_argument("--start-counter", type=int, help="with --gpu: the step counter the product's batch starts at (it wraps at 12 252 240; the in-order "
                    "chain and the oracle ignore it), e.g. 12252240 minus half the scenario's steps")
    args = ap.parse_args(argv)
    listed = {s[0]: s for s in SEEDS}.get(args.seed)
    B = args.B or (listed[1] if listed else 5)
    H = args.H or (listed[2] if listed else 1)
    phases = [(p.split(":")[0], int(p.split(":")[1])) for p in args.phases.split(",")] if args.phases else (listed[3] if listed else [("D", 40), ("A", 6)])
    scn = make_scenario(args.seed, B, H, phases)
    if args.dump:
        with open(args.dump, "w") as f:
            json.dump(scn, f)
    print("%s, phases %s, chunks %s, stage pipelining under the resident I/O phases %s" % (scenario_id(scn), scn["phases"], scn["chunks"], scn["depths"]))
    print("actors %s, oracle sample %s, planted %s" % (scn["actors"], scn["sample"], scn["planted"]))
    for k, (evs, ab) in enumerate(zip(scn["events"], scn["absent"])):
        if evs or ab:
            print("  step %3d: %s%s" % (k, evs, "  sit out: %s" % ab if ab else ""))
    for name, hits in interactions_detail(scn).items():
        if hits:
            print("%-36s %s" % (name, [(h["step"], h["stream"]) for h in hits][:10]))
    if args.gpu:
        import importlib.util
        import tempfile
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        sys.path.insert(0, os.path.join(root, "tools"))
        import make_model
        spec = importlib.util.spec_from_file_location("beatrice_vst_amd", os.path.join(root, "beatrice-vst_amd", "__init__.py"))
        bv = importlib.util.module_from_spec(spec)
        sys.modules["beatrice_vst_amd"] = bv
        spec.loader.exec_module(bv)
        with tempfile.TemporaryDirectory() as d:
            make_model.make_model(d, n_speakers=N_SPEAKERS)
            env = Env(bv, bv.Abi(os.path.join(root, "oracle", "libbeatrice_oracle.so")), bv.load_product(), d)
            problems = compare(env, scn, start_counter=args.start_counter)
        for p in problems:
            print(p)
        return 1 if problems else 0
    return 0


if __name__ == "__main__":
    sys.exit(main())
