"""Seeded scenarios of the IN-FLIGHT calls against the oracle (test plumbing: generator, model, runners; no pytest in here).

tests/scenario.py walks ONE batch through the drained state machine.  This family is its sibling for the calls that change a stream's
state while the tick pipeline keeps running -- BeatriceBatch_ResetStreamInFlight, InstallSpeakersInFlight, SpeakerEntryBusy,
StreamQuiescent, ExportStreamsInFlight, ImportStreamsInFlight, MoveStreamsInFlight --, which the hand-written tests
(test_gpu_reset_in_flight.py, test_gpu_install_in_flight.py, test_gpu_stream_move_in_flight.py) show one at a time.

A scenario has TWO product batches X and Y (Bx, By streams, the same H; 16 table entries each on the 8-speaker synthetic model: X holds
real voice e at entry e, Y holds voice (e + 3) % 8 there, entries 8..15 are free at the start and take the derived voices of
test_gpu_install_in_flight.Voices in flight) that walk the same phase list in lockstep, step k of X, then step k of Y.  Chunk sizes (and so
the drains) and start_counter are per batch: the two step counters and tick counts are never equal.  What is compared is a LOGICAL stream:
it has its own audio and one independent oracle stream, and its j-th present step is the oracle's step j, whichever batch and slot made
it, and whenever.  A slot holds one logical stream at a time; a move carries the logical stream to the destination slot, the source slot
then sits out until it is turned over for a new logical stream (ResetStreamInFlight plus settings) or fed again as it is (the oracle
stream is then forked: re-run from the start).

  make_scenario(seed, Bx, By, H, phases)   plain data (json-able), from np.random.default_rng(seed) and the model only
  World                                    the model, plain Python: per batch and step every slot's logical stream, presence, pending-install
                                           count, reset flag, target / key-value entries, ticks launched, drains; it PREDICTS StreamQuiescent
                                           for every slot and SpeakerEntryBusy for every entry before every step, and the return code (0 / -3)
                                           of every in-flight call; it writes every logical stream's timeline (the oracle's script)
  replay(scn)                              the model run over a scenario: predictions, timelines, the named interactions it really contains
  run_legs / run_in_order / run_product    the oracle legs, the product's in-order chain (reference of the streams no call ever touches),
                                           the two product batches
  compare(env, scn)                        the comparison of tests/test_gpu_scenarios_in_flight.py: a list of problems, empty = fine

Phases are D (tick mode with the silent-block rule; moves are planned only in steps where both batches are in D), E (host streaming: reset
and install) and A (in order: the same calls as their documented fall-backs -- ResetStreamInFlight is ResetStream, InstallSpeakersInFlight
drains).  OUT OF SCOPE: morph calls and the codebook lottery (the oracle has no model of them and the header promises float rounding,
not bits), and the modes F / G / P / S, whose reference is the wrapper oracle, the leg of tests/wrapper_walk.py.

ONE CHOREOGRAPHY.  Unlike tests/scenario.py, whose generator draws recipes at random, every scenario here runs the same play (make_scenario:
play, by_count, phase_end, other_phases), because most of the interactions are chains of several calls on two batches that only exist in
one order.  The seed varies the chunk sizes (and so where the drains fall and how a stream comes to rest), the slots, the voices, the
lengths of the sit-outs, blobs or device to device, and whether a source is fed again; the model, not the play, names what a scenario
contains.  Two calls the play never puts next to each other are never generated: another seed does not find a new ordering.

Replay one scenario:  python tests/scenario_in_flight.py --seed N [--gpu] [--dump scenario.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle_batch import OracleBatch, pick_streams  # noqa: E402

STAGES = 28          # BeatriceBatch_TickStages(): a constant of the tick plan (csrc/tick.hip.h Plan::count); the runner asserts it
ENTRIES, REAL = 16, 8
Y_HOLDS = [(e + 3) % REAL for e in range(REAL)]     # the real voice at Y's entry e
NEVER = None

INTERACTIONS = [
    "reset_in_flight_while_pending", "reset_in_flight_while_absent", "switch_after_reset_in_flight_while_absent",
    "setting_after_reset_in_flight_while_absent", "reset_in_flight_twice_before_taken", "reset_in_flight_then_drained_reset",
    "reset_in_flight_travelling_at_drain", "reset_in_flight_pending_at_mode_change", "reset_in_flight_all_streams",
    "install_then_switch_same_gap", "install_refused_then_accepted", "entry_freed_by_drain", "entry_freed_by_absent_stream_switching_away",
    "entry_freed_by_import_over_slot", "install_reuses_entry_with_other_voice", "five_installs_between_two_ticks",
    "move_with_installs_pending", "move_onto_entry_installed_in_flight", "move_after_reset_taken", "move_refused_reset_pending",
    "import_cancels_pending_reset", "move_at_rest_by_drain", "move_round_trip", "move_by_blobs", "move_device_to_device",
    "move_of_tile_corner_stream", "moves_of_several_streams_one_call", "source_slot_turned_over", "source_fed_again_after_move",
    "move_as_drained_fallback",
    # the planted refusals that are no interaction of the issue's list by name
    "move_refused_one_tick_short", "install_refused_entry_named_inside_pipeline"]
# (interaction, H) cells of the D steps that cannot exist, and why
UNREACHABLE = {("move_as_drained_fallback", H): "defined for A steps: in order a move is the drained pair BeatriceBatch_ExportStreams / ImportStreams; "
               "in a D step the same event is the in-flight call" for H in (1, 2, 4)}

# the committed list: (seed, Bx, By, H, phases)
SEEDS = [
    (5001, 1, 1, 1, [("D", 50)]),
    (5002, 5, 3, 1, [("D", 36), ("A", 4), ("D", 16)]),
    (5003, 5, 3, 2, [("D", 50)]),
    (5004, 5, 3, 4, [("A", 4), ("D", 40)]),
    (5005, 24, 5, 1, [("D", 30), ("E", 14)]),
    (5006, 24, 5, 2, [("E", 12), ("D", 40)]),
    (5007, 24, 5, 4, [("D", 50)]),
    (5008, 37, 24, 1, [("D", 50)]),
    (5009, 37, 24, 2, [("D", 36), ("A", 4), ("D", 16)]),
    (5010, 37, 24, 4, [("D", 30), ("E", 14)]),
    (5011, 37, 37, 1, [("A", 4), ("D", 40)]),
    (5012, 37, 37, 2, [("D", 50)]),
    (5013, 37, 37, 4, [("E", 12), ("D", 40)]),
    (5014, 256, 37, 4, [("D", 44)]),
]
ACROSS_THE_WRAP = (5002, 5006, 5007, 5012)


def scenarios():
    return [make_scenario(*s) for s in SEEDS]


def scenario_id(scn):
    return "seed%d-X%d-Y%d-H%d" % (scn["seed"], scn["B"]["X"], scn["B"]["Y"], scn["H"])


def _phase_table(phases):
    at, starts, k = [], [], 0
    for i, (mode, n) in enumerate(phases):
        starts.append(k)
        at += [(i, mode)] * n
        k += n
    return at, starts


def drain_steps(scn, b):
    """the steps after which batch b is drained inside a D phase (its chunk ends)"""
    out, k = set(), 0
    for (mode, n), sizes in zip(scn["phases"], scn["chunks"][b]):
        j = k
        for c in sizes:
            j += c
            out.add(j - 1)
        k += n
    return out


# -------------------------------------------------------------------------------------------------------------------------------- the model
class BatchModel:
    """One batch's host bookkeeping as include/beatrice_batch.h states it.  busy(e): rule (a), some stream's settings name the entry, or
    (b) the stamp: when an entry's last naming setting goes, fewer than STAGES ticks have been launched since the batch's last step fed at
    that moment (when key/value installs at several hops per step took it away: since the step being fed), and nothing drained since."""

    def __init__(self, world, name, B, H, holds):
        self.w, self.name, self.B, self.H = world, name, B, H
        self.voice = list(holds) + [None] * (ENTRIES - REAL)     # the voice an entry holds (None: never written)
        self.prev_voice = [None] * ENTRIES
        self.installed_at = [-10 ** 6] * ENTRIES                 # the tick count at the in-flight install (this stay in a mode)
        self.mode, self.tick, self.last_feed = None, 0, -1000
        self.free_at = [0] * ENTRIES
        self.refs = [0] * ENTRIES
        self.freed_how = [None] * ENTRIES                        # what took the last reference (for the names of the coverage table)
        self.refused = [False] * ENTRIES
        self.installs_this_gap = 0
        self.drains = 0
        self.trace, self.ragged = [], False      # the marks csrc/stream_move_plan.h's Presence is given (tests/test_cpu_scenarios_in_flight.py)
        self.slots = []
        for s in range(B):
            e = s % REAL
            sl = dict(L=None, target=e, kv=[e] * 4, count=4, last=NEVER, reset=False, reset_k=None, lag=0, ghost=None,
                      settings={"SetVQNumNeighbors": [1]}, reset_taken=False, away_switch=False)
            self.slots.append(sl)
            self.refs[e] += 7

    # ---- the entries
    def named(self, s):
        sl = self.slots[s]
        return [sl["target"]] * 3 + list(sl["kv"])

    def _rename(self, s, change, stamp, how):
        before = self.named(s)
        change()
        for e in before:
            self.refs[e] -= 1
        for e in self.named(s):
            self.refs[e] += 1
        for e in set(before):
            if self.refs[e] == 0:
                self.free_at[e] = stamp
                self.freed_how[e] = how

    def busy(self, e):
        return 1 if self.refs[e] > 0 or (self.mode in "DE" and self.tick < self.free_at[e]) else 0

    def quiescent(self, s):
        if self.mode != "D":
            return -1
        t = self.slots[s]["last"]
        return 1 if t is NEVER or self.tick - t >= STAGES else 0

    # ---- the calls
    def set_target(self, s, e):
        sl = self.slots[s]

        def change():
            sl["target"], sl["count"] = e, 0
        self._rename(s, change, self.last_feed + STAGES, "switch")

    def flush(self, s, stamp=None, how="flush"):
        sl = self.slots[s]

        def change():
            sl["kv"], sl["count"] = [sl["target"]] * 4, 4
        self._rename(s, change, self.last_feed + STAGES if stamp is None else stamp, how)

    def drain(self):
        if self.mode in "DE":
            for s, sl in enumerate(self.slots):
                if sl["reset_k"] is not None and self.tick - sl["reset_k"] < STAGES:      # the step that took the reset is still inside
                    self.w.hit("reset_in_flight_travelling_at_drain", self.name, s)
                sl["last"], sl["lag"], sl["reset_k"] = NEVER, 0, None
            for e in range(ENTRIES):      # freed by this drain EARLIER than by the tick count: still busy by its stamp when it comes
                if self.refs[e] == 0 and self.refused[e] and self.freed_how[e] is not None and self.tick < self.free_at[e] \
                        and not self.freed_how[e].endswith("+drain"):
                    self.freed_how[e] += "+drain"
            if self.tick <= self.last_feed + STAGES - 1:
                self.tick = self.last_feed + STAGES
            self.ragged = False
            if self.mode == "D":
                self.trace.append(("drained",))
        self.drains += 1

    def enter(self, mode):
        self.mode = mode
        if mode in "DE":
            self.tick, self.last_feed = 0, -1000
            self.free_at = [0] * ENTRIES
            self.installed_at = [-10 ** 6] * ENTRIES
            for sl in self.slots:
                sl["last"], sl["lag"] = NEVER, 0
            self.ragged = False
            if mode == "D":
                self.trace.append(("start",))

    def leave(self):
        if self.mode is None:
            return
        if self.mode in "DE":
            self.drain()
            for s, sl in enumerate(self.slots):
                if sl["reset"]:      # a reset still waiting for its step: the drained form, now
                    self.w.hit("reset_in_flight_pending_at_mode_change", self.name, s)
                    self._take_reset(s, self.last_feed + STAGES)
        self.mode = None

    def _take_reset(self, s, stamp):
        sl = self.slots[s]
        sl["reset"], sl["reset_taken"] = False, True
        self.flush(s, stamp, "reset")
        if self.w.mutant != "reset_at_call":
            self.w.op(sl["L"], ("reset",))
            if self.w.mutant == "reset_restores_defaults":
                self.w.op(sl["L"], ("defaults",))

    def step(self, absent):
        """one step fed: the present streams install key/value blocks (one per hop), take a waiting reset, and make their hops"""
        k = self.w.k
        ticking = self.mode in "DE"
        for s, sl in enumerate(self.slots):
            if s in absent:
                sl["lag"] += 1
                continue
            stamp = (self.tick if self.H > 1 else self.last_feed) + STAGES
            if ticking and sl["reset"]:
                sl["reset_k"] = self.tick
                self._take_reset(s, stamp)
            elif sl["count"] < 4:
                def change(sl=sl):
                    n = min(self.H, 4 - sl["count"])
                    for i in range(sl["count"], sl["count"] + n):
                        sl["kv"][i] = sl["target"]
                    sl["count"] += n
                self._rename(s, change, stamp, "away_install" if sl["away_switch"] else "install")
                if sl["count"] == 4:
                    sl["away_switch"] = False
            sl["last"] = self.tick if ticking else NEVER
            L = sl["L"]
            self.w.op(L, ("hop", k, self.name, s, self.w.next_idx[L]))
            self.w.next_idx[L] += 1
        if self.mode == "D":
            self.ragged = self.ragged or bool(absent)
            self.trace.append(("step", self.tick, sorted(absent) if self.ragged else None))
        if ticking:
            self.last_feed = self.tick
            self.tick += 1
        self.installs_this_gap = 0


class World:
    """Both batches and the logical streams.  mutant: one deliberate deviation of the ORACLE's script (tests/test_cpu_scenarios_in_flight.py)."""

    def __init__(self, B, H, mutant=None):
        self.H, self.mutant = H, mutant
        self.k = -1
        self.timeline, self.next_idx, self.audio_of, self.forked_from = {}, {}, {}, {}
        self.hits = {name: [] for name in INTERACTIONS}
        self.M = {"X": BatchModel(self, "X", B["X"], H, range(REAL)), "Y": BatchModel(self, "Y", B["Y"], H, Y_HOLDS)}
        self.moved = set()
        for b in "XY":
            m = self.M[b]
            for s, sl in enumerate(m.slots):
                L = self.new_logical()
                sl["L"] = L
                self.op(L, ("voice", m.voice[sl["target"]]))
                self.op(L, ("set", "SetVQNumNeighbors", [1]))
                self.op(L, ("flush",))

    def new_logical(self, audio=None):
        L = len(self.timeline)
        self.timeline[L], self.next_idx[L] = [], 0
        self.audio_of[L] = L if audio is None else audio
        return L

    def op(self, L, what):
        if L is not None:      # (a slot that holds nobody: a stream left it)
            self.timeline[L].append(what)

    def hit(self, name, b, s, L=None):
        m = self.M[b]
        self.hits[name].append({"step": self.k, "batch": b, "slot": s, "mode": m.mode, "H": self.H,
                                "L": L if L is not None else (m.slots[s]["L"] if s >= 0 else -1)})

    # ---- one event; returns the predicted return code
    def apply(self, ev):
        kind = ev[0]
        if kind == "set":
            _, b, s, name, args = ev
            m = self.M[b]
            sl = m.slots[s]
            if sl["reset"] and s in self.absent_now[b]:
                self.hit("switch_after_reset_in_flight_while_absent" if name == "SetTargetSpeaker" else "setting_after_reset_in_flight_while_absent", b, s)
            if name == "SetTargetSpeaker":
                e = args[0]
                if m.installs_this_gap and m.installed_at[e] == m.tick:
                    self.hit("install_then_switch_same_gap", b, s)
                old = sl["target"]
                m.set_target(s, e)
                if s in self.absent_now[b] and old >= REAL and old != e:
                    sl["away_switch"] = True
                voice = m.prev_voice[e] if self.mutant == "previous_voice" and m.prev_voice[e] is not None else m.voice[e]
                self.op(sl["L"], ("voice", voice))
            else:
                sl["settings"][name] = list(args)
                self.op(sl["L"], ("set", name, list(args)))
            return 0
        if kind == "reset":
            _, b, s = ev
            m = self.M[b]
            todo = range(m.B) if s < 0 else [s]
            if s < 0 and m.mode == "D" and self.absent_now[b]:
                self.hit("reset_in_flight_all_streams", b, -1)
            for t in todo:
                sl = m.slots[t]
                if m.mode in "DE":
                    if sl["count"] < 4:
                        self.hit("reset_in_flight_while_pending", b, t)
                    if t in self.absent_now[b] and sl["ghost"] is None:
                        self.hit("reset_in_flight_while_absent", b, t)
                    if sl["reset"]:
                        self.hit("reset_in_flight_twice_before_taken", b, t)
                    sl["reset"] = True
                    m.flush(t)
                    if self.mutant == "reset_at_call":
                        self.op(sl["L"], ("reset",))
                else:       # in order: the call IS BeatriceBatch_ResetStream
                    m._take_reset(t, 0)
                    if self.mutant == "reset_at_call":
                        self.op(sl["L"], ("reset",))
            return 0
        if kind == "dreset":
            _, b, s = ev
            m = self.M[b]
            if m.slots[s]["reset"]:
                self.hit("reset_in_flight_then_drained_reset", b, s)
            m.drain()
            m.flush(s)
            self.op(m.slots[s]["L"], ("reset",))
            return 0
        if kind == "install":
            _, b, entries, voices = ev
            m = self.M[b]
            if any(m.busy(e) for e in entries):
                for e in entries:
                    if m.busy(e):
                        m.refused[e] = True
                        if m.refs[e] == 0:
                            self.hit("install_refused_entry_named_inside_pipeline", b, -1)
                return -3
            m.installs_this_gap += 1
            if m.installs_this_gap == 5 and m.mode == "D":
                self.hit("five_installs_between_two_ticks", b, -1)
            for e, v in zip(entries, voices):
                if m.refused[e]:
                    self.hit("install_refused_then_accepted", b, -1)
                    how = m.freed_how[e] or ""
                    if how.endswith("+drain"):
                        self.hit("entry_freed_by_drain", b, -1)
                    if how.startswith("away_install"):
                        self.hit("entry_freed_by_absent_stream_switching_away", b, -1)
                    if how.startswith("import"):
                        self.hit("entry_freed_by_import_over_slot", b, -1)
                    m.refused[e] = False
                if m.voice[e] is not None and m.voice[e] != v:
                    self.hit("install_reuses_entry_with_other_voice", b, -1)
                    m.prev_voice[e] = m.voice[e]
                m.voice[e] = v
                m.installed_at[e] = m.tick if m.mode in "DE" else -10 ** 6
            return 0
        if kind == "move":
            return self._move(ev)
        if kind == "turnover":
            _, b, s = ev
            m = self.M[b]
            sl = m.slots[s]
            assert sl["ghost"] is not None
            L = self.new_logical()
            sl["L"], sl["ghost"], sl["reset_taken"] = L, None, False
            self.op(L, ("voice", m.voice[sl["target"]]))
            for name, args in sorted(sl["settings"].items()):
                self.op(L, ("set", name, list(args)))
            self.op(L, ("flush",))
            self.hit("source_slot_turned_over", b, s)
            return 0
        if kind == "refeed":
            _, b, s = ev
            m = self.M[b]
            sl = m.slots[s]
            old, n = sl["ghost"]
            L = self.new_logical(audio=self.audio_of[old])
            self.forked_from[L] = old
            for what in self.timeline[old][:n]:
                self.op(L, ("replayed",) + what[1:] if what[0] == "hop" else what)
            self.next_idx[L] = sum(1 for what in self.timeline[old][:n] if what[0] == "hop")
            if self.mutant == "refeed_from_zeros":
                self.op(L, ("reset",))
            sl["L"], sl["ghost"] = L, None
            self.moved.add(L)
            self.hit("source_fed_again_after_move", b, s)
            return 0
        raise AssertionError(ev)

    def entry_map(self, src, dst):
        """source entry -> the lowest destination entry that holds the same voice (0 where there is none: such an entry is never named)"""
        out = []
        for e in range(ENTRIES):
            v = self.M[src].voice[e]
            same = [d for d in range(ENTRIES) if v is not None and self.M[dst].voice[d] == v]
            out.append(same[0] if same else 0)
        return out

    def _move(self, ev):
        _, how, src, frm, dst, to, emap = ev
        ms, md = self.M[src], self.M[dst]
        in_flight = ms.mode == "D"
        if in_flight:
            src_rest = all(ms.quiescent(s) == 1 for s in frm)
            rest = src_rest and all(md.quiescent(t) == 1 for t in to)
            flagged = [s for s in frm if ms.slots[s]["reset"]]
            if not rest or flagged:
                if src_rest and flagged:
                    self.hit("move_refused_reset_pending", src, flagged[0])
                elif not flagged and all(md.quiescent(t) == 1 for t in to):
                    short = [s for s in frm if ms.quiescent(s) == 0]
                    if all(ms.tick - ms.slots[s]["last"] == STAGES - 1 for s in short):
                        self.hit("move_refused_one_tick_short", src, short[0])
                return -3
        for s, t in zip(frm, to):
            a, d = ms.slots[s], md.slots[t]
            L = a["L"]
            assert a["ghost"] is None and a["L"] is not None
            for e in [a["target"]] + a["kv"]:
                assert md.voice[emap[e]] == ms.voice[e], "the destination does not hold the voice of source entry %d" % e
            if in_flight:
                self.hit("move_by_blobs" if how == "blobs" else "move_device_to_device", src, s)
                if a["count"] < 4:
                    self.hit("move_with_installs_pending", src, s)
                if any(md.tick - md.installed_at[emap[e]] < STAGES for e in [a["target"]] + a["kv"]):
                    self.hit("move_onto_entry_installed_in_flight", src, s)
                if a["reset_taken"]:
                    self.hit("move_after_reset_taken", src, s)
                if d["reset"]:
                    self.hit("import_cancels_pending_reset", dst, t, L)
                if a["lag"] == 0 and ms.drains > 0 and a["last"] is NEVER:
                    self.hit("move_at_rest_by_drain", src, s)
                if L in self.moved and a.get("came_from") == dst and d["lag"] > 0 and t != a.get("came_from_slot"):
                    self.hit("move_round_trip", src, s)
                corners = {15, 16, 31, 32}
                if (ms.B >= 24 and (s in corners or s == ms.B - 1)) or (md.B >= 24 and (t in corners or t == md.B - 1)):
                    self.hit("move_of_tile_corner_stream", src, s)
                if len(frm) > 1:
                    self.hit("moves_of_several_streams_one_call", src, s)
            if not in_flight:
                self.hit("move_as_drained_fallback", src, s)
            if self.mutant == "pending_flushed" and a["count"] < 4:
                self.op(L, ("flush",))
            if self.mutant == "pitch_context_lost":
                self.op(L, ("losepitch",))
            if self.mutant == "reset_survives_import" and d["reset"]:
                self.op(L, ("reset",))
            new = dict(target=emap[a["target"]], kv=[emap[e] for e in a["kv"]], count=a["count"])

            def change(d=d, new=new):
                d.update(new)
            md._rename(t, change, md.last_feed + STAGES, "import")
            d.update(L=L, reset=False, ghost=None, settings=dict(a["settings"]), reset_taken=a["reset_taken"], away_switch=False,
                     came_from=src, came_from_slot=s)
            a["ghost"] = (L, len(self.timeline[L]))
            a["L"] = None
            self.moved.add(L)
        return 0

    # ---- the walk
    def start_step(self, k, scn):
        """phase changes in front of step k; afterwards the events of the step may be applied"""
        self.k = k
        at, starts = _phase_table(scn["phases"])
        self.absent_now = {b: set(scn["absent"][b][k]) for b in "XY"}
        if k == starts[at[k][0]]:
            for b in "XY":
                self.M[b].leave()
                self.M[b].enter(at[k][1])
            return at[k][1]
        return None

    def feed(self, k, scn, b):
        m = self.M[b]
        for s in scn["absent"][b][k]:
            assert m.mode == "D"
        for s, sl in enumerate(m.slots):
            assert sl["L"] is not None or s in self.absent_now[b], "slot %s%d holds nobody and is fed at step %d" % (b, s, k)
        m.step(self.absent_now[b])

    def end_step(self, k, scn, b):
        if k in self._drains(scn)[b]:
            self.M[b].drain()

    def _drains(self, scn):
        if not hasattr(self, "_dr"):
            self._dr = {b: drain_steps(scn, b) for b in "XY"}
        return self._dr

    def finish(self):
        for b in "XY":
            self.M[b].leave()


def replay(scn, mutant=None, check=True):
    """The model over the scenario.  -> dict: world, per step the predicted probes {b: (quiescent [B], busy [16])}, the ticks after every step,
    the predicted return codes (asserted equal to those the generator stored)."""
    w = World(scn["B"], scn["H"], mutant)
    probes, ticks = [], []
    steps = len(scn["events"])
    for k in range(steps):
        w.start_step(k, scn)
        for ev, rc in scn["events"][k]:
            got = w.apply(ev)
            assert not check or got == rc, "step %d, %s: the model predicts %d, the scenario holds %d" % (k, ev, got, rc)
        probes.append({b: ([w.M[b].quiescent(s) for s in range(w.M[b].B)], [w.M[b].busy(e) for e in range(ENTRIES)]) for b in "XY"})
        for b in "XY":
            if w.M[b].mode == "D":
                w.M[b].trace.append(("ask", w.M[b].tick, k))
            w.feed(k, scn, b)
        w.absent_now = {b: set() for b in "XY"}
        for ev, rc in scn["after"][k]:
            got = w.apply(ev)
            assert not check or got == rc
        for b in "XY":
            w.end_step(k, scn, b)
        ticks.append({b: w.M[b].tick for b in "XY"})
    w.finish()
    return {"world": w, "probes": probes, "ticks": ticks}


def interactions_detail(scn):
    return replay(scn)["world"].hits


def interactions(scn):
    return {name for name, hits in interactions_detail(scn).items() if hits}


def oracle_hops(scn, w):
    return sum(scn["H"] for L in scn["legs"] for what in w.timeline[L] if what[0] in ("hop", "replayed"))


# ------------------------------------------------------------------------------------------------------------------------------ the generator
class Gen:
    def __init__(self, seed, Bx, By, H, phases):
        self.rng = np.random.default_rng(seed)
        self.seed, self.H = seed, H
        self.B = {"X": Bx, "Y": By}
        self.phases = [[str(m), int(n)] for m, n in phases]
        self.at, self.starts = _phase_table(self.phases)
        self.steps = len(self.at)
        rng = self.rng
        self.long = self.phases[0][0] == "D" and self.phases[0][1] >= 44 and seed % 2 == 0 and Bx >= 5 and By >= 5
        self.chunks = {}
        for b in "XY":
            per = []
            for mode, n in self.phases:
                sizes, left = [], n
                long_one = self.long and mode == "D" and b == "Y"      # one chunk long enough for a stream to come to rest by tick count
                while mode == "D" and left > 0:
                    if long_one and not sizes:
                        c = min(left, int(rng.integers(30, 35)))
                    else:
                        c = min(left, int(rng.integers(4, 10)))
                    sizes.append(c)
                    left -= c
                per.append(sizes)
            self.chunks[b] = per
        self.events = [[] for _ in range(self.steps)]
        self.after = [[] for _ in range(self.steps)]
        self.absent = {b: [set() for _ in range(self.steps)] for b in "XY"}
        self.w = World(self.B, H)
        self.scn_view = {"phases": self.phases, "chunks": self.chunks, "absent": self.absent}
        self.drains = {b: drain_steps(self.scn_view, b) for b in "XY"}
        self.touched, self.late = set(), []
        self.k = 0

    def emit(self, ev, late=False):
        if late:      # handed over after the step has been fed (the main loop applies it there)
            self.late.append(ev)
            return None
        rc = self.w.apply(ev)
        self.events[self.k].append([ev, rc])
        if ev[0] in ("set", "reset", "dreset", "turnover", "refeed") and ev[2] >= 0:
            L = self.w.M[ev[1]].slots[ev[2]]["L"]
            if L is not None:
                self.touched.add(L)
        return rc

    def sit(self, b, s):
        self.absent[b][self.k].add(s)
        self.w.absent_now[b].add(s)
        L = self.w.M[b].slots[s]["L"]
        if L is not None:
            self.touched.add(L)

    def both_d(self, k=None):
        k = self.k if k is None else k
        return k < self.steps and self.at[k][1] == "D"

    def last_of_phase(self, k=None):
        k = self.k if k is None else k
        return k + 1 >= self.steps or self.at[k + 1][0] != self.at[k][0]

    def corner(self, b, taken):
        B = self.B[b]
        pool = [s for s in ([15, 16, 31, 32, B - 1] if B >= 24 else pick_streams(B, 8)) if 0 <= s < B and s not in taken]
        if not pool:
            return None
        return int(pool[int(self.rng.integers(0, len(pool)))])


def make_scenario(seed, Bx, By, H, phases):
    g = Gen(seed, Bx, By, H, phases)
    rng, w = g.rng, g.w
    X, Y = w.M["X"], w.M["Y"]
    act = {}
    for b in "XY":
        taken = []
        for _ in range(min(3 if g.long else 2, g.B[b] - 1) if g.B[b] >= 3 else 1):
            s = g.corner(b, taken)
            if s is not None:
                taken.append(s)
        act[b] = taken
    bystander = {b: g.corner(b, act[b]) for b in "XY"}
    how_of = lambda: "blobs" if rng.random() < 0.5 else "move"       # noqa: E731
    real_other = lambda m, s: int((m.slots[s]["target"] % REAL + 1 + rng.integers(0, REAL - 1)) % REAL)   # noqa: E731
    parked = {b: set() for b in "XY"}      # slots the play keeps out of the steps (waiting for rest, or left by a move)

    def free_entry(m, avoid=()):
        for e in range(REAL, ENTRIES):
            if not m.busy(e) and m.voice[e] is None and e not in avoid:
                return e
        for e in range(REAL, ENTRIES):
            if not m.busy(e) and e not in avoid:
                return e
        return None

    def entry_of(m, v):
        for e in range(ENTRIES):
            if m.voice[e] == v:
                return e
        return None

    def at_rest(b, s):
        return w.M[b].quiescent(s) == 1

    # ---- the play of the D phases: one script on two actors per batch, written as a generator; each `yield` is one step
    def reinstall(st):
        """the entries an install was refused for: asked again at the first step the model says free"""
        for e, (b, v) in list(st.items()):
            if not w.M[b].busy(e):
                g.emit(["install", b, [e], [v]])
                del st[e]
                s = act[b][0]      # the batch's first actor, when somebody is in it, goes onto the entry: it has held another voice before
                if w.M[b].slots[s]["L"] is not None and s not in parked[b] and w.M[b].slots[s]["count"] == 4 and not w.M[b].slots[s]["reset"]:
                    g.emit(["set", b, s, "SetTargetSpeaker", [e]])

    def bring(src, dst, slots):
        """the voices the slots name into free entries of the destination"""
        ms, md = w.M[src], w.M[dst]
        for s in slots:
            for e in [ms.slots[s]["target"]] + ms.slots[s]["kv"]:
                if entry_of(md, ms.voice[e]) is None:
                    g.emit(["install", dst, [free_entry(md)], [ms.voice[e]]])

    def play():
        a1 = act["X"][0]
        b1 = act["Y"][0]
        a2 = act["X"][1] if len(act["X"]) > 1 else None
        b2 = act["Y"][1] if len(act["Y"]) > 1 else None
        again = {}
        # 1. a new voice into X and a1 onto it in the same gap; five installs between two ticks in Y, b1 (and b2) onto two of them
        v0, v1, v2 = (int(v) for v in rng.choice(np.arange(REAL, ENTRIES), size=3, replace=False))
        e0 = free_entry(X)
        g.emit(["install", "X", [e0], [v0]])
        g.emit(["set", "X", a1, "SetTargetSpeaker", [e0]])
        ys = list(range(REAL, REAL + 5))
        for i, e in enumerate(ys):
            g.emit(["install", "Y", [e], [int(REAL + (v2 - REAL + 1 + i) % 8)]])
        f0 = ys[0]
        g.emit(["set", "Y", b1, "SetTargetSpeaker", [f0]])      # b1 is the only stream on Y's entry f0
        if b2 is not None:
            g.emit(["set", "Y", b2, "SetTargetSpeaker", [ys[1]]])
        yield
        yield
        parked["Y"].add(b1)                                     # b1's first user ends here: the slot waits for the stream that moves in
        # 2. the reset family on a1: with installs pending, then inside a sit-out with a switch and a setting behind it, and twice
        g.emit(["set", "X", a1, "SetTargetSpeaker", [real_other(X, a1)]])
        g.emit(["reset", "X", a1])
        yield
        for i in range(int(rng.integers(3, 5))):
            g.sit("X", a1)
            if i == 0:
                g.emit(["reset", "X", -1])      # every stream of X is asked to start over while a1 sits out
            if i == 1:
                g.emit(["reset", "X", a1])
            if i == 2:      # behind the last reset asked for: the step that takes it must start on all four blocks of THIS target
                g.emit(["set", "X", a1, "SetTargetSpeaker", [e0]])
                g.emit(["set", "X", a1, "SetPitchShift", [float(rng.integers(-6, 7))]])
            yield
        # b2 switches away from its entry while it sits out: the entry stays named by its key/value entries until it returns and installs;
        # asked for at once, the entry is refused (the steps that named it are inside the pipeline)
        if b2 is not None:
            for i in range(3):
                g.sit("Y", b2)
                if i == 1:
                    g.emit(["set", "Y", b2, "SetTargetSpeaker", [real_other(Y, b2)]])
                yield
            for _ in range(4 // H):
                yield
            if g.emit(["install", "Y", [ys[1]], [v1]]) == -3:
                again[ys[1]] = ("Y", v1)
        yield
        # 3. a reset in flight and the drained one in the gap behind a chunk end of X (the pipeline is empty: nothing more drains)
        while g.both_d() and not (g.k - 1 in g.drains["X"] and X.tick > 0):
            reinstall(again)
            yield
        if not g.both_d():
            return
        who = a2 if a2 is not None else a1
        g.emit(["reset", "X", who])
        g.emit(["dreset", "X", who])
        yield
        # ... and one that is travelling while X drains: taken by the last step of a chunk
        while g.both_d() and g.k not in g.drains["X"]:
            reinstall(again)
            yield
        if not g.both_d() or g.last_of_phase():
            return
        g.emit(["reset", "X", a1])
        yield
        # 4. the first move: a1 switches onto a voice installed in this gap and sits out with all four installs pending; b1 has a
        #    reset waiting; Y installs the voice in the gap of the move: a1 -> b1
        e1 = free_entry(X, avoid=[e0])
        g.emit(["install", "X", [e1], [v1]])
        first = True
        while g.both_d() and not g.last_of_phase():
            g.sit("X", a1)
            if first:
                g.emit(["set", "X", a1, "SetTargetSpeaker", [e1]])
                first = False
            reinstall(again)
            if at_rest("X", a1) and at_rest("Y", b1):
                break
            yield
        if not (g.both_d() and at_rest("X", a1) and at_rest("Y", b1)) or first:
            return
        f1 = entry_of(Y, v1)
        if f1 is None or Y.tick - Y.installed_at[f1] >= STAGES:
            f1 = f1 if f1 is not None and not Y.busy(f1) else free_entry(Y)
            g.emit(["install", "Y", [f1], [v1]])
        bring("X", "Y", [a1])
        if not Y.slots[b1]["reset"]:
            g.emit(["reset", "Y", b1])
        if g.emit(["move", how_of(), "X", [a1], "Y", [b1], w.entry_map("X", "Y")]) != 0:
            return
        parked["X"].add(a1)
        parked["Y"].discard(b1)
        if g.emit(["install", "Y", [f0], [v0]]) == -3:          # f0: its only stream was imported over; the step that named it may be inside
            again[f0] = ("Y", v0)
        if b2 is not None:
            parked["Y"].add(b2)                                 # b2's first user ends here
        yield
        reinstall(again)
        yield
        # 5. the source slot is turned over for a new stream; asked to move before a step has taken the reset, it is refused
        if not g.both_d() or g.last_of_phase():
            return
        reinstall(again)
        g.emit(["turnover", "X", a1])
        g.emit(["reset", "X", a1])
        g.emit(["set", "X", a1, "SetTargetSpeaker", [real_other(X, a1)]])
        g.emit(["set", "X", a1, "SetFormantShift", [float(rng.integers(-2, 3)) / 2.0]])
        if at_rest("X", a1):
            bring("X", "Y", [a1])
            g.emit(["move", how_of(), "X", [a1], "Y", [b2 if b2 is not None else b1], w.entry_map("X", "Y")])
        parked["X"].discard(a1)
        yield
        if a2 is None or b2 is None:
            return
        # 6. the second move, at rest by the drain alone: a2 takes part in the last step of a chunk of X and goes in the gap behind it
        while g.both_d() and not g.last_of_phase():
            reinstall(again)
            if g.k - 1 in g.drains["X"] and at_rest("Y", b2) and at_rest("X", a2):
                break
            yield
        if not (g.both_d() and at_rest("X", a2) and at_rest("Y", b2)) or g.last_of_phase():
            return
        bring("X", "Y", [a2])
        if g.emit(["move", how_of(), "X", [a2], "Y", [b2], w.entry_map("X", "Y")]) != 0:
            return
        parked["X"].add(a2)
        parked["Y"].discard(b2)
        yield
        # the source is fed again as it is in some scenarios: the stream goes on there too (the oracle stream is forked)
        if seed % 2 == 1 and g.both_d():
            g.emit(["refeed", "X", a2])
            parked["X"].discard(a2)
        for _ in range(2):
            reinstall(again)
            yield
        # 7. the way back, both in one call: b1, b2 -> a2, a1 (another slot of X than the one the stream left), the slots' own counters
        #    lagging X's by the steps they sat out
        for b, s in (("Y", b1), ("Y", b2), ("X", a1), ("X", a2)):
            parked[b].add(s)
        while g.both_d() and not g.last_of_phase():
            reinstall(again)
            if all(at_rest("Y", s) for s in (b1, b2)) and all(at_rest("X", s) and X.slots[s]["lag"] > 0 for s in (a1, a2)):
                break
            yield
        if not (g.both_d() and all(at_rest("Y", s) for s in (b1, b2)) and all(at_rest("X", s) for s in (a1, a2))) or g.last_of_phase():
            return
        bring("Y", "X", [b1, b2])
        if g.emit(["move", how_of(), "Y", [b1, b2], "X", [a2, a1], w.entry_map("Y", "X")]) != 0:
            return
        parked["X"].discard(a1)
        parked["X"].discard(a2)
        while True:
            reinstall(again)
            yield

    def by_count():
        """In the scenarios whose first chunk of Y is long: a stream of Y comes to rest by the tick count alone, is asked to move one tick
        short of it (refused) and goes one step later, into a slot of X that has not taken part since tick mode was entered."""
        if not g.long or len(act["Y"]) < 3 or len(act["X"]) < 3:
            return
        b3, a3 = act["Y"][2], act["X"][2]
        parked["X"].add(a3)
        yield
        yield
        parked["Y"].add(b3)
        while g.both_d() and not g.last_of_phase():
            last = Y.slots[b3]["last"]
            if at_rest("Y", b3):
                if at_rest("X", a3):
                    g.emit(["move", how_of(), "Y", [b3], "X", [a3], w.entry_map("Y", "X")])
                    parked["X"].discard(a3)
                return
            if last is not NEVER and Y.tick - last == STAGES - 1 and at_rest("X", a3):
                g.emit(["move", how_of(), "Y", [b3], "X", [a3], w.entry_map("Y", "X")])
            yield

    def phase_end():
        """a reset asked for after the last step of a D phase: it is still waiting when the mode changes"""
        while True:
            if g.both_d() and g.last_of_phase():
                for s in act["X"]:
                    if X.slots[s]["L"] is not None and s not in parked["X"]:
                        g.emit(["reset", "X", s], late=True)
                        break
            yield

    def other_phases():
        """E: install, switch, reset in flight and a refused install; A: the same calls as their fall-backs"""
        while True:
            mode = g.at[g.k][1]
            j = g.k - g.starts[g.at[g.k][0]]
            if mode in "AE" and act["X"]:
                s = act["X"][0]
                m = X
                if m.slots[s]["L"] is not None:
                    if j == 1:
                        e = free_entry(m)
                        if e is not None:
                            v = int(rng.integers(REAL, ENTRIES))
                            if entry_of(m, v) is None:
                                g.emit(["install", "X", [e], [v]])
                                g.emit(["set", "X", s, "SetTargetSpeaker", [e]])
                    if j == 2:
                        g.emit(["reset", "X", s])
                        g.emit(["set", "X", s, "SetPitchShift", [float(rng.integers(-5, 6))]])
                    if j == 1 and mode == "A" and len(act["X"]) > 1 and len(act["Y"]) > 1:
                        # a move as its documented fall-back, the drained pair: X's second actor goes on in Y's second actor's slot; in
                        # order nobody can sit out, so the source slot is fed again as it is from this very step on
                        a2, b2 = act["X"][1], act["Y"][1]
                        if X.slots[a2]["L"] is not None and Y.slots[b2]["L"] is not None:
                            need = {X.voice[e] for e in [X.slots[a2]["target"]] + X.slots[a2]["kv"] if entry_of(Y, X.voice[e]) is None}
                            room = [e for e in range(REAL, ENTRIES) if not Y.busy(e)]
                            if len(need) <= len(room):
                                for e, v in zip(room, sorted(need)):
                                    g.emit(["install", "Y", [e], [v]])
                                g.touched.add(Y.slots[b2]["L"])
                                g.emit(["move", "blobs", "X", [a2], "Y", [b2], w.entry_map("X", "Y")])
                                g.emit(["refeed", "X", a2])
                    if j == 3 and mode == "E":
                        old = m.slots[s]["target"]
                        g.emit(["set", "X", s, "SetTargetSpeaker", [real_other(m, s)]])
                        if old >= REAL:
                            g.emit(["install", "X", [old], [int(REAL + (m.voice[old] - REAL + 1) % 8)]])
            yield

    threads = [play(), by_count(), phase_end(), other_phases()]
    alive = [True] * len(threads)
    for k in range(g.steps):
        g.k = k
        w.start_step(k, g.scn_view)
        if g.at[k][1] == "D":
            for b in "XY":
                for s in parked[b]:
                    g.sit(b, s)
        else:
            for b in "XY":           # outside tick mode everybody takes part: a slot a stream left is fed again as it is
                for s in sorted(parked[b]):
                    if w.M[b].slots[s]["ghost"] is not None:
                        g.emit(["refeed", b, s])
                parked[b].clear()
        for i, t in enumerate(threads):
            if alive[i] and (i > 1 or g.at[k][1] == "D"):
                try:
                    next(t)
                except StopIteration:
                    alive[i] = False
        if g.at[k][1] == "D":
            for b in "XY":               # whoever holds nobody sits out
                for s, sl in enumerate(w.M[b].slots):
                    if sl["L"] is None:
                        g.sit(b, s)
        for b in "XY":
            w.feed(k, g.scn_view, b)
        w.absent_now = {b: set() for b in "XY"}
        for ev in g.late:
            g.after[k].append([ev, w.apply(ev)])
            if ev[2] >= 0 and w.M[ev[1]].slots[ev[2]]["L"] is not None:
                g.touched.add(w.M[ev[1]].slots[ev[2]]["L"])
        g.late = []
        for b in "XY":
            w.end_step(k, g.scn_view, b)
    w.finish()
    legs = sorted(g.touched | w.moved | {w_initial(b, g.B, bystander[b]) for b in "XY" if bystander[b] is not None})
    return {"seed": int(seed), "B": dict(g.B), "H": int(H), "phases": g.phases, "chunks": g.chunks, "events": g.events, "after": g.after,
            "absent": {b: [sorted(a) for a in g.absent[b]] for b in "XY"}, "actors": act, "bystanders": bystander, "legs": [int(x) for x in legs]}


def w_initial(b, B, s):
    """the logical stream that starts in slot s of batch b"""
    return s if b == "X" else B["X"] + s


# ------------------------------------------------------------------------------------------------------------------------------- the story
def stream_story(scn, L, upto, rep=None):
    """One logical stream across the moves up to step `upto`: its events, the slots it lived in, presence, pending count and reset flag, and
    the model's quiescence and busy answers around the step."""
    rep = rep or replay(scn)
    w = rep["world"]
    lines = ["%s, phases %s, chunks %s: logical stream %d up to step %d" % (scenario_id(scn), scn["phases"], scn["chunks"], L, upto)]
    if L in w.forked_from:
        lines.append("  forked from logical stream %d (the source slot was fed again after a move)" % w.forked_from[L])
    homes, history = [], {}
    for what in w.timeline[L]:
        if what[0] == "hop":
            history[what[1]] = "%s%d" % (what[2], what[3])
            if not homes or homes[-1][1] != history[what[1]]:
                homes.append((what[1], history[what[1]]))
    lines.append("  lived in (from step, slot): %s" % homes)
    lines.append("  present (.: not): %s" % "".join("#" if k in history else "." for k in range(upto + 1)))
    w2 = World(scn["B"], scn["H"])
    for k in range(min(upto + 1, len(scn["events"]))):
        w2.start_step(k, scn)
        for ev, rc in scn["events"][k]:
            where = [(b, s) for b in "XY" for s, sl in enumerate(w2.M[b].slots) if sl["L"] == L]
            mine = ev[0] == "move" and any((ev[2], s) in where for s in ev[3]) or ev[0] != "move" and ev[0] != "install" and (ev[1], ev[2]) in where \
                or ev[0] in ("reset",) and ev[2] < 0 and any(b == ev[1] for b, _ in where)
            w2.apply(ev)
            now = [(b, s) for b in "XY" for s, sl in enumerate(w2.M[b].slots) if sl["L"] == L]
            if mine or now != where:
                sl = w2.M[now[0][0]].slots[now[0][1]] if now else None
                lines.append("  step %3d: %s -> %d%s" % (k, ev, rc, "; now in %s%d, pending %d, reset flag %d" % (
                    now[0][0], now[0][1], 4 - sl["count"], sl["reset"]) if sl else ""))
        for b in "XY":
            w2.feed(k, scn, b)
        for ev, rc in scn["after"][k]:
            w2.apply(ev)
        for b in "XY":
            w2.end_step(k, scn, b)
    for k in range(max(0, upto - 2), min(upto + 1, len(scn["events"]))):
        lines.append("  before step %d the model says: %s" % (k, {b: "quiescent %s busy %s" % (
            "".join("-01"[q + 1] for q in rep["probes"][k][b][0][:40]), "".join(str(v) for v in rep["probes"][k][b][1])) for b in "XY"}))
    for name, hits in w.hits.items():
        mine = [h["step"] for h in hits if h["L"] == L and h["step"] <= upto]
        if mine:
            lines.append("  %s at steps %s" % (name, mine))
    return "\n".join(lines)


# ------------------------------------------------------------------------------------------------------------------------------- runners
class Voices:
    """the derived voices 8..15, as tests/test_gpu_install_in_flight.py derives them: the model's own tables with the speaker axis rotated by
    one and the codebook rows reversed"""

    def __init__(self, t):
        self.cb = np.ascontiguousarray(np.roll(t.codebooks[:REAL], 1, axis=0)[:, ::-1])
        self.add = np.ascontiguousarray(np.roll(t.additive[:REAL], 1, axis=0))
        self.kv = np.ascontiguousarray(np.roll(t.kv[:REAL], 1, axis=0))


def voice_tables(t):
    """(codebooks, additive, kv) of the 16 voices: 0..7 real, 8..15 derived"""
    v = Voices(t)
    return (np.ascontiguousarray(np.concatenate([t.codebooks[:REAL], v.cb])), np.ascontiguousarray(np.concatenate([t.additive[:REAL], v.add])),
            np.ascontiguousarray(np.concatenate([t.kv[:REAL], v.kv])))


class Env:
    def __init__(self, bv, oracle, product, model_dir8):
        self.bv, self.oracle, self.model_dir = bv, oracle, model_dir8
        self.product = bv.bind_batch(product) if product is not None else None


def audio(bv, scn, who, n):
    return bv.synth_audio(160 * scn["H"] * n, seed=7000 + 41 * (scn["seed"] % 1000) + who).reshape(n, scn["H"] * 160)


def oracle_models(env):
    """the oracle's models with the speaker tables extended by the derived voices: Stream1.set_target_speaker indexes them by VOICE"""
    om = env.bv.Models(env.oracle, env.model_dir)
    om.tables.codebooks, om.tables.additive, om.tables.kv = voice_tables(om.tables)
    return om


def run_leg(env, scn, om, ops, xs, stop_after=None):
    """one logical stream's timeline on one oracle stream -> ([(step, batch, slot, samples [H * 240])] of its compared steps, raw bins seen)"""
    bv, H = env.bv, scn["H"]
    ob = OracleBatch(bv, env.oracle, env.model_dir, 1, sample=[0], models=om, hops_per_step=H)
    out, bins = [], set()
    try:
        for what in ops:
            c = ob.st[0]
            if what[0] == "voice":
                ob.a.BeatriceBatch_SetTargetSpeaker(None, 0, what[1])
            elif what[0] == "set":
                assert getattr(ob.a, "BeatriceBatch_" + what[1])(None, 0, *what[2]) == 0
            elif what[0] == "flush":
                ob.a.BeatriceBatch_FlushSpeaker(None, 0)
            elif what[0] == "reset":
                ob.a.BeatriceBatch_ResetStream(None, 0)
            elif what[0] == "defaults":
                ob.a.BeatriceBatch_SetPitchShift(None, 0, 0.0)
                ob.a.BeatriceBatch_SetFormantShift(None, 0, 0.0)
            elif what[0] == "losepitch":
                s1 = c["s1"]
                s1.a.DestroyPitchContext1(s1.tc)
                s1.tc = s1.a.CreatePitchContext1()
                s1.a.SetMinQuantizedPitch(s1.tc, c["min_q"])
                s1.a.SetMaxQuantizedPitch(s1.tc, c["max_q"])
            else:
                x = xs[what[4]]
                ys = []
                for hh in range(H):
                    y, _, q, _, _ = c["s1"].hop(x[hh * 160:(hh + 1) * 160], return_all=True)
                    ys.append(y)
                    bins.add(int(q))
                if what[0] == "hop":
                    out.append((what[1], what[2], what[3], np.concatenate(ys)))
                    if stop_after is not None and what[1] >= stop_after:
                        break
    finally:
        ob.close()
    return out, bins


def run_legs(env, scn, w):
    from concurrent.futures import ThreadPoolExecutor
    om = oracle_models(env)
    steps = len(scn["events"])
    try:
        def leg(L):
            return run_leg(env, scn, om, w.timeline[L], audio(env.bv, scn, w.audio_of[L], steps))
        with ThreadPoolExecutor(max_workers=8) as pool:
            return dict(zip(scn["legs"], pool.map(leg, scn["legs"])))
    finally:
        om.close()


def make_batch(bv, m, B, H, holds, start_counter=None):
    """a 16-entry batch: the real voices in the order `holds` in entries 0..7, entries 8..15 empty; every stream s on entry s % 8 with one
    k-NN neighbour (the k-NN stage is there from before the first step and never goes: that would drain)"""
    t = m.tables
    cb = np.zeros((ENTRIES,) + t.codebooks.shape[1:], np.float32)
    add = np.zeros((ENTRIES, t.additive.shape[1]), np.float32)
    kv = np.zeros((ENTRIES,) + t.kv.shape[1:], np.float32)
    order = list(holds)
    cb[:REAL], add[:REAL], kv[:REAL] = t.codebooks[order], t.additive[order], t.kv[order]
    batch = bv.Batch(m, B, max_speakers=ENTRIES, hops_per_step=H, upload_tables=False, start_counter=start_counter)
    a, h = batch.a, batch.h
    assert a.BeatriceBatch_SetSpeakerTables(h, ENTRIES, bv.fptr(cb), bv.fptr(add), bv.fptr(t.formant), bv.fptr(kv)) == 0
    batch.apply_defaults()
    ss = np.arange(B, dtype=np.int32)
    sp = np.ascontiguousarray(ss % REAL, np.int32)
    assert a.BeatriceBatch_SetTargetSpeakers(h, B, bv.iptr(ss), bv.iptr(sp)) == 0
    assert a.BeatriceBatch_SetVQNumNeighbors(h, -1, 1) == 0
    assert a.BeatriceBatch_FlushSpeaker(h, -1) == 0
    return batch


def inputs_of(env, scn, w):
    """{b: [steps][B][H * 160]}: every slot's input at every step it takes part in, from the timelines"""
    steps, H = len(scn["events"]), scn["H"]
    x = {b: np.zeros((steps, scn["B"][b], H * 160), np.float32) for b in "XY"}
    cache = {}
    for L, ops in w.timeline.items():
        for what in ops:
            if what[0] == "hop":
                who = w.audio_of[L]
                if who not in cache:
                    cache[who] = audio(env.bv, scn, who, steps)
                x[what[2]][what[1], what[3]] = cache[who][what[4]]
    return x


def untouched(scn, w):
    """{b: slots} whose logical stream no event but a reset of all streams ever touches: compared with the in-order chain"""
    out = {}
    for b in "XY":
        out[b] = [s for s in range(scn["B"][b]) if w_initial(b, scn["B"], s) not in scn["legs"]]
    return out


def run_in_order(env, scn, x):
    """{b: [steps][B][H * 240]} from the product's in-order chain at one hop per step: the reference of the streams nobody touches (a reset of
    every stream of the batch is the one event they see)"""
    bv, H = env.bv, scn["H"]
    steps = len(scn["events"])
    m = bv.Models(env.product, env.model_dir)
    out = {}
    try:
        for b, holds in (("X", range(REAL)), ("Y", Y_HOLDS)):
            batch = make_batch(bv, m, scn["B"][b], 1, holds)
            try:
                y = np.zeros((steps, scn["B"][b], H * 240), np.float32)
                for k in range(steps):
                    for ev, rc in scn["events"][k] + scn["after"][k - 1] if k > 0 else scn["events"][k]:
                        if ev[0] == "reset" and ev[1] == b and ev[2] < 0:
                            assert batch.a.BeatriceBatch_ResetStream(batch.h, -1) == 0
                    for hh in range(H):
                        y[k, :, hh * 240:(hh + 1) * 240] = batch.convert(np.ascontiguousarray(x[b][k, :, hh * 160:(hh + 1) * 160]))
                out[b] = y
            finally:
                batch.close()
    finally:
        m.close()
    return out


def i32(v):
    return np.ascontiguousarray(v, np.int32)


def run_product(env, scn, x, rep, start_counter=None, say=print):
    """The two product batches through the scenario.  Every probe, return code and tick count is asserted against the model `rep` on the
    way.  -> ({b: [steps][B][H * 240]}, problems)"""
    from tick_driver import Resident
    bv, H = env.bv, scn["H"]
    steps = len(scn["events"])
    at, starts = _phase_table(scn["phases"])
    m = bv.Models(env.product, env.model_dir)
    vcb, vadd, vkv = voice_tables(m.tables)
    start = start_counter or {"X": None, "Y": None}
    batches = {"X": make_batch(bv, m, scn["B"]["X"], H, range(REAL), start["X"]), "Y": make_batch(bv, m, scn["B"]["Y"], H, Y_HOLDS, start["Y"])}
    out = {b: np.zeros((steps, scn["B"][b], H * 240), np.float32) for b in "XY"}
    problems = []
    res, first_of = {}, {}
    w = World(scn["B"], H)
    drains = {b: drain_steps(scn, b) for b in "XY"}

    def state(b):
        a, h = batches[b].a, batches[b].h
        return (a.BeatriceBatch_TicksLaunched(h), a.BeatriceBatch_StepCounter(h), a.BeatriceBatch_ResidentBlocksOwed(h),
                tuple(a.BeatriceBatch_StreamQuiescent(h, s) for s in range(batches[b].B)))

    def do(ev, mode):
        kind = ev[0]
        if kind in ("turnover", "refeed"):
            return 0
        batch = batches[ev[1]] if kind != "move" else None
        if kind == "set":
            return getattr(batch.a, "BeatriceBatch_" + ev[3])(batch.h, ev[2], *ev[4])
        if kind == "reset":
            return batch.a.BeatriceBatch_ResetStreamInFlight(batch.h, ev[2])
        if kind == "dreset":
            return batch.a.BeatriceBatch_ResetStream(batch.h, ev[2])
        if kind == "install":
            cb, add, kv = vcb[ev[3]].copy(), vadd[ev[3]].copy(), vkv[ev[3]].copy()
            return batch.a.BeatriceBatch_InstallSpeakersInFlight(batch.h, len(ev[2]), bv.iptr(i32(ev[2])), bv.fptr(cb), bv.fptr(add), bv.fptr(kv))
        _, how, sb, frm, db, to, emap = ev
        src, dst = batches[sb], batches[db]
        em = i32(emap)
        if mode != "D":       # the documented fall-back: the drained pair
            dst.import_streams(to, src.export_streams(frm), emap)
            return 0
        before = (state(sb), state(db))
        if how == "blobs":
            buf = C.create_string_buffer(len(frm) * src.stream_blob_bytes())
            rc = src.a.BeatriceBatch_ExportStreamsInFlight(src.h, len(frm), bv.iptr(i32(frm)), C.cast(buf, C.c_void_p))
            assert before == (state(sb), state(db)), "an in-flight export changed a tick count, a counter, the blocks owed or a quiescence answer"
            if rc == 0:
                rc = dst.a.BeatriceBatch_ImportStreamsInFlight(dst.h, len(to), bv.iptr(i32(to)), C.cast(buf, C.c_void_p), bv.iptr(em), len(em))
        else:
            rc = src.a.BeatriceBatch_MoveStreamsInFlight(src.h, dst.h, len(frm), bv.iptr(i32(frm)), bv.iptr(i32(to)), bv.iptr(em), len(em))
        assert before == (state(sb), state(db)), "an in-flight move changed a tick count, a counter, the blocks owed or a quiescence answer"
        return rc

    def enter(mode, k0, n):
        for b in "XY":
            batch = batches[b]
            a, h = batch.a, batch.h
            if mode == "D":
                assert a.BeatriceBatch_TickStages(h) == STAGES
                r = Resident(bv, batch, slots=max(n, STAGES + 1), tick=True)
                r.buf[:n] = x[b][k0:k0 + n]
                r.hip.h2d(r.d_in, r.buf)
                assert a.BeatriceBatch_EnableSilentBlockRule(h, 1) == 0
                res[b] = r
            elif mode == "E":
                assert a.BeatriceBatch_EnableHostStreaming(h, 1) == 0
                res[b] = {"done": k0}
            first_of[b] = k0

    def leave(mode, k0, n):
        for b in "XY":
            batch = batches[b]
            a, h = batch.a, batch.h
            if mode == "D":
                r = res.pop(b)
                assert a.BeatriceBatch_Synchronize(h) == 0
                y = np.zeros((r.slots, batch.B, H * 240), np.float32)
                r.hip.d2h(y, r.d_out)
                out[b][k0:k0 + n] = y[:n]
                r.leave()
                assert a.BeatriceBatch_EnableSilentBlockRule(h, 0) == 0
                r.free()
            elif mode == "E":
                e = res.pop(b)
                y = np.zeros((batch.B, H * 240), np.float32)
                while a.BeatriceBatch_StreamFlush(h, bv.fptr(y)) == 1:
                    out[b][e["done"]] = y
                    e["done"] += 1
                assert e["done"] == k0 + n
                assert a.BeatriceBatch_EnableHostStreaming(h, 0) == 0

    def handed(evs, k, mode, late=""):
        for ev, rc in evs:
            want = w.apply(ev)
            got = do(ev, mode)
            if got != want or want != rc:
                problems.append("step %d%s: %s returned %d, the model predicts %d (the scenario holds %d)" % (k, late, ev, got, want, rc))

    try:
        mode = None
        for k in range(steps):
            if k == starts[at[k][0]]:
                if mode is not None:
                    leave(mode, starts[at[k - 1][0]], scn["phases"][at[k - 1][0]][1])
                mode = at[k][1]
                enter(mode, k, scn["phases"][at[k][0]][1])
            w.start_step(k, scn)
            handed(scn["events"][k], k, mode)
            for b in "XY":
                a, h, B = batches[b].a, batches[b].h, batches[b].B
                q = [a.BeatriceBatch_StreamQuiescent(h, s) for s in range(B)]
                busy = [a.BeatriceBatch_SpeakerEntryBusy(h, e) for e in range(ENTRIES)]
                wq, wb = rep["probes"][k][b]
                if q != wq and len(problems) < 8:
                    bad = [s for s in range(B) if q[s] != wq[s]]
                    problems.append("before step %d: StreamQuiescent of %s slots %s is %s, the model says %s" % (k, b, bad[:8], [q[s] for s in bad[:8]], [wq[s] for s in bad[:8]]))
                if busy != wb and len(problems) < 8:
                    problems.append("before step %d: SpeakerEntryBusy of %s is %s, the model says %s" % (k, b, busy, wb))
            for b in "XY":
                batch = batches[b]
                a, h = batch.a, batch.h
                ab = scn["absent"][b][k]
                w.feed(k, scn, b)
                if mode == "D":
                    if ab:
                        assert a.BeatriceBatch_SetSilentStreams(h, bytes(1 if s in ab else 0 for s in range(batch.B))) == 0
                    assert a.BeatriceBatch_ConvertFramesDevice(h, None, None) == 0
                elif mode == "A":
                    out[b][k] = batch.convert(np.ascontiguousarray(x[b][k]))
                else:
                    y = np.zeros((batch.B, H * 240), np.float32)
                    rc = a.BeatriceBatch_StreamFrames(h, bv.fptr(np.ascontiguousarray(x[b][k])), bv.fptr(y))
                    assert rc in (0, 1)
                    if rc == 1:
                        out[b][res[b]["done"]] = y
                        res[b]["done"] += 1
                if mode in "DE":
                    t = a.BeatriceBatch_TicksLaunched(h)
                    if t != w.M[b].tick and len(problems) < 8:
                        problems.append("after step %d: %s has launched %d ticks, the model counts %d (something drained)" % (k, b, t, w.M[b].tick))
            w.absent_now = {b: set() for b in "XY"}
            handed(scn["after"][k], k, mode, " (after the step)")
            for b in "XY":
                if k in drains[b] and mode == "D":
                    assert batches[b].a.BeatriceBatch_Synchronize(batches[b].h) == 0
                w.end_step(k, scn, b)
                if mode == "D":
                    t = batches[b].a.BeatriceBatch_TicksLaunched(batches[b].h)
                    if t != w.M[b].tick and len(problems) < 8:
                        problems.append("behind step %d: %s has launched %d ticks, the model counts %d" % (k, b, t, w.M[b].tick))
        leave(mode, starts[at[steps - 1][0]], scn["phases"][at[steps - 1][0]][1])
        if start_counter:
            for b in "XY":
                end = batches[b].step_counter()
                say("%s %s: step counter %d before, %d after %d steps" % (scenario_id(scn), b, start[b], end, steps))
                assert end == (start[b] + steps) % bv.STEP_WRAP
    finally:
        for r in res.values():
            if hasattr(r, "free"):
                r.free()
        for b in "XY":
            batches[b].close()
        m.close()
    return out, problems


def wrap_starts(bv, scn):
    """start counters that put the wrap inside the scenario, at another step for X than for Y, with a move between the two wraps"""
    moves = [k for k, evs in enumerate(scn["events"]) for ev, rc in evs if ev[0] == "move" and rc == 0]
    k = moves[len(moves) // 2] if moves else len(scn["events"]) // 2
    return {"X": bv.STEP_WRAP - max(k - 1, 1), "Y": bv.STEP_WRAP - min(k + 2, len(scn["events"]) - 1)}


def compare(env, scn, say=print, start_counter=None, references=None):
    """The comparison of tests/test_gpu_scenarios_in_flight.py for one scenario; returns the list of problems (strings, empty = fine)."""
    rep = replay(scn)
    w = rep["world"]
    x = inputs_of(env, scn, w)
    key = scenario_id(scn)
    if references is None or key not in references:
        legs = (run_legs(env, scn, w), run_in_order(env, scn, x))
        if references is not None:
            references[key] = legs
    else:
        legs = references[key]
    want, ref = legs
    got, problems = run_product(env, scn, x, rep, start_counter, say)
    first = None
    for L in scn["legs"]:
        for k, b, s, y in want[L][0]:
            if not np.array_equal(got[b][k, s], y) and (first is None or k < first[0]):
                first = (k, b, s, L, float(np.abs(got[b][k, s] - y).max()))
    if first:
        problems.append("product vs the oracle: first differing (batch, slot, step, logical stream, max-abs) = (%s, %d, %d, %d, %g)\n%s"
                        % (first[1], first[2], first[0], first[3], first[4], stream_story(scn, first[3], first[0], rep)))
    rest = untouched(scn, w)
    for b in "XY":
        bad = [(k, s) for k in range(got[b].shape[0]) for s in rest[b] if not np.array_equal(got[b][k, s], ref[b][k, s])]
        if bad:
            k, s = bad[0]
            problems.append("product vs its in-order chain: first differing (batch, slot, step, max-abs) = (%s, %d, %d, %g)"
                            % (b, s, k, float(np.abs(got[b][k, s] - ref[b][k, s]).max())))
    loud = max([float(np.abs(y).max()) for L in scn["legs"] for _, _, _, y in want[L][0]] or [0.0])
    if not loud > 0.05:
        problems.append("the oracle leg is silence (max-abs %g)" % loud)
    bins = set().union(*[want[L][1] for L in scn["legs"]]) if scn["legs"] else set()
    if len(bins) < 2:
        problems.append("fewer than two distinct raw pitch bins over the whole run: %s" % sorted(bins))
    if not problems:
        say("%s: bit-identical to the oracle (%d logical streams) and to in-order (%d + %d streams); every probe, return code and tick count as "
            "the model says; interactions: %s" % (key, len(scn["legs"]), len(rest["X"]), len(rest["Y"]), ", ".join(sorted(interactions(scn)))))
    return problems


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--seed", type=int, required=True)
    ap.add_argument("--dump", help="write the scenario as json")
    ap.add_argument("--gpu", action="store_true", help="run the two product batches against the oracle and the in-order chain")
    ap.add_argument("--across-the-wrap", action="store_true", help="with --gpu: start counters that put the step counter's wrap inside the scenario")
    args = ap.parse_args(argv)
    listed = {s[0]: s for s in SEEDS}.get(args.seed)
    scn = make_scenario(*(listed or (args.seed, 5, 3, 1, [("D", 50)])))
    if args.dump:
        with open(args.dump, "w") as f:
            json.dump(scn, f)
    rep = replay(scn)
    print("%s, phases %s, chunks %s" % (scenario_id(scn), scn["phases"], scn["chunks"]))
    print("actors %s, bystanders %s, oracle legs %s (%d oracle hops)" % (scn["actors"], scn["bystanders"], scn["legs"], oracle_hops(scn, rep["world"])))
    for k in range(len(scn["events"])):
        if scn["events"][k] or scn["after"][k] or scn["absent"]["X"][k] or scn["absent"]["Y"][k]:
            print("  step %3d: %s%s  sit out: X %s Y %s" % (k, [(e if e[0] != "move" else e[:6], rc) for e, rc in scn["events"][k]],
                                                        "  after: %s" % scn["after"][k] if scn["after"][k] else "", scn["absent"]["X"][k], scn["absent"]["Y"][k]))
    for name, hits in rep["world"].hits.items():
        if hits:
            print("%-48s %s" % (name, [(h["step"], "%s%d" % (h["batch"], h["slot"])) for h in hits][:8]))
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
            make_model.make_model(d, n_speakers=REAL)
            env = Env(bv, bv.Abi(os.path.join(root, "oracle", "libbeatrice_oracle.so")), bv.load_product(), d)
            problems = compare(env, scn, start_counter=wrap_starts(bv, scn) if args.across_the_wrap else None)
        for p in problems:
            print(p)
        return 1 if problems else 0
    return 0


if __name__ == "__main__":
    sys.exit(main())
