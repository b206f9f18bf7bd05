"""BeatriceBatch_InstallSpeakersInFlight / MorphSpeakersInFlight in the wrapper modes around the ticks -- F (BindResidentIO48k), G
(BindResidentBlocks) and P (BindResidentBlocksRagged) -- where they used to drain (csrc/speaker_entry_plan.h; csrc/batch.hip entry_busy).

Every case runs one script three times on the 8-speaker synthetic model with 16 table entries and compares the whole resident output at
max-abs 0: the batch that makes the in-flight calls, twin A, which makes the drained single-entry calls (BeatriceBatch_UpdateSpeaker /
MorphSpeaker) at the same boundaries, and twin B, whose table held the voices from the start.  The script installs two voices and a morph,
moves streams onto them (the k-NN stream proves the codebook), moves a stream off again, asks for the entry while only a step inside the
pipeline still reads it (-3; the twins never ask) and writes it again as soon as BeatriceBatch_SpeakerEntryBusy answers 0.

THE assertion that shows the feature: BeatriceBatch_TicksLaunched and BeatriceBatch_ResidentBlocksOwed read the same before and after every
in-flight call (Checked).  Where the call drains -- every commit before this one -- the tick counter moves.

The busy window is held against the header's rule in ticks: the entry's last name goes at a move followed by BeatriceBatch_FlushSpeaker, so
the stamp counts from the last tick that fed a step -- every tick of these scripts feeds one -- and the entry is busy exactly while
TicksLaunched < that tick + TickStages().  In G at two hops per step the move falls while a step is half filled, a
BeatriceBatch_Synchronize follows it, and the entry must stay busy until the tick that then feeds the filling step + TickStages().  In F
the move is left to the per-hop key/value protocol and the window is D's: the first free poll comes TickStages() calls after the last step
that named the entry (tests/test_gpu_install_in_flight.py)."""
import ctypes as C

import numpy as np
import pytest

import wrapperlib
from test_gpu_install_in_flight import KNN_STREAM, N, S, Api, Voices, i32, make_batch, settings  # noqa: F401
from test_gpu_morph_device import model_dir8  # noqa: F401  (fixture: the 8-speaker synthetic model)
from tick_driver import Hip

pytestmark = pytest.mark.gpu

B, CH = 7, 1
W_M = np.array([0.4, 0.0, 0.35, 0.0, 0.0, 0.25, 0.0, 0.0], np.float32)
RATES = [16000.0, 44100.0, 48000.0, 96000.0]
ZERO_STREAM, ZERO_CALLS = 4, range(3, 10)     # P: this stream hands in n_samples = 0 over an install and a move
T_INSTALL, T_ON, T_MORPH, T_OFF = 5, 7, 12, 20


class Checked(Api):
    """The in-flight calls must launch no tick and run no output half."""

    def _standing(self, fn):
        a, h = self.a, self.h
        before = (a.BeatriceBatch_TicksLaunched(h), a.BeatriceBatch_ResidentBlocksOwed(h))
        rc = fn()
        after = (a.BeatriceBatch_TicksLaunched(h), a.BeatriceBatch_ResidentBlocksOwed(h))
        if self.how == "inflight":
            assert before == after, "an in-flight call moved (TicksLaunched, ResidentBlocksOwed) from %s to %s" % (before, after)
        return rc

    def install(self, entries, voices, raw=False):
        return self._standing(lambda: Api.install(self, entries, voices))

    def morph(self, slot, w):
        return self._standing(lambda: Api.morph(self, slot, w))

    def ticks(self):
        return self.a.BeatriceBatch_TicksLaunched(self.h)

    def flush(self, s):
        assert self.a.BeatriceBatch_FlushSpeaker(self.h, s) == 0


# ---- the three bindings: run(script) -> state with the whole resident output -------------------------------------------------------
def run_F(bv, product, model_dir, H, how, script, calls, state=None, placed=None):
    m = bv.Models(product, model_dir)
    batch = make_batch(bv, m, B, H, placed=placed if how == "preloaded" else None)
    a, h = batch.a, batch.h
    api = Checked(bv, batch, how)
    settings(api)
    st = dict(state or {})
    st["stages"] = a.BeatriceBatch_TickStages(h)
    hip = Hip()
    slots = calls + 2
    x = np.stack([wrapperlib.test_signal(480 * H * calls * CH, 48000, seed=7300 + s) for s in range(B)]).astype(np.float32).reshape(B, calls, H, CH, 480)
    buf = np.zeros((slots, B, H, CH, 480), np.float32)
    buf[:calls] = x.transpose(1, 0, 2, 3, 4)
    d_in, d_out = hip.malloc(buf.nbytes), hip.malloc(buf.nbytes)
    try:
        hip.h2d(d_in, buf)
        assert hip.lib.hipMemset(d_out, 0, C.c_size_t(buf.nbytes)) == 0
        assert a.BeatriceBatch_BindResidentIO48k(h, d_in, d_out, CH, slots) == 0
        for k in range(calls):
            script(api, k, st)
            assert a.BeatriceBatch_ConvertBlocks48kDevice(h, None, None, CH) == 0
        st["ticks"] = a.BeatriceBatch_TicksLaunched(h)
        assert a.BeatriceBatch_Synchronize(h) == 0
        out = np.zeros_like(buf)
        hip.d2h(out, d_out)
        st["out"] = out[:calls].copy()
        batch.close()      # (with the slots still allocated)
    finally:
        hip.free(d_in)
        hip.free(d_out)
        m.close()
    return st


def run_G(bv, product, model_dir, H, how, script, calls, state=None, placed=None):
    sr, block = 44100, 441      # 10 ms: one model hop per call, so at two hops per step every second call feeds a step
    m = bv.Models(product, model_dir)
    batch = make_batch(bv, m, B, H, placed=placed if how == "preloaded" else None)
    a, h = batch.a, batch.h
    api = Checked(bv, batch, how)
    settings(api)
    st = dict(state or {})
    st["stages"] = a.BeatriceBatch_TickStages(h)
    assert a.BeatriceBatch_ConfigureWrapper(h, float(sr)) == 0
    delay = a.BeatriceBatch_ResidentBlocksDelayFor(h, block)
    assert delay > 0
    slots = calls + delay + 2
    hip = Hip()
    x = np.stack([wrapperlib.test_signal(block * calls, sr, seed=7400 + s) for s in range(B)]).astype(np.float32).reshape(B, calls, CH, block)
    buf = np.zeros((slots, B, CH, block), np.float32)
    buf[:calls] = x.transpose(1, 0, 2, 3)
    d_in, d_out = hip.malloc(buf.nbytes), hip.malloc(buf.nbytes)
    try:
        hip.h2d(d_in, buf)
        assert hip.lib.hipMemset(d_out, 0, C.c_size_t(buf.nbytes)) == 0
        assert a.BeatriceBatch_BindResidentBlocks(h, d_in, d_out, CH, block, slots) == 0
        st["fed"] = []       # per call: did it launch a tick
        for k in range(calls):
            script(api, k, st)
            t0 = api.ticks()
            assert a.BeatriceBatch_ProcessBlocksDevice(h, None, None, CH, block) == 0
            st["fed"].append(api.ticks() - t0)
        st["ticks"] = api.ticks()
        assert a.BeatriceBatch_FlushResidentBlocks(h) == 0 and a.BeatriceBatch_ResidentBlocksOwed(h) == 0   # (a fresh or a waiting entry in the table)
        assert a.BeatriceBatch_Synchronize(h) == 0
        out = np.zeros_like(buf)
        hip.d2h(out, d_out)
        st["out"] = out[:calls].copy()
        assert a.BeatriceBatch_BindResidentBlocks(h, None, None, 0, 0, 0) == 0
        batch.close()
    finally:
        hip.free(d_in)
        hip.free(d_out)
        m.close()
    return st


def run_P(bv, product, model_dir, H, how, script, calls, state=None, placed=None):
    assert H == 1
    rates = [RATES[s % 4] for s in range(B)]
    # block lengths differ per stream and per call: 10 to 12 ms, so every call fires a hop of some stream and every tick feeds a step
    length = lambda s, k: 0 if (s == ZERO_STREAM and k in ZERO_CALLS) else int(rates[s] / 100) + ((k + 2 * s) % 3) * int(rates[s] / 1000)   # noqa: E731
    cap = max(length(s, k) for s in range(B) for k in range(calls))
    m = bv.Models(product, model_dir)
    batch = make_batch(bv, m, B, 1, placed=placed if how == "preloaded" else None)
    a, h = batch.a, batch.h
    api = Checked(bv, batch, how)
    settings(api)
    st = dict(state or {})
    st["stages"] = stages = a.BeatriceBatch_TickStages(h)
    assert a.BeatriceBatch_ConfigureWrapperRates(h, (C.c_double * B)(*rates)) == 0
    slots = calls + stages + 2
    hip = Hip()
    buf = np.zeros((slots, B, CH * cap), np.float32)
    for s in range(B):
        sig = wrapperlib.test_signal(sum(length(s, k) for k in range(calls)) + 1, int(rates[s]), seed=7500 + s).astype(np.float32)
        pos = 0
        for k in range(calls):
            n = length(s, k)
            buf[k, s, :n] = sig[pos:pos + n]
            pos += n
    d_in, d_out = hip.malloc(buf.nbytes), hip.malloc(buf.nbytes)
    try:
        hip.h2d(d_in, buf)
        assert hip.lib.hipMemset(d_out, 0, C.c_size_t(buf.nbytes)) == 0
        assert a.BeatriceBatch_BindResidentBlocksRagged(h, d_in, d_out, CH, cap, slots) == 0
        st["fed"] = []
        for k in range(calls):
            script(api, k, st)
            t0 = api.ticks()
            assert a.BeatriceBatch_ProcessBlocksRaggedDevice(h, (C.c_int * B)(*[length(s, k) for s in range(B)])) == 0
            st["fed"].append(api.ticks() - t0)
        st["ticks"] = api.ticks()
        assert a.BeatriceBatch_Synchronize(h) == 0 and a.BeatriceBatch_ResidentBlocksOwed(h) == 0
        out = np.zeros_like(buf)
        hip.d2h(out, d_out)
        st["out"] = out[:calls].copy()
        assert a.BeatriceBatch_BindResidentBlocksRagged(h, None, None, 0, 0, 0) == 0
        batch.close()
    finally:
        hip.free(d_in)
        hip.free(d_out)
        m.close()
    return st


RUN = {"F": run_F, "G": run_G, "P": run_P}


# ---- the script ---------------------------------------------------------------------------------------------------------------------
def make_script(mode, H, extras=False):
    """Entries 8, 9: voices 0, 1 installed before call 5, streams 0 and 1 (the k-NN stream) on them from call 7; entry 12: a morph made
    before call 12 with stream 2 on it; stream 0 leaves entry 8 before call T_OFF (G at two hops per step: before the first call from
    there on that finds a step half filled); entry 8 -- in twin B entry 11, which held voice 5 from the start -- takes voice 5 and the k-NN
    stream as soon as it is free."""
    flush_moves = mode != "F"       # F: the move off is left to the per-hop protocol, the window is D's

    def script(api, k, st):
        inflight = api.how == "inflight"
        a, h = api.a, api.h
        if extras and k == T_INSTALL - 1:       # a reset / restart still travelling when the install comes
            if mode == "F":
                assert a.BeatriceBatch_ResetStreamInFlight(h, 6) == 0
            if mode == "P":
                assert a.BeatriceBatch_RestartStreamInFlight(h, 5, 0.0, 1) == 0
        if k == T_INSTALL:
            assert api.install([8, 9], [0, 1]) == 0
        if k == T_INSTALL + 1 and mode == "G":  # a fresh entry nobody names yet, across a drained point
            assert a.BeatriceBatch_Synchronize(h) == 0
            if inflight:
                assert api.busy(8) == 0 and api.busy(9) == 0
        if k == T_ON:
            api.move([0, 1], [8, 9])
        if k == T_MORPH:
            assert api.morph(12, W_M) == 0
            api.move([2], [12])
        # the move off
        if inflight and st.get("off_at") is None and k >= T_OFF and (mode != "G" or H == 1 or st["fed"][k - 1] == 0):
            st["off_at"] = k
        if k == st.get("off_at"):
            if inflight:
                assert api.busy(8) == 1
            api.move([0], [3])
            if flush_moves:
                api.flush(0)
                if mode == "G" and H > 1:       # the step still filling survives a drained point, and so does the entry's wait for it
                    assert a.BeatriceBatch_Synchronize(h) == 0
                    if inflight:
                        assert api.busy(8) == 1, "entry 8 was freed by a drain while the step that may read it is still filling"
                if inflight:
                    # every tick of these scripts feeds a step: the stamp's base is the last tick launched -- or, with a step filling,
                    # the next one, which feeds it
                    st["bound"] = api.ticks() + st["stages"] - (0 if mode == "G" and H > 1 else 1)
        if inflight and st.get("off_at") is not None and k > st["off_at"] and st.get("reuse_at") is None:
            busy = api.busy(8)
            st.setdefault("polls", []).append((k, api.ticks(), busy))
            if busy == 1 and k in (st["off_at"] + 3, st["off_at"] + 9):
                assert api.install([8], [5]) == -3 and api.install([10, 8], [5, 6]) == -3     # nothing changes: the twins never ask
                assert api.morph(8, W_M) == -3
            if busy == 0:
                st["reuse_at"] = k
        if k == st.get("reuse_at"):
            e = 11 if api.how == "preloaded" else 8
            assert api.install([e], [5]) == 0
            api.move([KNN_STREAM], [e])
            if flush_moves:
                api.flush(KNN_STREAM)
    return script


PLACED = {8: 0, 9: 1, 11: 5}


def last_step_naming_8(H, steps, off_at):
    """tests/test_gpu_install_in_flight.py: the last step in which stream 0 names entry 8 under the reference's per-hop protocol."""
    target, kv, count, last = 0, [0] * 4, 4, -1
    for k in range(steps):
        if k in (T_ON, off_at):
            target, count = {T_ON: 8, off_at: 3}[k], 0
        for _ in range(H):
            if count < 4:
                kv[count] = target
                count += 1
            if 8 in [target] + kv:
                last = k
    return last


def check(bv, product, model_dir, mode, H, calls, extras=False):
    script = make_script(mode, H, extras)
    got = RUN[mode](bv, product, model_dir, H, "inflight", script, calls)
    print("%s H=%d: off at call %s, bound %s, polls %s, reuse at %s, ticks %d" % (mode, H, got.get("off_at"), got.get("bound"), got.get("polls"),
                                                                                   got.get("reuse_at"), got["ticks"]))
    assert got.get("off_at") is not None and got.get("reuse_at") is not None, "entry 8 never became free: %s" % got.get("polls")
    stages, polls = got["stages"], got["polls"]
    if mode == "F":
        # one feeding tick per call and nothing drained: ticks are calls, and the window is D's
        assert got["ticks"] == calls
        last = last_step_naming_8(H, calls, got["off_at"])
        assert got["reuse_at"] == last + stages, "first free call %d, predicted %d + %d: %s" % (got["reuse_at"], last, stages, polls)
    else:
        assert all(f >= 1 for f in got["fed"][T_OFF - 2:]) if (mode == "P" or H == 1) else sum(got["fed"]) >= calls // H - 1, got["fed"]
        for (k, ticks, busy) in polls:
            assert busy == (1 if ticks < got["bound"] else 0), "call %d, %d ticks launched, bound %d: busy %d; %s" % (k, ticks, got["bound"], busy, polls)
        assert any(busy == 1 for (_, _, busy) in polls) and polls[-1][2] == 0
    keys = {"off_at": got["off_at"], "reuse_at": got["reuse_at"]}
    twin_a = RUN[mode](bv, product, model_dir, H, "drained", script, calls, state=keys)
    twin_b = RUN[mode](bv, product, model_dir, H, "preloaded", script, calls, state=keys, placed=PLACED)
    assert np.abs(twin_a["out"]).max() > 0.05
    assert twin_a["ticks"] > got["ticks"]          # every drained call costs ticks
    print("%s H=%d: max-abs vs the drained twin %g, vs the preloaded twin %g" % (
        mode, H, float(np.abs(got["out"] - twin_a["out"]).max()), float(np.abs(got["out"] - twin_b["out"]).max())))
    assert np.array_equal(twin_a["out"], twin_b["out"]), "the twins disagree: max-abs %g" % float(np.abs(twin_a["out"] - twin_b["out"]).max())
    assert np.array_equal(got["out"], twin_a["out"]), "in flight vs the drained twin: max-abs %g" % float(np.abs(got["out"] - twin_a["out"]).max())


@pytest.mark.parametrize("H", [1, 2, 4])
def test_48k_blocks_around_the_ticks(bv, product, model_dir8, H):
    check(bv, product, model_dir8, "F", H, 70)


def test_blocks_with_clocks_per_stream(bv, product, model_dir8):
    check(bv, product, model_dir8, "P", 1, 70)


@pytest.mark.parametrize("H,calls", [(1, 70), (2, 110)])
def test_any_rate_blocks_with_one_set_of_clocks(bv, product, model_dir8, H, calls):
    check(bv, product, model_dir8, "G", H, calls)


@pytest.mark.parametrize("mode", ["F", "P"])
def test_a_reset_or_restart_travelling_around_the_install(bv, product, model_dir8, mode):
    """F: BeatriceBatch_ResetStreamInFlight of a stream, P: BeatriceBatch_RestartStreamInFlight(reset_model = 1), one call in front of the
    install, so that it is still travelling when the tables are written; the drained twin drains in the middle of it."""
    check(bv, product, model_dir8, mode, 1, 70, extras=True)


# ---- a stream moved between two F batches onto a freshly installed entry ------------------------------------------------------------
MB, N1 = 3, 4       # streams per batch; the steps the source's stream 1 makes before it falls silent


def run_move(bv, product, model_dir, how, state=None):
    """Batches X and Y, both bound to resident 48 kHz blocks with the silent-block rule on.  X's stream 1 (the k-NN stream) makes N1 steps
    and sits out until it is at rest; Y's stream 0 never takes part.  Before call T: voice 0 goes into entry 8 of BOTH tables (Y also gets
    entry 9) while both pipelines are full, X's stream is pointed at entry 8, and BeatriceBatch_MoveStreams48kInFlight carries it into
    Y's slot 0 -- entry numbers travel in the destination's numbering, so Y's entry 8 is named from the import on.  Y's stream 0 then goes
    on with the stream's material, leaves entry 8 six calls later, and the entry is written again as soon as it is free."""
    m = bv.Models(product, model_dir)
    X = make_batch(bv, m, MB, 1, placed=PLACED if how == "preloaded" else None)
    Y = make_batch(bv, m, MB, 1, placed=PLACED if how == "preloaded" else None)
    ax, ay = Checked(bv, X, how), Checked(bv, Y, how)
    settings(ax)
    settings(ay)
    inflight = how == "inflight"
    st = dict(state or {})
    st["stages"] = stages = ay.a.BeatriceBatch_TickStages(ay.h)
    T, calls = N1 + stages + 1, N1 + stages + 1 + 6 + stages + 8
    t_off = T + 6
    hip, slots = Hip(), calls + 2
    sig = lambda seed: wrapperlib.test_signal(480 * calls, 48000, seed=seed).astype(np.float32).reshape(calls, 480)   # noqa: E731
    xin, yin = np.zeros((slots, MB, 1, CH, 480), np.float32), np.zeros((slots, MB, 1, CH, 480), np.float32)
    moved = sig(7601)
    for s in range(MB):
        xin[:calls, s, 0, 0] = sig(7600 + s)
        yin[:calls, s, 0, 0] = sig(7610 + s)
    xin[N1:, 1] = 0                                  # X's stream 1 sits out from step N1 on ...
    yin[:, 0] = 0
    yin[T:calls, 0, 0, 0] = moved[N1:N1 + calls - T]  # ... and goes on as Y's stream 0 from step T
    bufs = [hip.malloc(xin.nbytes) for _ in range(4)]
    try:
        for (api, d_in, d_out, buf) in ((ax, bufs[0], bufs[1], xin), (ay, bufs[2], bufs[3], yin)):
            hip.h2d(d_in, buf)
            assert hip.lib.hipMemset(d_out, 0, C.c_size_t(buf.nbytes)) == 0
            assert api.a.BeatriceBatch_BindResidentIO48k(api.h, d_in, d_out, CH, slots) == 0
            assert api.a.BeatriceBatch_EnableSilentBlockRule(api.h, 1) == 0
        for k in range(calls):
            if k == T:
                if inflight:
                    assert ax.a.BeatriceBatch_Stream48kQuiescent(ax.h, 1) == 1 and ay.a.BeatriceBatch_Stream48kQuiescent(ay.h, 0) == 1
                    assert ay.busy(8) == 0
                assert ax.install([8], [0]) == 0 and ay.install([8, 9], [0, 1]) == 0
                ax.move([1], [8])
                ax.flush(1)
                if inflight:
                    assert ay.busy(8) == 0 and ay.busy(9) == 0          # written, and nobody names them yet
                before = (ax.ticks(), ay.ticks())
                X.move_streams48k_in_flight(Y, [1], [0])
                assert before == (ax.ticks(), ay.ticks())
                if inflight:
                    assert ay.busy(8) == 1 and ay.busy(9) == 0, "the import's names did not reach the counts"
                    assert ay.install([8], [5]) == -3 and ax.install([8], [5]) == -3
            if k == t_off:
                ay.move([0], [3])
                ay.flush(0)
                if inflight:
                    st["bound"] = ay.ticks() + stages - 1          # (every tick of Y feeds a step: its streams 1 and 2 never sit out)
            if inflight and k > t_off and st.get("reuse_at") is None:
                busy = ay.busy(8)
                st.setdefault("polls", []).append((k, ay.ticks(), busy))
                if busy == 1 and k == t_off + 5:
                    assert ay.install([8], [5]) == -3
                if busy == 0:
                    st["reuse_at"] = k
            if k == st.get("reuse_at"):
                e = 11 if how == "preloaded" else 8
                assert ay.install([e], [5]) == 0
                ay.move([0], [e])
                ay.flush(0)
            if k >= N1:
                assert ax.a.BeatriceBatch_SetSilentStreams(ax.h, bytes([0, 1, 0])) == 0
            if k < T:
                assert ay.a.BeatriceBatch_SetSilentStreams(ay.h, bytes([1, 0, 0])) == 0
            assert ax.a.BeatriceBatch_ConvertBlocks48kDevice(ax.h, None, None, CH) == 0
            assert ay.a.BeatriceBatch_ConvertBlocks48kDevice(ay.h, None, None, CH) == 0
        st["ticks"] = (ax.ticks(), ay.ticks())
        outs = []
        for (api, d_out) in ((ax, bufs[1]), (ay, bufs[3])):
            assert api.a.BeatriceBatch_Synchronize(api.h) == 0
            out = np.zeros_like(xin)
            hip.d2h(out, d_out)
            outs.append(out[:calls].copy())
        st["out"], st["calls"], st["T"] = np.stack(outs), calls, T
        X.close()
        Y.close()
    finally:
        for p in bufs:
            hip.free(p)
        m.close()
    return st


def test_a_stream_moved_between_two_48k_batches_onto_a_fresh_entry(bv, product, model_dir8):
    got = run_move(bv, product, model_dir8, "inflight")
    print("move: bound %s, polls %s, reuse at %s, ticks %s" % (got.get("bound"), got.get("polls"), got.get("reuse_at"), got["ticks"]))
    assert got.get("reuse_at") is not None, got.get("polls")
    assert got["ticks"] == (got["calls"], got["calls"])            # nothing drained in either batch
    for (k, ticks, busy) in got["polls"]:
        assert busy == (1 if ticks < got["bound"] else 0), "call %d, %d ticks launched, bound %d: busy %d" % (k, ticks, got["bound"], busy)
    assert any(busy == 1 for (_, _, busy) in got["polls"])
    keys = {"reuse_at": got["reuse_at"]}
    twin_a = run_move(bv, product, model_dir8, "drained", state=keys)
    twin_b = run_move(bv, product, model_dir8, "preloaded", state=keys)
    assert twin_a["ticks"][0] > got["ticks"][0] and twin_a["ticks"][1] > got["ticks"][1]
    assert np.abs(twin_a["out"][1, got["T"] + 2:, 0]).max() > 0.05  # the moved stream is heard in Y's slot 0
    print("move: max-abs vs the drained twin %g, vs the preloaded twin %g" % (
        float(np.abs(got["out"] - twin_a["out"]).max()), float(np.abs(got["out"] - twin_b["out"]).max())))
    assert np.array_equal(twin_a["out"], twin_b["out"]), "the twins disagree: max-abs %g" % float(np.abs(twin_a["out"] - twin_b["out"]).max())
    assert np.array_equal(got["out"], twin_a["out"]), "in flight vs the drained twin: max-abs %g" % float(np.abs(got["out"] - twin_a["out"]).max())
