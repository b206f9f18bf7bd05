"""BeatriceBatch_StreamQuiescent / ExportStreamsInFlight / ImportStreamsInFlight / MoveStreamsInFlight: a stream leaves one batch in plain
tick mode and goes on in another while BOTH go on ticking -- nothing drains, no tick is launched, nobody else is disturbed.

Yardsticks, all at max-abs 0, those of tests/test_gpu_stream_migration.py (whose oracle runs, computed once, are shared): one OracleBatch
stream that simply keeps running -- a stream's k-th PRESENT step is the oracle's step k, wherever and whenever it is made -- and, where the
oracle has no leg, a twin product batch.  Source batches have 3 streams, destination batches 2, unless a case is about the size;
N1 = N2 = 20 steps; between the two the moving stream sits out TickStages() - 1 steps while its neighbours go on with their own audio.

The driver (Flow) gives every step of a run its own resident slot, uploads all input before the first step, feeds WITHOUT synchronising
and reads the output ring back at the very end after one BeatriceBatch_Synchronize: a drain in between would hide everything these calls
are about, so every step fed asserts BeatriceBatch_TicksLaunched == steps fed."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_mode_matrix as mode_matrix
import wrapperlib
from test_gpu_stream_migration import N1, N2, _free_bytes, models, oracle_models, oracle_run, run_in_order, settings_script  # noqa: F401
from tick_driver import Resident

pytestmark = pytest.mark.gpu

WRAP = 12252240   # BEATRICE_HIP_STEP_WRAP
_audio = {}


def audio(bv, seed, H):
    """one stream's input, [80][H * 160]: the prefix of it is what oracle_run feeds"""
    if (seed, H) not in _audio:
        _audio[(seed, H)] = bv.synth_audio(160 * H * 80, seed=seed).reshape(80, H * 160)
    return _audio[(seed, H)]


def i32(v):
    return np.ascontiguousarray(v, np.int32).ctypes.data_as(C.POINTER(C.c_int))


class Flow:
    """A batch in plain tick mode with the silent-block rule, n_steps steps planned in advance.  Stream s consumes the audio of its
    current source (seed, next index) at every step it is present in; sit_out() and feed_from() edit the plan before start()."""

    def __init__(self, bv, batch, seeds, n_steps):
        self.bv, self.batch, self.n = bv, batch, n_steps
        self.S = batch.a.BeatriceBatch_TickStages(batch.h)
        self.out = np.zeros((n_steps, batch.B), np.uint8)
        self.sources = {s: [(0, seeds[s], 0)] for s in range(batch.B)}
        self.scripts = {}   # stream -> script(a, h, s, k), k = the index of the stream's own step (test_gpu_stream_migration's scripts)
        self.r, self.fed = None, 0

    def sit_out(self, s, k0, k1):
        self.out[k0:k1, s] = 1

    def feed_from(self, s, k, seed, idx):
        self.sources[s].append((k, seed, idx))

    def start(self):
        b, H = self.batch, self.batch.H
        x = np.zeros((self.n, b.B, H * 160), np.float32)
        self.took = {s: [] for s in range(b.B)}   # (step, seed, index) of every present step
        for s in range(b.B):
            seg = sorted(self.sources[s])
            seed = idx = None
            for k in range(self.n):
                while seg and seg[0][0] <= k:
                    _, seed, idx = seg.pop(0)
                if not self.out[k, s]:
                    x[k, s] = audio(self.bv, seed, H)[idx]
                    self.took[s].append((k, seed, idx))
                    idx += 1
        self.r = Resident(self.bv, b, slots=max(self.n, self.S + 1), tick=True)
        self.r.buf[:self.n] = x
        self.r.hip.h2d(self.r.d_in, self.r.buf)
        assert b.a.BeatriceBatch_EnableSilentBlockRule(b.h, 1) == 0
        self.idx_at = {(k, s): i for s in self.took for (k, _, i) in self.took[s]}
        return self

    def ticks(self):
        return self.batch.a.BeatriceBatch_TicksLaunched(self.batch.h)

    def run_to(self, k_end):
        a, h = self.batch.a, self.batch.h
        for k in range(self.fed, k_end):
            for s, script in self.scripts.items():
                if (k, s) in self.idx_at:
                    script(a, h, s, self.idx_at[(k, s)])
            if self.out[k].any():
                assert a.BeatriceBatch_SetSilentStreams(h, self.out[k].tobytes()) == 0
            assert a.BeatriceBatch_ConvertFramesDevice(h, None, None) == 0
            self.fed += 1
            assert self.ticks() == self.fed   # one tick per step: nothing has drained
        return self

    def finish(self):
        self.run_to(self.n)
        a, h = self.batch.a, self.batch.h
        assert self.ticks() == self.n
        assert a.BeatriceBatch_Synchronize(h) == 0
        y = np.zeros((self.r.slots, self.batch.B, self.batch.H * 240), np.float32)
        self.r.hip.d2h(y, self.r.d_out)
        self.y = y[:self.n]
        self.y[self.out.astype(bool)] = 0   # (a step sat out writes nothing: its row of the slot is whatever the allocation held)
        return self

    def heard(self, s, seed):
        """(audio indices, samples) of the steps stream s made on `seed`'s audio"""
        rows = [(k, i) for (k, sd, i) in self.took[s] if sd == seed]
        return [i for _, i in rows], self.y[[k for k, _ in rows], s]

    def quiescent(self, s):
        return self.batch.a.BeatriceBatch_StreamQuiescent(self.batch.h, s)

    def state(self):
        a, h = self.batch.a, self.batch.h
        return (self.ticks(), a.BeatriceBatch_StepCounter(h), tuple(self.quiescent(s) for s in range(self.batch.B)))

    def free(self):
        if self.r is not None:
            self.r.free()


class Env:
    def __init__(self, bv, oracle, oracle_models, model_dir, models):
        self.bv, self.oracle, self.oracle_models, self.model_dir, self.models = bv, oracle, oracle_models, model_dir, models

    def want(self, H, seed, steps, script=None, key=None):
        return oracle_run(self.bv, self.oracle, self.oracle_models, self.model_dir, H, seed, steps, script, key)

    def check(self, flow, s, seed, script=None, key=None, what=""):
        idx, got = flow.heard(s, seed)
        assert len(idx) > 0
        want = self.want(flow.batch.H, seed, max(idx) + 1, script, key)[idx]
        assert np.abs(want).max() > 1e-3
        bad = [i for i, (g, w) in zip(idx, zip(got, want)) if not np.array_equal(g, w)]
        assert not bad, "%s stream %d on audio %d: steps %s differ" % (what, s, seed, bad)


@pytest.fixture
def env(bv, product, oracle, models, oracle_models, model_dir):
    return Env(bv, oracle, oracle_models, model_dir, models)


def vq1(a, h, s, k):
    """a neighbour that keeps the k-NN stage on from the first step, so that no stream's VQ setting makes the stage come or go (that drains)"""
    if k == 0:
        assert a.BeatriceBatch_SetVQNumNeighbors(h, s, 1) == 0


def export_in_flight(batch, streams):
    before = (batch.a.BeatriceBatch_TicksLaunched(batch.h), batch.a.BeatriceBatch_StepCounter(batch.h))
    blob = batch.export_streams_in_flight(streams)
    assert before == (batch.a.BeatriceBatch_TicksLaunched(batch.h), batch.a.BeatriceBatch_StepCounter(batch.h))
    return blob


def carry(how, src, dst, frm, to, entry_map=None):
    """the move itself, by the blob pair or device to device"""
    if how == "blobs":
        dst.import_streams_in_flight(to, export_in_flight(src, frm), entry_map)
    else:
        src.move_streams_in_flight(dst, frm, to, entry_map)


class Walk:
    """The walk every case is a variation of.  Source: N1 steps of everyone, then stream 1 sits out S - 1 steps, then N2 steps of
    everyone again (the source is unchanged by the move: fed again, the stream goes on).  Destination: slot 0 takes part in `dst_first`
    steps on its own audio, then sits out S - 1 + d steps while its batch runs on -- its own counter lags the batch's by that much --, takes
    the stream in and makes N2 steps on the stream's audio."""

    def __init__(self, env, H, d=1, dst_first=5, src_kw=None, dst_kw=None, Bs=3, Bd=2, tail=0):
        bv, self.env = env.bv, env
        self.src_b = bv.Batch(env.models, Bs, hops_per_step=H, **(src_kw or {}))
        self.dst_b = bv.Batch(env.models, Bd, hops_per_step=H, **(dst_kw or {}))
        S = self.src_b.a.BeatriceBatch_TickStages(self.src_b.h)
        self.S, self.H = S, H
        self.at_src, self.at_dst = N1 + S - 1, dst_first + S - 1 + d
        self.src = Flow(bv, self.src_b, [100 + s for s in range(Bs)], self.at_src + N2)
        self.dst = Flow(bv, self.dst_b, [110 + s for s in range(Bd)], self.at_dst + N2 + tail)
        self.src.sit_out(1, N1, self.at_src)
        self.dst.sit_out(0, dst_first, self.at_dst)
        self.dst.feed_from(0, self.at_dst, 101, N1)

    def start(self):
        self.src.start()
        self.dst.start()
        return self

    def to_the_move(self):
        self.src.run_to(self.at_src)
        self.dst.run_to(self.at_dst)
        return self

    def check(self, script=None, key=None, src_scripts=None, dst_scripts=None):
        e, src, dst = self.env, self.src, self.dst
        e.check(src, 1, 101, script, key, "source")        # before the move, and fed again after it
        assert max(src.heard(1, 101)[0]) == N1 + N2 - 1
        e.check(dst, 0, 101, script, key, "destination")   # the moved stream's N2 steps
        assert dst.heard(0, 101)[0][:N2] == list(range(N1, N1 + N2))
        if dst.heard(0, 110)[0]:
            e.check(dst, 0, 110, *(dst_scripts or {}).get(0, ()), what="destination, the slot's first user")
        for s in range(src.batch.B):
            if s != 1:
                e.check(src, s, 100 + s, *(src_scripts or {}).get(s, ()), what="source")
        for s in range(1, dst.batch.B):
            e.check(dst, s, 110 + s, *(dst_scripts or {}).get(s, ()), what="destination")

    def close(self):
        self.src.free()
        self.dst.free()
        self.src_b.close()
        self.dst_b.close()


# ---- 1. the blob pair, counters apart -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,d", [(1, 1), (1, 6), (2, 1), (2, 6), (4, 1)])
def test_the_blob_pair_moves_a_stream_between_ticking_batches(env, H, d):
    """The destination slot's own counter is 5, its batch's 5 + S - 1 + d: turning by the batch's counter would put every ring of more
    than one slot out of place (S - 1 + d is no multiple of 17)."""
    w = Walk(env, H, d)
    try:
        w.start().to_the_move()
        assert (w.S - 1 + d) % 17 != 0
        assert w.src.quiescent(1) == 1 and w.src.quiescent(0) == 0 and w.dst.quiescent(0) == 1 and w.dst.quiescent(1) == 0
        before = (w.src.state(), w.dst.state())
        carry("blobs", w.src_b, w.dst_b, [1], [0])
        assert before == (w.src.state(), w.dst.state())
        w.dst.finish()
        w.src.finish()
        w.check()
    finally:
        w.close()


# ---- 2. device to device ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("one_stream", [False, True], ids=["each batch on its own stream", "both on one caller-made stream"])
def test_the_device_to_device_move(env, one_stream):
    hip = C.CDLL("libamdhip64.so")
    made = C.c_void_p()
    w = Walk(env, 2, 1)
    try:
        if one_stream:
            assert hip.hipStreamCreateWithFlags(C.byref(made), 1) == 0
            for b in (w.src_b, w.dst_b):
                assert b.a.BeatriceBatch_SetStream(b.h, made) == 0
        w.start().to_the_move()
        before = (w.src.state(), w.dst.state())
        carry("move", w.src_b, w.dst_b, [1], [0])
        assert before == (w.src.state(), w.dst.state())
        w.dst.finish()
        w.src.finish()
        w.check()
    finally:
        w.close()
        if made:
            hip.hipStreamDestroy(made)


# ---- 3. the quiescence boundary -------------------------------------------------------------------------------------------------------------
def test_the_quiescence_boundary(env):
    """One tick too early everything is refused with -3 and nothing changes (a twin that was never asked); one tick later the move goes
    through.  The destination slot never took part since tick mode was entered: it is at rest from the start."""
    H = 1
    w, twin = Walk(env, H, 1, dst_first=0), Walk(env, H, 1, dst_first=0)
    try:
        w.start()
        twin.start()
        a, size = w.src_b.a, w.src_b.stream_blob_bytes()
        w.dst.run_to(1)
        assert w.dst.quiescent(0) == 1 and w.dst.quiescent(1) == 0
        w.dst.run_to(w.at_dst)
        good = export_in_flight(w.dst_b, [0])   # (a blob to offer: the destination slot's own, at rest)
        w.src.run_to(w.at_src - 1)              # S - 2 sat-out ticks
        assert w.src.quiescent(1) == 0
        out = C.create_string_buffer(size)
        before = (w.src.state(), w.dst.state())
        assert a.BeatriceBatch_ExportStreamsInFlight(w.src_b.h, 1, i32([1]), C.cast(out, C.c_void_p)) == -3
        assert a.BeatriceBatch_ImportStreamsInFlight(w.src_b.h, 1, i32([1]), C.cast(C.create_string_buffer(good, size), C.c_void_p), None, 0) == -3
        assert a.BeatriceBatch_MoveStreamsInFlight(w.src_b.h, w.dst_b.h, 1, i32([1]), i32([0]), None, 0) == -3
        assert a.BeatriceBatch_MoveStreamsInFlight(w.dst_b.h, w.src_b.h, 1, i32([0]), i32([1]), None, 0) == -3   # ... as a destination too
        assert before == (w.src.state(), w.dst.state())
        w.src.run_to(w.at_src)                  # one tick later
        assert w.src.quiescent(1) == 1
        for t in (w.src, w.dst, twin.src, twin.dst):
            t.finish()                          # nothing is moved yet: N2 more steps of both pairs, bit for bit the same
        assert np.array_equal(w.src.y, twin.src.y) and np.array_equal(w.dst.y, twin.dst.y)
        assert np.abs(twin.src.y).max() > 1e-3
    finally:
        w.close()
        twin.close()
    w = Walk(env, H, 1, dst_first=0)
    try:
        w.start().to_the_move()
        assert w.src.quiescent(1) == 1
        carry("move", w.src_b, w.dst_b, [1], [0])
        w.dst.finish()
        w.src.finish()
        w.check()
    finally:
        w.close()


# ---- 4. pending installs and every setting --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,how", [(1, "blobs"), (2, "move")])
def test_pending_installs_and_every_setting_travel(env, H, how):
    """test_gpu_stream_migration's settings walk: the speaker switch two hops before the stream's last present step, two key/value blocks
    still to come -- they install one per hop in the destination.  The destination holds the voices in the order (2, 0, 1)."""
    bv, t = env.bv, env.models.tables
    order, entry_map = [2, 0, 1, 3], [1, 2, 0, 3]   # destination entry i holds the source's entry order[i]; source entry v sits at entry_map[v]
    w = Walk(env, H, 1, dst_kw=dict(max_speakers=t.n_speakers + 1, upload_tables=False))
    try:
        cb, add, kv = (np.ascontiguousarray(x[order]) for x in (t.codebooks, t.additive, t.kv))
        dst = w.dst_b
        assert dst.a.BeatriceBatch_SetSpeakerTables(dst.h, t.n_speakers + 1, bv.fptr(cb), bv.fptr(add), bv.fptr(t.formant), bv.fptr(kv)) == 0
        dst.apply_defaults()   # (every stream on the destination's entry 0: the source's voice 2)
        script = settings_script(H)

        def voice2_vq1(a, h, s, k):   # what the destination's streams are, in the oracle's terms (its tables are in the source's order)
            if k == 0 and h is None:
                assert a.BeatriceBatch_SetTargetSpeaker(h, s, 2) == 0 and a.BeatriceBatch_FlushSpeaker(h, s) == 0
            vq1(a, h, s, k)
        w.src.scripts = {0: vq1, 1: script}
        w.dst.scripts = {0: voice2_vq1, 1: voice2_vq1}
        w.start().to_the_move()
        carry(how, w.src_b, w.dst_b, [1], [0], entry_map)
        w.dst.finish()
        w.src.finish()
        plain = env.want(H, 101, N1 + N2)
        moved = env.want(H, 101, N1 + N2, script, "settings")
        assert not np.array_equal(moved[N1:], plain[N1:])   # (the settings are audible)
        both = (voice2_vq1, "voice 2 and one neighbour from the start")
        w.check(script, "settings", src_scripts={0: (vq1, "one neighbour from the start")}, dst_scripts={0: both, 1: both})
    finally:
        w.close()


# ---- 5. the lottery (twin) ----------------------------------------------------------------------------------------------------------------
def test_the_lottery_engine_continues_its_sequence(env):
    bv, H = env.bv, 1
    wgt = np.array([0.5, 0.5, 0.0], np.float32)

    def on_the_morph(a, h, s, k):
        if k == 0:
            assert a.BeatriceBatch_SetTargetSpeaker(h, s, 3) == 0 and a.BeatriceBatch_SetVQNumNeighbors(h, s, 2) == 0

    twin = bv.Batch(env.models, 3)
    try:
        assert twin.a.BeatriceBatch_MorphSpeaker(twin.h, 3, bv.fptr(wgt), 3, 7) == 0
        xs = np.ascontiguousarray(np.stack([audio(bv, 100 + s, H)[:N1 + N2] for s in range(3)]).transpose(1, 0, 2))
        stayed = run_in_order(twin, xs, {1: on_the_morph})[:, 1]   # never moved, never sat out
    finally:
        twin.close()
    w = Walk(env, H, 1)
    try:
        for b in (w.src_b, w.dst_b):
            assert b.a.BeatriceBatch_MorphSpeaker(b.h, 3, bv.fptr(wgt), 3, 7) == 0
        w.src.scripts = {1: on_the_morph}
        w.dst.scripts = {1: vq1}
        w.start().to_the_move()
        carry("blobs", w.src_b, w.dst_b, [1], [0])
        w.dst.finish()
        w.src.finish()
        assert np.abs(stayed[N1:]).max() > 1e-3
        idx, got = w.dst.heard(0, 101)
        assert idx == list(range(N1, N1 + N2)) and np.array_equal(got, stayed[N1:])
        idx, got = w.src.heard(1, 101)
        assert np.array_equal(got, stayed[idx])   # the export drew nothing from the source's engine either
        env.check(w.src, 0, 100, what="source")
        env.check(w.src, 2, 102, what="source")
        env.check(w.dst, 1, 111, vq1, "one neighbour from the start", what="destination")
    finally:
        w.close()


# ---- 6. a reset in flight ---------------------------------------------------------------------------------------------------------------------
def test_a_pending_reset_refuses_the_source_and_is_cancelled_on_the_destination(env):
    H = 1
    w = Walk(env, H, 1)
    try:
        w.start().to_the_move()
        a, size = w.src_b.a, w.src_b.stream_blob_bytes()
        blob = export_in_flight(w.src_b, [1])
        assert a.BeatriceBatch_ResetStreamInFlight(w.src_b.h, 1) == 0 and a.BeatriceBatch_ResetStreamInFlight(w.dst_b.h, 0) == 0
        out = C.create_string_buffer(size)
        before = (w.src.state(), w.dst.state())
        assert a.BeatriceBatch_ExportStreamsInFlight(w.src_b.h, 1, i32([1]), C.cast(out, C.c_void_p)) == -3
        assert a.BeatriceBatch_MoveStreamsInFlight(w.src_b.h, w.dst_b.h, 1, i32([1]), i32([0]), None, 0) == -3
        assert before == (w.src.state(), w.dst.state())
        w.dst_b.import_streams_in_flight([0], blob)   # cancels the reset waiting on the slot
        w.dst.finish()
        w.src.finish()
        env.check(w.dst, 0, 101, what="destination")    # the oracle's next step, not a first step
        env.check(w.dst, 0, 110, what="destination, the slot's first user")
        env.check(w.dst, 1, 111, what="destination")
        env.check(w.src, 0, 100, what="source")
        env.check(w.src, 2, 102, what="source")
        idx, got = w.src.heard(1, 101)                  # the source's own reset did happen: its next steps are a new stream's
        want = env.want(H, 101, N1 + N2)
        assert np.array_equal(got[:N1], want[:N1]) and not np.array_equal(got[N1:], want[N1:])
    finally:
        w.close()


# ---- 7. afterwards the batch is an ordinary batch ---------------------------------------------------------------------------------------------
def test_afterwards_the_batch_is_an_ordinary_batch(env):
    """relevel at the drained point, out of tick mode, unbound: five in-order steps of every stream still equal the oracle"""
    H = 2
    w = Walk(env, H, 6)
    try:
        w.start().to_the_move()
        carry("blobs", w.src_b, w.dst_b, [1], [0])
        w.dst.finish()
        w.src.finish()
        w.check()
        for flow, seeds in ((w.dst, {0: 101, 1: 111}), (w.src, {0: 100, 1: 101, 2: 102})):
            flow.r.leave()
            nxt = {s: max(flow.heard(s, seed)[0]) + 1 for s, seed in seeds.items()}
            got = np.stack([flow.batch.convert(np.stack([audio(env.bv, seeds[s], H)[nxt[s] + j] for s in sorted(seeds)])) for j in range(5)])
            for s, seed in seeds.items():
                want = env.want(H, seed, nxt[s] + 5)[nxt[s]:]
                assert np.array_equal(got[:, s], want), (s, seed)
    finally:
        w.close()


# ---- 8. interchangeable blobs -----------------------------------------------------------------------------------------------------------------
def test_blobs_of_either_export_are_taken_by_either_import(env):
    bv, H = env.bv, 1
    w = Walk(env, H, 1)
    plain = bv.Batch(env.models, 2)
    try:
        w.start().to_the_move()
        # in flight out of the ticking source, drained into an in-order batch
        xd = np.ascontiguousarray(np.stack([audio(bv, 120 + s, H)[:N1 + 1 + N2] for s in range(2)]).transpose(1, 0, 2))
        before = run_in_order(plain, xd[:N1 + 1])
        plain.import_streams([0], export_in_flight(w.src_b, [1]))
        xm = xd[N1 + 1:].copy()
        xm[:, 0] = audio(bv, 101, H)[N1:N1 + N2]
        after = run_in_order(plain, xm)
        assert np.array_equal(after[:, 0], env.want(H, 101, N1 + N2)[N1:])
        assert np.array_equal(np.concatenate([before[:, 1], after[:, 1]]), env.want(H, 121, N1 + 1 + N2))
        # drained out of the in-order batch (its stream 0 stands before step N1 + N2 of audio 101), in flight into the ticking destination
        w.dst_b.import_streams_in_flight([0], plain.export_streams([0]))
        w.dst.finish()            # (the plan feeds the slot audio 101 from N1 on; what it now holds is that stream N2 steps later)
        w.src.finish()
        rows = [k for (k, sd, i) in w.dst.took[0] if sd == 101]
        # the same audio as steps N1 .. N1 + N2 on a stream that has heard them once already: a second oracle leg, one stream that is fed
        # audio 101's steps N1 .. N1 + N2 twice in a row
        assert len(rows) == N2
        ob_audio = np.concatenate([audio(bv, 101, H)[:N1 + N2], audio(bv, 101, H)[N1:N1 + N2]])
        from oracle_batch import OracleBatch
        ob = OracleBatch(bv, env.oracle, env.model_dir, 1, models=env.oracle_models, hops_per_step=H)
        try:
            want = np.stack([ob.step_stream(0, x) for x in ob_audio])[N1 + N2:]
        finally:
            ob.close()
        assert np.array_equal(w.dst.y[rows, 0], want)
        env.check(w.dst, 1, 111, what="destination")
        env.check(w.src, 1, 101, what="source")
        env.check(w.src, 0, 100, what="source")
    finally:
        plain.close()
        w.close()


# ---- 9. across the counter's wrap ---------------------------------------------------------------------------------------------------------------
def test_across_the_counters_wrap(env):
    w = Walk(env, 1, 1, src_kw=dict(start_counter=WRAP - 25), dst_kw=dict(start_counter=3))
    try:
        w.start().to_the_move()
        assert w.src_b.step_counter() < 100 and w.dst_b.step_counter() == 3 + w.at_dst   # the source has wrapped
        carry("move", w.src_b, w.dst_b, [1], [0])
        w.dst.finish()
        w.src.finish()
        w.check()
    finally:
        w.close()


# ---- 10. seventeen streams --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["blobs", "move"])
def test_seventeen_streams_take_two_rounds(env, how):
    bv, H, B, n = env.bv, 1, 18, 17
    src_b, dst_b = bv.Batch(env.models, B), bv.Batch(env.models, B)
    S = src_b.a.BeatriceBatch_TickStages(src_b.h)
    frm = list(range(1, 1 + n))                 # source streams 1 .. 17
    to = [(7 * i + 3) % B for i in range(n)]    # seventeen different places, in another order
    assert len(set(to)) == n and all(f != t for f, t in zip(frm, to))
    src = Flow(bv, src_b, [200 + s for s in range(B)], N1 + S - 1)
    dst = Flow(bv, dst_b, [300 + s for s in range(B)], 5 + S + N2)
    try:
        for f, t in zip(frm, to):
            src.sit_out(f, N1, N1 + S - 1)
            dst.sit_out(t, 5, 5 + S)
            dst.feed_from(t, 5 + S, 200 + f, N1)
        src.start().run_to(N1 + S - 1)
        dst.start().run_to(5 + S)
        before = (src.state(), dst.state())
        carry(how, src_b, dst_b, frm, to)
        assert before == (src.state(), dst.state())
        dst.finish()
        src.finish()
        for i in (0, 15, 16):   # the first and the last of the first round, the one stream of the second
            env.check(src, frm[i], 200 + frm[i], what="source")
            env.check(dst, to[i], 200 + frm[i], what="destination")
            assert dst.heard(to[i], 200 + frm[i])[0] == list(range(N1, N1 + N2))
        stayed = sorted(set(range(B)) - set(to))[0]
        env.check(dst, stayed, 300 + stayed, what="destination")
        env.check(src, 0, 200, what="source")
    finally:
        src.free()
        dst.free()
        src_b.close()
        dst_b.close()


# ---- 11. refusals change nothing --------------------------------------------------------------------------------------------------------------
def test_refused_calls_change_nothing_and_allocate_nothing(env):
    bv, H, steps = env.bv, 1, 30
    other_h = bv.Batch(env.models, 2, hops_per_step=2)
    other_flow = Flow(bv, other_h, [130, 131], 4).start()   # a ticking batch of two hops per step: no partner for a move
    got, ran = {}, {}
    try:
        for name in ("asked", "never"):
            src_b, dst_b = bv.Batch(env.models, 3), bv.Batch(env.models, 2)
            src, dst = Flow(bv, src_b, [100, 101, 102], steps), Flow(bv, dst_b, [110, 111], steps)
            src.sit_out(1, 0, steps)   # at rest throughout: only the arguments can be the reason
            dst.sit_out(0, 0, steps)
            try:
                src.start()
                dst.start()
                a, size = src_b.a, src_b.stream_blob_bytes()
                for k in (4, 17, steps):
                    src.run_to(k)
                    dst.run_to(k)
                    if name == "never" or k == steps:
                        continue
                    good = export_in_flight(src_b, [1])
                    out = C.create_string_buffer(2 * size)
                    vp = lambda b: C.cast(C.create_string_buffer(b, len(b)), C.c_void_p)   # noqa: E731
                    ex = lambda n, st, o=out: a.BeatriceBatch_ExportStreamsInFlight(src_b.h, n, st, C.cast(o, C.c_void_p) if o is not None else None)   # noqa: E731
                    im = lambda n, st, blob=good * 2, em=None, n_map=0: a.BeatriceBatch_ImportStreamsInFlight(   # noqa: E731
                        dst_b.h, n, st, vp(blob) if blob is not None else None, em, n_map)
                    mv = lambda n, fr, to_, em=None, n_map=0, s=src_b.h, d=dst_b.h: a.BeatriceBatch_MoveStreamsInFlight(s, d, n, fr, to_, em, n_map)   # noqa: E731

                    def damaged(off, xor=0x01):
                        b = bytearray(good)
                        b[off] ^= xor
                        return bytes(b)

                    def refused():
                        rcs = []
                        for call, B in ((ex, 3), (im, 2)):
                            rcs += [call(0, i32([0])), call(-1, i32([0])), call(B + 1, i32([0, 1, 2, 0])), call(1, None),
                                    call(1, i32([B])), call(1, i32([-1])), call(2, i32([1, 1]))]
                        rcs += [ex(1, i32([1]), None), im(1, i32([0]), None)]
                        rcs += [im(1, i32([0]), damaged(0)), im(1, i32([0]), damaged(4)), im(1, i32([0]), damaged(8, 0x10)),      # magic, version, size
                                im(1, i32([0]), damaged(16, 0x03)), im(1, i32([0]), damaged(48 + 8)), im(1, i32([0]), damaged(40)),  # hops, a ring's m, the check word
                                im(2, i32([0, 1]), good + damaged(0)),                                                              # the second blob bad
                                im(1, i32([0]), good, i32([0, 1, 2, 3]), -1), im(1, i32([0]), good, None, 4), im(1, i32([0]), good, i32([0, 1, 2, 3]), 0),
                                im(1, i32([0]), good, i32([4, 1, 2, 3]), 4), im(1, i32([0]), good, i32([-1, 1, 2, 3]), 4)]
                        rcs += [mv(0, i32([1]), i32([0])), mv(3, i32([0, 1, 2]), i32([0, 1, 0])), mv(1, None, i32([0])), mv(1, i32([1]), None),
                                mv(1, i32([3]), i32([0])), mv(1, i32([1]), i32([2])), mv(2, i32([1, 1]), i32([0, 1])), mv(2, i32([0, 1]), i32([0, 0])),
                                mv(1, i32([1]), i32([0]), None, 4), mv(1, i32([1]), i32([0]), i32([0, 1, 2, 3]), 0), mv(1, i32([1]), i32([0]), i32([4, 1, 2, 3]), 4),
                                mv(1, i32([1]), i32([0]), d=src_b.h), mv(1, i32([1]), i32([0]), s=None), mv(1, i32([1]), i32([0]), d=None),
                                mv(1, i32([1]), i32([0]), d=other_h.h), mv(1, i32([0]), i32([0]), s=other_h.h)]   # other hops per step, either way round
                        return rcs
                    before = (src.state(), dst.state())
                    rcs = refused()
                    assert rcs and set(rcs) == {-1}, rcs
                    if k == 4:   # no staging, no event, no piece table is made by a refused call
                        free = _free_bytes()
                        for _ in range(50):
                            assert set(refused()) == {-1}
                        assert _free_bytes() == free
                    assert before == (src.state(), dst.state())
                    ran[k] = len(rcs)
                src.finish()
                dst.finish()
                got[name] = (src.y, dst.y)
            finally:
                src.free()
                dst.free()
                src_b.close()
                dst_b.close()
    finally:
        other_flow.free()
        other_h.close()
    assert sorted(ran) == [4, 17]
    assert np.abs(got["never"][0]).max() > 1e-3
    assert np.array_equal(got["asked"][0], got["never"][0]) and np.array_equal(got["asked"][1], got["never"][1])


def test_accepted_rounds_do_not_leak(env):
    """Three streams a round, by all three calls: a staging entry or an event left behind per round would show -- 30 rounds of three
    blobs are well above the allowance (tests/test_gpu_lifecycle.py's 8 MB for the allocator's own pools)."""
    bv, B = env.bv, 4
    a_b, b_b = bv.Batch(env.models, B), bv.Batch(env.models, B)
    fa, fb = Flow(bv, a_b, [140 + s for s in range(B)], 40), Flow(bv, b_b, [150 + s for s in range(B)], 40)
    try:
        for f in (fa, fb):
            f.sit_out(1, 0, 40)
            f.sit_out(2, 0, 40)
            f.sit_out(3, 0, 40)
            f.start()

        def cycle(i):
            fa.run_to(fa.fed + 1)
            fb.run_to(fb.fed + 1)
            b_b.import_streams_in_flight([3, 1, 2], export_in_flight(a_b, [1, 2, 3]))
            b_b.move_streams_in_flight(a_b, [1, 2, 3], [2, 3, 1])

        for i in range(3):
            cycle(i)   # (the piece tables, the staging and the events are made here, once)
        before = _free_bytes()
        for i in range(30):
            cycle(i)
        after = _free_bytes()
        print("free device memory: %.1f MB -> %.1f MB, a blob: %.2f MB" % (before / 2**20, after / 2**20, a_b.stream_blob_bytes() / 2**20))
        assert 30 * 3 * a_b.stream_blob_bytes() > 2 * (8 << 20)
        assert before - after <= 8 << 20
        fa.finish()
        fb.finish()
        env.check(fa, 0, 140, what="a")
        env.check(fb, 0, 150, what="b")
    finally:
        fa.free()
        fb.free()
        a_b.close()
        b_b.close()


# ---- 12. mode gating --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def partner(bv, product, models):
    """a batch in plain tick mode whose streams are at rest: the other side of a move for a batch in any other mode"""
    batch = bv.Batch(models, mode_matrix.B)
    r = Resident(bv, batch, tick=True)
    yield batch
    r.free()
    batch.close()


@pytest.mark.parametrize("mode", ["in_order", "stage_pipelining", "resident_io", "host_streaming", "blocks48k_around_ticks", "resident_blocks",
                                  "resident_blocks_per_stream_clocks", "silent_rule_in_order"])
def test_every_other_mode_refuses_the_four_calls(bv, product, model_dir, partner, mode):
    """A, B, C, E, F, G, P, S (built as tests/test_gpu_mode_matrix.py builds them, one hop per step): -1, and the batch then equals a twin
    that never asked."""
    product = bv.bind_batch(product)
    B, CH, H = mode_matrix.B, mode_matrix.CH, 1
    steps = 7 if not mode.startswith("resident_blocks") else 10
    x16 = np.stack([bv.synth_audio(160 * H * steps, seed=8800 + s) for s in range(B)]).reshape(B, steps, H * 160)
    x48 = np.stack([wrapperlib.test_signal(480 * H * steps * CH, 48000, seed=8900 + s) for s in range(B)]).astype(np.float32).reshape(B, steps, H, CH, 480)
    results = []
    for tries in (True, False):
        c = mode_matrix.Ctx(bv, product, model_dir, H)
        try:
            mode_matrix.enter(c, mode)
            size = c.batch.stream_blob_bytes()
            got = []
            for k in range(steps):
                if tries and k in (1, 4):
                    a, h = c.a, c.h
                    buf = C.create_string_buffer(size)
                    assert a.BeatriceBatch_StreamQuiescent(h, 0) == -1
                    assert a.BeatriceBatch_ExportStreamsInFlight(h, 1, i32([0]), C.cast(buf, C.c_void_p)) == -1
                    assert a.BeatriceBatch_ImportStreamsInFlight(h, 1, i32([0]), C.cast(buf, C.c_void_p), None, 0) == -1
                    assert a.BeatriceBatch_MoveStreamsInFlight(h, partner.h, 1, i32([0]), i32([0]), None, 0) == -1
                    assert a.BeatriceBatch_MoveStreamsInFlight(partner.h, h, 1, i32([0]), i32([0]), None, 0) == -1
                y = mode_matrix.step(c, mode, k, x16[:, k], x48[:, k])
                if y is not None:
                    got.append(np.array(y, copy=True))
            got += mode_matrix.finish(c, mode)
            results.append(got)
        finally:
            c.close()
    tried, control = results
    assert len(tried) == len(control) and len(tried) > 0
    assert max(float(np.abs(y).max()) for y in control) > 1e-3
    for p, q in zip(tried, control):
        assert np.array_equal(p, q)
