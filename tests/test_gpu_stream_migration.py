"""BeatriceBatch_ExportStreams / BeatriceBatch_ImportStreams: a stream leaves one batch and goes on in another, bit for bit.

Yardsticks, all at max-abs 0: tests/oracle_batch.py's OracleBatch -- for the oracle a migrated stream is simply ONE Stream1 that keeps
running, N1 + N2 steps of it -- and, where the oracle has no leg (the morph lottery, the refusals), a TWIN product batch in which the stream
never moved / nothing was asked.  N1 = N2 = 20 steps: the deepest ring has 17 step slots, so 20 steps fill every history and 20 more read
all of it back.  Source batches have 3 streams, destination batches 2, unless a case is about the size."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from oracle_batch import OracleBatch
from tick_driver import Resident

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N1 = N2 = 20


@pytest.fixture(scope="module")
def shard():
    spec = importlib.util.spec_from_file_location("bv_shard", os.path.join(REPO, "beatrice-vst_amd", "shard.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def models(bv, product, model_dir):
    m = bv.Models(product, model_dir)
    yield m
    m.close()


@pytest.fixture(scope="module")
def oracle_models(bv, oracle, model_dir):
    m = bv.Models(oracle, model_dir)
    yield m
    m.close()


def audio(bv, seed, steps, H):
    """One stream's input, [steps][H * 160]."""
    return bv.synth_audio(160 * H * steps, seed=seed).reshape(steps, H * 160)


_oracle_runs = {}


def oracle_run(bv, oracle, oracle_models, model_dir, H, seed, steps, script=None, key=None, absent=()):
    """[steps][H * 240] of ONE oracle stream on audio(seed): script(a, h, stream, k) runs before step k; the steps in `absent` are sat
    out (no hop is made, no input consumed by the stream's state; their rows stay zero).  Computed once per (H, seed, script key, absent)
    and at the longest length asked so far; a shorter run is its prefix."""
    ck = (H, seed, key, tuple(absent))
    have = _oracle_runs.get(ck)
    if have is not None and len(have) >= steps:
        return have[:steps]
    ob = OracleBatch(bv, oracle, model_dir, 1, models=oracle_models, hops_per_step=H)
    x = audio(bv, seed, steps, H)
    out = np.zeros((steps, H * 240), np.float32)
    for k in range(steps):
        if script is not None:
            script(ob.a, None, 0, k)
        if k not in absent:
            out[k] = ob.step_stream(0, x[k])
    ob.close()
    _oracle_runs[ck] = out
    return out


def run_in_order(batch, xs, scripts=None, k0=0):
    """xs [steps][B][H * 160] through BeatriceBatch_ConvertFrames; scripts {stream: script}, step numbers start at k0."""
    out = np.zeros((len(xs), batch.B, batch.H * 240), np.float32)
    for j in range(len(xs)):
        for s, script in (scripts or {}).items():
            script(batch.a, batch.h, s, k0 + j)
        out[j] = batch.convert(xs[j])
    return out


def stack(bv, seeds, steps, H):
    """[steps][len(seeds)][H * 160]"""
    return np.ascontiguousarray(np.stack([audio(bv, s, steps, H) for s in seeds]).transpose(1, 0, 2))


# ---- 1. counter phase, in order ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [0, 1, 6])
@pytest.mark.parametrize("H", [1, 2])
def test_a_moved_stream_goes_on_bit_for_bit_whatever_the_counters(bv, product, oracle, models, oracle_models, model_dir, shard, H, d):
    """The destination has run N1 + d steps: d = 1 turns every ring with more than one slot, d = 6 some and not others."""
    src, dst = bv.Batch(models, 3, hops_per_step=H), bv.Batch(models, 2, hops_per_step=H)
    try:
        xs = stack(bv, [100, 101, 102], N1 + N2, H)
        xd = stack(bv, [110, 111], N1 + 6 + N2, H)
        got_src = run_in_order(src, xs[:N1])
        before = run_in_order(dst, xd[:N1 + d])
        blob = shard.move_streams(src, [1], dst, [0])
        assert len(blob) == src.stream_blob_bytes() == dst.stream_blob_bytes()
        xm = xd[N1 + d:N1 + d + N2].copy()
        xm[:, 0] = xs[N1:, 1]   # the moved stream's own audio goes on in its new place
        after = run_in_order(dst, xm)
        rest_src = run_in_order(src, xs[N1:])   # the export changed nothing: the source goes on as if nothing had been asked
        moved = oracle_run(bv, oracle, oracle_models, model_dir, H, 101, N1 + N2)
        assert np.abs(moved[N1:]).max() > 1e-3
        assert np.array_equal(got_src[:, 1], moved[:N1])
        assert np.array_equal(after[:, 0], moved[N1:])
        assert np.array_equal(rest_src[:, 1], moved[N1:])
        other = oracle_run(bv, oracle, oracle_models, model_dir, H, 111, N1 + 6 + N2)[:N1 + d + N2]
        assert np.array_equal(np.concatenate([before[:, 1], after[:, 1]]), other)   # the destination's other stream: untouched
        stay = oracle_run(bv, oracle, oracle_models, model_dir, H, 100, N1 + N2)
        assert np.array_equal(np.concatenate([got_src[:, 0], rest_src[:, 0]]), stay)
    finally:
        src.close()
        dst.close()


# ---- 2. pending installs and settings -----------------------------------------------------------------------------------------------------
def settings_script(H):
    """Everything a blob's settings part carries, and a speaker switch two hops before the export: two key/value blocks are still to come
    (at two hops per step the switch is made right before the last source step, whose two hops install the first two)."""
    switch_at = N1 - 2 // H

    def script(a, h, s, k):
        if k == 3:
            assert a.BeatriceBatch_SetFormantShift(h, s, 1.0) == 0
            assert a.BeatriceBatch_SetPitchShift(h, s, 3.0) == 0
            assert a.BeatriceBatch_SetVQNumNeighbors(h, s, 2) == 0
            assert a.BeatriceBatch_SetMinSourcePitch(h, s, 40.0) == 0
            assert a.BeatriceBatch_SetMaxSourcePitch(h, s, 70.0) == 0
            assert a.BeatriceBatch_SetIntonationIntensity(h, s, 1.5) == 0
        if k == 5:
            assert a.BeatriceBatch_SetTargetSpeaker(h, s, 2) == 0
        if k == switch_at:
            assert a.BeatriceBatch_SetTargetSpeaker(h, s, 1) == 0
    return script


@pytest.mark.parametrize("H", [1, 2])
def test_pending_installs_and_every_setting_travel(bv, product, oracle, models, oracle_models, model_dir, H):
    src, dst = bv.Batch(models, 3, hops_per_step=H), bv.Batch(models, 2, hops_per_step=H)
    try:
        script = settings_script(H)
        xs = stack(bv, [100, 101, 102], N1 + N2, H)
        xd = stack(bv, [110, 111], N1 + 1 + N2, H)
        got_src = run_in_order(src, xs[:N1], {1: script})
        before = run_in_order(dst, xd[:N1 + 1])
        dst.import_streams([0], src.export_streams([1]))
        xm = xd[N1 + 1:].copy()
        xm[:, 0] = xs[N1:, 1]
        after = run_in_order(dst, xm)
        moved = oracle_run(bv, oracle, oracle_models, model_dir, H, 101, N1 + N2, script, "settings")
        plain = oracle_run(bv, oracle, oracle_models, model_dir, H, 101, N1 + N2)
        assert not np.array_equal(moved[N1:], plain[N1:])   # (the settings are audible)
        assert np.array_equal(got_src[:, 1], moved[:N1])
        assert np.array_equal(after[:, 0], moved[N1:])
        other = oracle_run(bv, oracle, oracle_models, model_dir, H, 111, N1 + 6 + N2)[:N1 + 1 + N2]
        assert np.array_equal(np.concatenate([before[:, 1], after[:, 1]]), other)
    finally:
        src.close()
        dst.close()


# ---- 3. tick mode on both sides ----------------------------------------------------------------------------------------------------------
class Ticks:
    """A batch in tick mode over resident I/O, fed WITHOUT waiting: the steps are still inside the pipeline when the next call comes."""

    def __init__(self, bv, batch):
        self.r = Resident(bv, batch, tick=True)
        self.batch = batch

    def feed(self, xs, before_step=None):
        r, a, h = self.r, self.batch.a, self.batch.h
        assert len(xs) <= r.slots
        for j in range(len(xs)):
            r.buf[(r.fed + j) % r.slots] = xs[j]
        r.hip.h2d(r.d_in, r.buf)
        for j in range(len(xs)):
            if before_step is not None:
                before_step(j)
            assert a.BeatriceBatch_ConvertFramesDevice(h, None, None) == 0
        self.pending = len(xs)

    def collect(self):
        """(after something has drained the pipeline) the samples of the steps fed last, [n][B][H * 240]"""
        r, a, h = self.r, self.batch.a, self.batch.h
        assert a.BeatriceBatch_Synchronize(h) == 0
        out = np.zeros((r.slots, self.batch.B, self.batch.H * 240), np.float32)
        r.hip.d2h(out, r.d_out)
        got = np.stack([out[(r.fed + j) % r.slots] for j in range(self.pending)])
        r.fed += self.pending
        return got


@pytest.mark.parametrize("silent", [False, True], ids=["every step", "two of the last five steps sat out"])
def test_tick_mode_on_both_sides_drains_and_moves(bv, product, oracle, models, oracle_models, model_dir, silent):
    H = 2
    src, dst = bv.Batch(models, 3, hops_per_step=H), bv.Batch(models, 2, hops_per_step=H)
    ts = td = None
    try:
        ts, td = Ticks(bv, src), Ticks(bv, dst)
        absent = (N1 - 5, N1 - 3) if silent else ()
        if silent:
            assert src.a.BeatriceBatch_EnableSilentBlockRule(src.h, 1) == 0

        def flags(j):
            if j in absent:
                assert src.a.BeatriceBatch_SetSilentStreams(src.h, bytes([0, 1, 0])) == 0
        xs = stack(bv, [100, 101, 102], N1 + N2, H)
        xd = stack(bv, [110, 111], N1 + 1 + N2, H)
        ts.feed(xs[:N1], flags)
        td.feed(xd[:N1 + 1])
        ticks_src, ticks_dst = src.a.BeatriceBatch_TicksLaunched(src.h), dst.a.BeatriceBatch_TicksLaunched(dst.h)
        assert ticks_src == N1 and ticks_dst == N1 + 1   # nothing has drained yet: the last steps are inside both pipelines
        blob = src.export_streams([1])
        assert src.a.BeatriceBatch_TicksLaunched(src.h) > ticks_src   # the export drained the source
        dst.import_streams([0], blob)
        assert dst.a.BeatriceBatch_TicksLaunched(dst.h) > ticks_dst   # ... and the import the destination
        got_src, before = ts.collect(), td.collect()
        xm = xd[N1 + 1:].copy()
        xm[:, 0] = xs[N1:, 1]
        td.feed(xm)
        after = td.collect()
        ts.feed(xs[N1:])
        rest_src = ts.collect()
        moved = oracle_run(bv, oracle, oracle_models, model_dir, H, 101, N1 + N2, absent=absent)
        present = [k for k in range(N1) if k not in absent]
        assert np.abs(moved[N1:]).max() > 1e-3
        assert np.array_equal(got_src[present, 1], moved[present])
        assert np.array_equal(after[:, 0], moved[N1:])
        assert np.array_equal(rest_src[:, 1], moved[N1:])
        other = oracle_run(bv, oracle, oracle_models, model_dir, H, 111, N1 + 6 + N2)[:N1 + 1 + N2]
        assert np.array_equal(np.concatenate([before[:, 1], after[:, 1]]), other)
        stay = oracle_run(bv, oracle, oracle_models, model_dir, H, 100, N1 + N2)
        assert np.array_equal(np.concatenate([got_src[:, 0], rest_src[:, 0]]), stay)
    finally:
        for t in (ts, td):
            if t is not None:
                t.r.free()
        src.close()
        dst.close()


# ---- 4. one-stream batches (the team launches) ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [(3, 1), (1, 2)], ids=["3 -> 1", "1 -> 2"])
def test_into_and_out_of_a_one_stream_batch(bv, product, oracle, models, oracle_models, model_dir, sizes):
    H = 1
    Bs, Bd = sizes
    s_from = Bs - 1 if Bs == 1 else 1
    src, dst = bv.Batch(models, Bs), bv.Batch(models, Bd)
    try:
        seeds_src = [100 + i for i in range(Bs)]
        seeds_src[s_from] = 101
        xs = stack(bv, seeds_src, N1 + N2, H)
        xd = stack(bv, [110, 111][:Bd], N1 + 1 + N2, H)
        got_src = run_in_order(src, xs[:N1])
        before = run_in_order(dst, xd[:N1 + 1])
        dst.import_streams([0], src.export_streams([s_from]))
        xm = xd[N1 + 1:].copy()
        xm[:, 0] = xs[N1:, s_from]
        after = run_in_order(dst, xm)
        rest_src = run_in_order(src, xs[N1:])
        moved = oracle_run(bv, oracle, oracle_models, model_dir, H, 101, N1 + N2)
        assert np.array_equal(got_src[:, s_from], moved[:N1])
        assert np.array_equal(after[:, 0], moved[N1:])
        assert np.array_equal(rest_src[:, s_from], moved[N1:])
        if Bd > 1:
            other = oracle_run(bv, oracle, oracle_models, model_dir, H, 111, N1 + 6 + N2)[:N1 + 1 + N2]
            assert np.array_equal(np.concatenate([before[:, 1], after[:, 1]]), other)
    finally:
        src.close()
        dst.close()


# ---- 5. entry_map ------------------------------------------------------------------------------------------------------------------------
def test_entry_map_sends_every_voice_to_its_place(bv, product, oracle, models, oracle_models, model_dir):
    """The destination holds the same three voices in the order (2, 0, 1); a speaker switch is pending at the export."""
    H = 1
    order = [2, 0, 1, 3]            # destination entry i holds the source's entry order[i]
    entry_map = [1, 2, 0, 3]        # so the source's entry v sits at destination entry entry_map[v]
    assert all(order[entry_map[v]] == v for v in range(4))
    t = models.tables
    src = bv.Batch(models, 3)
    dst = bv.Batch(models, 2, max_speakers=t.n_speakers + 1, upload_tables=False)
    try:
        cb, add, kv = (np.ascontiguousarray(x[order]) for x in (t.codebooks, t.additive, t.kv))
        assert dst.a.BeatriceBatch_SetSpeakerTables(dst.h, t.n_speakers + 1, bv.fptr(cb), bv.fptr(add), bv.fptr(t.formant), bv.fptr(kv)) == 0
        dst.apply_defaults()        # (every stream on the destination's entry 0: the source's voice 2)

        def script(a, h, s, k):
            if k == 5:
                assert a.BeatriceBatch_SetTargetSpeaker(h, s, 2) == 0
                assert a.BeatriceBatch_SetVQNumNeighbors(h, s, 1) == 0
            if k == N1 - 2:
                assert a.BeatriceBatch_SetTargetSpeaker(h, s, 1) == 0

        def voice2(a, h, s, k):
            if k == 0:
                assert a.BeatriceBatch_SetTargetSpeaker(h, s, 2) == 0 and a.BeatriceBatch_FlushSpeaker(h, s) == 0
        xs = stack(bv, [100, 101, 102], N1 + N2, H)
        xd = stack(bv, [110, 111], N1 + 1 + N2, H)
        got_src = run_in_order(src, xs[:N1], {1: script})
        before = run_in_order(dst, xd[:N1 + 1])
        blob = src.export_streams([1])
        with pytest.raises(RuntimeError):
            dst.import_streams([0], blob, entry_map[:2])   # the blob names entry 2: a map of two entries does not reach it
        dst.import_streams([0], blob, entry_map)
        xm = xd[N1 + 1:].copy()
        xm[:, 0] = xs[N1:, 1]
        after = run_in_order(dst, xm)
        moved = oracle_run(bv, oracle, oracle_models, model_dir, H, 101, N1 + N2, script, "voices 2 then 1")
        assert np.array_equal(got_src[:, 1], moved[:N1])
        assert np.array_equal(after[:, 0], moved[N1:])
        other = oracle_run(bv, oracle, oracle_models, model_dir, H, 111, N1 + 1 + N2, voice2, "voice 2 from the start")
        assert np.array_equal(np.concatenate([before[:, 1], after[:, 1]]), other)
    finally:
        src.close()
        dst.close()


# ---- 6. the lottery (twin) ---------------------------------------------------------------------------------------------------------------
def test_the_lottery_engine_continues_its_sequence(bv, product, models):
    H = 1
    w = np.array([0.5, 0.5, 0.0], np.float32)
    xs = stack(bv, [100, 101, 102], N1 + N2, H)
    xd = stack(bv, [110, 111], N1 + 1 + N2, H)

    def morphing(batch):
        assert batch.a.BeatriceBatch_MorphSpeaker(batch.h, 3, bv.fptr(w), 3, 7) == 0
        return batch

    def on_the_morph(a, h, s, k):
        if k == 0:
            assert a.BeatriceBatch_SetTargetSpeaker(h, s, 3) == 0 and a.BeatriceBatch_SetVQNumNeighbors(h, s, 2) == 0

    twin = morphing(bv.Batch(models, 3))
    try:
        stayed = run_in_order(twin, xs, {1: on_the_morph})[:, 1]
    finally:
        twin.close()
    after = {}
    for reseed in (False, True):
        src, dst = morphing(bv.Batch(models, 3)), morphing(bv.Batch(models, 2))
        try:
            got_src = run_in_order(src, xs[:N1], {1: on_the_morph})
            run_in_order(dst, xd[:N1 + 1])
            dst.import_streams([0], src.export_streams([1]))
            if reseed:
                assert dst.a.BeatriceBatch_SeedLottery(dst.h, 0, 8) == 0
            xm = xd[N1 + 1:].copy()
            xm[:, 0] = xs[N1:, 1]
            after[reseed] = run_in_order(dst, xm)[:, 0]
            assert np.array_equal(got_src[:, 1], stayed[:N1])
        finally:
            src.close()
            dst.close()
    assert np.abs(stayed[N1:]).max() > 1e-3
    assert np.array_equal(after[False], stayed[N1:])
    assert not np.array_equal(after[True], stayed[N1:])   # not vacuous: another engine state is audible within these steps


# ---- 7. refusals change nothing ------------------------------------------------------------------------------------------------------------
def test_refused_calls_change_nothing_and_do_not_drain(bv, product, models):
    H, B, steps = 1, 3, 30
    xs = stack(bv, [100, 101, 102], steps, H)
    donor, donor2 = bv.Batch(models, 2), bv.Batch(models, 2, hops_per_step=2)
    try:
        donor.convert(np.zeros((2, 160), np.float32))
        good = donor.export_streams([0])
        two_hops = donor2.export_streams([0])
        size = donor.stream_blob_bytes()
        assert donor2.stream_blob_bytes() != size
    finally:
        donor.close()
        donor2.close()

    def damaged(off, xor=0x01):
        b = bytearray(good)
        b[off] ^= xor
        return bytes(b)

    i32 = lambda v: bv.iptr(np.ascontiguousarray(v, np.int32))   # noqa: E731
    ran = {}

    def asks(batch, k):
        a, h = batch.a, batch.h
        out = C.create_string_buffer(2 * size)
        vp = lambda b: C.cast(C.create_string_buffer(b, len(b)), C.c_void_p)   # noqa: E731
        ex = lambda n, st, dst=out: a.BeatriceBatch_ExportStreams(h, n, st, C.cast(dst, C.c_void_p) if dst is not None else None)   # noqa: E731
        im = lambda n, st, blob, em=None, n_map=0: a.BeatriceBatch_ImportStreams(h, n, st, vp(blob) if blob is not None else None, em, n_map)   # noqa: E731
        if k in (4, 17):
            for call in (ex, lambda n, st: im(n, st, good * 2)):
                assert call(0, i32([0])) == -1 and call(-1, i32([0])) == -1 and call(B + 1, i32([0, 1, 2, 0])) == -1
                assert call(1, None) == -1
                assert call(1, i32([B])) == -1 and call(1, i32([-1])) == -1 and call(2, i32([1, 1])) == -1
            assert ex(1, i32([0]), None) == -1 and im(1, i32([0]), None) == -1
            assert im(1, i32([0]), damaged(0)) == -1            # magic
            assert im(1, i32([0]), damaged(4)) == -1            # version
            assert im(1, i32([0]), damaged(8, 0x10)) == -1      # size
            assert im(1, i32([0]), damaged(16, 0x03)) == -1     # hops per step, in the header alone
            assert im(1, i32([0]), two_hops) == -1              # ... and a whole blob of a batch with two hops per step
            assert im(1, i32([0]), damaged(48 + 8)) == -1       # the first ring's m
            assert im(1, i32([0]), damaged(40)) == -1           # the check word
            assert im(2, i32([0, 1]), good + damaged(0)) == -1  # the second blob bad: the first is not taken either
            assert im(1, i32([0]), good, i32([0, 1, 2, 3]), -1) == -1 and im(1, i32([0]), good, None, 4) == -1
            assert im(1, i32([0]), good, i32([0, 1, 2, 3]), 0) == -1    # an index outside entry_map (the blob names entry 0)
            assert im(1, i32([0]), good, i32([4, 1, 2, 3]), 4) == -1    # a mapped index at n_speakers
            assert im(1, i32([0]), good, i32([-1, 1, 2, 3]), 4) == -1
            ran["refused"] = ran.get("refused", 0) + 1
        if k == 11:
            assert a.BeatriceBatch_ResetStreamInFlight(h, 2) == 0
            ran["minus3"] = ex(1, i32([2]))                     # pending, no step has taken it yet
            ran["other stream"] = ex(2, i32([0, 2]))

    def never(batch, k):
        if k == 11:
            assert batch.a.BeatriceBatch_ResetStreamInFlight(batch.h, 2) == 0

    got = {}
    for name, change in (("asked", asks), ("never", never)):
        batch = bv.Batch(models, B)
        t = None
        try:
            t = Ticks(bv, batch)
            t.feed(xs, lambda j: change(batch, j))
            ticks = batch.a.BeatriceBatch_TicksLaunched(batch.h)
            got[name] = (t.collect(), ticks)
        finally:
            if t is not None:
                t.r.free()
            batch.close()
    assert ran == {"refused": 2, "minus3": -3, "other stream": -3}
    assert np.abs(got["never"][0]).max() > 1e-3
    assert np.array_equal(got["asked"][0], got["never"][0])
    assert got["asked"][1] == got["never"][1] == steps   # one tick per step: no refused call drained


# ---- 8. several at once --------------------------------------------------------------------------------------------------------------------
def test_three_streams_in_one_call_into_other_places(bv, product, oracle, models, oracle_models, model_dir, shard):
    H = 1
    src, dst = bv.Batch(models, 4), bv.Batch(models, 4)
    try:
        xs = stack(bv, [100, 101, 102, 103], N1 + N2, H)
        xd = stack(bv, [110, 111, 112, 113], N1 + 1 + N2, H)
        script = settings_script(H)
        got_src = run_in_order(src, xs[:N1], {3: script})
        before = run_in_order(dst, xd[:N1 + 1])
        frm, to = [3, 0, 1], [1, 2, 0]
        shard.move_streams(src, frm, dst, to, reset_source=True)
        xm = xd[N1 + 1:].copy()
        for f, t in zip(frm, to):
            xm[:, t] = xs[N1:, f]
        after = run_in_order(dst, xm)
        for f, t in zip(frm, to):
            moved = oracle_run(bv, oracle, oracle_models, model_dir, H, 100 + f, N1 + N2, *((script, "settings") if f == 3 else ()))
            assert np.array_equal(got_src[:, f], moved[:N1]), f
            assert np.array_equal(after[:, t], moved[N1:]), (f, t)
        other = oracle_run(bv, oracle, oracle_models, model_dir, H, 113, N1 + 1 + N2)
        assert np.array_equal(np.concatenate([before[:, 3], after[:, 3]]), other)
        # reset_source: the slots the streams left start from silence, the stream that stayed goes on
        rest = run_in_order(src, xs[N1:])
        assert np.array_equal(rest[:, 2], oracle_run(bv, oracle, oracle_models, model_dir, H, 102, N1 + N2)[N1:])
        fresh = bv.Batch(models, 4)
        try:
            again = run_in_order(fresh, xs[N1:])
        finally:
            fresh.close()
        assert np.array_equal(rest[:, 0], again[:, 0]) and np.array_equal(rest[:, 1], again[:, 1])
    finally:
        src.close()
        dst.close()


def test_seventeen_streams_take_two_staging_rounds(bv, product, oracle, models, oracle_models, model_dir):
    H, B, n = 1, 20, 17
    src, dst = bv.Batch(models, B), bv.Batch(models, B)
    try:
        xs = stack(bv, [200 + s for s in range(B)], N1 + N2, H)
        xd = stack(bv, [300 + s for s in range(B)], N1 + 1 + N2, H)
        got_src = run_in_order(src, xs[:N1])
        before = run_in_order(dst, xd[:N1 + 1])
        frm = list(range(2, 2 + n))            # source streams 2 .. 18
        to = [(7 * i + 3) % B for i in range(n)]   # seventeen different places, in another order
        assert len(set(to)) == n
        dst.import_streams(to, src.export_streams(frm))
        xm = xd[N1 + 1:].copy()
        for f, t in zip(frm, to):
            xm[:, t] = xs[N1:, f]
        after = run_in_order(dst, xm)
        for i in (0, 15, 16):   # the first and the last of the first round, the one stream of the second
            f, t = frm[i], to[i]
            moved = oracle_run(bv, oracle, oracle_models, model_dir, H, 200 + f, N1 + N2)
            assert np.array_equal(got_src[:, f], moved[:N1]), f
            assert np.array_equal(after[:, t], moved[N1:]), (f, t)
        stayed = sorted(set(range(B)) - set(to))[0]
        other = oracle_run(bv, oracle, oracle_models, model_dir, H, 300 + stayed, N1 + 1 + N2)
        assert np.array_equal(np.concatenate([before[:, stayed], after[:, stayed]]), other)
    finally:
        src.close()
        dst.close()


# ---- 9. lifecycle --------------------------------------------------------------------------------------------------------------------------
def _free_bytes():
    hip = C.CDLL("libamdhip64.so")
    assert hip.hipDeviceSynchronize() == 0
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_export_and_import_rounds_do_not_leak(bv, product, models):
    """Every call moves all 16 streams, so the staging pair is 16 blobs from the first call on and one device staging buffer left behind
    per round would take 20 x 16 blobs; the allowance is tests/test_gpu_lifecycle.py's 8 MB for the allocator's own pools."""
    B = 16
    a, b = bv.Batch(models, B), bv.Batch(models, B)
    try:
        x = np.zeros((B, 160), np.float32)
        everyone = list(range(B))

        def cycle(i):
            a.convert(x)
            b.import_streams([(s + i) % B for s in everyone], a.export_streams(everyone))
            b.convert(x)
            a.import_streams(everyone[::-1], b.export_streams(everyone))

        for i in range(3):
            cycle(i)   # (the piece tables and the staging pairs are made here, once)
        before = _free_bytes()
        for i in range(20):
            cycle(i)
        after = _free_bytes()
        print("free device memory: %.1f MB -> %.1f MB, a blob: %.2f MB" % (before / 2**20, after / 2**20, a.stream_blob_bytes() / 2**20))
        assert 20 * B * a.stream_blob_bytes() > 2 * (8 << 20)   # (what is looked for is well above the allowance)
        assert before - after <= 8 << 20
    finally:
        a.close()
        b.close()
