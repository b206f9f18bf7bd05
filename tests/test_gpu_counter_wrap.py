"""Every drive across the step counter's wrap.  Every ring of the product is addressed by (step counter mod its slot count) and the
counter wraps to 0 after bv.STEP_WRAP - 1 = lcm(1..17) - 1: 34 hours of 10 ms steps, which no test can feed.  The test hooks
BeatriceBatch_SetStepCounter / BeatriceHip_SetHopCount[Legacy] (include/beatrice_batch.h) start a FRESH batch or context a few steps
in front of the wrap instead: all its rings are zeros, so it must compute exactly what one started at 0 computes.

A case starts at wrap - 24 and runs 48 steps unless it says otherwise: no ring has more than 24 step slots, so every ring wraps its
slots with live history on both sides, and 24 keeps the counter congruent to the number of steps modulo 3 and modulo 4, as production
does.  Three assertions per case: (a) the counter did wrap (BeatriceBatch_StepCounter before and after), (b) the samples are
np.array_equal to a TWIN of the same build started at 0 -- same code, same arithmetic, other slot indices: no tolerance --, (c) the
samples are within TOL of the oracle, which has no step counter at all (its histories are shifted, not rotated)."""
import os

import numpy as np
import pytest

import regimes as R
import test_gpu_stream_migration as mig
import wrapperlib
from oracle_batch import OracleBatch, oracle_leg
from tick_driver import Hip, Resident, run_tick

pytestmark = pytest.mark.gpu
TOL = 1e-4          # test_gpu_segment_loop_shapes.py's bound on output PCM
B, STEPS, AHEAD = 5, 48, 24
MAX_HOPS = 4 * STEPS


@pytest.fixture(scope="module")
def models(bv, product, model_dir):
    m = bv.Models(bv.bind_batch(product), model_dir)
    yield m
    m.close()


@pytest.fixture(scope="module")
def oracle_models(bv, oracle, model_dir):
    m = bv.Models(oracle, model_dir)
    yield m
    m.close()


@pytest.fixture(scope="module")
def audio(bv):
    """[B][MAX_HOPS][160]; a run of n hops is its prefix"""
    return np.stack([bv.synth_audio(160 * MAX_HOPS, seed=9700 + s) for s in range(B)]).reshape(B, MAX_HOPS, 160)


def _settings(batch):
    for s in range(B):
        assert batch.a.BeatriceBatch_SetTargetSpeaker(batch.h, s, s % 3) == 0
    assert batch.a.BeatriceBatch_FlushSpeaker(batch.h, -1) == 0


@pytest.fixture(scope="module")
def plain_hops(bv, oracle, model_dir, audio):
    """The oracle's samples of the uninterrupted streams, [MAX_HOPS][B][240]: one run, shared (a run of n hops is its prefix)."""
    sample, want = oracle_leg(bv, oracle, model_dir, B, lambda j: audio[:, j], MAX_HOPS, _settings, lambda ob, j: None, list(range(B)))
    assert sample == list(range(B))
    want.setflags(write=False)
    return want


def _as_steps(hops, H, steps):
    """[hops][B][240] -> [steps][B][H * 240]"""
    return hops[:steps * H].reshape(steps, H, B, 240).transpose(0, 2, 1, 3).reshape(steps, B, H * 240)


def _x(audio, H, k):
    return np.ascontiguousarray(audio[:, k * H:(k + 1) * H].reshape(B, H * 160))


def _verdict(what, got, twin, want, counters=()):
    """Prints every figure first, then asserts: (a) counters = [(seen, expected), ...], (b) the twin, (c) the oracle."""
    dev = float(np.abs(got - want).max())
    print("%s: vs ORACLE max-abs %g, array_equal %s; vs TWIN at 0 array_equal %s (max-abs %g)" %
          (what, dev, np.array_equal(got, want), np.array_equal(got, twin), float(np.abs(got - twin).max())))
    for seen, expected in counters:
        assert seen == expected
    assert np.abs(got).max() > 1e-3
    assert np.array_equal(got, twin)
    assert dev <= TOL


def _cross(bv, models, H, what, drive, want, steps=STEPS, ahead=AHEAD, mask=None):
    """drive(batch) -> samples, on a batch started `ahead` steps in front of the wrap and on its twin started at 0; `steps` = the steps
    the drive takes; mask(samples): zeroes what is not specified."""
    wrap = bv.STEP_WRAP
    assert steps > ahead
    outs, counters = [], []
    for start in (wrap - ahead, 0):
        batch = bv.Batch(models, B, hops_per_step=H, start_counter=start)
        try:
            _settings(batch)
            before = batch.step_counter()
            out = drive(batch)
            after = batch.step_counter()
        finally:
            batch.close()
        print("%s: step counter %d before, %d after %d steps" % (what, before, after, steps))
        counters += [(before, start), (after, steps - ahead if start else steps)]      # (a): the batch in front of the wrap has crossed it
        outs.append(out if mask is None else mask(out.copy()))
    _verdict(what, outs[0], outs[1], want if mask is None else mask(want.copy()), counters)


# ---- in order: the device's own increment ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [1, 0], ids=["graph replay", "plain launches"])
@pytest.mark.parametrize("H", [1, 4])
def test_in_order_convert_frames(bv, models, audio, plain_hops, H, graph):
    """BeatriceBatch_ConvertFrames: the front end's last body stores hop_next(counter) for the next step, replayed from the captured
    graphs or launched plainly (BeatriceBatch_EnableGraph)."""
    def drive(batch):
        assert batch.a.BeatriceBatch_EnableGraph(batch.h, graph) == 0
        return np.stack([batch.convert(_x(audio, H, k)) for k in range(STEPS)])
    _cross(bv, models, H, "in order, %d hop(s) per step, graph %d" % (H, graph), drive, _as_steps(plain_hops, H, STEPS))


@pytest.mark.parametrize("depth", [2, 0], ids=["EnablePipelining(2)", "resident I/O"])
@pytest.mark.parametrize("H", [1, 4])
def test_stage_pipelining_and_resident_io(bv, models, audio, plain_hops, H, depth):
    """48 steps enqueued without waiting over resident I/O, in order and with two pipeline stages: the settings copies and the
    events of step t sit at (counter & 3)."""
    def drive(batch):
        r = Resident(bv, batch, slots=STEPS, tick=False)
        try:
            if depth:
                assert batch.a.BeatriceBatch_EnablePipelining(batch.h, depth) == 0
            got = r.feed([_x(audio, H, k) for k in range(STEPS)])
            if depth:
                assert batch.a.BeatriceBatch_EnablePipelining(batch.h, 0) == 0
            r.leave()
        finally:
            r.free()
        return got
    _cross(bv, models, H, "resident I/O, pipelining %d, %d hop(s) per step" % (depth, H), drive, _as_steps(plain_hops, H, STEPS))


# ---- tick mode -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [1, 2, 4])
def test_tick_mode(bv, models, audio, plain_hops, H):
    """Chunks of 7: the fourth chunk feeds the steps with counters wrap-3 .. 3 back to back, so one launch holds stages at wrap-2,
    wrap-1, 0 and 1, and its drain and the next chunk's fill run with stage counters on both sides."""
    def drive(batch):
        return run_tick(bv, batch, STEPS, lambda k: _x(audio, H, k), chunk=7)
    assert 3 * 7 < AHEAD - 2 and AHEAD + 1 < 4 * 7
    _cross(bv, models, H, "tick mode, %d hop(s) per step" % H, drive, _as_steps(plain_hops, H, STEPS))


def test_ragged_tick_relevels_across_the_wrap(bv, oracle, models, model_dir, audio):
    """H = 4, the silent-block rule on: stream 3 sits the steps with counters wrap-2, wrap-1 and 0 out (as
    test_gpu_flat_to_global_shapes.py does it), so its own counter wraps three steps after the batch's.  Tick mode is left after the
    step with counter 1, the batch at 2 and stream 3 at wrap-1: the drain brings it back to the batch's counter across the wrap (the
    rings rotated by 3).  Then 8 steps in order.  Oracle: the hops of a step a stream sits out are never made; what the slots of
    those steps hold is not specified."""
    H, n_tick, n_tail = 4, AHEAD + 2, 8
    out = {3: {AHEAD - 2, AHEAD - 1, AHEAD}}
    steps = n_tick + n_tail

    ob = OracleBatch(bv, oracle, model_dir, B, hops_per_step=H)
    _settings(ob)
    want = np.zeros((steps, B, H * 240), np.float32)
    for k in range(steps):
        for s, y in ob.convert(_x(audio, H, k), absent={s for s in ob.sample if k in out.get(s, ())}).items():
            want[k, s] = y
    ob.close()

    def drive(batch):
        a, h = batch.a, batch.h
        r = Resident(bv, batch, tick=True)
        assert r.slots >= n_tick
        try:
            assert a.BeatriceBatch_EnableSilentBlockRule(h, 1) == 0      # (inside tick mode)

            def flag(k):
                flags = bytes(1 if k in out.get(s, ()) else 0 for s in range(B))
                if any(flags):
                    assert a.BeatriceBatch_SetSilentStreams(h, flags) == 0
            half = n_tick // 2
            first = r.feed([_x(audio, H, k) for k in range(half)], flag)
            # the second half WITHOUT a drain of its own: leaving tick mode finds stream 3 three steps behind, on the far side of the wrap
            for k in range(half, n_tick):
                r.buf[k % r.slots] = _x(audio, H, k)
            r.hip.h2d(r.d_in, r.buf)
            for k in range(half, n_tick):
                flag(k)
                assert a.BeatriceBatch_ConvertFramesDevice(h, None, None) == 0
            r.leave()
            res = np.zeros((r.slots, B, H * 240), np.float32)
            r.hip.d2h(res, r.d_out)
            second = np.stack([res[k % r.slots] for k in range(half, n_tick)])
        finally:
            r.free()
        assert a.BeatriceBatch_EnableSilentBlockRule(h, 0) == 0
        tail = np.stack([batch.convert(_x(audio, H, k)) for k in range(n_tick, steps)])
        return np.concatenate([first, second, tail])

    def mask(y):
        for s, ks in out.items():
            for k in ks:
                y[k, s] = 0.0
        return y
    _cross(bv, models, H, "ragged tick mode, stream 3 three steps behind across the wrap, then in order", drive, want, steps=steps, mask=mask)


@pytest.mark.parametrize("H", [1, 4])
def test_reset_in_flight_on_both_sides_of_the_wrap(bv, oracle, models, model_dir, audio, H):
    """BeatriceBatch_ResetStreamInFlight of stream 1 at the step with counter wrap-1 and of stream 2 at counter 0, both inside one
    chunk: the travelling resets clear slot (counter mod m) of every ring as their steps pass.  The oracle resets the streams at the
    same steps (fresh contexts), as test_gpu_reset_in_flight.py does it."""
    at = {AHEAD - 1: 1, AHEAD: 2}

    def change_hop(ob, j):
        if j % H == 0 and j // H in at:
            assert ob.a.BeatriceBatch_ResetStream(None, at[j // H]) == 0
    _, want = oracle_leg(bv, oracle, model_dir, B, lambda j: audio[:, j], STEPS * H, _settings, change_hop, list(range(B)))

    def change(batch, k):
        if k in at:
            assert batch.a.BeatriceBatch_ResetStreamInFlight(batch.h, at[k]) == 0

    def drive(batch):
        return run_tick(bv, batch, STEPS, lambda k: _x(audio, H, k), change=change, chunk=7)
    _cross(bv, models, H, "resets in flight at wrap-1 and 0, %d hop(s) per step" % H, drive, _as_steps(want, H, STEPS))


# ---- stream migration ------------------------------------------------------------------------------------------------------------------------
def _on_speaker(speaker):
    def script(a, h, s, k):
        if k == 0:
            assert a.BeatriceBatch_SetTargetSpeaker(h, s, speaker) == 0
            assert a.BeatriceBatch_FlushSpeaker(h, s) == 0
    return script


@pytest.mark.parametrize("direction", ["from wrap-3 into 5", "from 5 into wrap-3"])
@pytest.mark.parametrize("H", [1, 4])
def test_streams_move_between_the_two_sides_of_the_wrap(bv, oracle, models, oracle_models, model_dir, H, direction):
    """BeatriceBatch_ExportStreams / ImportStreams with source and destination on different sides of the wrap: shift 8, and
    shift wrap - 8.  Streams 1 and 3 of the source become streams 0 and 2 of the destination and go on for 24 steps (the destination
    at wrap-3 crosses too).  Oracle: every stream is one uninterrupted stream.  Twin: the same move between batches that stand at 24
    and 32."""
    wrap, n = bv.STEP_WRAP, AHEAD
    far, near = wrap - 3 - n, wrap + 5 - n      # a batch started there stands at wrap-3 / at 5 after n steps
    if direction == "from wrap-3 into 5":
        starts, twin_starts, shift = (far, near), (0, 8), 8
    else:
        starts, twin_starts, shift = (near, far), (8, 0), wrap - 8
    src_seeds, dst_seeds, moved = [100, 101, 102, 103, 104], [110, 111, 112, 113, 114], {1: 0, 3: 2}
    xs, xd = mig.stack(bv, src_seeds, 2 * n, H), mig.stack(bv, dst_seeds, 2 * n, H)
    xm = xd[n:].copy()
    for s, t in moved.items():
        xm[:, t] = xs[n:, s]      # a moved stream's own audio goes on in its new place

    def run(s0, d0):
        src, dst = bv.Batch(models, B, hops_per_step=H, start_counter=s0), bv.Batch(models, B, hops_per_step=H, start_counter=d0)
        try:
            _settings(src)
            _settings(dst)
            got_src = mig.run_in_order(src, xs[:n])
            before = mig.run_in_order(dst, xd[:n])
            stand = src.step_counter(), dst.step_counter()
            dst.import_streams(list(moved.values()), src.export_streams(list(moved.keys())))
            after = mig.run_in_order(dst, xm)
            return got_src, before, after, stand, dst.step_counter()
        finally:
            src.close()
            dst.close()

    got_src, before, after, stand, end = run(*starts)
    print("%s, %d hop(s) per step: source at %d, destination at %d (shift %d), destination at %d after %d more steps" %
          (direction, H, stand[0], stand[1], (stand[1] - stand[0]) % wrap, end, n))
    twin = run(*twin_starts)
    counters = [(stand, (wrap - 3, 5) if shift == 8 else (5, wrap - 3)), ((stand[1] - stand[0]) % wrap, shift), (end, (stand[1] + n) % wrap),      # (a)
                ((twin[3][1] - twin[3][0]) % wrap, shift)]      # (the twin turns the rings by the same shift, far from the wrap)

    def oracle_of(seed, speaker):
        return mig.oracle_run(bv, oracle, oracle_models, model_dir, H, seed, 2 * n, _on_speaker(speaker), "speaker %d" % speaker)
    want_src = np.stack([oracle_of(src_seeds[s], s % 3)[:n] for s in range(B)], axis=1)
    came_from = {t: s for s, t in moved.items()}
    want_dst = np.stack([oracle_of(src_seeds[came_from[t]], came_from[t] % 3)[n:] if t in came_from else oracle_of(dst_seeds[t], t % 3)[n:]
                         for t in range(B)], axis=1)
    want_before = np.stack([oracle_of(dst_seeds[t], t % 3)[:n] for t in range(B)], axis=1)
    got = np.concatenate([got_src, before, after])
    _verdict("streams moved %s, %d hop(s) per step" % (direction, H), got, np.concatenate(twin[:3]),
             np.concatenate([want_src, want_before, want_dst]), counters)


# ---- the wrappers around the ticks -------------------------------------------------------------------------------------------------------
def _wrapper_oracle(bv, oracle_models, sr, block, mono):
    """The wrapper tests' oracle leg: per stream the wrapper oracle (pinned to the reference's gain.h / resample.h) around one oracle
    stream, block by block.  mono [B][n_blocks * block] -> (samples of the same shape, model hops fired per stream)."""
    wo = wrapperlib.oracle_wrapper()
    want, hops = np.zeros_like(mono), []
    for s in range(B):
        st = bv.Stream1(oracle_models, speaker=s % 3)
        fired = [0]

        def hop(in160, out240, _u, st=st, fired=fired):
            fired[0] += 1
            np.ctypeslib.as_array(out240, (240,))[:] = st.hop(np.ctypeslib.as_array(in160, (160,)).copy())
        cb = wrapperlib.HOP_FN(hop)
        p = wo.f_create(float(sr), cb, None)
        x, out = np.ascontiguousarray(mono[s]), np.zeros(mono.shape[1], np.float32)
        for k in range(mono.shape[1] // block):
            assert wo.f_process(p, x[k * block:(k + 1) * block].ctypes.data_as(wrapperlib._f32p),
                                out[k * block:(k + 1) * block].ctypes.data_as(wrapperlib._f32p), block) == 0
        wo.f_destroy(p)
        st.close()
        want[s] = out
        hops.append(fired[0])
    assert len(set(hops)) == 1      # the batch's clocks are every stream's
    return want, hops[0]


def test_48k_wrapper_around_the_ticks(bv, models, oracle_models):
    """BeatriceBatch_BindResidentIO48k, one hop per step, mono: 48 blocks fed without waiting -- the block a tick completes leaves
    through the wrapper launch of the NEXT tick (deferred step and slot), beside stage counters on both sides of the wrap.  On
    test_gpu_wrapper48k.py's oracle leg (the wrapper oracle around oracle streams)."""
    blocks = STEPS
    x = np.stack([wrapperlib.test_signal(480 * blocks, 48000, seed=9800 + 7 * s) for s in range(B)]).astype(np.float32)
    want, hops = _wrapper_oracle(bv, oracle_models, 48000, 480, x)
    assert hops == blocks
    hip = Hip()

    def drive(batch):
        a, h = batch.a, batch.h
        slots = blocks
        assert slots > a.BeatriceBatch_TickStages(h)
        d_in, d_out = hip.malloc(slots * B * 480 * 4), hip.malloc(slots * B * 480 * 4)
        try:
            assert a.BeatriceBatch_BindResidentIO48k(h, d_in, d_out, 1, slots) == 0
            hip.h2d(d_in, np.ascontiguousarray(x.reshape(B, blocks, 480).transpose(1, 0, 2)))      # [slots][B][1][480]
            for k in range(blocks):
                assert a.BeatriceBatch_ConvertBlocks48kDevice(h, None, None, 1) == 0
            assert a.BeatriceBatch_Synchronize(h) == 0
            out = np.zeros((slots, B, 480), np.float32)
            hip.d2h(out, d_out)
            assert a.BeatriceBatch_BindResidentIO48k(h, None, None, 0, 0) == 0
        finally:
            hip.free(d_in)
            hip.free(d_out)
        return np.ascontiguousarray(out.transpose(1, 0, 2)).reshape(B, blocks * 480)
    _cross(bv, models, 1, "48 kHz wrapper around the ticks", drive, want)


def test_any_rate_wrapper_around_the_ticks(bv, models, oracle_models):
    """BeatriceBatch_BindResidentBlocks at 44.1 kHz, blocks of 441 samples, mono, one hop per step: every call fed without waiting.
    On test_gpu_wrapper_tick.py's oracle leg."""
    sr, block, n_blocks = 44100, 441, STEPS + 4
    total = block * n_blocks
    x = np.stack([wrapperlib.test_signal(total, sr, seed=9900 + 7 * s) for s in range(B)]).astype(np.float32)
    want, hops = _wrapper_oracle(bv, oracle_models, sr, block, x)
    assert STEPS <= hops <= n_blocks      # that many model steps
    hip = Hip()

    def drive(batch):
        a, h = batch.a, batch.h
        assert a.BeatriceBatch_ConfigureWrapper(h, float(sr)) == 0
        slots = n_blocks + a.BeatriceBatch_ResidentBlocksDelayFor(h, block) + 2
        d_in, d_out = hip.malloc(slots * B * block * 4), hip.malloc(slots * B * block * 4)
        try:
            assert a.BeatriceBatch_BindResidentBlocks(h, d_in, d_out, 1, block, slots) == 0
            buf = np.zeros((slots, B, block), np.float32)      # [slots][B][1][block]
            buf[:n_blocks] = x.reshape(B, n_blocks, block).transpose(1, 0, 2)
            hip.h2d(d_in, buf)
            for k in range(n_blocks):
                assert a.BeatriceBatch_ProcessBlocksDevice(h, None, None, 1, block) == 0
            assert a.BeatriceBatch_Synchronize(h) == 0
            assert a.BeatriceBatch_ResidentBlocksOwed(h) == 0
            out = np.zeros((slots, B, block), np.float32)
            hip.d2h(out, d_out)
            assert a.BeatriceBatch_BindResidentBlocks(h, None, None, 0, 0, 0) == 0
        finally:
            hip.free(d_in)
            hip.free(d_out)
        return np.ascontiguousarray(out[:n_blocks].transpose(1, 0, 2)).reshape(B, total)
    _cross(bv, models, 1, "any-rate wrapper (44.1 kHz) around the ticks", drive, want, steps=hops)


# ---- the 1-stream ABI -------------------------------------------------------------------------------------------------------------------------
KEYS = ("phone", "q", "feat", "pcm")


def _identical(what, got, want, twin):
    for key in KEYS:
        dev = float(np.abs(np.asarray(got[key], np.float64) - np.asarray(want[key], np.float64)).max())
        print("%s %s: vs ORACLE max-abs %g, array_equal %s; vs TWIN at 0 array_equal %s" %
              (what, key, dev, np.array_equal(got[key], want[key]), np.array_equal(got[key], twin[key])))
    for key in KEYS:
        assert np.array_equal(got[key], twin[key]), key
        assert np.array_equal(got[key], want[key]), key


@pytest.mark.parametrize("launches", ["team", "per layer"])
def test_one_stream_abi(bv, oracle, product, model_dir, launches):
    """Beatrice20rc0_*: contexts started at wrap - 24, 48 hops; phone vector, bin, features and samples per hop bit-identical to the
    oracle (regimes.drive, as test_gpu_regimes.py asserts it) and to a twin started at 0.  Both drives: the team launches, and the
    per-layer chain -- which a context runs once a team launch has timed out (test_gpu_realtime_contract.py): the time-out is
    injected into all three contexts before a hop in front of the 48, which returns zeros and restarts them from silence."""
    bv.bind_batch(product)
    wrap, lead = bv.STEP_WRAP, 1 if launches == "per layer" else 0
    x = bv.synth_audio(160 * (STEPS + lead), seed=9950)
    kw = dict(speaker=1, formant_index=6, vq_k=2, min_q=1, max_q=447)
    seen = {}

    def change(st, h):
        if h == 0:
            seen["before"] = st.hop_counts()
            if lead:
                assert product.BeatriceHip_InjectTeamTimeoutPhone(st.pc) == 0
                assert product.BeatriceHip_InjectTeamTimeoutPitch(st.tc) == 0
                assert product.BeatriceHip_InjectTeamTimeout(st.wc) == 0
        if h == STEPS + lead - 1:
            seen["last"] = st.hop_counts()

    def cut(d):
        if lead:
            assert not d["pcm"][:240].any() and not d["phone"][0].any()      # the call that hit the time-out: zeros
        return dict(pcm=d["pcm"][240 * lead:], phone=d["phone"][lead:], q=d["q"][lead:], feat=d["feat"][lead:])
    want = R.drive(bv, oracle, model_dir, x[160 * lead:], **kw)
    runs = []
    for start in (wrap - AHEAD - lead, 0):
        runs.append(cut(R.drive(bv, product, model_dir, x, change=change, start_counter=start, **kw)))
        print("1-stream ABI, %s launches: hop counters %r before, %r at the last hop" % (launches, seen["before"], seen["last"]))
        assert seen["before"] == (start,) * 3
        assert seen["last"] == ((STEPS - AHEAD - 1 if start else STEPS + lead - 1),) * 3      # (a)
    assert np.abs(want["pcm"]).max() > 1e-3
    _identical("1-stream ABI, %s launches" % launches, runs[0], want, runs[1])


def test_one_stream_abi_legacy(bv, built, product, tmp_path):
    """Beatrice20b1_*: the same for the legacy generation (regimes.drive_legacy; make_model's legacy package)."""
    import sys
    sys.path.insert(0, os.path.join(R.REPO, "tools"))
    import make_model
    d = str(tmp_path)
    make_model.make_model_legacy(d, n_speakers=3)
    wrap = bv.STEP_WRAP
    oracle = bv.AbiLegacy(os.path.join(R.REPO, "oracle", "libbeatrice_oracle.so"), "20b1")
    hip = bv.AbiLegacy(bv.PRODUCT_LIB, "20b1")
    x = bv.synth_audio(160 * STEPS, seed=9960)
    want = R.drive_legacy(bv, oracle, d, x, speaker=1)
    runs = []
    for start in (wrap - AHEAD, 0):
        m = bv.ModelsLegacy(hip, d)
        st = bv.StreamLegacy(m, speaker=1, start_counter=start)
        before = st.hop_counts()
        outs = [st.hop(x[h * 160:(h + 1) * 160], return_all=True) for h in range(STEPS)]
        after = st.hop_counts()
        assert hip.lib.BeatriceHip_SetHopCountLegacy(1, st.pc, 0) == -1 and st.hop_counts() == after      # not after the first hop
        st.close()
        m.close()
        print("legacy 1-stream ABI: hop counters %r before, %r after" % (before, after))
        assert before == (start,) * 3 and after == ((STEPS - AHEAD if start else STEPS),) * 3      # (a)
        runs.append(dict(pcm=np.concatenate([o[0] for o in outs]), phone=np.stack([o[1] for o in outs]), q=np.array([o[2] for o in outs]),
                         feat=np.stack([o[3] for o in outs])))
    assert np.abs(want["pcm"]).max() > 1e-3
    _identical("legacy 1-stream ABI", runs[0], want, runs[1])


# ---- starts that production never sees, and refusals ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drive_name", ["in order", "tick mode"])
def test_unaligned_start(bv, models, audio, plain_hops, drive_name):
    """wrap - 7: the counter is NOT congruent to the number of steps modulo 3 or 4.  Nothing may depend on that relation: the slots of
    the settings copies, events and phone vectors are the counter's, never the step number's."""
    H = 1

    def drive(batch):
        if drive_name == "in order":
            return np.stack([batch.convert(_x(audio, H, k)) for k in range(STEPS)])
        return run_tick(bv, batch, STEPS, lambda k: _x(audio, H, k), chunk=7)
    _cross(bv, models, H, "%s from wrap-7" % drive_name, drive, _as_steps(plain_hops, H, STEPS), ahead=7)


def test_refusals(bv, models, audio):
    wrap = bv.STEP_WRAP
    batch = bv.Batch(models, B)
    a, h = batch.a, batch.h
    try:
        _settings(batch)
        assert a.BeatriceBatch_StepCounter(None) == -1
        assert batch.step_counter() == 0
        for bad in (-1, wrap, wrap + 5):
            assert a.BeatriceBatch_SetStepCounter(h, bad) == -1 and batch.step_counter() == 0
        assert a.BeatriceBatch_SetStepCounter(h, wrap - 1) == 0 and batch.step_counter() == wrap - 1
        assert a.BeatriceBatch_SetStepCounter(h, 7) == 0 and batch.step_counter() == 7      # still fresh: may be set again
        r = Resident(bv, batch, tick=False)
        try:
            assert a.BeatriceBatch_SetStepCounter(h, 9) == -1 and batch.step_counter() == 7      # a binding
            assert a.BeatriceBatch_EnableTickPipeline(h, 1) == 0
            assert a.BeatriceBatch_SetStepCounter(h, 9) == -1 and batch.step_counter() == 7      # inside tick mode
            assert a.BeatriceBatch_EnableTickPipeline(h, 0) == 0
            assert a.BeatriceBatch_BindResidentIO(h, None, None, 0) == 0
        finally:
            r.free()
        assert a.BeatriceBatch_SetStepCounter(h, wrap - 2) == 0      # (no step was taken, nothing is bound any more)
        y = [batch.convert(_x(audio, 1, k)) for k in range(3)]
        assert batch.step_counter() == 1
        assert a.BeatriceBatch_SetStepCounter(h, 9) == -1 and batch.step_counter() == 1          # after the first step
        assert np.isfinite(np.stack(y)).all()
    finally:
        batch.close()
    # 1-stream contexts: range, kind, and not after the first hop
    st = bv.Stream1(models, start_counter=wrap - 1)
    try:
        fn = models.abi.BeatriceHip_SetHopCount
        assert st.hop_counts() == (wrap - 1,) * 3
        for kind, ctx in ((1, st.pc), (2, st.tc), (3, st.wc)):
            assert fn(kind, ctx, -1) == -1 and fn(kind, ctx, wrap) == -1 and fn(0, ctx, 5) == -1 and fn(4, ctx, 5) == -1
        assert fn(1, None, 5) == -1 and models.abi.BeatriceHip_HopCount(1, None) == -1
        assert st.hop_counts() == (wrap - 1,) * 3
        st.hop(audio[0, 0])
        assert st.hop_counts() == (0, 0, 0)
        for kind, ctx in ((1, st.pc), (2, st.tc), (3, st.wc)):
            assert fn(kind, ctx, 5) == -1
        assert st.hop_counts() == (0, 0, 0)
    finally:
        st.close()
