"""BeatriceBatch_ResetStreamInFlight in host streaming (BeatriceBatch_StreamFrames: the tick pipeline fed from and drained to host
buffers): resets in mid-stream and one inside the last BeatriceBatch_HostStreamDelay() calls, carried to the end by BeatriceBatch_StreamFlush.
Yardsticks, both at max-abs 0: an in-order BeatriceBatch_ConvertFrames twin with the drained BeatriceBatch_ResetStream at the same steps, and
the oracle on every stream."""
import numpy as np
import pytest

from oracle_batch import OracleBatch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("H", [1, 2])
def test_resets_in_flight_in_host_streaming(bv, oracle, product, model_dir, H):
    B, steps = 8, 60
    m = bv.Models(product, model_dir)
    bv.bind_batch(product)
    audio = np.stack([bv.synth_audio(160 * H * steps, seed=8300 + s) for s in range(B)]).reshape(B, steps, H * 160).copy()
    audio[2, 14:18] = 0.0

    def settings(a, h):
        for s in range(B):
            assert a.BeatriceBatch_SetTargetSpeaker(h, s, s % 3) == 0
        assert a.BeatriceBatch_SetVQNumNeighbors(h, 2, 2) == 0
        assert a.BeatriceBatch_FlushSpeaker(h, -1) == 0

    def script(a, h, reset, k):
        if k == 0:
            assert reset(7) == 0
        if k in (9, 12):
            assert reset(k - 8) == 0
        if k == 21:
            assert a.BeatriceBatch_SetTargetSpeaker(h, 5, 1) == 0
        if k in (22, 30):
            assert reset(5) == 0
        if k == 38:
            assert reset(-1) == 0
        if k == 44:
            assert reset(2) == 0
        if k == steps - 5:   # inside the last HostStreamDelay() calls: the flush carries it
            assert reset(3) == 0

    twin = bv.Batch(m, B, hops_per_step=H)
    settings(twin.a, twin.h)
    ref = []
    for k in range(steps):
        script(twin.a, twin.h, lambda s: twin.a.BeatriceBatch_ResetStream(twin.h, s), k)
        ref.append(twin.convert(np.ascontiguousarray(audio[:, k])))
    twin.close()
    ref = np.stack(ref)

    batch = bv.Batch(m, B, hops_per_step=H)
    a, h = batch.a, batch.h
    settings(a, h)
    assert a.BeatriceBatch_EnableHostStreaming(h, 1) == 0
    assert a.BeatriceBatch_HostStreamDelay(h) > 5
    out = np.zeros((B, H * 240), np.float32)
    got = []
    for k in range(steps):
        script(a, h, lambda s: a.BeatriceBatch_ResetStreamInFlight(h, s), k)
        rc = a.BeatriceBatch_StreamFrames(h, bv.fptr(np.ascontiguousarray(audio[:, k])), bv.fptr(out))
        assert rc in (0, 1)
        if rc == 1:
            got.append(out.copy())
    assert a.BeatriceBatch_TicksLaunched(h) == steps   # nothing drained on the way
    while True:
        rc = a.BeatriceBatch_StreamFlush(h, bv.fptr(out))
        assert rc in (0, 1)
        if rc == 0:
            break
        got.append(out.copy())
    assert a.BeatriceBatch_EnableHostStreaming(h, 0) == 0
    batch.close()
    m.close()
    got = np.stack(got)
    assert got.shape == ref.shape and np.abs(ref).max() > 0.05
    bad = [(k, s, float(np.abs(got[k, s] - ref[k, s]).max())) for k in range(steps) for s in range(B) if not np.array_equal(got[k, s], ref[k, s])]
    assert not bad, "host streaming vs the in-order twin, (step, stream, max-abs): %s" % bad[:12]

    ob = OracleBatch(bv, oracle, model_dir, B, hops_per_step=H)
    settings(ob.a, None)
    for k in range(steps):
        script(ob.a, None, lambda s: ob.a.BeatriceBatch_ResetStream(None, s), k)
        for s, y in ob.convert(audio[:, k]).items():
            assert np.array_equal(got[k, s], y), "stream %d step %d vs the oracle: max-abs %g" % (s, k, float(np.abs(got[k, s] - y).max()))
    ob.close()
