"""The device-side wrapper and the model behind it with a signal that decays through the subnormal range and returns (MODEL_SPEC
2.5): against oracle/wrapper_oracle.c -- pinned to the reference's headers on the same kind of signal by
tests/test_wrapper_oracle.py -- around the oracle model, per stream, bit for bit.  The model is the `vanishing` package of
tests/regimes.py, so the kernels behind the wrapper see subnormal values as well.

What this reaches is the wrapper's INPUT side: the stereo mix, the input gain (-30 dB) and the input resampler work on subnormal
samples and hand subnormal samples to the model (asserted below).  The OUTPUT side is not reached, and cannot be through the model:
the generator ends in MODEL_SPEC's tanh, which is 0 below 2^-25, so a hop's samples are 0 or at least 2^-25, and -60 dB of output
gain leaves them near 2^-35.  The output resampler and output gain with subnormal samples are covered on the CPU only, where
tests/test_wrapper_oracle.py puts a stub hop behind the wrapper oracle and the reference's own headers."""
import numpy as np
import pytest

import math_points as mp
import regimes as R
import wrapperlib

pytestmark = pytest.mark.gpu
B = 3


@pytest.fixture(scope="module")
def vanishing_dir(bv, tmp_path_factory):
    return R.package(bv, "vanishing", str(tmp_path_factory.mktemp("vanishing")))


@pytest.mark.parametrize("sr,block,channels", [(44100, 441, 1), (48000, 480, 2)])
def test_device_wrapper_with_a_vanishing_signal(bv, oracle, product, vanishing_dir, sr, block, channels):
    assert mp.oracle_keeps_subnormals(oracle), "this process flushes subnormals: the oracle cannot be trusted here"
    n_blocks = 16
    total = block * n_blocks
    x = np.zeros((B, channels, total), np.float32)
    for s in range(B):
        for c in range(channels):
            x[s, c] = (0.5 if c else 1.0) * wrapperlib.vanishing_signal(total, sr, seed=2100 + 7 * s + c)
    ev = {s: wrapperlib.vanishing_gain_events(total) for s in range(B)}
    ev_in = {s: [(p // block * block, g) for p, g in ev[s][0]] for s in range(B)}
    ev_out = {s: [(p // block * block, g - 6.0 * s) for p, g in ev[s][1]] for s in range(B)}

    mo = bv.Models(oracle, vanishing_dir)
    want = np.zeros((B, total), np.float32)
    fed = []      # every 160-sample frame the wrapper oracle hands to the model
    for s in range(B):
        st = bv.Stream1(mo, speaker=s % 3, vq_k=s % 2)

        def hop(in160, out240, _u, st=st):
            x160 = np.ctypeslib.as_array(in160, (160,)).copy()
            fed.append(x160)
            np.ctypeslib.as_array(out240, (240,))[:] = st.hop(x160)

        mono = x[s, 0] if channels == 1 else ((x[s, 0] + x[s, 1]) * np.float32(0.5)).astype(np.float32)
        want[s] = wrapperlib.oracle_wrapper().run_chain(sr, mono, block, hop=hop, in_gain_events=list(ev_in[s]), out_gain_events=list(ev_out[s]))
        st.close()
    mo.close()
    assert np.isfinite(want).all() and all(want[s].std() > 0 for s in range(B))
    fed = np.abs(np.concatenate(fed))
    share = ((fed > 0) & (fed < 2.0 ** -126)).mean()
    print("behind mix, input gain and input resampler: %.1f %% of the model's input samples are subnormal, %.1f %% are 0, peak %.3g" % (
        100 * share, 100 * (fed == 0).mean(), fed.max()))
    assert share >= 0.10 and fed.max() > 1e-3, "the input side of the wrapper works in the subnormal range and leaves it"

    m = bv.Models(product, vanishing_dir)
    batch = bv.Batch(m, B)
    a, h = batch.a, batch.h
    for s in range(B):
        a.BeatriceBatch_SetTargetSpeaker(h, s, s % 3)
        a.BeatriceBatch_SetVQNumNeighbors(h, s, s % 2)
    a.BeatriceBatch_FlushSpeaker(h, -1)
    assert a.BeatriceBatch_ConfigureWrapper(h, float(sr)) == 0
    got = np.zeros_like(x)
    for k in range(n_blocks):
        pos = k * block
        for s in range(B):
            while ev_in[s] and ev_in[s][0][0] <= pos:
                a.BeatriceBatch_SetInputGain(h, s, ev_in[s].pop(0)[1])
            while ev_out[s] and ev_out[s][0][0] <= pos:
                a.BeatriceBatch_SetOutputGain(h, s, ev_out[s].pop(0)[1])
        xin = np.ascontiguousarray(x[:, :, pos:pos + block])
        out = np.zeros_like(xin)
        assert a.BeatriceBatch_ProcessBlocks(h, bv.fptr(xin), bv.fptr(out), channels, block) == 0
        got[:, :, pos:pos + block] = out
    batch.close()
    m.close()
    same = np.array_equal(got[:, 0], want)
    print("device wrapper sr=%d block=%d ch=%d, vanishing: max-abs %g, %d of %d differ" % (sr, block, channels, np.abs(got[:, 0] - want).max(),
                                                                                          (got[:, 0] != want).sum(), want.size))
    if channels == 2:
        assert np.array_equal(got[:, 0], got[:, 1])
    assert same
