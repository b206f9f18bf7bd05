"""The oracle's restatement of the open-source wrapper (oracle/wrapper_oracle.c) against
  (a) the library built from the reference's own headers (oracle/_ref/libref_wrapper.so), live, and
  (b) the golden vectors minted from that library (tests/golden/wrapper_*.npz).
Bit-exact is required: both sides do the same float32 multiply-accumulate order."""
import os

import numpy as np
import pytest

import wrapperlib

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RATES = [16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 192000]


@pytest.fixture(scope="module")
def wo(built):
    if not os.path.exists(wrapperlib.ORACLE_WRAPPER):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(wrapperlib.REPO, "oracle"), "libwrapper_oracle.so"], env={k: v for k, v in os.environ.items() if k != "LD_PRELOAD"})
    return wrapperlib.oracle_wrapper()


@pytest.fixture(scope="module")
def ref():
    """the library built from the reference's headers, or None where oracle/_ref could not be built"""
    return wrapperlib.ref_wrapper()


@pytest.mark.parametrize("sr", RATES)
def test_chain_matches_golden(wo, sr):
    g = np.load(os.path.join(GOLD, "wrapper_chain.npz"))
    x, want = g["in_%d" % sr], g["out_%d" % sr]
    for block in (441, 64, 4096):  # streaming invariance: block size must not change a single sample
        got = wo.run_chain(sr, x, block)
        assert np.array_equal(got, want), "sr=%d block=%d max-abs %g" % (sr, block, np.abs(got - want).max())
    # sanity pinned by the reference's structure: first 480 samples @48 kHz (10 ms) are the FIFO's zeros
    assert np.all(want[: int(0.01 * sr) - 40] == 0.0)
    assert np.abs(want).max() > 0.01


def test_fraction_matches_golden(wo):
    g = np.load(os.path.join(GOLD, "wrapper_fraction.npz"))
    for r, (n, d) in zip(g["ratio"], g["frac"]):
        assert wo.fraction(float(r)) == (int(n), int(d))
    assert wo.fraction(48000 / 44100) == (160, 147)
    assert wo.fraction(1.0) == (1, 1)


def test_gain_matches_golden(wo):
    g = np.load(os.path.join(GOLD, "wrapper_gain.npz"))
    for sr in (16000, 48000, 96000):
        ev = [(int(a), float(b)) for a, b in g["ev_%d" % sr]]
        got = wo.gain_trace(sr, g["in_%d" % sr], ev)
        assert np.array_equal(got, g["out_%d" % sr])
    got = wo.run_chain(48000, g["chain_in"], 480, in_gain_events=[(0, -6.0), (2400, 3.0)], out_gain_events=[(960, 6.0)])
    assert np.array_equal(got, g["chain_out"])


LIVE_CASES = [(44100, 1), (48000, 512), (22050, 480), (192000, 441), (32000, 37)]


def live_chain_input(sr):
    return wrapperlib.test_signal(int(0.06 * sr), sr, seed=1000 + sr)


@pytest.mark.parametrize("sr,block", LIVE_CASES)
def test_chain_matches_reference_live(wo, ref, sr, block):
    """against the reference's library where oracle/_ref is built, and always against its outputs for these cases as recorded in
    reference_cases.npz (tools/make_golden.py); where the library is there, the recording must still be what it computes"""
    x = live_chain_input(sr)
    want = np.load(os.path.join(GOLD, "reference_cases.npz"))["chain_%d_%d" % (sr, block)]
    if ref is not None:
        a = ref.run_chain(sr, x, block)
        assert np.array_equal(a, want), "recording out of date: max-abs %g" % np.abs(a - want).max()
    b = wo.run_chain(sr, x, block)
    assert np.array_equal(want, b), "max-abs %g" % np.abs(want - b).max()


VANISHING_CASES = [(44100, 441), (48000, 480), (16000, 333)]


@pytest.mark.parametrize("sr,block", VANISHING_CASES)
def test_vanishing_chain_matches_reference_live(wo, ref, sr, block):
    """A signal that decays through the subnormal range and returns, input gain -30 dB, output gain moving to -60 dB across the decay
    (MODEL_SPEC 2.5: nothing is flushed): the wrapper oracle against the reference's own gain.h / resample.h, live where
    oracle/_ref is built, and always against its outputs as recorded in golden/wrapper_vanishing.npz."""
    n = int(0.12 * sr)
    x = wrapperlib.vanishing_signal(n, sr, seed=2000 + sr)
    ev_in, ev_out = wrapperlib.vanishing_gain_events(n)
    tiny = np.abs(x[(x != 0)])
    assert (tiny < 2.0 ** -126).sum() > 0.1 * n and (x == 0).any() and np.abs(x[-n // 4:]).max() > 0.1
    want = np.load(os.path.join(GOLD, "wrapper_vanishing.npz"))["chain_%d_%d" % (sr, block)]
    if ref is not None:
        a = ref.run_chain(sr, x, block, in_gain_events=ev_in, out_gain_events=ev_out)
        assert np.array_equal(a, want), "recording out of date: max-abs %g" % np.abs(a - want).max()
    b = wo.run_chain(sr, x, block, in_gain_events=ev_in, out_gain_events=ev_out)
    assert np.array_equal(want, b), "max-abs %g" % np.abs(want - b).max()
    out_tiny = np.abs(want[want != 0])
    assert (out_tiny < 2.0 ** -126).sum() > 0.05 * n, "the output passes through the subnormal range too"
    assert np.abs(want).max() > 1e-3


def test_dc_gain_is_half(wo):
    """Zero-stuffing 240 -> 480 has no make-up gain, so DC through an identity-like hop comes out at 0.5
    (SURVEY.md appendix A.3)."""
    x = np.full(48000 // 2, 0.25, np.float32)
    y = wo.run_chain(48000, x, 480)
    assert abs(float(y[-2000:].mean()) - 0.125) < 2e-3
