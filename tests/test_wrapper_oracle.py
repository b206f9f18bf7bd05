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


# The rates of tests/wrapper_edge_cases.py -- ratios 4, 6 and 8 on both sides of 48 kHz, tap tables beyond 7168 floats, fractions the < 1000
# search truncates -- with the table's own scripts: steady 10 ms blocks around 48 calls of one sample everywhere, and MaxWrapperBlock three
# times in a row where the table takes it (three calls at 384 kHz too: the recording stays small).  Both gains ramp in both directions.
EDGE_GAINS = {1: (-24.0, 6.0), 2: (3.0, -18.0), 20: (-9.0, 2.0)}


def edge_cases():
    import wrapper_edge_cases as E
    cases = [(rate, "ones", E.script_blocks(rate, "ones")) for rate in E.RATES if rate != 48000.0]
    cases += [(rate, "longest", E.script_blocks(rate, "longest")[:3]) for rate in (6000.0, 11025.0, 384000.0)]
    return cases


def edge_input(rate, kind, blocks):
    return wrapperlib.test_signal(sum(blocks), int(rate), seed=3000 + int(rate) % 977 + (500 if kind == "longest" else 0))


@pytest.mark.parametrize("rate,kind,blocks", edge_cases(), ids=lambda v: None if isinstance(v, list) else str(v))
def test_edge_rate_chain_matches_reference_live(wo, ref, rate, kind, blocks):
    """as test_chain_matches_reference_live, at the table's rates: live where oracle/_ref is built, and always against the reference's outputs
    as recorded in reference_cases_edge_rates.npz (tools/make_golden.py edge_rates).  Outputs only; the inputs come from seeds."""
    x = edge_input(rate, kind, blocks)
    want = np.load(os.path.join(GOLD, "reference_cases_edge_rates.npz"))["chain_%s_%s" % (repr(rate), kind)]
    if ref is not None:
        a = ref.run_blocks(rate, x, blocks, gains=EDGE_GAINS)
        assert np.array_equal(a, want), "recording out of date: max-abs %g" % np.abs(a - want).max()
    b = wo.run_blocks(rate, x, blocks, gains=EDGE_GAINS)
    assert np.array_equal(want, b), "max-abs %g, first at %d" % (np.abs(want - b).max(), int(np.argmax(want != b)))
    assert np.isfinite(want).all() and np.abs(want[int(0.03 * rate):]).max() > 1e-3


def test_edge_rate_fractions_match_the_reference(wo, ref):
    """the table's fractions (and the four rates the product refuses) through the oracle's search and, where built, the reference's"""
    import wrapper_edge_cases as E
    for rate, frac in list(E.RATES.items()) + [(r, None) for r in E.REFUSED_RATES]:
        ratio = max(rate, 48000.0) / min(rate, 48000.0)
        got = wo.fraction(ratio)
        assert got == E.simple_fraction(ratio) and (frac is None or got == frac), (rate, got, frac)
        if ref is not None:
            assert ref.fraction(ratio) == got, rate


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


# A host that changes its rate in mid-life (ProcessorCore2::SetSampleRate, processor_core_2.cc:421-429): every leg ends with the FIFO part
# filled and, from the second leg on, begins with both gain ramps in flight (a change of 40 dB and more set at the leg's start, legs
# shorter than the 20+ ms such a ramp takes); the fourth leg repeats the third's rate -- the reference's no-op: nothing restarts.
RATE_WALK_LEGS = [(44100, 441, 1500, -6.0, 3.0), (48000, 480, 700, -46.0, -40.0), (44100, 64, 900, 0.0, 6.0), (44100, 441, 1000, -40.0, -36.0),
                  (16000, 333, 800, 3.0, 0.0), (96000, 960, 3000, -40.0, 0.0), (44100, 441, 1500, 0.0, 0.0)]


def rate_walk_input():
    return wrapperlib.test_signal(sum(leg[2] for leg in RATE_WALK_LEGS), 44100, seed=4242)


def test_set_sample_rate_matches_reference_live(wo, ref):
    """wo_set_sample_rate against the reference's own AnyFreqInOut::SetSampleRate / Gain::Context::SetSampleRate, live where oracle/_ref is
    built, and always against its outputs as recorded in golden/wrapper_rate_walk.npz (tools/make_golden.py rate_walk)."""
    x = rate_walk_input()
    want = np.load(os.path.join(GOLD, "wrapper_rate_walk.npz"))["walk"]
    if ref is not None and ref.has_set_rate:
        a = ref.run_rate_walk(x, RATE_WALK_LEGS)
        assert np.array_equal(a, want), "recording out of date: max-abs %g" % np.abs(a - want).max()
    b = wo.run_rate_walk(x, RATE_WALK_LEGS)
    assert np.array_equal(want, b), "max-abs %g" % np.abs(want - b).max()
    # what the walk is about is in it: a restart empties the FIFO (the first 10 ms of a leg at a new rate are zeros), the no-op leg has none
    starts = np.cumsum([0] + [leg[2] for leg in RATE_WALK_LEGS])
    for i, (sr, _block, _n, _gi, _go) in enumerate(RATE_WALK_LEGS):
        head = want[starts[i]:starts[i] + int(0.009 * sr)]
        restarted = i == 0 or RATE_WALK_LEGS[i - 1][0] != sr
        assert (np.abs(head).max() == 0.0) == restarted, "leg %d" % i
    assert np.abs(want[starts[-2]:]).max() > 1e-3
    # a restart at the same rate is SetSampleRate(another rate), SetSampleRate(the rate): not the no-op
    again = wo.run_rate_walk(x, [leg for i, leg in enumerate(RATE_WALK_LEGS) for leg in ([(8000, 1, 0, leg[3], leg[4])] if i == 3 else []) + [leg]])
    assert np.array_equal(again[:starts[3]], want[:starts[3]]) and not np.array_equal(again[starts[3]:starts[4]], want[starts[3]:starts[4]])


def test_dc_gain_is_half(wo):
    """Zero-stuffing 240 -> 480 has no make-up gain, so DC through an identity-like hop comes out at 0.5
    (SURVEY.md appendix A.3)."""
    x = np.full(48000 // 2, 0.25, np.float32)
    y = wo.run_chain(48000, x, 480)
    assert abs(float(y[-2000:].mean()) - 0.125) < 2e-3
