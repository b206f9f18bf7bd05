"""The numeric regimes of tests/regimes.py on the CPU: (1) the float64 restatement WITNESSES that each package reaches its regime
(a regime that is not reached would make tests/test_gpu_regimes.py an ordinary parity test); (2) the oracle against the restatement,
module by module as in tests/test_cpu_spec_crosscheck.py, so that a misreading shared by oracle and kernels does not hide where
activations saturate, vanish or tie; (3) MODEL_SPEC 2.1's scalar functions, oracle against float64, on the point set of
tests/math_points.py.

Tolerances are not invented: RECORDED holds the maximum deviation observed per regime and module (oracle float32 against
float64, x86-64, glibc 2.35), each beside the scale of the compared output, and the tests assert twice that figure -- the oracle is
deterministic; the margin covers another libm behind numpy's float64 exp / tanh / log."""
import os

import numpy as np
import pytest

import math_points as mp
import regimes as R
import spec_numpy as sn

HOPS = R.HOPS
STREAM = dict(speaker=1, formant_index=6, min_q=1, max_q=447)

# (max-abs deviation, scale of the output it was observed at = max-abs of the float64 values; pcm: rms)
RECORDED = {
    "hot": dict(phone=(2.19e-4, 4.41), knn=(1.59e-7, 1.59), f0=(3.04e-5, 1.0), energy=(6.64e-8, 0.82), delta=(0.0, 1.0),
                voicing=(2.34e-6, 0.825), wave0=(1.23e-5, 0.539), wave3=(7.18e-6, 0.434)),
    "vanishing": dict(phone=(1.39e-7, 3.87e-7), knn=(1.19e-7, 1.52), f0=(1.81e-6, 0.81), energy=(6.64e-8, 1.84), delta=(0.0, 1.0),
                      voicing=(2.91e-7, 0.808), wave0=(7.07e-7, 0.0445), wave3=(6.24e-7, 0.0545)),
    # (f0 is exactly 1/4 on both sides: four tied maxima, every other term of the softmax below 2^-76)
    "ties": dict(phone=(1.83e-6, 2.74), knn=(5.96e-8, 0.898), f0=(0.0, 0.25), energy=(6.64e-8, 0.82), delta=(0.0, 1.0),
                 voicing=(4.63e-7, 0.826), wave0=(1.03e-6, 0.236), wave3=(9.15e-7, 0.204)),
}
# MODEL_SPEC 2.1, oracle against the float64 value of the definition (exp's argument clamp included), on math_points.points():
# ulp = float32's spacing at the true value.  The same figures stand in MODEL_SPEC 2.1's table.
MATH_RECORDED = {"exp": ("ulp", 2.73), "sigmoid": ("ulp", 3.39), "log": ("ulp", 2.65), "lrelu": ("ulp", 0.61),
                 "tanh": ("abs", 1.55e-7), "gelu": ("abs", 4.28e-7)}


LEGACY_RECORDED = {"hot": (2.03e-6, 0.52), "vanishing": (1.35e-6, 0.476)}     # generator of the legacy packages: (max-abs, pcm rms)


def _within(regime, what, dev, scale):
    rec, at = RECORDED[regime][what]
    print("%s %s: max-abs %.3g at scale %.3g (recorded %.3g at %.3g)" % (regime, what, dev, scale, rec, at))
    assert dev <= 2.0 * rec, "%s %s: %.3g > 2 x recorded %.3g" % (regime, what, dev, rec)


@pytest.fixture(scope="module", params=["hot", "vanishing", "ties"])
def regime(request, bv, oracle, tmp_path_factory):
    name = request.param
    d = R.package(bv, name, str(tmp_path_factory.mktemp("regime_" + name)))
    x = R.regime_audio(bv, name)
    rec, out = R.restate(d, x, speaker=1, formant_index=6, vq_k=8 if name == "ties" else 0)
    driven = {k: R.drive(bv, oracle, d, x, vq_k=k, **STREAM) for k in (0, 3)}
    return name, d, x, rec, out, driven


# ---- (1) witnesses -----------------------------------------------------------------------------------------------------------
def test_regime_is_reached(regime):
    name, d, x, rec, out, _ = regime
    assert all(np.isfinite(v).all() for v in out.values() if v is not None), "the restatement's outputs are finite"
    if name == "hot":
        for i in range(sn.N_BLOCKS):
            rows = (rec["wave.B%d.att.s" % i][0].min(1) < -86.0).sum()
            share = (np.abs(rec["wave.B%d.c1.out" % i][0]) > 5.0).mean()
            print("wave block %d: %d of %d attention rows reach below -86; %.2f of the gelu arguments beyond 5" % (i, rows, HOPS, share))
            assert rows >= HOPS // 2 and share >= 0.25
        for i in range(4):
            share = (np.abs(rec["phone.R%d.out" % i][0]) > 5.0).mean()
            print("phone residual conv %d: %.2f of the gelu arguments beyond 5" % (i, share))
            assert share >= 0.25
        for g in ("phone.gru.gate", "pitch.gru.gate"):
            a = np.array(rec[g])
            print("%s: arguments in [%.1f, %.1f]" % (g, a.min(), a.max()))
            assert a.max() > 17.0 and a.min() < -17.0
        f0 = out["feat"][:, 0].astype(np.float32)
        print("f0 rounds to 1.0 in %d hops" % (f0 == 1.0).sum())
        assert (f0 == 1.0).any()
        pcm = out["pcm"]
        sat, rms = (np.abs(pcm) >= 0.999).mean(), np.sqrt((pcm ** 2).mean())
        print("pcm: %.3f saturated, rms %.3f" % (sat, rms))
        assert sat < 0.10 and rms >= 0.05
    elif name == "vanishing":
        for layer in R.GEMM_INPUTS + ["pitch.fft.in", "pitch.energy.partials"]:
            a = np.concatenate([np.ravel(v) for v in rec[layer]])
            share = R.subnormal_share(a)
            print("%-22s subnormal share: max %.2f (hop %d), >= 0.1 in %d hops" % (layer, share.max(), share.argmax(), (share >= 0.1).sum()))
            assert share.max() >= 0.10, layer
        # the audio itself: normal, then subnormal, then nothing, and back: both directions
        peak = np.abs(x).reshape(HOPS, -1).max(1)
        sub = (peak > 0) & (peak < R.SUBNORMAL)
        first, last = np.nonzero(sub)[0][[0, -1]]
        assert peak[:first].min() >= R.SUBNORMAL and peak[last + 1:].max() >= 0.2 and (peak[first:last] < 1e-44).any()
        # before and after: the audio is in the normal range at both ends; every layer of the phone extractor ENTERS the range (its
        # share rises from hop 0 to the best hop: the drive starts at 1e-30, and behind the first conv's 2^-20 the deeper layers
        # already hold some subnormals in hop 0) and LEAVES it (under 10 % in the last hops).  The wave generator does neither: its
        # values hang on the embeddings, not on the level of the audio, and straddle 2^-126 in every hop -- its kernels see
        # subnormal and normal values side by side, but no hop without subnormals.
        assert R.subnormal_share(rec["phone.F0.in"][0])[[0, -1]].max() == 0.0
        for layer in R.PHONE_LAYERS:
            share = R.subnormal_share(np.concatenate([np.ravel(v) for v in rec[layer]]))
            assert share[0] < share.max() and share[-4:].max() < 0.10, layer
    else:
        order = np.argsort(out["dist"], axis=1, kind="stable")[:, :len(R.TIE_ROWS)]
        assert np.array_equal(order, np.tile(R.TIE_ROWS, (HOPS, 1))), "the duplicated row is the nearest one in every hop"
        assert np.all(out["dist"][:, list(R.TIE_ROWS)] == out["dist"][:, [0]])
        lg = out["logits"]
        assert np.all(lg[:, list(R.TIE_BINS)] == lg[:, [R.TIE_BINS[0]]]) and np.all(np.argmax(lg[:, 1:], axis=1) + 1 == R.TIE_BINS[0])
        rest = np.delete(lg, list(R.TIE_BINS), axis=1).max(1)
        assert np.all(lg[:, R.TIE_BINS[0]] > rest + 1.0), "the duplicated logits hold the maximum"


def test_ties_hold_for_every_stream_of_the_gpu_drives(bv, tmp_path):
    """tests/test_gpu_regimes.py drives five streams (audio seeds 2024 .. 2028, speaker s % 3): the planted ties are the nearest rows
    and the largest logits for each of them, not only for the stream the package was made from."""
    d = R.package(bv, "ties", str(tmp_path))
    for s in range(5):
        _, out = R.restate(d, R.regime_audio(bv, "ties", seed=2024 + s), speaker=s % 3, vq_k=8, wave=False)
        srt = np.sort(out["dist"], axis=1)
        order = np.argsort(out["dist"], axis=1, kind="stable")[:, :len(R.TIE_ROWS)]
        lg = out["logits"]
        lead = lg[:, R.TIE_BINS[0]] - np.delete(lg, list(R.TIE_BINS), axis=1).max(1)
        print("stream %d: margin to the seventh row %.1f, tied logits lead by %.1f" % (s, (srt[:, 6] - srt[:, 5]).min(), lead.min()))
        assert np.array_equal(order, np.tile(R.TIE_ROWS, (HOPS, 1))) and (srt[:, 6] - srt[:, 5]).min() > 1.0
        assert np.all(lg[:, list(R.TIE_BINS)] == lg[:, [R.TIE_BINS[0]]]) and lead.min() > 1.0 and np.all(out["bins"] == R.TIE_BINS[0])


# ---- (2) oracle against the restatement --------------------------------------------------------------------------------------
def test_phone_extractor_in_regime(regime):
    name, d, x, rec, out, driven = regime
    pe = sn.PhoneExtractor(d)
    want, _, _ = pe(x)
    _within(name, "phone", float(np.abs(driven[0]["phone"] - want).max()), float(np.abs(want).max()))
    cb = driven[0]["tables"].codebooks[1]
    vq, _, dist = pe(x, codebook=cb, k=3)
    srt = np.sort(dist, axis=1)
    clear = (srt[:, 3] - srt[:, 2]) > 1e-3
    if name == "ties":
        # the three nearest are copies of one row: whichever copies a reading picks, their mean is that row -- unless it drops or
        # repeats a tied candidate.  The restatement's stable sort picks the lowest indices (MODEL_SPEC 2.4); compared in every hop.
        assert np.array_equal(np.argsort(dist, axis=1, kind="stable")[:, :3], np.tile(R.TIE_ROWS[:3], (HOPS, 1)))
        clear = np.ones(HOPS, bool)
    assert clear.sum() >= HOPS // 2
    _within(name, "knn", float(np.abs(driven[3]["phone"][clear] - vq[clear]).max()), float(np.abs(vq).max()))


def test_pitch_estimator_in_regime(regime):
    name, d, x, rec, out, driven = regime
    bins, feat, logits = sn.PitchEstimator(d)(x, 1, 447)
    got = driven[0]
    if name == "ties":
        assert np.array_equal(got["q"], bins) and np.all(bins == R.TIE_BINS[0]), "the lowest of the tied bins, exactly, in every hop"
        clear = np.ones(HOPS, bool)
    else:
        top2 = np.sort(logits[:, 1:448], axis=1)[:, -2:]
        clear = (top2[:, 1] - top2[:, 0]) > 1e-3
        assert clear.sum() >= HOPS // 2
        assert np.array_equal(got["q"][clear], bins[clear])
    same = got["q"] == bins
    prev_same = np.concatenate([[True], same[:-1]])
    for i, what in enumerate(("f0", "energy", "delta", "voicing")):
        rows = same & prev_same if i == 2 else (same if i == 0 else np.ones(HOPS, bool))
        dev = float(np.abs(got["feat"][rows, i] - feat[rows, i]).max())
        _within(name, what, dev, float(np.abs(feat[:, i]).max()))


def test_waveform_generator_in_regime(regime):
    name, d, x, rec, out, driven = regime
    tables = driven[0]["tables"]
    wg = sn.WaveformGenerator(d)
    for k in (0, 3):
        r = driven[k]
        want = wg(r["phone"], r["q"], r["feat"], tables.additive[1], tables.formant[6], tables.kv[1])
        dev, rms = float(np.abs(r["pcm"] - want).max()), float(np.sqrt((want ** 2).mean()))
        assert np.isfinite(r["pcm"]).all() and r["pcm"].std() > 0
        assert rms > 0.02
        _within(name, "wave%d" % k, dev, rms)


@pytest.mark.parametrize("name", ["hot", "vanishing"])
def test_legacy_generator_in_regime(bv, built, tmp_path, name):
    """The legacy packages of the first two regimes: finite, audible, and the generator equal to its restatement."""
    legacy = bv.AbiLegacy(os.path.join(R.REPO, "oracle", "libbeatrice_oracle.so"), "20b1")
    d = R.package(bv, name, str(tmp_path), legacy=True)
    x = R.regime_audio(bv, name)
    r = R.drive_legacy(bv, legacy, d, x, speaker=1)
    want = sn.LegacyWaveformGenerator(d)(r["phone"], np.minimum(r["q"], 383), r["feat"], r["spk"])
    dev, rms = float(np.abs(r["pcm"] - want).max()), float(np.sqrt((want ** 2).mean()))
    print("legacy %s: max-abs %.3g, rms %.3g, %.3f saturated" % (name, dev, rms, (np.abs(want) >= 0.999).mean()))
    assert np.isfinite(r["pcm"]).all() and r["pcm"].std() > 0
    assert (np.abs(want) >= 0.999).mean() < 0.10 and rms >= 0.05
    assert dev <= 2.0 * LEGACY_RECORDED[name][0]


# ---- (3) the scalar functions against the truth ------------------------------------------------------------------------------
@pytest.mark.parametrize("which,name", list(enumerate(mp.FUNCTIONS)))
def test_spec_function_accuracy(oracle, which, name):
    pts = mp.points_for(name)
    got = mp.oracle_eval(oracle, which, pts).view(np.float32)
    true = mp.true_value(name, pts.view(np.float32))
    assert np.isfinite(got).all()
    unit, recorded = MATH_RECORDED[name]
    err = mp.ulp_error(got, true) if unit == "ulp" else np.abs(got.astype(np.float64) - true)
    i = int(err.argmax())
    print("%s: max error %.4g %s at x = %r over %d points (recorded %.4g)" % (name, err[i], unit, pts.view(np.float32)[i], pts.size, recorded))
    assert err[i] <= recorded


def test_oracle_keeps_subnormals(oracle):
    assert mp.oracle_keeps_subnormals(oracle)
