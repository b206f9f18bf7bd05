"""HIP against the oracle, bit for bit, in the numeric regimes of tests/regimes.py (witnessed on the CPU by
tests/test_cpu_regimes.py): `hot` (saturating softmax / gelu / sigmoid, f0 = 1.0), `vanishing` (subnormal inputs, intermediates and
weights, MODEL_SPEC 2.5) and `ties` (exact ties in the k-NN search and the pitch argmax, MODEL_SPEC 2.4).  Every drive sees every
regime: the 1-stream ABI (team and chain kernels; phone, bin, features and samples per hop), the in-order batch, tick mode with
one hop per step and with four (20 rows: one full 16-row tile and a ragged one)."""
import os

import numpy as np
import pytest

import math_points as mp
import regimes as R
from oracle_batch import oracle_leg
from tick_driver import run_tick

pytestmark = pytest.mark.gpu
B, HOPS = 5, R.HOPS
SWITCH_HOP = 8      # a step boundary for 1 and for 4 hops per step
VQ = {"hot": [0, 1, 3, 8, 2], "vanishing": [0, 3, 0, 8, 1], "ties": [1, 2, 3, 4, 8]}


def _bin_note(q):
    return 33.0 + q / 8.0      # the note whose quantised pitch is bin q


def _settings(regime):
    def settings(batch):
        a, h = batch.a, batch.h
        for s in range(B):
            a.BeatriceBatch_SetTargetSpeaker(h, s, s % 3)
            a.BeatriceBatch_SetVQNumNeighbors(h, s, VQ[regime][s])
        if regime == "ties":
            j = R.TIE_BINS
            a.BeatriceBatch_SetMinSourcePitch(h, 1, _bin_note(j[0] + 1))      # above the lowest duplicate: the next one (another lane) wins
            a.BeatriceBatch_SetMinSourcePitch(h, 2, _bin_note(j[1] + 1))      # above two: the one in the first's lane, next slot
            a.BeatriceBatch_SetMinSourcePitch(h, 3, _bin_note(j[2] + 1))
            a.BeatriceBatch_SetMinSourcePitch(h, 4, _bin_note(j[2] + 1))      # max < min: the range is the single bin `min`
            a.BeatriceBatch_SetMaxSourcePitch(h, 4, _bin_note(j[0]))
        a.BeatriceBatch_FlushSpeaker(h, -1)
    return settings


def _change(regime):
    def change(batch, hop):
        if regime == "hot" and hop == SWITCH_HOP:
            batch.a.BeatriceBatch_SetTargetSpeaker(batch.h, 3, 2)      # its four K/V blocks follow one per hop
    return change


def _assert_identical(what, got, want):
    same = np.array_equal(got, want)
    dev = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    print("%s: %s (max-abs %g, %d of %d values differ)" % (what, "bit-identical" if same else "DIFFERENT", dev.max(), (got != want).sum(), want.size))
    assert same, "%s: max-abs %g, %d of %d values differ, first at %r" % (what, dev.max(), (got != want).sum(), want.size,
                                                                           tuple(np.argwhere(got != want)[0]))


def _sane(want):
    assert np.isfinite(want).all() and want.std() > 0, "the oracle's output is finite and not constant"


@pytest.fixture(scope="module", params=["hot", "vanishing", "ties"])
def regime(request, bv, oracle, product, tmp_path_factory):
    """(name, package, audio [B][HOPS * 160], the oracle's samples [HOPS][B][240] under the regime's script)"""
    name = request.param
    if name == "vanishing":
        assert mp.oracle_keeps_subnormals(oracle), "this process flushes subnormals: the oracle cannot be trusted here"
    d = R.package(bv, name, str(tmp_path_factory.mktemp("regime_" + name)))
    audio = np.stack([R.regime_audio(bv, name, seed=2024 + s) for s in range(B)])
    _, want = oracle_leg(bv, oracle, d, B, lambda k: audio[:, k * 160:(k + 1) * 160], HOPS, _settings(name), _change(name), list(range(B)))
    _sane(want)
    for s in range(B):
        _sane(want[:, s])
    return name, d, audio, want


def _stream_cases(name):
    if name == "ties":
        j = R.TIE_BINS
        return [dict(vq_k=1), dict(vq_k=5), dict(vq_k=512), dict(vq_k=2, min_q=j[0] + 1), dict(vq_k=0, min_q=j[1] + 1),
                dict(vq_k=0, min_q=j[2] + 1, max_q=j[0])]
    return [dict(vq_k=0), dict(vq_k=3)]


def test_one_stream_abi(bv, oracle, product, regime):
    name, d, audio, _ = regime

    def change(st, hop):
        if name == "hot" and hop == SWITCH_HOP:
            st.set_target_speaker(2)

    for case in _stream_cases(name):
        kw = dict(dict(speaker=1, formant_index=6, min_q=1, max_q=447), **case)
        want = R.drive(bv, oracle, d, audio[0], change=change, **kw)
        got = R.drive(bv, product, d, audio[0], change=change, **kw)
        _sane(want["pcm"])
        for key in ("phone", "q", "feat", "pcm"):
            _assert_identical("%s 1-stream %r %s" % (name, case, key), got[key], want[key])
        if name == "ties" and "min_q" in case:
            lo = case["min_q"]
            expect = lo if case.get("max_q", 447) < lo else min(b for b in R.TIE_BINS if b >= lo)
            assert np.all(want["q"] == expect), "the lowest tied bin inside the limits"


def test_in_order_batch(bv, product, regime):
    name, d, audio, want = regime
    m = bv.Models(bv.bind_batch(product), d)
    batch = bv.Batch(m, B)
    _settings(name)(batch)
    got = np.zeros_like(want)
    for k in range(HOPS):
        _change(name)(batch, k)
        got[k] = batch.convert(audio[:, k * 160:(k + 1) * 160])
    batch.close()
    m.close()
    _assert_identical("%s in-order batch" % name, got, want)


@pytest.mark.parametrize("H", [1, 4])
def test_tick_mode(bv, product, regime, H):
    name, d, audio, want = regime
    m = bv.Models(bv.bind_batch(product), d)
    batch = bv.Batch(m, B, hops_per_step=H)
    _settings(name)(batch)
    got = run_tick(bv, batch, HOPS // H, lambda k: audio[:, k * H * 160:(k + 1) * H * 160], lambda b, k: _change(name)(b, k * H))
    batch.close()
    m.close()
    wantH = want.reshape(HOPS // H, H, B, 240).transpose(0, 2, 1, 3).reshape(HOPS // H, B, H * 240)
    _assert_identical("%s tick mode, %d hops per step" % (name, H), got, wantH)


@pytest.mark.parametrize("name", ["hot", "vanishing"])
def test_legacy_one_stream_abi(bv, built, product, tmp_path, name):
    """The legacy generations have no batched path: the 1-stream ABI only."""
    oracle = bv.AbiLegacy(os.path.join(R.REPO, "oracle", "libbeatrice_oracle.so"), "20b1")
    hip = bv.AbiLegacy(bv.PRODUCT_LIB, "20b1")
    if name == "vanishing":
        assert mp.oracle_keeps_subnormals(bv.Abi(oracle.path)), "this process flushes subnormals: the oracle cannot be trusted here"
    d = R.package(bv, name, str(tmp_path), legacy=True)
    x = R.regime_audio(bv, name)
    want = R.drive_legacy(bv, oracle, d, x, speaker=1)
    got = R.drive_legacy(bv, hip, d, x, speaker=1)
    _sane(want["pcm"])
    for key in ("phone", "q", "feat", "pcm"):
        _assert_identical("legacy %s %s" % (name, key), got[key], want[key])
