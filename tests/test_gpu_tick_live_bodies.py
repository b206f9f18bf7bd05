"""The table kernels of the tick launch hold only the bodies their tables can contain (tick.hip.h Ops<H>::L: no one-workgroup-per-stream
tail anywhere, the sparse table's types only at one hop per step).  Every live body, in both instances of every kernel, against the
oracle: H in {1, 2, 4} hops per step x B in {1, 5, 33} streams -- B = 1: partly filled T1 / T2 / T3 workgroups and a single row tile,
B = 5: a padded row tile, B = 33: across the 32-row convolution tile and the 16-row block tile -- for exactly one fill and one drain
of the pipeline (BeatriceBatch_TickStages + 6 steps fed without waiting: at H = 1 the fill's first ticks run the sparse table), one
stream sitting a step out in the middle (the ragged instance runs from there on).  And at H = 4 a drained return to the in-order chain
and back: the tail stages' state block is the one wave_tail.hip.h's kernel works on there.

Expected max-abs against the oracle: 0 (same arithmetic in the same order)."""
import numpy as np
import pytest

from oracle_batch import OracleBatch, pick_streams
from tick_driver import Resident

pytestmark = pytest.mark.gpu


def _one_speaker(batch):
    batch.a.BeatriceBatch_SetTargetSpeaker(batch.h, -1, 0)
    batch.a.BeatriceBatch_FlushSpeaker(batch.h, -1)


def _audio(bv, B, H, steps, seed):
    return np.stack([bv.synth_audio(160 * H * steps, seed=seed + s) for s in range(B)]).reshape(B, steps, H * 160)


def _oracle(bv, oracle, model_dir, B, H, x, sample, out):
    """[steps][len(sample)][H * 240]; out = {stream: steps it sits out} (those hops are never made; their rows stay 0)."""
    steps = x.shape[1]
    ob = OracleBatch(bv, oracle, model_dir, B, sample=sample, hops_per_step=H)
    _one_speaker(ob)
    want = np.zeros((steps, len(ob.sample), H * 240), np.float32)
    for k in range(steps):
        for s, y in ob.convert(x[:, k], absent={s for s in ob.sample if k in out.get(s, ())}).items():
            want[k, ob.sample.index(s)] = y
    ob.close()
    return want


def _compare(what, got, want):
    dev = float(np.abs(got - want).max())
    print("%s vs ORACLE: max-abs %g, array_equal %s" % (what, dev, np.array_equal(got, want)))
    assert np.abs(got).max() > 1e-3
    assert dev == 0.0


@pytest.mark.parametrize("H", [1, 2, 4])
@pytest.mark.parametrize("B", [1, 5, 33])
def test_one_fill_and_drain_with_a_stream_sitting_out_matches_oracle(bv, oracle, product, model_dir, B, H):
    m = bv.Models(product, model_dir)
    batch = bv.Batch(m, B, hops_per_step=H)
    a, h = batch.a, batch.h
    _one_speaker(batch)
    steps = a.BeatriceBatch_TickStages(h) + 6
    absent, at = B // 2, steps // 2
    out = {absent: {at}}
    sample = pick_streams(B)
    assert absent in sample
    x = _audio(bv, B, H, steps, 9700 + 100 * H)
    r = Resident(bv, batch, slots=steps, tick=True)
    try:
        assert a.BeatriceBatch_EnableSilentBlockRule(h, 1) == 0

        def before_step(k):
            if k == at:
                assert a.BeatriceBatch_SetSilentStreams(h, bytes(1 if s == absent else 0 for s in range(B))) == 0

        got = r.feed([x[:, k] for k in range(steps)], before_step)
        assert a.BeatriceBatch_EnableSilentBlockRule(h, 0) == 0
        r.leave()
    finally:
        r.free()
    batch.close()
    m.close()
    got = got[:, sample]
    got[at, sample.index(absent)] = 0.0   # (what the slot of a step that a stream sat out holds is not specified)
    _compare("tick mode, %d stream(s) x %d hop(s) per step, stream %d absent at step %d of %d" % (B, H, absent, at, steps),
             got, _oracle(bv, oracle, model_dir, B, H, x, sample, out))


def test_drained_return_to_the_in_order_chain_and_back_matches_oracle(bv, oracle, product, model_dir):
    B, H = 5, 4
    m = bv.Models(product, model_dir)
    batch = bv.Batch(m, B, hops_per_step=H)
    _one_speaker(batch)
    n_tick = batch.a.BeatriceBatch_TickStages(batch.h) + 6
    n_chain = 3
    legs = [(True, n_tick), (False, n_chain), (True, n_tick)]
    steps = sum(n for _, n in legs)
    x = _audio(bv, B, H, steps, 9900)
    got, k0 = [], 0
    for tick, n in legs:
        r = Resident(bv, batch, slots=n, tick=tick)
        try:
            got.append(r.feed([x[:, k] for k in range(k0, k0 + n)]))
            r.leave()
        finally:
            r.free()
        k0 += n
    batch.close()
    m.close()
    _compare("tick mode, in-order chain, tick mode: 5 streams x 4 hops per step", np.concatenate(got),
             _oracle(bv, oracle, model_dir, B, H, x, list(range(B)), {}))
