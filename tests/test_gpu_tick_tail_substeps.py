"""The tail stages T2 and T3 of the tick launch at four hops per step run a stream's step as two SUB-STEPS inside one workgroup
(tail_stages.hip.h: prologue / carry_histories; the layers' histories travel from the first sub-step to the second in LDS, only the
first reads them from the state block and only the last writes them back).  Against the oracle: H = 4 with B in {1, 3}, and H = 2 with
B = 3 as the control that has no sub-steps -- for exactly one fill and one drain of the pipeline (BeatriceBatch_TickStages + 6 steps fed
without waiting, then the drain).  At B = 3 the middle stream sits one middle step out, so the ragged instances of T2 / T3 run from there
on (an absent stream's rows compute on zeros, nothing of it is written, and its histories stay where its last step left them).

Why these shapes: B = 1 is the smallest shape in which a sub-step boundary, the step-to-step histories (state block) and the two-slot
ring parity between T1, T2 and T3 all occur -- TickStages + 6 steps take every ring through both of its slots several times.  B = 3
adds a second and a third workgroup (one stream per workgroup at H = 4; at H = 2 T1 holds two streams per workgroup, so its second one
is half full) and the absent stream.

Every stream is compared.  Expected max-abs against the oracle: 0 (same arithmetic in the same order)."""
import numpy as np
import pytest

from oracle_batch import OracleBatch, pick_streams
from tick_driver import Resident

pytestmark = pytest.mark.gpu


def _one_speaker(batch):
    batch.a.BeatriceBatch_SetTargetSpeaker(batch.h, -1, 0)
    batch.a.BeatriceBatch_FlushSpeaker(batch.h, -1)


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


@pytest.mark.parametrize("H,B", [(4, 1), (4, 3), (2, 3)])
def test_tail_sub_steps_through_one_fill_and_drain_match_oracle(bv, oracle, product, model_dir, H, B):
    m = bv.Models(product, model_dir)
    batch = bv.Batch(m, B, hops_per_step=H)
    a, h = batch.a, batch.h
    _one_speaker(batch)
    steps = a.BeatriceBatch_TickStages(h) + 6
    absent, at = (B // 2, steps // 2) if B > 1 else (None, None)
    sample = pick_streams(B)
    assert sample == list(range(B))   # every stream is compared
    x = np.stack([bv.synth_audio(160 * H * steps, seed=9100 + 100 * H + s) for s in range(B)]).reshape(B, steps, H * 160)
    r = Resident(bv, batch, slots=steps, tick=True)
    try:
        if absent is not None:
            assert a.BeatriceBatch_EnableSilentBlockRule(h, 1) == 0

        def before_step(k):
            if absent is not None and k == at:
                assert a.BeatriceBatch_SetSilentStreams(h, bytes(1 if s == absent else 0 for s in range(B))) == 0

        got = r.feed([x[:, k] for k in range(steps)], before_step)
        if absent is not None:
            assert a.BeatriceBatch_EnableSilentBlockRule(h, 0) == 0
        r.leave()
    finally:
        r.free()
    batch.close()
    m.close()
    got = got[:, sample]
    out = {}
    if absent is not None:
        got[at, sample.index(absent)] = 0.0   # (what the slot of a step that a stream sat out holds is not specified)
        out = {absent: {at}}
    want = _oracle(bv, oracle, model_dir, B, H, x, sample, out)
    dev = float(np.abs(got - want).max())
    print("tail sub-steps, %d stream(s) x %d hop(s) per step, %s, %d steps vs ORACLE: max-abs %g, array_equal %s"
          % (B, H, "stream %d absent at step %d" % (absent, at) if absent is not None else "no stream absent", steps, dev, np.array_equal(got, want)))
    assert np.abs(got).max() > 1e-3
    assert dev == 0.0
