"""The GRU cells of the tick tables at several hops per step are the rows cell (rowchain.hip.h gru_rows_body: 32 streams x 64 hidden
units per workgroup, the six gate sums of a lane's four hidden units meet in registers; linked hop to hop inside a launch); the table
of one hop per step, and hop 0 of the phone GRU at four hops, keep the column-split cell (fused_small.hip.h).  Against the oracle: H in
{1, 2, 4} hops per step x B in {1, 17, 33} streams -- B = 1: one row of a row tile, B = 17: across the 16-row tile inside one
workgroup, B = 33: a second row group that holds one row -- for exactly one fill and one drain of the pipeline
(BeatriceBatch_TickStages + 6 steps fed without waiting, so every link of the chain runs with partly filled neighbours), one stream
sitting a step out in the middle (the ragged instance of the cells runs from there on: an absent row is zeros in both tiles, writes no
state and publishes nothing).

What runs the rows cell: H = 2 (both cells, publishing and polling forms) and H = 4 (all three link forms of the pitch cell, the
polling and the polling-and-publishing form of the phone cell).  The H = 1 cases run the column-split cell in the same table kernel
and dispatch order as before; the rows cell's unlinked form (LINK = 0) is in no table, only in tools/microbench/gru_cell.hip.

Expected max-abs against the oracle: 0 (same arithmetic in the same order)."""
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


@pytest.mark.parametrize("H", [1, 2, 4])
@pytest.mark.parametrize("B", [1, 17, 33])
def test_gru_cells_through_one_fill_and_drain_match_oracle(bv, oracle, product, model_dir, B, H):
    m = bv.Models(product, model_dir)
    batch = bv.Batch(m, B, hops_per_step=H)
    a, h = batch.a, batch.h
    _one_speaker(batch)
    steps = a.BeatriceBatch_TickStages(h) + 6
    absent, at = B // 2, steps // 2
    sample = pick_streams(B)
    assert absent in sample
    x = np.stack([bv.synth_audio(160 * H * steps, seed=8300 + 100 * H + s) for s in range(B)]).reshape(B, steps, H * 160)
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
    want = _oracle(bv, oracle, model_dir, B, H, x, sample, {absent: {at}})
    dev = float(np.abs(got - want).max())
    print("GRU cells, %d stream(s) x %d hop(s) per step, stream %d absent at step %d of %d vs ORACLE: max-abs %g, array_equal %s"
          % (B, H, absent, at, steps, dev, np.array_equal(got, want)))
    assert np.abs(got).max() > 1e-3
    assert dev == 0.0
