"""The smallest batches at which the addressing of the row-local bodies' segment loops (rowchain.hip.h: a wave-uniform weight base
plus the lane's offset, the row gather as global loads off the ring's base) can be wrong while the large parity tests still pass:
partly filled 16-row tiles, a second row tile of an RT = 2 workgroup that is a quarter full, a last workgroup of 4 rows, tiles per
K/V slot with padding and the quad bodies' 8-row layers.  Every stream against the oracle."""
import numpy as np
import pytest

from oracle_batch import oracle_leg
from tick_driver import Resident, run_tick

pytestmark = pytest.mark.gpu
TOL = 1e-4   # test_gpu_throughput_vs_oracle.py's bound on output PCM


def _compare(what, got, want):
    dev = float(np.abs(got - want).max())
    print("%s vs ORACLE: max-abs %g, array_equal %s" % (what, dev, np.array_equal(got, want)))
    assert np.abs(got).max() > 1e-3
    assert dev <= TOL


def _oracle(bv, oracle, model_dir, B, H, steps, audio, settings):
    sample, want = oracle_leg(bv, oracle, model_dir, B, lambda j: audio[:, j], steps * H, settings, lambda ob, j: None, list(range(B)))
    assert sample == list(range(B))
    return want.reshape(steps, H, B, 240).transpose(0, 2, 1, 3).reshape(steps, B, H * 240)


@pytest.mark.parametrize("H", [1, 4])
@pytest.mark.parametrize("B", [1, 5, 17])
def test_small_batches_in_tick_mode_match_oracle(bv, oracle, product, model_dir, B, H):
    """B = 1: one live row in a 16-row tile.  B = 5, H = 4: 20 rows, the second row tile of an RT = 2 workgroup a quarter full.
    B = 17, H = 4: 68 rows, the last workgroup holds 4.  40 steps drained in chunks of 7."""
    steps = 40
    audio = np.stack([bv.synth_audio(160 * H * steps, seed=8800 + s) for s in range(B)]).reshape(B, steps * H, 160)

    def settings(batch):
        batch.a.BeatriceBatch_SetTargetSpeaker(batch.h, -1, 0)
        batch.a.BeatriceBatch_FlushSpeaker(batch.h, -1)

    m = bv.Models(product, model_dir)
    batch = bv.Batch(m, B, hops_per_step=H)
    settings(batch)
    got = run_tick(bv, batch, steps, lambda k: audio[:, k * H:(k + 1) * H].reshape(B, H * 160), chunk=7)
    batch.close()
    m.close()
    _compare("tick mode, %d stream(s) x %d hop(s) per step" % (B, H), got, _oracle(bv, oracle, model_dir, B, H, steps, audio, settings))


def test_three_speakers_in_tick_mode_match_oracle(bv, oracle, product, model_dir):
    """B = 7 on three speakers (stream s on speaker s % 3), H = 4: 12 + 8 + 8 rows -- tiles per K/V slot with padding, and the quad
    bodies' 8-row layers."""
    B, H, steps = 7, 4, 40
    audio = np.stack([bv.synth_audio(160 * H * steps, seed=8900 + s) for s in range(B)]).reshape(B, steps * H, 160)

    def settings(batch):
        for s in range(B):
            batch.a.BeatriceBatch_SetTargetSpeaker(batch.h, s, s % 3)
        batch.a.BeatriceBatch_FlushSpeaker(batch.h, -1)

    m = bv.Models(product, model_dir)
    batch = bv.Batch(m, B, hops_per_step=H)
    settings(batch)
    got = run_tick(bv, batch, steps, lambda k: audio[:, k * H:(k + 1) * H].reshape(B, H * 160), chunk=7)
    batch.close()
    m.close()
    _compare("tick mode, 7 streams on 3 speakers x 4 hops per step", got, _oracle(bv, oracle, model_dir, B, H, steps, audio, settings))


def test_in_order_chain_matches_oracle(bv, oracle, product, model_dir):
    """BeatriceBatch_EnableTickPipeline off: the in-order chain over resident I/O, B = 17, H = 1, 12 steps."""
    B, H, steps = 17, 1, 12
    audio = np.stack([bv.synth_audio(160 * steps, seed=9000 + s) for s in range(B)]).reshape(B, steps, 160)

    def settings(batch):
        batch.a.BeatriceBatch_SetTargetSpeaker(batch.h, -1, 0)
        batch.a.BeatriceBatch_FlushSpeaker(batch.h, -1)

    m = bv.Models(product, model_dir)
    batch = bv.Batch(m, B, hops_per_step=H)
    settings(batch)
    r = Resident(bv, batch, slots=steps, tick=False)
    try:
        got = r.feed([audio[:, k] for k in range(steps)])
        r.leave()
    finally:
        r.free()
    batch.close()
    m.close()
    _compare("in-order chain, 17 streams", got, _oracle(bv, oracle, model_dir, B, H, steps, audio, settings))
