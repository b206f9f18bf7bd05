"""The smallest batches at which the addressing of the tail stages (tail_stages.hip.h: weights, ring frames, state block and output
samples as global accesses off a workgroup's scalar bases) can be wrong while the large parity tests still pass -- last workgroups of
1, 2 or 3 streams, one live stream with every padded row recomputed from the last row, the two sub-steps of a four-hop step, the fill /
drain table's two streams per workgroup, the ragged instance -- and the shapes that do the same for the bodies that share the launch
(the GRU cells of fused_small.hip.h: a second workgroup that holds one stream; the quad attention body and the epilogues of
rowchain.hip.h: K/V slots of 12 + 8 + 8 rows) and for the in-order chain.  Every stream against the oracle."""
import numpy as np
import pytest

from oracle_batch import OracleBatch, oracle_leg, pick_streams
from tick_driver import Resident, run_tick

pytestmark = pytest.mark.gpu
TOL = 1e-4   # test_gpu_segment_loop_shapes.py's bound on output PCM


def _compare(what, got, want):
    dev = float(np.abs(got - want).max())
    print("%s vs ORACLE: max-abs %g, array_equal %s" % (what, dev, np.array_equal(got, want)))
    assert np.abs(got).max() > 1e-3
    assert dev <= TOL


def _oracle(bv, oracle, model_dir, B, H, steps, audio, settings, sample=None):
    sample = list(range(B)) if sample is None else sample
    got_sample, want = oracle_leg(bv, oracle, model_dir, B, lambda j: audio[:, j], steps * H, settings, lambda ob, j: None, sample)
    assert got_sample == sorted(sample)
    n = len(got_sample)
    return want.reshape(steps, H, n, 240).transpose(0, 2, 1, 3).reshape(steps, n, H * 240)


def _audio(bv, B, H, steps, seed):
    return np.stack([bv.synth_audio(160 * H * steps, seed=seed + s) for s in range(B)]).reshape(B, steps * H, 160)


def _one_speaker(batch):
    batch.a.BeatriceBatch_SetTargetSpeaker(batch.h, -1, 0)
    batch.a.BeatriceBatch_FlushSpeaker(batch.h, -1)


def _tick(bv, product, model_dir, B, H, steps, audio, settings, chunk):
    m = bv.Models(product, model_dir)
    batch = bv.Batch(m, B, hops_per_step=H)
    settings(batch)
    got = run_tick(bv, batch, steps, lambda k: audio[:, k * H:(k + 1) * H].reshape(B, H * 160), chunk=chunk)
    batch.close()
    m.close()
    return got


@pytest.mark.parametrize("H", [1, 2, 4])
@pytest.mark.parametrize("B", [1, 5, 7])
def test_last_tail_workgroups_in_tick_mode_match_oracle(bv, oracle, product, model_dir, B, H):
    """Full ticks give the tail stages 4 / 3 / 2 streams per workgroup at H = 1 (T1 / T2 / T3): B = 5 leaves a last workgroup of 1, 2
    and 1 streams, B = 7 of 3, 1 and 1; B = 1 is one live stream, every padded row recomputed from the last row.  H = 4 runs the two
    sub-steps of T2 / T3 (carry_histories), H = 2 the one-sub-step form.  40 steps drained in chunks of 7: the fill / drain table's
    tail stages take 2 streams per workgroup."""
    steps = 40
    audio = _audio(bv, B, H, steps, 9100)
    got = _tick(bv, product, model_dir, B, H, steps, audio, _one_speaker, 7)
    _compare("tick mode, %d stream(s) x %d hop(s) per step" % (B, H), got, _oracle(bv, oracle, model_dir, B, H, steps, audio, _one_speaker))


def test_second_gru_workgroup_of_one_stream_matches_oracle(bv, oracle, product, model_dir):
    """B = 33, H = 4, 34 steps: the column-split GRU cell has 32 streams per workgroup, so the second workgroup holds one stream -- and
    the step's four hops run the chain of four linked cells.  The oracle follows the streams at the corners of the 16- and 32-row
    tiles (pick_streams: 0, 1, 2, 15, 16, 31, 32, ...)."""
    B, H, steps = 33, 4, 34
    audio = _audio(bv, B, H, steps, 9200)
    sample = pick_streams(B)
    assert 31 in sample and 32 in sample
    got = _tick(bv, product, model_dir, B, H, steps, audio, _one_speaker, None)
    _compare("tick mode, 33 streams x 4 hops per step", got[:, sample], _oracle(bv, oracle, model_dir, B, H, steps, audio, _one_speaker, sample))


def test_three_speakers_through_the_quad_body_match_oracle(bv, oracle, product, model_dir):
    """B = 7 on three speakers (stream s on speaker s % 3), H = 4: slots of 12 + 8 + 8 rows go through the quad body's K / V reads."""
    B, H, steps = 7, 4, 40
    audio = _audio(bv, B, H, steps, 9300)

    def settings(batch):
        for s in range(B):
            batch.a.BeatriceBatch_SetTargetSpeaker(batch.h, s, s % 3)
        batch.a.BeatriceBatch_FlushSpeaker(batch.h, -1)

    got = _tick(bv, product, model_dir, B, H, steps, audio, settings, 7)
    _compare("tick mode, 7 streams on 3 speakers x 4 hops per step", got, _oracle(bv, oracle, model_dir, B, H, steps, audio, settings))


def test_ragged_instance_matches_oracle(bv, oracle, product, model_dir):
    """The RAG = true instance of the launch (its tail and GRU bodies): B = 5, H = 4, stream 3 flagged to sit steps 9 and 10 out, as
    tests/test_gpu_tick_ragged.py does it (BeatriceBatch_SetSilentStreams before the step), against that test's oracle leg: the hops
    of a step a stream sits out are never made."""
    B, H, steps = 5, 4, 24
    out = {3: {9, 10}}
    x = _audio(bv, B, H, steps, 9400).reshape(B, steps, H * 160)
    ob = OracleBatch(bv, oracle, model_dir, B, hops_per_step=H)
    _one_speaker(ob)
    want = np.zeros((steps, B, H * 240), np.float32)
    for k in range(steps):
        for s, y in ob.convert(x[:, k], absent={s for s in ob.sample if k in out.get(s, ())}).items():
            want[k, s] = y
    ob.close()

    m = bv.Models(product, model_dir)
    batch = bv.Batch(m, B, hops_per_step=H)
    a, h = batch.a, batch.h
    _one_speaker(batch)
    enabled = []

    def change(batch_, k):
        if not enabled:   # (tick mode is on by now: the rule is enabled inside it)
            assert a.BeatriceBatch_EnableSilentBlockRule(h, 1) == 0
            enabled.append(1)
        flags = bytes(1 if k in out.get(s, ()) else 0 for s in range(B))
        if any(flags):
            assert a.BeatriceBatch_SetSilentStreams(h, flags) == 0

    got = run_tick(bv, batch, steps, lambda k: x[:, k], change=change, chunk=13)
    assert a.BeatriceBatch_EnableSilentBlockRule(h, 0) == 0
    batch.close()
    m.close()
    for s, ks in out.items():   # (what the slots of a step that a stream sat out hold is not specified)
        for k in ks:
            got[k, s] = want[k, s] = 0.0
    _compare("ragged tick mode, 5 streams x 4 hops per step, stream 3 absent for two steps", got, want)


def test_in_order_chain_matches_oracle(bv, oracle, product, model_dir):
    """BeatriceBatch_EnableTickPipeline off: the in-order chain over resident I/O (it shares fused_small.hip.h and the epilogues),
    B = 5, H = 1, 12 steps."""
    B, H, steps = 5, 1, 12
    audio = _audio(bv, B, H, steps, 9500)
    m = bv.Models(product, model_dir)
    batch = bv.Batch(m, B, hops_per_step=H)
    _one_speaker(batch)
    r = Resident(bv, batch, slots=steps, tick=False)
    try:
        got = r.feed([audio[:, k] for k in range(steps)])
        r.leave()
    finally:
        r.free()
    batch.close()
    m.close()
    _compare("in-order chain, 5 streams", got, _oracle(bv, oracle, model_dir, B, H, steps, audio, _one_speaker))
