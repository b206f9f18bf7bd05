"""Continuous batching of utterances with BeatriceBatch_ResetStreamInFlight (tests/utterance_queue.py): 20 seeded utterances of 3 - 40
hops with two speakers over 6 streams.  Every utterance's output must equal, bit for bit, that utterance converted ALONE on a fresh
oracle stream; and nothing drains on the way: the ticks launched are the steps fed plus the final drain."""
import numpy as np
import pytest

from oracle_batch import OracleBatch
from utterance_queue import make_queue, run_queue

pytestmark = pytest.mark.gpu
_alone = {}


def converted_alone(bv, oracle, model_dir, queue):
    """Each utterance on a fresh oracle stream of its speaker (computed once, shared by the cases, left unchanged)."""
    if "out" not in _alone:
        ob = OracleBatch(bv, oracle, model_dir, 1)
        outs = []
        for x, spk in queue:
            assert ob.a.BeatriceBatch_SetTargetSpeaker(None, 0, spk) == 0
            assert ob.a.BeatriceBatch_ResetStream(None, 0) == 0   # fresh contexts, all four key/value blocks of the speaker
            outs.append(np.concatenate([ob.convert(x[None, k * 160:(k + 1) * 160])[0] for k in range(len(x) // 160)]))
        ob.close()
        _alone["out"] = outs
    return _alone["out"]


@pytest.mark.parametrize("H", [1, 4])
def test_every_utterance_of_the_queue_equals_itself_converted_alone(bv, oracle, product, model_dir, H):
    B = 6
    queue = make_queue(bv, 20, 3, 40, 2, seed=3)
    want = converted_alone(bv, oracle, model_dir, queue)
    m = bv.Models(product, model_dir)
    batch = bv.Batch(m, B, hops_per_step=H)
    got, stats = run_queue(bv, batch, queue, in_flight=True)
    batch.close()
    m.close()
    print(stats)
    assert max(float(np.abs(w).max()) for w in want) > 0.05
    bad = [(i, len(w) // 240, float(np.abs(g - w).max())) for i, (g, w) in enumerate(zip(got, want)) if not np.array_equal(g, w)]
    assert not bad, "(utterance, hops, max-abs) that differ from the utterance converted alone: %s" % bad
    assert stats["resets"] == len(queue)
    assert stats["ticks_before_final_drain"] == stats["steps"]
    assert stats["ticks"] == stats["steps"] + stats["tick_stages"] - 1
