"""One batch walked across the wrapper-mode transitions -- in order, bound (F / G / P), flushed, bound again, left through the other
form's call, configured at another rate, with clocks per stream and back, with the silent-block rule (S, F) and with streams reset beside
a transition -- against the yardstick of tests/wrapper_walk.py: per stream the ref-pinned wrapper oracle around an
independent stream of the CPU oracle, walked through the same script.  Every output block that include/beatrice_batch.h says is produced
is compared bit for bit; tests/test_cpu_wrapper_walk.py shows that every case contains what it is about and that the yardstick tells each
contract from its opposite."""
import time

import numpy as np
import pytest

import wrapper_walk as ww

pytestmark = pytest.mark.gpu

CASES = ww.all_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_walk_matches_the_yardstick(bv, oracle, product, model_dir, case):
    t0 = time.time()
    mo = bv.Models(oracle, model_dir)
    res = ww.yardstick(bv, mo, case)
    mo.close()
    t1 = time.time()
    scheds = {s: w.sched for s, w in res.items()}
    m = bv.Models(product, model_dir)
    try:
        got = ww.run_product(bv, m, case, scheds)
    except (ww.HipFailure, RuntimeError) as e:
        pytest.exit("%s: %s -- nothing more is started on this GPU" % (case.name, e), returncode=3)
    m.close()
    t2 = time.time()
    compared, skipped = ww.compared_calls(case, scheds[0])
    marks = [T for _i, _j, T in case.transitions]
    bad, dev, blocks, holes = [], 0.0, 0, 0
    for c in compared:
        assert got[c] is not None, "call %d: the header says its block is produced" % c
        for s in range(case.B):
            want = res[s].out[c]
            if want is None:      # (an absent or silent call: no block is produced)
                assert got[c][s] is None
                holes += 1
                continue
            for ch in range(got[c][s].shape[0]):
                blocks += 1
                if not np.array_equal(got[c][s][ch], want):
                    bad.append((c, s, ch))
                    d = np.abs(got[c][s][ch] - want)
                    dev = max(dev, float(np.nanmax(d)) if np.isfinite(d).any() else float("inf"))
    for c in skipped:
        assert got[c] is None
    print("%s: B=%d H=%d, %d calls, transitions at calls %s: %d blocks compared, %d calls not compared (owed at an unbind without flush: %s), %d blocks of absent or silent calls; "
          "%d blocks differ (max-abs %g), first %s; yardstick %.2f s, batch %.2f s" % (
              case.name, case.B, case.H, case.n_calls, marks, blocks, len(skipped), skipped, holes, len(bad), dev, bad[:6], t1 - t0, t2 - t1))
    assert max(float(np.abs(w.out[c]).max()) for w in res.values() for c in compared if w.out[c] is not None and len(w.out[c])) > 1e-3
    assert not bad, "%d blocks differ from the yardstick, the first at (call, stream, channel) %s" % (len(bad), bad[:6])
