"""The yardstick of the wrapper-mode walks (tests/wrapper_walk.py) alone, without a GPU: every case really contains what it is about (the
witnesses, from the yardstick's own state at each transition), and the yardstick can tell the contract it follows from the opposite one
(the negative controls).  tests/test_gpu_wrapper_walk.py holds the product against the same yardstick."""
import numpy as np
import pytest

import wrapper_walk as ww

CASES = ww.all_cases()


@pytest.fixture(scope="module")
def oracle_models(bv, oracle, model_dir):
    mo = bv.Models(oracle, model_dir)
    yield mo
    mo.close()


def test_the_flush_cases_are_the_sub_cases_they_are_named_for():
    kinds = set()
    for case in CASES:
        if case.want_flush:
            sched = ww.dry_run(case, 0)
            got = [sched.flush_kind[oi] for oi, op in enumerate(case.ops) if op[0] == "flush"]
            assert all(w is None or w == g for w, g in zip(case.want_flush, got)), (case.name, got)
            kinds.update(g for w, g in zip(case.want_flush, got) if w)
            for oi, op in enumerate(case.ops):
                if op[0] == "flush" and sched.flush_kind[oi] == "over_leftover":
                    assert sched.dropped[oi] > 0
                if op[0] == "flush" and sched.flush_kind[oi] in ("exact", "over_full"):
                    assert sched.dropped[oi] == 0 and sched.made_up[oi] > 0
    assert kinds == {"noop", "exact", "over_leftover", "over_full"}
    assert {c.H for c in CASES if c.want_flush} == {2, 4}


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_contains_what_it_is_about_and_its_controls_differ(bv, oracle_models, case):
    res = ww.yardstick(bv, oracle_models, case)
    sched = res[0].sched
    compared, skipped = ww.compared_calls(case, sched)
    print("%s: %d streams, %d calls, %d compared; not compared (owed at an unbind without flush): %s" % (case.name, case.B, case.n_calls, len(compared), skipped))
    assert len(compared) + len(skipped) == case.n_calls and len(skipped) <= 2 * case.H * len(case.transitions)
    for s, w in res.items():
        assert len(w.out) == case.n_calls and max(float(np.abs(o).max()) for o in w.out if o is not None and len(o)) > 1e-3
    holes = sorted((c, s) for c in range(case.n_calls) for s in range(case.B) if res[s].out[c] is None)
    assert holes == sorted(case.absent | case.silent)
    print("  blocks of absent or silent calls, not compared: %d %s" % (len(holes), holes))
    marks = [0] + [T for _i, _j, T in case.transitions]
    for _i, _j, T in case.transitions:
        wit = {s: w.witness[T] for s, w in res.items()}
        print("  transition at call %d: " % T + "; ".join("s%d fill %d gin %.1f->%.1f gout %.1f->%.1f kv %d" % (
            s, v["fill"], v["gin"][1], v["gin"][0], v["gout"][1], v["gout"][0], v["kv_pending"]) for s, v in wit.items()))
        # at least 22 model hops on each side of the transition, in every stream
        before = marks[marks.index(T) - 1]
        for s, v in wit.items():
            hops_then = res[s].witness[before]["hops_before"] if before else 0
            assert v["hops_before"] - hops_then >= 22, (s, T)
        aligned = ww.hop_aligned(case, T)
        assert all(0 < v["fill"] < 480 for s, v in wit.items() if not aligned[s]), "the FIFO is part filled at the transition"
        if case.holes:     # absent and silent blocks in the two calls on each side; a stream sits out the very call before
            sides = [side for side in ((T - 2, T - 1), (T, T + 1)) if case.calls[side[0]][0] in ("rag", "p", "io48", "f")]
            assert sides      # (the uniform calls of R3 cannot leave a stream out: the side with clocks per stream carries the holes)
            for side in sides:
                assert any(c in side for c, _s in case.silent) and (case.family48 or any(c in side for c, _s in case.absent))
            assert case.family48 or case.calls[T - 1][0] not in ("rag", "p") or any(c == T - 1 for c, _s in case.absent)
        if case.resets:    # a stream reset in the call before the transition and another in the call behind it
            assert {e[0] for e in case.events if e[1] == "reset"} >= {T - 1, T}
        if not case.family48:
            for v in wit.values():
                assert abs(v["gin"][0] - v["gin"][1]) > 1.0 and abs(v["gout"][0] - v["gout"][1]) > 1.0, "both gain ramps in progress"
        if case.family48 and case.H == 4:     # (a call takes all four installs there: the switch rides with the first call behind the transition)
            assert any(e[0] == T and e[1] == "spk" for e in case.events)
        else:
            assert any(0 < v["kv_pending"] for v in wit.values()), "a speaker switch whose key/value installs are still to come"
        assert any(v["knn"] for v in wit.values()) and not all(v["knn"] for v in wit.values())
    for s, w in res.items():     # ... and behind the last one
        last = case.transitions[-1][2]
        assert w.n_model - w.witness[last]["hops_before"] >= 22
    # negative controls: the opposite contract at one transition, on two streams, must show within two calls
    for i, _j, T in case.transitions:
        kinds = [None]
        if case.ops[i][0] == "flush" and sched.dropped[i] > 0:
            kinds.append("all_hops")
        for kind in kinds:
            for s in (0, 1):
                ctl = ww.yardstick(bv, oracle_models, case, streams=[s], control=(T, kind), stop_after_call=T + 2)[s]
                assert all(np.array_equal(ctl.out[c], res[s].out[c]) for c in range(T)), "a control changes nothing before its transition"
                differs = [c for c in (T, T + 1) if not np.array_equal(ctl.out[c], res[s].out[c])]
                print("  control %s at call %d, stream %d: differs in calls %s" % (kind or ww.control_kind(case, s, T, sched), T, s, differs))
                assert differs, "the control does not differ: the case tests nothing at this transition"
