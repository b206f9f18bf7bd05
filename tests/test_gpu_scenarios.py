"""Seeded scenarios of the batch's per-stream state machine against the oracle (tests/scenario.py; the list, its coverage of the named
interactions and its power to tell a wrong reference apart are held by tests/test_cpu_scenarios.py).

Per scenario: ONE batch of H hops per step is walked through the scenario's phases (in order, stage pipelining, resident I/O, tick mode with
streams sitting steps out, host streaming), state carried over.  Its samples must equal, bit for bit,
  * the product's own in-order chain at one hop per step, for every stream that never sits a step out, and
  * one independent oracle stream driven through the reference's per-hop protocol, for the sampled streams: every stream that sits out or
    that a planted interaction touches, plus tile corners
(MODEL_SPEC section 1 allows 1e-4 on the samples; every recorded run reports 0, and a state bug is loud -- no tolerance here), and the raw
pitch bins at the end must equal the in-order chain's.  Cells of steps a stream sits out are not compared.
A failure prints the seed, the first differing (step, stream, max-abs), that stream's own events with its pending-install count and its
present / absent history, and the interactions that touch it; `python tests/scenario.py --seed N --gpu` runs that scenario alone."""
import pytest

import scenario as sc

pytestmark = pytest.mark.gpu

SCENARIOS = sc.scenarios()
# the same scenarios with the step counter's wrap (bv.STEP_WRAP) near their middle: in order / tick mode / in order / tick mode at H = 4, stage
# pipelining behind tick mode, host streaming, resident I/O with and without ticks, two tile shapes
ACROSS_THE_WRAP = [s for s in SCENARIOS if s["seed"] in (3004, 3005, 3006, 3011, 3013, 3018)]
_references = {}


@pytest.mark.parametrize("scn", SCENARIOS, ids=[sc.scenario_id(s) for s in SCENARIOS])
def test_scenario_matches_in_order_chain_and_oracle(bv, oracle, product, model_dir, scn):
    keep = _references if scn in ACROSS_THE_WRAP else None
    problems = sc.compare(sc.Env(bv, oracle, product, model_dir), scn, references=keep)
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("scn", ACROSS_THE_WRAP, ids=[sc.scenario_id(s) + "-across-the-wrap" for s in ACROSS_THE_WRAP])
def test_scenario_across_the_counter_wrap(bv, oracle, product, model_dir, scn):
    """The batch that walks through the phases starts half the scenario's steps in front of the step counter's wrap
    (BeatriceBatch_SetStepCounter); the in-order chain and the oracle are the same legs as above.  run_product asserts that the counter
    ends at (start + steps) mod the wrap."""
    steps = sum(n for _, n in scn["phases"])
    start = bv.STEP_WRAP - steps // 2
    problems = sc.compare(sc.Env(bv, oracle, product, model_dir), scn, start_counter=start, references=_references)
    _references.pop(sc.scenario_id(scn), None)
    assert not problems, "\n".join(problems)
