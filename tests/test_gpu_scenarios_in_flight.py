"""Seeded scenarios of the in-flight calls against the oracle (tests/scenario_in_flight.py; the list, its coverage of the named interactions,
the model's agreement with csrc/stream_move_plan.h and the scenarios' power to tell a wrong reference apart are held by
tests/test_cpu_scenarios_in_flight.py).

Per scenario: two product batches X and Y walk the scenario's phases in lockstep -- tick mode over resident I/O with the silent-block rule,
nothing synchronises inside a chunk -- while BeatriceBatch_ResetStreamInFlight, InstallSpeakersInFlight and the in-flight exports, imports
and moves are handed over between the steps.  Before every step BeatriceBatch_StreamQuiescent of every slot and
BeatriceBatch_SpeakerEntryBusy of every entry must equal the model's prediction, every in-flight call must return the code the model
predicts (0 or -3), and after every step BeatriceBatch_TicksLaunched must equal the model's count: one tick per step, whatever was asked.
The samples must equal, bit for bit,
  * one independent oracle stream per followed LOGICAL stream: its j-th present step is the oracle's step j, whichever batch and slot made it;
  * the product's own in-order chain for the streams no call but a reset of every stream ever touches.
A failure prints the first differing (batch, slot, step, logical stream, max-abs) and that logical stream's story across the moves;
`python tests/scenario_in_flight.py --seed N --gpu` runs that scenario alone."""
import os
import sys

import pytest

import scenario_in_flight as si

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENARIOS = si.scenarios()
ACROSS_THE_WRAP = [s for s in SCENARIOS if s["seed"] in si.ACROSS_THE_WRAP]
_references = {}


@pytest.fixture(scope="module")
def model_dir8(tmp_path_factory):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import make_model
    d = str(tmp_path_factory.mktemp("model8f"))
    make_model.make_model(d, n_speakers=si.REAL)
    return d


@pytest.mark.parametrize("scn", SCENARIOS, ids=[si.scenario_id(s) for s in SCENARIOS])
def test_scenario_matches_the_oracle_and_the_model(bv, oracle, product, model_dir8, scn):
    keep = _references if scn in ACROSS_THE_WRAP else None
    problems = si.compare(si.Env(bv, oracle, product, model_dir8), scn, references=keep)
    assert not problems, "\n".join(problems)


def test_four_scenarios_across_the_counter_wrap(bv, oracle, product, model_dir8):
    """The two batches start in front of the step counter's wrap (BeatriceBatch_SetStepCounter) so that it falls inside the scenario, at
    another step for X than for Y, with a move between the two; the oracle legs and the in-order chains are those of the test above.
    run_product asserts that each counter ends at (start + steps) mod the wrap."""
    problems = []
    for scn in ACROSS_THE_WRAP:
        problems += si.compare(si.Env(bv, oracle, product, model_dir8), scn, start_counter=si.wrap_starts(bv, scn), references=_references)
        _references.pop(si.scenario_id(scn), None)
    assert not problems, "\n".join(problems)
