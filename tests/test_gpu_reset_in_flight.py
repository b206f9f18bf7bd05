"""BeatriceBatch_ResetStreamInFlight: a stream starts over INSIDE the tick pipeline -- nothing drains, the reset travels through the 28
stages with the step it applies to (csrc/tick_reset.hip.h).  Two yardsticks, both at max-abs 0 (the path has argmax and k-NN decisions):
a TWIN batch on which the same script uses the drained BeatriceBatch_ResetStream at the same steps, and tests/oracle_batch.py's
OracleBatch (its BeatriceBatch_ResetStream = fresh reference contexts) on sampled streams."""
import functools

import numpy as np
import pytest

from oracle_batch import OracleBatch
from tick_driver import Hip, Resident

pytestmark = pytest.mark.gpu

SHAPES = [(7, 70, 1), (7, 70, 2), (40, 64, 4)]
_ctx = {}


class Api:
    """What a script sees: the batch's calls, its handle, and reset(stream) -- in flight, drained, or the oracle's."""

    def __init__(self, obj, how):
        self.a, self.h, self.B = obj.a, obj.h, obj.B
        self.reset = {"inflight": lambda s: obj.a.BeatriceBatch_ResetStreamInFlight(obj.h, s),
                      "drained": lambda s: obj.a.BeatriceBatch_ResetStream(obj.h, s),
                      "oracle": lambda s: obj.a.BeatriceBatch_ResetStream(None, s)}[how]


def inputs(bv, B, steps, H):
    """Seeded noise with a few silent stretches."""
    x = np.stack([bv.synth_audio(160 * H * steps, seed=9100 + s) for s in range(B)]).reshape(B, steps, H * 160).copy()
    x[0, 5:9] = 0.0
    x[3, 38:43] = 0.0
    x[B - 1, 0:3] = 0.0
    return x


def settings(api):
    for s in range(api.B):
        assert api.a.BeatriceBatch_SetTargetSpeaker(api.h, s, s % 3) == 0
    assert api.a.BeatriceBatch_SetVQNumNeighbors(api.h, 2, 2) == 0   # the k-NN stream
    assert api.a.BeatriceBatch_FlushSpeaker(api.h, -1) == 0


def script_all(H):
    """The listed interactions: a reset before step 0, two streams three steps apart, one stream twice within TickStages() steps, -1,
    a stream with a speaker switch two hops old (H = 4: of this very step) whose key/value blocks are still pending, the k-NN stream."""
    def script(api, k):
        if k == 0:
            assert api.reset(0) == 0
        if k == 10:
            assert api.reset(1) == 0
        if k == 13:
            assert api.reset(3) == 0
        if k in (20, 30, 31):
            assert api.reset(4) == 0
        if k == 40:
            assert api.reset(-1) == 0
        if k == 50 - (2 // H):
            assert api.a.BeatriceBatch_SetTargetSpeaker(api.h, 5, 2) == 0
        if k == 50:
            assert api.reset(5) == 0
        if k == 55:
            assert api.reset(2) == 0
    return script


SIT_OUT = {1: {20, 21, 22}, 3: {31}, 6: {4, 5, 44}, 0: {12}}


def script_rule(H):
    """The same with streams that sit steps out: a reset issued inside a sit-out run of three steps (it waits for the stream's next
    present step), and one on the step before a sit-out."""
    base = script_all(H)

    def script(api, k):
        base(api, k)
        if k == 21:
            assert api.reset(1) == 0
        if k == 30:
            assert api.reset(3) == 0
    return script


def run_product(bv, product, model_dir, B, steps, H, script, how, rule=False, sync_before=(), tail=0, x=None):
    """-> (samples [steps][B][H * 240], in-order samples after tick mode [tail][B][H * 240], ticks launched before the final drain)"""
    x = inputs(bv, B, steps + tail, H) if x is None else x
    m = bv.Models(product, model_dir)
    batch = bv.Batch(m, B, hops_per_step=H)
    a, h = batch.a, batch.h
    api = Api(batch, how)
    settings(api)
    assert a.BeatriceBatch_TicksLaunched(h) == 0   # (outside tick mode)
    r = Resident(bv, batch, slots=steps + 2, tick=True)
    try:
        if rule:
            assert a.BeatriceBatch_EnableSilentBlockRule(h, 1) == 0
        for k in range(steps):
            r.buf[k] = x[:, k]
        r.hip.h2d(r.d_in, r.buf)
        for k in range(steps):
            script(api, k)
            if k in sync_before:
                assert a.BeatriceBatch_Synchronize(h) == 0
            if rule:
                flags = bytes(1 if k in SIT_OUT.get(s, ()) else 0 for s in range(B))
                if any(flags):
                    assert a.BeatriceBatch_SetSilentStreams(h, flags) == 0
            assert a.BeatriceBatch_ConvertFramesDevice(h, None, None) == 0
        ticks = a.BeatriceBatch_TicksLaunched(h)
        assert a.BeatriceBatch_Synchronize(h) == 0
        out = np.zeros((r.slots, B, H * 240), np.float32)
        r.hip.d2h(out, r.d_out)
        got = out[:steps].copy()
        r.leave()
        if rule:
            assert a.BeatriceBatch_EnableSilentBlockRule(h, 0) == 0
        assert a.BeatriceBatch_TicksLaunched(h) == 0
    finally:
        r.free()
    got_tail = np.stack([batch.convert(np.ascontiguousarray(x[:, steps + k])) for k in range(tail)]) if tail else None
    batch.close()
    m.close()
    return got, got_tail, ticks


def run_oracle(bv, oracle, model_dir, B, steps, H, script, sample, rule=False, tail=0):
    x = inputs(bv, B, steps + tail, H)
    ob = OracleBatch(bv, oracle, model_dir, B, sample=sample, hops_per_step=H)
    api = Api(ob, "oracle")
    settings(api)
    want = np.zeros((steps + tail, B, H * 240), np.float32)
    for k in range(steps + tail):
        if k < steps:
            script(api, k)
        absent = {s for s in ob.sample if rule and k < steps and k in SIT_OUT.get(s, ())}
        for s, y in ob.convert(x[:, k], absent=absent).items():
            want[k, s] = y
    sample = ob.sample
    ob.close()
    return sample, want


def sample_of(B):
    return list(range(B)) if B <= 8 else sorted({0, 1, 2, 3, 4, 5, 6, 16, B - 1})


@functools.lru_cache(maxsize=None)
def _oracle_cached(key):
    bv, oracle, model_dir = _ctx["bv"], _ctx["oracle"], _ctx["model_dir"]
    B, steps, H, rule, tail = key
    return run_oracle(bv, oracle, model_dir, B, steps, H, script_rule(H) if rule else script_all(H), sample_of(B), rule=rule, tail=tail)


def oracle_ref(bv, oracle, model_dir, B, steps, H, rule=False, tail=0):
    """One oracle run per (shape, script), shared by the tests that need it and left unchanged."""
    _ctx.update(bv=bv, oracle=oracle, model_dir=model_dir)
    return _oracle_cached((B, steps, H, rule, tail))


def differing(got, want, streams, steps, absent=None):
    return [(s, k, float(np.abs(got[k, s] - want[k, s]).max())) for s in streams for k in range(steps)
            if not (absent and k in absent.get(s, ())) and not np.array_equal(got[k, s], want[k, s])]


@pytest.mark.parametrize("B,steps,H", SHAPES)
def test_resets_in_flight_equal_the_drained_twin_and_the_oracle(bv, oracle, product, model_dir, B, steps, H):
    got, _, ticks = run_product(bv, product, model_dir, B, steps, H, script_all(H), "inflight")
    twin, _, ticks_twin = run_product(bv, product, model_dir, B, steps, H, script_all(H), "drained")
    sample, want = oracle_ref(bv, oracle, model_dir, B, steps, H)
    assert np.abs(want).max() > 0.05
    bad = differing(got, twin, range(B), steps)
    print("in flight vs drained twin: max-abs %g" % float(np.abs(got - twin).max()))
    assert not bad, "in flight vs the drained twin, (stream, step, max-abs): %s" % bad[:12]
    bad = differing(got, want, sample, steps)
    print("in flight vs oracle: max-abs %g" % max(float(np.abs(got[:, s] - want[:steps, s]).max()) for s in sample))
    assert not bad, "in flight vs the oracle, (stream, step, max-abs): %s" % bad[:12]
    # the no-drain property: N fed steps, the resets above among them, no Synchronize -> N tick launches; every drained reset costs more
    assert ticks == steps
    assert ticks_twin > steps


@pytest.mark.parametrize("B,steps,H", SHAPES)
def test_resets_in_flight_with_streams_that_sit_steps_out(bv, oracle, product, model_dir, B, steps, H):
    got, _, ticks = run_product(bv, product, model_dir, B, steps, H, script_rule(H), "inflight", rule=True)
    twin, _, _ = run_product(bv, product, model_dir, B, steps, H, script_rule(H), "drained", rule=True)
    sample, want = oracle_ref(bv, oracle, model_dir, B, steps, H, rule=True)
    absent = {s: ks for s, ks in SIT_OUT.items() if s < B}
    bad = differing(got, twin, range(B), steps, absent)
    assert not bad, "ragged launch, in flight vs the drained twin, (stream, step, max-abs): %s" % bad[:12]
    bad = differing(got, want, sample, steps, absent)
    assert not bad, "ragged launch, in flight vs the oracle, (stream, step, max-abs): %s" % bad[:12]
    assert ticks == steps


@pytest.mark.parametrize("B,steps,H", SHAPES)
def test_synchronize_and_leaving_tick_mode_while_a_reset_travels(bv, oracle, product, model_dir, B, steps, H):
    """Synchronize while the resets of steps 10 and 13 are five and two stages deep (the drain ticks carry them on), more steps, a reset
    that is still waiting for its step when tick mode is left, then in-order steps: relevel and the hand-over see the same state."""
    tail = 4

    def script(api, k, base=script_all(H)):
        base(api, k)
        if k == steps - 3:
            assert api.reset(6) == 0

    def leaving(api, k):
        script(api, k)

    got, got_tail, _ = run_product(bv, product, model_dir, B, steps, H, leaving, "inflight", sync_before=(15,), tail=tail)
    twin, twin_tail, _ = run_product(bv, product, model_dir, B, steps, H, leaving, "drained", sync_before=(15,), tail=tail)
    bad = differing(got, twin, range(B), steps)
    assert not bad, "in flight vs the drained twin, (stream, step, max-abs): %s" % bad[:12]
    bad = differing(got_tail, twin_tail, range(B), tail)
    assert not bad, "in order after tick mode, in flight vs the drained twin, (stream, step, max-abs): %s" % bad[:12]
    x = inputs(bv, B, steps + tail, H)
    ob = OracleBatch(bv, oracle, model_dir, B, sample=[1, 3, 4, 6], hops_per_step=H)
    api = Api(ob, "oracle")
    settings(api)
    for k in range(steps + tail):
        if k < steps:
            script(api, k)
        for s, y in ob.convert(x[:, k]).items():
            ref = got[k, s] if k < steps else got_tail[k - steps, s]
            assert np.array_equal(ref, y), "stream %d step %d vs the oracle: max-abs %g" % (s, k, float(np.abs(ref - y).max()))
    ob.close()


def test_a_reset_asked_for_after_the_last_step_is_applied_when_tick_mode_is_left(bv, product, model_dir):
    B, steps, H, tail = 7, 8, 1, 3
    x = inputs(bv, B, steps + tail, H)
    outs = {}
    for how in ("inflight", "drained"):
        m = bv.Models(product, model_dir)
        batch = bv.Batch(m, B, hops_per_step=H)
        api = Api(batch, how)
        settings(api)
        r = Resident(bv, batch, tick=True)
        try:
            r.feed([x[:, k] for k in range(steps)])
            assert api.reset(3) == 0   # no step follows in tick mode
            r.leave()
        finally:
            r.free()
        outs[how] = np.stack([batch.convert(np.ascontiguousarray(x[:, steps + k])) for k in range(tail)])
        batch.close()
        m.close()
    assert np.array_equal(outs["inflight"], outs["drained"])


@pytest.mark.parametrize("H", [1, 2, 4])
def test_a_switch_between_the_call_and_the_step_that_takes_the_reset(bv, oracle, product, model_dir, H):
    """The reset belongs to the stream's next present step, not to the call (found by tests/scenario_in_flight.py,
    switch_after_reset_in_flight_while_absent): stream 1 is asked to start over in the first step of its sit-out (SIT_OUT: 20..22) and
    switched to another speaker in the second; stream 2 is asked and switched in one gap.  The step that takes the reset is
    BeatriceBatch_ResetStream followed by that step with the settings of THAT moment -- all four key/value blocks of the new target at
    once (at H = 4 from the step's first hop on); the switch must not go on installing one block per hop behind the reset.  The oracle makes the switch, then the reset, in front
    of the step that takes it."""
    B, steps = 7, 30

    def asked(api, k):
        if k == 10:
            assert api.reset(2) == 0 and api.a.BeatriceBatch_SetTargetSpeaker(api.h, 2, 1) == 0
        if k == 20:
            assert api.reset(1) == 0
        if k == 21:
            assert api.a.BeatriceBatch_SetTargetSpeaker(api.h, 1, 2) == 0

    def taken(api, k):
        if k == 10:
            assert api.a.BeatriceBatch_SetTargetSpeaker(api.h, 2, 1) == 0 and api.reset(2) == 0
        if k == 21:
            assert api.a.BeatriceBatch_SetTargetSpeaker(api.h, 1, 2) == 0
        if k == 23:
            assert api.reset(1) == 0

    got, _, ticks = run_product(bv, product, model_dir, B, steps, H, asked, "inflight", rule=True)
    sample, want = run_oracle(bv, oracle, model_dir, B, steps, H, taken, [0, 1, 2], rule=True)
    assert ticks == steps and np.abs(want[:, 1]).max() > 0.05
    absent = {s: ks for s, ks in SIT_OUT.items() if s < B}
    bad = differing(got, want, sample, steps, absent)
    assert not bad, "in flight vs the oracle, (stream, step, max-abs): %s" % bad[:12]


def test_fallback_in_order_is_the_drained_reset(bv, product, model_dir):
    """Mode A: BeatriceBatch_ResetStreamInFlight is BeatriceBatch_ResetStream."""
    B, steps, H = 7, 14, 1
    x = inputs(bv, B, steps, H)
    outs = {}
    for how in ("inflight", "drained"):
        m = bv.Models(product, model_dir)
        batch = bv.Batch(m, B, hops_per_step=H)
        api = Api(batch, how)
        settings(api)
        got = []
        for k in range(steps):
            if k == 5:
                assert api.reset(2) == 0
            if k == 9:
                assert api.reset(-1) == 0
            got.append(batch.convert(np.ascontiguousarray(x[:, k])))
            assert batch.a.BeatriceBatch_TicksLaunched(batch.h) == 0
        outs[how] = np.stack(got)
        batch.close()
        m.close()
    assert np.abs(outs["drained"]).max() > 0.05
    assert np.array_equal(outs["inflight"], outs["drained"])


def test_fallback_around_the_48k_wrapper_is_the_drained_reset(bv, product, model_dir):
    """Mode F (resident 48 kHz blocks around the ticks): the wrapper's per-stream state is part of the reset, so it is the drained one."""
    import wrapperlib
    B, steps, H, channels, n = 7, 40, 1, 1, 480
    x = np.stack([wrapperlib.test_signal(steps * n, 48000, seed=6100 + s) for s in range(B)]).astype(np.float32).reshape(B, steps, 1, channels, n)
    xs = np.ascontiguousarray(x.transpose(1, 0, 2, 3, 4))   # [step][B][H][channels][n]
    outs = {}
    hip = Hip()
    for how in ("inflight", "drained"):
        m = bv.Models(product, model_dir)
        batch = bv.Batch(m, B, hops_per_step=H)
        a, h = batch.a, batch.h
        api = Api(batch, how)
        settings(api)
        slots = steps + 1
        d_in, d_out = hip.malloc(slots * B * H * channels * n * 4), hip.malloc(slots * B * H * channels * n * 4)
        try:
            assert a.BeatriceBatch_BindResidentIO48k(h, d_in, d_out, channels, slots) == 0
            buf = np.zeros((slots, B, H, channels, n), np.float32)
            buf[:steps] = xs
            hip.h2d(d_in, buf)
            for k in range(steps):
                if k in (6, 33):
                    assert api.reset(k % B) == 0
                if k == 20:
                    assert api.reset(-1) == 0
                assert a.BeatriceBatch_ConvertBlocks48kDevice(h, None, None, channels) == 0
            assert a.BeatriceBatch_Synchronize(h) == 0
            out = np.zeros((slots, B, H, channels, n), np.float32)
            hip.d2h(out, d_out)
            outs[how] = out[:steps].copy()
            batch.close()
            m.close()
        finally:
            hip.free(d_in)
            hip.free(d_out)
    assert np.abs(outs["drained"]).max() > 1e-3
    assert np.array_equal(outs["inflight"], outs["drained"])


def test_an_out_of_range_stream_is_refused_and_changes_nothing(bv, product, model_dir):
    B, steps, H = 7, 40, 1

    def asked(api, k):
        if k in (0, 7, 20):
            assert api.a.BeatriceBatch_ResetStreamInFlight(api.h, B) == -1
            assert api.a.BeatriceBatch_ResetStreamInFlight(api.h, -2) == -1
            assert api.a.BeatriceBatch_ResetStreamInFlight(api.h, 1 << 20) == -1

    got, _, ticks = run_product(bv, product, model_dir, B, steps, H, asked, "inflight")
    never, _, ticks_never = run_product(bv, product, model_dir, B, steps, H, lambda api, k: None, "inflight")
    assert np.abs(never).max() > 0.05
    assert np.array_equal(got, never)
    assert ticks == ticks_never == steps
