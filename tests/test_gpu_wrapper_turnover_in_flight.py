"""One stream's life cycle INSIDE a binding with clocks per stream (mode P: BeatriceBatch_ConfigureWrapperRates, BindResidentBlocksRagged,
ProcessBlocksRaggedDevice): BeatriceBatch_SetStreamRateInFlight / RestartStreamInFlight / BoundStreamRate.  Nothing drains, the blocks that
are owed come out as if nothing had been asked, no bit of any other stream changes.

Yardstick per stream, at array_equal: ONE Proxy of tests/test_host_proxy.py on the oracle core, through Spec / proxy_run of
tests/test_gpu_stream_wrapper_lifecycle.py.  The events "rate", "restart" and "reset" land at the same block boundary; a slot turned over
is restart plus ResetContext.  Where the oracle has no leg (the refusals, the tick counts) a twin product batch that never asked.

Shape: 5 streams at 44.1 / 48 / 96 / 32 / 48 kHz with blocks of 441 / 480 / 1024 / 300 / 64 samples, 3 x TickStages() + 12 calls, so that
more than ResidentBlocksDelay() calls lie on each side of every cluster of events; every call's slot is its own (n_slots = the calls), so
nothing but the events' own BeatriceBatch_Synchronize drains before the end.  Silent and absent blocks are handed in as n_samples = 0.
Behind the unbind every stream gets one more block through the in-order BeatriceBatch_ProcessBlocksRagged (the proxies: a restart, then
that block)."""
import ctypes as C

import numpy as np
import pytest

import wrapperlib
from test_gpu_stream_wrapper_lifecycle import Spec, proxy_run
from tick_driver import Hip

pytestmark = pytest.mark.gpu

RATES = (44100.0, 48000.0, 96000.0, 32000.0, 48000.0)
BLOCKS = (441, 480, 1024, 300, 64)
B = len(RATES)
CAP = max(BLOCKS)


@pytest.fixture(scope="module")
def models(bv, product, model_dir):
    m = bv.Models(product, model_dir)
    yield m
    m.close()


@pytest.fixture(scope="module")
def stages(bv, models):
    batch = bv.Batch(models, 1)
    n = batch.a.BeatriceBatch_TickStages(batch.h)
    batch.close()
    assert n >= 14   # (the clusters of events below are up to 10 calls wide and must fit inside the delay)
    return n


class Script:
    """Five streams in terms of the product's CALLS: events[s] = (boundary in front of call c, op, arg), silent[s] / absent[s] = calls.  A
    stream's Spec counts ITS blocks (an absent call is no block of the proxy's): an event at boundary c stands before the stream's next
    block, wherever that lies.  The last block of every Spec is the in-order one behind the unbind."""

    def __init__(self, channels, calls, seed, events=None, silent=None, absent=None):
        events, silent, absent = events or {}, silent or {}, absent or {}
        self.channels, self.calls = channels, calls
        self.present = [[c for c in range(calls) if c not in absent.get(s, ())] for s in range(B)]
        self.boundary = [dict() for _ in range(B)]     # stream -> call boundary -> [(op, arg)]
        self.specs = []
        for s in range(B):
            ev = []
            for c, op, arg in events.get(s, ()):
                ev.append((sum(1 for p in self.present[s] if p < c), op, arg))
                self.boundary[s].setdefault(c, []).append((op, arg))
            n = len(self.present[s])
            ev.append((n, "restart", 8000.0))          # the unbind restarts every stream's wrapper
            sil = tuple(self.present[s].index(c) for c in silent.get(s, ()))
            self.specs.append(Spec(RATES[s], (BLOCKS[s],) * (n + 1), channels, True, seed + 10 * s, s % 3, s % 3, events=tuple(ev), silent=sil))


def drive(bv, models, script, ask=True, syncs=(), bind_rates=None, extra=None):
    """The script through one batch in mode P.  ask = False: the twin that makes none of the three new calls.  syncs: boundaries with a
    BeatriceBatch_Synchronize behind the events.  bind_rates: the rates configured while the binding is made (the streams' own rates are set
    in flight before the first call).  extra(batch, c): called at every boundary, before the events."""
    channels, calls, specs = script.channels, script.calls, script.specs
    batch = bv.Batch(models, B)
    a, h = batch.a, batch.h
    hip = Hip()
    cell = channels * CAP
    d_in, d_out = hip.malloc(calls * B * cell * 4), hip.malloc(calls * B * cell * 4)
    res = {"no_drain": 0, "rates": []}
    try:
        for s, sp in enumerate(specs):
            assert a.BeatriceBatch_SetTargetSpeaker(h, s, sp.voice) == 0 and a.BeatriceBatch_SetVQNumNeighbors(h, s, sp.vq) == 0
        rates0 = list(bind_rates or RATES)
        assert a.BeatriceBatch_ConfigureWrapperRates(h, (C.c_double * B)(*rates0)) == 0
        assert a.BeatriceBatch_BoundStreamRate(h, 0) == 0.0      # not bound yet
        assert a.BeatriceBatch_BindResidentBlocksRagged(h, d_in, d_out, channels, CAP, calls) == 0
        delay = a.BeatriceBatch_ResidentBlocksDelay(h)
        x = [sp.signal() for sp in specs]
        buf_in = np.zeros((calls, B, cell), np.float32)
        for s in range(B):
            n = BLOCKS[s]
            for k, c in enumerate(script.present[s]):
                buf_in[c, s, :channels * n] = x[s][:, k * n:(k + 1) * n].reshape(-1)
        hip.h2d(d_in, buf_in)
        assert hip.lib.hipMemset(d_out, 0, C.c_size_t(buf_in.nbytes)) == 0

        def quiet(fn, *args):
            """one of the new calls: it returns 0 and neither a tick nor an output half has run"""
            before = (a.BeatriceBatch_TicksLaunched(h), a.BeatriceBatch_ResidentBlocksOwed(h))
            assert fn(h, *args) == 0, (fn, args)
            assert (a.BeatriceBatch_TicksLaunched(h), a.BeatriceBatch_ResidentBlocksOwed(h)) == before, (fn, args)
            res["no_drain"] += 1

        for s in range(B):
            if rates0[s] != RATES[s]:
                quiet(a.BeatriceBatch_SetStreamRateInFlight, s, RATES[s])
        nxt = [0] * B
        for c in range(calls):
            if extra is not None:
                extra(batch, c)
            for s in range(B):
                ops = script.boundary[s].get(c, ())
                reset = any(op == "reset" for op, _ in ops)
                for op, arg in ops:
                    if op == "voice":
                        assert a.BeatriceBatch_SetTargetSpeaker(h, s, arg) == 0
                    elif op == "out_gain":
                        assert a.BeatriceBatch_SetOutputGain(h, s, float(arg)) == 0
                    elif not ask or op == "reset":
                        continue
                    elif op == "rate":
                        quiet(a.BeatriceBatch_SetStreamRateInFlight, s, float(arg))
                        assert a.BeatriceBatch_BoundStreamRate(h, s) == arg
                    elif op == "restart":   # (with "reset" at the same boundary: the slot is turned over)
                        quiet(a.BeatriceBatch_RestartStreamInFlight, s, 0.0, 1 if reset else 0)
            if c in syncs:
                assert a.BeatriceBatch_Synchronize(h) == 0 and a.BeatriceBatch_ResidentBlocksOwed(h) == 0
            ns = [0] * B
            for s in range(B):
                k = nxt[s]
                if k < len(script.present[s]) and script.present[s][k] == c:
                    ns[s] = 0 if k in specs[s].silent else BLOCKS[s]
                    nxt[s] += 1
            assert a.BeatriceBatch_ProcessBlocksRaggedDevice(h, (C.c_int * B)(*ns)) == 0
            assert a.BeatriceBatch_ResidentBlocksOwed(h) == min(delay, c + 1 - max([0] + [t for t in syncs if t <= c]))
            res["rates"].append([a.BeatriceBatch_BoundStreamRate(h, s) for s in range(B)])
        assert a.BeatriceBatch_Synchronize(h) == 0 and a.BeatriceBatch_ResidentBlocksOwed(h) == 0
        res["ticks"] = a.BeatriceBatch_TicksLaunched(h)
        out = np.zeros_like(buf_in)
        hip.d2h(out, d_out)
        res["out"] = out
        got = [np.zeros_like(x[s]) for s in range(B)]
        for s in range(B):
            n = BLOCKS[s]
            for k, c in enumerate(script.present[s]):
                if k not in specs[s].silent:
                    got[s][:, k * n:(k + 1) * n] = out[c, s, :channels * n].reshape(channels, n)
        bound = [a.BeatriceBatch_BoundStreamRate(h, s) for s in range(B)]
        assert a.BeatriceBatch_StreamRate(h, 0) == 0.0                           # (the in-order getter is refused inside the binding)
        assert a.BeatriceBatch_BindResidentBlocksRagged(h, None, None, 0, 0, 0) == 0
        res["rates_after_unbind"] = [a.BeatriceBatch_StreamRate(h, s) for s in range(B)]
        assert res["rates_after_unbind"] == bound and a.BeatriceBatch_BoundStreamRate(h, 0) == 0.0
        # back in order with every stream's wrapper restarted: one more block each
        xin = np.concatenate([np.ascontiguousarray(x[s][:, -BLOCKS[s]:]).reshape(-1) for s in range(B)]).astype(np.float32)
        tail = np.zeros_like(xin)
        assert a.BeatriceBatch_ProcessBlocksRagged(h, bv.fptr(xin), bv.fptr(tail), channels, (C.c_int * B)(*BLOCKS), 0) == 0
        offs = np.cumsum([0] + [channels * n for n in BLOCKS])
        for s in range(B):
            got[s][:, -BLOCKS[s]:] = tail[offs[s]:offs[s + 1]].reshape(channels, BLOCKS[s])
        res["got"] = got
    finally:
        batch.close()
        hip.free(d_in)
        hip.free(d_out)
    return res


def compare(script, res, model_dir, streams=range(B)):
    """(bound blocks, the block behind the unbind) per stream: what differs from the proxies"""
    bad = []
    for s in streams:
        want, got, n = proxy_run(model_dir, script.specs[s]), res["got"][s], BLOCKS[s]
        assert np.abs(want[:, :-n]).max() > 1e-3
        for name, sl in (("bound", slice(0, -n)), ("behind the unbind", slice(-n, None))):
            if not np.array_equal(got[:, sl], want[:, sl]):
                d = np.abs(got[:, sl] - want[:, sl]).max(axis=0)
                k = int(np.argmax(d > 0)) // n
                bad.append("stream %d (%s): max-abs %g, first differing block %d = call %d" % (s, name, d.max(), k, (script.present[s] + [script.calls])[k]))
    return bad


_runs = {}


def once(key, fn):
    if key not in _runs:
        _runs[key] = fn()
    return _runs[key]


# ---- 1. two rate changes fewer than `delay` calls apart; the others do not notice -----------------------------------------------------------
def rate_script(channels, stages):
    """Stream 0: 44.1 -> 48 kHz in front of call E, an equal-rate call (nothing), -> 22.05 kHz ten calls later: the calls that are owed
    then name three sets of taps, and nobody is on the 44.1 kHz class while calls planned with it are owed.  22.05 kHz fires more hops per
    call than any rate the streams start with, so the binding is made while stream 0 is configured at 22.05 kHz, as the header says."""
    e = stages + 2
    events = {0: ((e - 1, "out_gain", -30.0), (e, "rate", 48000.0), (e + 5, "rate", 48000.0), (e + 10, "rate", 22050.0)),
              1: ((e + 4, "voice", 0),), 3: ((e + 10, "voice", 1),)}
    return Script(channels, 3 * stages + 12, 6100, events, silent={2: (e + 1, e + 11), 3: (5,)}, absent={4: (e, e + 1, e + 12)})


def rate_run(bv, models, stages, channels):
    def go():
        script = rate_script(channels, stages)
        return script, drive(bv, models, script, bind_rates=(22050.0,) + RATES[1:])
    return once(("rate", channels), go)


@pytest.mark.parametrize("channels", [1, 2], ids=["mono", "stereo"])
def test_a_stream_changes_its_rate_twice_inside_the_binding_and_the_others_do_not_notice(bv, models, model_dir, stages, channels):
    script, res = rate_run(bv, models, stages, channels)
    e = stages + 2
    assert res["rates"][e - 1][0] == 44100.0 and res["rates"][e][0] == 48000.0 and res["rates"][e + 9][0] == 48000.0 and res["rates"][e + 10][0] == 22050.0
    assert all(r[1:] == list(RATES[1:]) for r in res["rates"]) and res["no_drain"] == 4   # (44.1 kHz behind the bind, two changes, the equal-rate call)
    bad = compare(script, res, model_dir)
    assert not bad, "; ".join(bad)


# ---- 2. restart and turn-over ------------------------------------------------------------------------------------------------------------------
def turn_script(stages, ask_seed=6300):
    """In front of call E: stream 0 restarts at its rate with an output-gain ramp in flight, and its next block is silent.  E + 3: stream
    1's slot goes to a new caller (another voice set just before) while its hops are in the pipeline -- it fires one every call.  E + 6:
    stream 3's slot is turned over and then sits three calls out.  T: stream 4's slot is turned over right before a BeatriceBatch_Synchronize
    (it fires a hop every 7.5 calls: the reset waits across the drain).  Stream 2 is never asked anything."""
    e, t = stages + 2, 2 * stages + 10
    events = {0: ((e - 1, "out_gain", -40.0), (e, "restart", 48000.0)),
              1: ((e + 3, "voice", 0), (e + 3, "restart", 44100.0), (e + 3, "reset", None)),
              3: ((e + 5, "voice", 2), (e + 6, "restart", 48000.0), (e + 6, "reset", None)),
              4: ((t, "voice", 2), (t, "restart", 44100.0), (t, "reset", None))}
    return Script(2, 3 * stages + 12, ask_seed, events, silent={0: (e,), 2: (e + 4,)}, absent={3: (e + 6, e + 7, e + 8), 4: (3,)}), (t,)


def turn_run(bv, models, stages, ask):
    def go():
        script, syncs = turn_script(stages)
        return script, drive(bv, models, script, ask=ask, syncs=syncs)
    return once(("turn", ask), go)


def test_a_restart_and_three_slots_turned_over_inside_the_binding(bv, models, model_dir, stages):
    script, res = turn_run(bv, models, stages, True)
    assert res["no_drain"] == 4 and all(r == list(RATES) for r in res["rates"])
    bad = compare(script, res, model_dir)
    assert not bad, "; ".join(bad)


# ---- 3. nothing drains ---------------------------------------------------------------------------------------------------------------------------
def test_no_call_launches_a_tick_or_runs_an_owed_output_half(bv, models, stages):
    """drive() reads BeatriceBatch_TicksLaunched and BeatriceBatch_ResidentBlocksOwed around every one of the new calls.  Over the whole run
    the ticks are those of a twin that never asked: a call runs one tick per FIFO piece in which some stream fires, at least one; streams
    0 and 1 fire in their first piece in every call whatever their fill (480 inner samples per call), streams 3 and 4 never fire in a
    second piece (450 and 64 inner samples), so the count depends on stream 2 alone -- which neither run asks anything."""
    _, asked = turn_run(bv, models, stages, True)
    _, never = turn_run(bv, models, stages, False)
    assert asked["no_drain"] == 4 and never["no_drain"] == 0
    assert asked["ticks"] == never["ticks"] > 3 * stages + 12
    # (and the twin is a control for case 2: the streams that were asked differ, the stream that was not does not)
    assert np.array_equal(asked["out"][:, 2], never["out"][:, 2])
    for s in (0, 1, 3, 4):
        assert not np.array_equal(asked["out"][:, s], never["out"][:, s]), s


# ---- 4. after the unbind -------------------------------------------------------------------------------------------------------------------------
def test_after_the_unbind_the_in_order_getter_reports_the_new_rate(bv, models, model_dir, stages):
    """... and one in-order BeatriceBatch_ProcessBlocksRagged call matches the proxies that went on (compare()'s second part; drive() holds
    BeatriceBatch_StreamRate behind the unbind against BeatriceBatch_BoundStreamRate in front of it)."""
    script, res = rate_run(bv, models, stages, 1)
    assert res["rates_after_unbind"] == [22050.0] + list(RATES[1:])
    want = proxy_run(model_dir, script.specs[0])
    assert np.abs(want[:, -BLOCKS[0]:]).max() > 0 and np.array_equal(res["got"][0][:, -BLOCKS[0]:], want[:, -BLOCKS[0]:])


# ---- 5. refusals change nothing --------------------------------------------------------------------------------------------------------------------
def new_calls_refused(batch):
    a, h = batch.a, batch.h
    return [a.BeatriceBatch_SetStreamRateInFlight(h, 0, 44100.0), a.BeatriceBatch_SetStreamRateInFlight(h, 0, 22050.0),
            a.BeatriceBatch_RestartStreamInFlight(h, 0, 0.0, 0), a.BeatriceBatch_RestartStreamInFlight(h, 0, 0.0, 1),
            a.BeatriceBatch_RestartStreamInFlight(h, 0, 48000.0, 1), a.BeatriceBatch_BoundStreamRate(h, 0)] == [-1, -1, -1, -1, -1, 0.0]


@pytest.mark.parametrize("mode", ["rates_in_order", "silent_rule_in_order", "tick", "blocks48k_around_ticks", "resident_blocks"])
def test_the_new_calls_are_refused_in_every_mode_but_p(bv, product, model_dir, mode):
    """A with rates configured, S, D, F and G: -1 (0.0), and the batch goes on to the bit like one that never asked."""
    import test_gpu_mode_matrix as mm
    product = bv.bind_batch(product)
    H, steps = 1, 10
    x16 = np.stack([bv.synth_audio(160 * steps, seed=8800 + s) for s in range(mm.B)]).reshape(mm.B, steps, 160)
    x48 = np.stack([wrapperlib.test_signal(480 * steps * mm.CH, 48000, seed=8900 + s) for s in range(mm.B)]).astype(np.float32).reshape(mm.B, steps, H, mm.CH, 480)
    ns = [441, 480, 320]
    results = []
    for tries in (True, False):
        c = mm.Ctx(bv, product, model_dir, H)
        try:
            if mode == "rates_in_order":
                assert c.a.BeatriceBatch_ConfigureWrapperRates(c.h, (C.c_double * mm.B)(44100.0, 48000.0, 32000.0)) == 0
            else:
                mm.enter(c, mode)
            got = []
            for k in range(steps):
                if tries and k in (1, 4):
                    assert new_calls_refused(c.batch), (mode, k)
                if mode == "rates_in_order":
                    xin = np.concatenate([x48[s, k, 0, :, :ns[s]].reshape(-1) for s in range(mm.B)]).astype(np.float32)
                    y = np.zeros_like(xin)
                    assert c.a.BeatriceBatch_ProcessBlocksRagged(c.h, bv.fptr(xin), bv.fptr(y), mm.CH, (C.c_int * mm.B)(*ns), 0) == 0
                else:
                    y = mm.step(c, mode, k, x16[:, k], x48[:, k])
                if y is not None:
                    got.append(np.array(y, copy=True))
            got += mm.finish(c, mode)
            results.append(got)
        finally:
            c.close()
    tried, control = results
    assert len(tried) == len(control) > 0 and max(float(np.abs(y).max()) for y in control) > 1e-3
    for p, q in zip(tried, control):
        assert np.array_equal(p, q)


def test_refused_arguments_change_nothing_inside_the_binding(bv, models, stages):
    """Streams -1 and B; rates 0, negative, NaN, Inf and 1e9; 8 kHz -- 6144 inner samples from a 1024-sample block, 14 hops a call, under a
    binding sized for 5 (its lowest rate is 32 kHz).  Asked in front of calls 4 and 17 with blocks in flight; the accepted call in the
    same places is audible in the same blocks."""
    calls = stages + 25
    script = Script(1, calls, 6500)
    nan, inf = float("nan"), float("inf")
    ran = []

    def asks(batch, c):
        if c not in (4, 17):
            return
        a, h = batch.a, batch.h
        before = (a.BeatriceBatch_TicksLaunched(h), a.BeatriceBatch_ResidentBlocksOwed(h))
        for s in (-1, B, 1 << 20):
            assert a.BeatriceBatch_SetStreamRateInFlight(h, s, 44100.0) == -1 and a.BeatriceBatch_RestartStreamInFlight(h, s, 0.0, 0) == -1
            assert a.BeatriceBatch_RestartStreamInFlight(h, s, 44100.0, 1) == -1 and a.BeatriceBatch_BoundStreamRate(h, s) == 0.0
        for rate in (0.0, -44100.0, nan, inf, 1e9, 8000.0):
            assert a.BeatriceBatch_SetStreamRateInFlight(h, 1, rate) == -1, rate
            if rate != 0.0:   # (0.0 is "the present rate" there)
                assert a.BeatriceBatch_RestartStreamInFlight(h, 1, rate, 0) == -1 and a.BeatriceBatch_RestartStreamInFlight(h, 3, rate, 1) == -1, rate
        assert [a.BeatriceBatch_BoundStreamRate(h, s) for s in range(B)] == list(RATES)
        assert (a.BeatriceBatch_TicksLaunched(h), a.BeatriceBatch_ResidentBlocksOwed(h)) == before
        ran.append(c)

    def lands(batch, c):
        if c == 4:
            batch.restart_stream_in_flight(1)
            assert batch.bound_stream_rate(1) == 48000.0
        if c == 17:
            batch.set_stream_rate_in_flight(3, 44100.0)   # (a rate the binding has no class for)
            assert batch.bound_stream_rate(3) == 44100.0

    asked = drive(bv, models, script, extra=asks)
    never = drive(bv, models, script)
    landed = drive(bv, models, script, extra=lands)
    assert ran == [4, 17] and np.abs(never["out"]).max() > 1e-3
    assert np.array_equal(asked["out"], never["out"]) and asked["ticks"] == never["ticks"]
    for s in range(B):
        assert np.array_equal(asked["got"][s], never["got"][s])
    assert np.array_equal(landed["out"][:4], never["out"][:4])
    assert not np.array_equal(landed["out"][4:17, 1], never["out"][4:17, 1]) and not np.array_equal(landed["out"][17:, 3], never["out"][17:, 3])
    for s in (0, 2, 4):
        assert np.array_equal(landed["out"][:, s], never["out"][:, s]), s
