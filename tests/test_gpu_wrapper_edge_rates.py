"""The any-rate wrapper's four resampling kernel forms (csrc/wrapper.hip.h) at the rate and block classes their control flow branches on --
the table of tests/wrapper_edge_cases.py: ratios 4, 6 and 8 on both sides of 48 kHz (the 257-sample history at capacity), tap tables read
from global memory (n_taps > kTapsLds) next to tables staged in LDS, the two sizes on either side of that threshold, fractions the < 1000
search truncates, the longest block a rate takes (x[], amp[], the inner buffer and ten FIFO pieces filled), and calls that yield no inner
sample at all.  tests/test_cpu_wrapper_edge_rates.py has walked the same (case, call)s through the plan header and the kernels' index
arithmetic on the CPU before any of this runs.

Expected values: ONE wrapper-oracle chain (oracle/wrapper_oracle.c, pinned to the reference's own headers at these rates by
tests/test_wrapper_oracle.py) around ONE oracle model stream per product stream, as tests/test_gpu_wrapper_rates.py builds them; computed
once per (case, stream, channel count) and shared by the four forms.  Every sample of every stream and channel is compared, with
np.array_equal: both sides do the same float32 mul-then-add in the same order."""
import ctypes as C

import numpy as np
import pytest

import wrapper_edge_cases as E
import wrapperlib
from tick_driver import Hip

pytestmark = pytest.mark.gpu
B = E.B


@pytest.fixture(scope="module")
def models(bv, product, model_dir):
    m = bv.Models(product, model_dir)
    yield m
    m.close()


@pytest.fixture(scope="module")
def oracle_models(bv, oracle, model_dir):
    m = bv.Models(oracle, model_dir)
    yield m
    m.close()


_signal, _want = {}, {}


def signal(case, s, channels):
    key = (case.id, s, channels)
    if key not in _signal:
        _signal[key] = E.signal(case, s, channels)
    return _signal[key]


def chain(bv, oracle_models, s, rate, mono, blocks, gains, rate_at=None):
    st = bv.Stream1(oracle_models, speaker=E.VOICE[s], vq_k=E.KNN[s])

    def hop(in160, out240, _u):
        np.ctypeslib.as_array(out240, (240,))[:] = st.hop(np.ctypeslib.as_array(in160, (160,)).copy())

    out = wrapperlib.oracle_wrapper().run_blocks(rate, mono, blocks, hop=hop, gains=gains, rate_at=rate_at)
    st.close()
    return out


def downmix(x):
    return np.ascontiguousarray(x[0] if x.shape[0] == 1 else ((x[0] + x[1]) * np.float32(0.5)).astype(np.float32))


def expected(bv, oracle_models, case, s, channels):
    """stream s of a case: its own seed, voice, k-NN setting and gains; left unchanged once computed"""
    key = (case.id, s, channels)
    if key not in _want:
        want = chain(bv, oracle_models, s, case.rate, downmix(signal(case, s, channels)), case.blocks, E.gain_events(case, s))
        want.setflags(write=False)
        _want[key] = want
    return _want[key]


def check(name, cases, channels, got, want):
    """got[s]: [channels][total]; want[s]: [total].  The oracle's sanity per stream, then every sample."""
    for s, case in enumerate(cases):
        w = want[s]
        assert np.isfinite(w).all(), (name, s)
        assert np.abs(w[int(0.02 * case.rate):]).max() > 1e-4, "%s stream %d: the oracle is silent behind the FIFO's 10 ms" % (name, s)
    for s in range(len(cases)):
        for t in range(s + 1, len(cases)):
            n = min(len(want[s]), len(want[t]))
            assert not np.array_equal(want[s][:n], want[t][:n]), (name, s, t)
    bad = []
    for s, case in enumerate(cases):
        for c in range(channels):
            if not np.array_equal(got[s][c], want[s]):
                d = np.abs(got[s][c] - want[s])
                first = int(np.argmax(d > 0))
                call = int(np.searchsorted(np.cumsum(case.blocks), first, side="right"))
                bad.append("stream %d (%s) channel %d: max-abs %g, first at sample %d = call %d (n = %d)" % (s, case.id, c, d.max(), first, call, case.blocks[call]))
    print("%s: %d streams x %d channels, max-abs %g" % (name, len(cases), channels, max(float(np.abs(got[s][c] - want[s]).max()) for s in range(len(cases)) for c in range(channels))))
    assert not bad, "%s: %s" % (name, "; ".join(bad))


def settings(a, h):
    for s in range(B):
        assert a.BeatriceBatch_SetTargetSpeaker(h, s, E.VOICE[s]) == 0 and a.BeatriceBatch_SetVQNumNeighbors(h, s, E.KNN[s]) == 0
    assert a.BeatriceBatch_FlushSpeaker(h, -1) == 0


def set_gains(a, h, s, case, k):
    gin, gout = E.gain_events(case, s).get(k, (None, None))
    if gin is not None:
        assert a.BeatriceBatch_SetInputGain(h, s, gin) == 0
    if gout is not None:
        assert a.BeatriceBatch_SetOutputGain(h, s, gout) == 0


# ---- form 1: wrap_in_kernel / wrap_out_kernel -------------------------------------------------------------------------------------------------
def run_form1(bv, models, case, extra=None):
    ch = case.channels
    x = np.stack([signal(case, s, ch) for s in range(B)])
    batch = bv.Batch(models, B)
    a, h = batch.a, batch.h
    try:
        settings(a, h)
        assert a.BeatriceBatch_ConfigureWrapper(h, case.rate) == 0
        assert a.BeatriceBatch_MaxWrapperBlock(h) == E.Rate(case.rate).longest >= max(case.blocks)
        got = np.zeros_like(x)
        pos = 0
        for k, n in enumerate(case.blocks):
            if extra is not None:
                extra(a, h, k)
            for s in range(B):
                set_gains(a, h, s, case, k)
            xin = np.ascontiguousarray(x[:, :, pos:pos + n])
            out = np.zeros_like(xin)
            assert a.BeatriceBatch_ProcessBlocks(h, bv.fptr(xin), bv.fptr(out), ch, n) == 0
            got[:, :, pos:pos + n] = out
            pos += n
    finally:
        batch.close()
    return got


@pytest.mark.parametrize("case", E.cases_of_form(1), ids=lambda c: c.id)
def test_form1_uniform_in_order(bv, models, oracle_models, case):
    got = run_form1(bv, models, case)
    check("form 1 " + case.id, [case] * B, case.channels, got, [expected(bv, oracle_models, case, s, case.channels) for s in range(B)])


# ---- form 2: wrap_call_kernel and its post half (one block length per binding) -------------------------------------------------------------
def run_form2(bv, models, case, H):
    ch, n, calls = case.channels, case.blocks[0], len(case.blocks)
    assert all(v == n for v in case.blocks)
    x = np.stack([signal(case, s, ch) for s in range(B)])
    batch = bv.Batch(models, B, hops_per_step=H)
    a, h = batch.a, batch.h
    hip = Hip()
    d_in = d_out = None
    try:
        settings(a, h)
        assert a.BeatriceBatch_ConfigureWrapper(h, case.rate) == 0
        delay = a.BeatriceBatch_ResidentBlocksDelayFor(h, n)
        assert delay > 0
        slots = max(calls, delay + 2)                      # every call has a slot of its own
        buf_in = np.zeros((slots, B, ch, n), np.float32)
        buf_in[:calls] = x.reshape(B, ch, calls, n).transpose(2, 0, 1, 3)
        d_in, d_out = hip.malloc(buf_in.nbytes), hip.malloc(buf_in.nbytes)
        hip.h2d(d_in, buf_in)
        assert hip.lib.hipMemset(d_out, 0, C.c_size_t(buf_in.nbytes)) == 0
        assert a.BeatriceBatch_BindResidentBlocks(h, d_in, d_out, ch, n, slots) == 0
        for k in range(calls):
            for s in range(B):
                set_gains(a, h, s, case, k)
            assert a.BeatriceBatch_ProcessBlocksDevice(h, None, None, ch, n) == 0
        if H > 1:     # the last calls end on a step that is still filling: made-up silence brings them out
            assert a.BeatriceBatch_FlushResidentBlocks(h) == 0
        assert a.BeatriceBatch_Synchronize(h) == 0 and a.BeatriceBatch_ResidentBlocksOwed(h) == 0
        out = np.zeros_like(buf_in)
        hip.d2h(out, d_out)
        assert a.BeatriceBatch_BindResidentBlocks(h, None, None, 0, 0, 0) == 0
    finally:
        batch.close()
        for p in (d_in, d_out):
            if p is not None:
                hip.free(p)
    return np.ascontiguousarray(out[:calls].transpose(1, 2, 0, 3)).reshape(B, ch, calls * n)


@pytest.mark.parametrize("case,H", [(c, H) for c in E.cases_of_form(2) for H in c.hops_per_step], ids=lambda v: v.id if isinstance(v, E.Case) else "H%d" % v)
def test_form2_uniform_around_the_ticks(bv, models, oracle_models, case, H):
    got = run_form2(bv, models, case, H)
    check("form 2 H=%d %s" % (H, case.id), [case] * B, case.channels, got, [expected(bv, oracle_models, case, s, case.channels) for s in range(B)])


# ---- forms 3 and 4: clocks per stream; stream s of a mix is stream s of its case ---------------------------------------------------------
def mix_blocks(cases, k):
    return [c.blocks[k] if k < len(c.blocks) else 0 for c in cases]


def run_form3(bv, models, cases, ch, extra=None):
    x = [signal(c, s, ch) for s, c in enumerate(cases)]
    calls = max(len(c.blocks) for c in cases)
    batch = bv.Batch(models, B)
    a, h = batch.a, batch.h
    try:
        settings(a, h)
        assert a.BeatriceBatch_ConfigureWrapperRates(h, (C.c_double * B)(*[c.rate for c in cases])) == 0
        got = [np.zeros_like(v) for v in x]
        pos = [0] * B
        for k in range(calls):
            if extra is not None:
                extra(a, h, k)
            ns = mix_blocks(cases, k)
            for s in range(B):
                if ns[s]:
                    set_gains(a, h, s, cases[s], k)
            xin = np.concatenate([np.ascontiguousarray(x[s][:, pos[s]:pos[s] + ns[s]]).reshape(-1) for s in range(B)]).astype(np.float32)
            out = np.zeros_like(xin)
            assert a.BeatriceBatch_ProcessBlocksRagged(h, bv.fptr(xin), bv.fptr(out), ch, (C.c_int * B)(*ns), 0) == 0
            at = 0
            for s in range(B):
                got[s][:, pos[s]:pos[s] + ns[s]] = out[at:at + ch * ns[s]].reshape(ch, ns[s])
                at += ch * ns[s]
                pos[s] += ns[s]
    finally:
        batch.close()
    return got


def run_form4(bv, models, cases, ch, extra=None, bind_rates=None, rate_at=None):
    """bind_rates: the rates configured while the binding is made (a stream's own rate is then set in flight before the first call);
    rate_at: stream -> call -> rate, BeatriceBatch_SetStreamRateInFlight in front of that call"""
    x = [signal(c, s, ch) for s, c in enumerate(cases)]
    calls = max(len(c.blocks) for c in cases)
    cap = max(max(c.blocks) for c in cases)
    cell = ch * cap
    batch = bv.Batch(models, B)
    a, h = batch.a, batch.h
    hip = Hip()
    d_in = d_out = None
    try:
        settings(a, h)
        rates0 = list(bind_rates or [c.rate for c in cases])
        assert a.BeatriceBatch_ConfigureWrapperRates(h, (C.c_double * B)(*rates0)) == 0
        buf_in = np.zeros((calls, B, cell), np.float32)
        pos = [0] * B
        for k in range(calls):
            ns = mix_blocks(cases, k)
            for s in range(B):
                buf_in[k, s, :ch * ns[s]] = x[s][:, pos[s]:pos[s] + ns[s]].reshape(-1)
                pos[s] += ns[s]
        d_in, d_out = hip.malloc(buf_in.nbytes), hip.malloc(buf_in.nbytes)
        hip.h2d(d_in, buf_in)
        assert hip.lib.hipMemset(d_out, 0, C.c_size_t(buf_in.nbytes)) == 0
        stages = a.BeatriceBatch_TickStages(h)
        assert a.BeatriceBatch_BindResidentBlocksRagged(h, d_in, d_out, ch, cap, max(calls, stages + 1)) == 0
        for s in range(B):
            if rates0[s] != cases[s].rate:
                assert a.BeatriceBatch_SetStreamRateInFlight(h, s, cases[s].rate) == 0
        for k in range(calls):
            if extra is not None:
                extra(a, h, k)
            for s in range(B):
                if rate_at and k in rate_at.get(s, {}):
                    assert a.BeatriceBatch_SetStreamRateInFlight(h, s, rate_at[s][k]) == 0
                    assert a.BeatriceBatch_BoundStreamRate(h, s) == rate_at[s][k]
            ns = mix_blocks(cases, k)
            for s in range(B):
                if ns[s]:
                    set_gains(a, h, s, cases[s], k)
            assert a.BeatriceBatch_ProcessBlocksRaggedDevice(h, (C.c_int * B)(*ns)) == 0
        assert a.BeatriceBatch_Synchronize(h) == 0 and a.BeatriceBatch_ResidentBlocksOwed(h) == 0
        out = np.zeros_like(buf_in)
        hip.d2h(out, d_out)
        assert a.BeatriceBatch_BindResidentBlocksRagged(h, None, None, 0, 0, 0) == 0
    finally:
        batch.close()
        for p in (d_in, d_out):
            if p is not None:
                hip.free(p)
    got = [np.zeros_like(v) for v in x]
    pos = [0] * B
    for k in range(calls):
        ns = mix_blocks(cases, k)
        for s in range(B):
            got[s][:, pos[s]:pos[s] + ns[s]] = out[k, s, :ch * ns[s]].reshape(ch, ns[s])
            pos[s] += ns[s]
    return got


@pytest.mark.parametrize("mix", E.MIXES, ids=lambda m: m[0])
def test_form3_clocks_per_stream_in_order(bv, models, oracle_models, mix):
    name, ch, cases = E.mix_cases(mix)
    got = run_form3(bv, models, cases, ch)
    check("form 3 " + name, cases, ch, got, [expected(bv, oracle_models, c, s, ch) for s, c in enumerate(cases)])


@pytest.mark.parametrize("mix", E.MIXES, ids=lambda m: m[0])
def test_form4_clocks_per_stream_around_the_ticks(bv, models, oracle_models, mix):
    """(every rate of a mix is configured while the binding is made: the stream that fires most hops per call sizes its slot ring)"""
    name, ch, cases = E.mix_cases(mix)
    got = run_form4(bv, models, cases, ch)
    check("form 4 " + name, cases, ch, got, [expected(bv, oracle_models, c, s, ch) for s, c in enumerate(cases)])


# ---- turnover: one stream walks 44 100 -> 47 952 -> 6 000 -> 384 000 inside a binding ----------------------------------------------------
def test_a_stream_walks_the_edge_rates_inside_the_binding(bv, models, oracle_models):
    """Stream 0 changes its rate every eight calls -- fewer than ResidentBlocksDelay(), so the records of the rate before are still owed when
    the next tables arrive, and the tap arena grows from about 10 k to about 64 k floats meanwhile.  Both its gains are ramping across
    every change.  The binding is made while stream 0 is configured at 6 kHz, the rate of the walk that fires most hops per call, and its
    first rate is set in flight before the first call.  Streams 1 and 2 (48 048 Hz, 176.4 kHz) are never asked anything."""
    legs = E.TURNOVER_LEGS
    blocks = [n for _, leg in legs for n in leg]
    starts = np.cumsum([0] + [len(leg) for _, leg in legs])
    gains0 = {7: (-20.0, 4.0), 15: (2.0, -10.0), 23: (-6.0, 0.0)}
    walk = E.Case(legs[0][0], "steady", 1, (4,), blocks=blocks, name="turnover-walk", gains={0: gains0})
    x0 = np.concatenate([wrapperlib.test_signal(sum(leg), int(rate), seed=7900 + i) for i, (rate, leg) in enumerate(legs)]).astype(np.float32)
    _signal[(walk.id, 0, 1)] = x0[None, :]
    cases = [walk, E.Case(48048.0, "steady", 1, (4,), blocks=[480] * len(blocks), name="turnover-48048"),
             E.Case(176400.0, "steady", 1, (4,), blocks=[1764] * len(blocks), name="turnover-176400")]
    rate_at = {int(starts[i]): legs[i][0] for i in range(1, len(legs))}
    got = run_form4(bv, models, cases, 1, bind_rates=[6000.0, 48048.0, 176400.0], rate_at={0: rate_at})
    want = [chain(bv, oracle_models, 0, legs[0][0], x0, blocks, gains0, rate_at=rate_at)] + [expected(bv, oracle_models, c, s, 1) for s, c in enumerate(cases) if s]
    # every leg is audible behind its own restarted FIFO
    for i, (rate, leg) in enumerate(legs):
        lo = sum(blocks[:starts[i]])
        seg = want[0][lo:lo + sum(leg)]
        assert np.abs(seg[:int(0.009 * rate)]).max() == 0.0 and np.abs(seg[int(0.03 * rate):]).max() > 1e-4, i
    check("turnover walk", cases, 1, got, want)


# ---- refusals at the edge change nothing --------------------------------------------------------------------------------------------------
def test_form1_refusals_at_the_edge_change_nothing(bv, models, oracle_models):
    """5 900, 5 000, 390 000 and 400 000 Hz (histories of 261, 308, 261 and 267 > 257) at BeatriceBatch_ConfigureWrapper and a block of
    MaxWrapperBlock + 1 samples at BeatriceBatch_ProcessBlocks, between the blocks of a batch at 8 kHz: -1, and the next blocks are those of
    a twin that never asked -- and of the oracle."""
    case = E.BY_ID["8000-steady-stereo"]
    asked = []

    def extra(a, h, k):
        if k not in (1, 4):
            return
        for rate in E.REFUSED_RATES:
            assert a.BeatriceBatch_ConfigureWrapper(h, rate) == -1, rate
        n = a.BeatriceBatch_MaxWrapperBlock(h) + 1
        assert n == E.Rate(case.rate).longest + 1
        z = np.zeros((B, case.channels, n), np.float32)
        assert a.BeatriceBatch_ProcessBlocks(h, bv.fptr(z), bv.fptr(z.copy()), case.channels, n) == -1
        asked.append(k)

    got, twin = run_form1(bv, models, case, extra), run_form1(bv, models, case)
    assert asked == [1, 4] and np.abs(twin).max() > 1e-3
    assert np.array_equal(got, twin)
    check("form 1 refusals", [case] * B, case.channels, got, [expected(bv, oracle_models, case, s, case.channels) for s in range(B)])


@pytest.mark.parametrize("form", [3, 4])
def test_clocks_per_stream_refusals_at_the_edge_change_nothing(bv, models, oracle_models, form):
    """the same rates at BeatriceBatch_ConfigureWrapperRates and BeatriceBatch_SetStreamRate (in order), at
    BeatriceBatch_SetStreamRateInFlight (inside the binding), and a block one sample longer than a stream may hand in"""
    name, ch, cases = E.mix_cases(E.MIXES[4])
    rates = [c.rate for c in cases]
    asked = []

    def extra(a, h, k):
        if k not in (1, 4):
            return
        ns = mix_blocks(cases, k)
        for rate in E.REFUSED_RATES:
            if form == 3:
                assert a.BeatriceBatch_ConfigureWrapperRates(h, (C.c_double * B)(rates[0], rate, rates[2])) == -1, rate
                assert a.BeatriceBatch_SetStreamRate(h, 1, rate) == -1, rate
            else:
                assert a.BeatriceBatch_SetStreamRateInFlight(h, 1, rate) == -1, rate
                assert a.BeatriceBatch_BoundStreamRate(h, 1) == rates[1]
        if form == 3:
            ns[2] = E.Rate(rates[2]).longest + 1
            z = np.zeros(ch * sum(ns), np.float32)
            assert a.BeatriceBatch_ProcessBlocksRagged(h, bv.fptr(z), bv.fptr(z.copy()), ch, (C.c_int * B)(*ns), 0) == -1
        else:
            ns[2] = max(max(c.blocks) for c in cases) + 1          # (one more than the binding's cell)
            assert a.BeatriceBatch_ProcessBlocksRaggedDevice(h, (C.c_int * B)(*ns)) == -1
        asked.append(k)

    run = run_form3 if form == 3 else run_form4
    got, twin = run(bv, models, cases, ch, extra), run(bv, models, cases, ch)
    assert asked == [1, 4]
    for s in range(B):
        assert np.abs(twin[s]).max() > 1e-3 and np.array_equal(got[s], twin[s]), s
    check("form %d refusals" % form, cases, ch, got, [expected(bv, oracle_models, c, s, ch) for s, c in enumerate(cases)])
