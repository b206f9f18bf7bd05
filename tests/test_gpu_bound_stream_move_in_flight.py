"""A stream moves between two bindings with clocks per stream (mode P: BeatriceBatch_ConfigureWrapperRates, BindResidentBlocksRagged,
ProcessBlocksRaggedDevice) and neither batch drains: BeatriceBatch_BoundStreamQuiescent / MoveBoundStreamsInFlight /
ExportBoundStreamsInFlight / ImportBoundStreamsInFlight / BoundWrapperBlobBytes (rules: beatrice-vst_amd/csrc/bound_move_plan.h).

Yardstick per stream, at array_equal: ONE Proxy of tests/test_host_proxy.py on the oracle core, through Spec / proxy_run of
tests/test_gpu_stream_wrapper_lifecycle.py.  A moved stream is one uninterrupted proxy: its blocks before the move come from the source
batch's output slots, its blocks after the move from the destination's -- and from the source's as well, because the source is unchanged
and is fed the same blocks again.  Where the oracle has no leg (refusals, counts) a twin product run that never asked.

Shape: a source batch of 3 streams (the mover is stream 1, its neighbours run 48 kHz / 480 and 32 kHz / 300), a destination of 2 (a
neighbour at 44.1 kHz / 300; slot 1's first user runs four 480-sample blocks at 48 kHz and then sits out).  delay + 6 calls of everyone,
the mover sits `delay` calls out, the move, delay + 6 more calls of both batches.  Every call has an input / output slot of its own, so
nothing but the final BeatriceBatch_Synchronize drains; every call checks BeatriceBatch_ResidentBlocksOwed and every new call is bracketed
by BeatriceBatch_TicksLaunched / ResidentBlocksOwed / BoundStreamRate.  Behind the unbind every stream gets one more in-order block (the
proxies: a restart, then that block)."""
import ctypes as C
import struct

import numpy as np
import pytest

from test_gpu_stream_migration import _free_bytes
from test_gpu_stream_wrapper_lifecycle import BLOB, HEADER, Spec, proxy_run
from test_host_proxy import K_IN_GAIN, K_MODEL, K_OUT_GAIN, K_VOICE, K_VQ, Proxy
from tick_driver import Hip

pytestmark = pytest.mark.gpu

CAP = 1024
# (441 samples at 44.1 kHz are exactly 480 at 48 kHz: that stream's FIFO is empty at every block boundary, so 44.1 kHz runs a second time with
#  300-sample blocks -- 326.5 inner samples a call, less than a hop -- and THAT case must have a fill at the move)
MOVERS = [(44100.0, 441), (48000.0, 64), (96000.0, 1024), (32000.0, 300), (44100.0, 300)]
MOVER_IDS = ["44.1k-441", "48k-64", "96k-1024", "32k-300", "44.1k-300"]
LOWEST = 32000.0   # (the bindings are made while a stream of the lowest rate is configured: include/beatrice_batch.h)
_f32p = C.POINTER(C.c_float)


def i32(v):
    return (C.c_int * len(v))(*v)


@pytest.fixture(scope="module")
def models(bv, product, model_dir):
    m = bv.Models(product, model_dir)
    yield m
    m.close()


@pytest.fixture(scope="module")
def delay(bv, models):
    batch = bv.Batch(models, 1)
    n = batch.a.BeatriceBatch_TickStages(batch.h)
    batch.close()
    assert n >= 2
    return n - 1


# ---- the yardstick -------------------------------------------------------------------------------------------------------------------------
_proxy_runs = {}


def proxy_of(model_dir, spec):
    """proxy_run; a script with an ("in_gain", dB) event goes through the same loop with that one setter added"""
    if not any(op == "in_gain" for _, op, _ in spec.events):
        return proxy_run(model_dir, spec)
    if spec.key() in _proxy_runs:
        return _proxy_runs[spec.key()]
    assert not spec.rule and not spec.silent
    x = spec.signal()
    want = np.zeros_like(x)
    p = Proxy(spec.rate)
    assert p.call("SetString", K_MODEL, (model_dir + "/model.toml").encode()) == 0
    assert p.call("SetInt", K_VOICE, spec.voice) == 0 and p.call("SetNumber", K_VQ, float(spec.vq)) == 0
    pos = 0
    for k, n in enumerate(spec.lens):
        for at, op, arg in spec.events:
            if at != k:
                continue
            if op == "voice":
                assert p.call("SetInt", K_VOICE, arg) == 0
            elif op in ("in_gain", "out_gain"):
                assert p.call("SetNumber", K_IN_GAIN if op == "in_gain" else K_OUT_GAIN, float(arg)) == 0
            elif op == "restart":
                assert arg != spec.rate and p.call("SetSampleRate", float(arg)) == 0 and p.call("SetSampleRate", float(spec.rate)) == 0
            else:
                raise AssertionError(op)
        sl = slice(pos, pos + n)
        mono = np.ascontiguousarray(x[0, sl] if spec.channels == 1 else ((x[0, sl] + x[1, sl]) * np.float32(0.5)).astype(np.float32))
        o = np.zeros(n, np.float32)
        assert p.call("Process", mono.ctypes.data_as(_f32p), o.ctypes.data_as(_f32p), n) == 0
        want[:, sl] = o
        pos += n
    p.close()
    _proxy_runs[spec.key()] = want
    return want


class Caller:
    """One logical stream = one proxy: `blocks` bound blocks of n samples, then (tail) the in-order block behind the unbind."""

    def __init__(self, rate, n, blocks, channels, seed, voice, vq, events=(), tail=True):
        ev = tuple(events) + (((blocks, "restart", 8000.0),) if tail else ())
        self.spec = Spec(rate, (n,) * (blocks + (1 if tail else 0)), channels, False, seed, voice, vq, events=ev)
        self.rate, self.n, self.blocks, self.tail = rate, n, blocks, tail
        self.x = self.spec.signal()

    def block(self, k):
        return np.ascontiguousarray(self.x[:, k * self.n:(k + 1) * self.n])


class Head:
    """A caller in one slot of one batch, at block k; a moved stream has one head per batch, both on the same proxy."""

    def __init__(self, caller, k=0):
        self.caller, self.k, self.got = caller, k, {}

    def differs(self, model_dir):
        want, n = proxy_of(model_dir, self.caller.spec), self.caller.n
        assert self.got and np.abs(want).max() > 1e-3
        return [k for k, y in sorted(self.got.items()) if not np.array_equal(y, want[:, k * n:(k + 1) * n])]


class Side:
    """One batch in mode P, driven call by call; every call reads and writes a slot of its own."""

    def __init__(self, bv, models, rates, calls, channels=1, cap=CAP, hip_stream=None, voice_map=None, bind_rates=None, **batch_kw):
        self.bv, self.B, self.channels, self.cap, self.calls = bv, len(rates), channels, cap, calls
        self.batch = bv.Batch(models, self.B, **batch_kw)
        self.a, self.h, self.hip = self.batch.a, self.batch.h, Hip()
        self.voice_map = voice_map or (lambda v: v)
        self.cell = channels * cap
        self.bytes = calls * self.B * self.cell * 4
        self.d_in, self.d_out = self.hip.malloc(self.bytes), self.hip.malloc(self.bytes)
        self.heads, self.log, self.ticks, self.c, self.quiet_calls = [None] * self.B, [], [], 0, 0
        self.bind_rates = list(bind_rates or rates)
        self.rates = list(rates)
        self.hip_stream = hip_stream

    def bind(self):
        a, h = self.a, self.h
        if self.hip_stream is not None:
            assert a.BeatriceBatch_SetStream(h, self.hip_stream) == 0
        assert a.BeatriceBatch_ConfigureWrapperRates(h, (C.c_double * self.B)(*self.bind_rates)) == 0
        assert a.BeatriceBatch_BoundWrapperBlobBytes(h) == 0 and a.BeatriceBatch_BoundStreamQuiescent(h, 0) == -1   # not bound yet
        assert a.BeatriceBatch_BindResidentBlocksRagged(h, self.d_in, self.d_out, self.channels, self.cap, self.calls) == 0
        assert self.hip.lib.hipMemset(self.d_out, 0, C.c_size_t(self.bytes)) == 0
        self.delay = a.BeatriceBatch_ResidentBlocksDelay(h)
        for s in range(self.B):
            if self.bind_rates[s] != self.rates[s]:
                assert a.BeatriceBatch_SetStreamRateInFlight(h, s, self.rates[s]) == 0
        assert a.BeatriceBatch_BoundWrapperBlobBytes(h) == BLOB
        return self

    def attach(self, s, head):
        self.heads[s] = head
        c = head.caller
        if head.k == 0:   # a new caller: its voice and lottery setting (a moved stream brings them)
            assert self.a.BeatriceBatch_SetTargetSpeaker(self.h, s, self.voice_map(c.spec.voice)) == 0
            assert self.a.BeatriceBatch_SetVQNumNeighbors(self.h, s, c.spec.vq) == 0
        return head

    def state(self):
        a, h = self.a, self.h
        return (a.BeatriceBatch_TicksLaunched(h), a.BeatriceBatch_ResidentBlocksOwed(h), tuple(a.BeatriceBatch_BoundStreamRate(h, s) for s in range(self.B)))

    def call(self, active):
        a, h = self.a, self.h
        blk, ns = np.zeros((self.B, self.cell), np.float32), [0] * self.B
        for s in active:
            hd = self.heads[s]
            cal, k = hd.caller, hd.k
            for at, op, arg in cal.spec.events:
                if at != k or op == "restart":
                    continue
                if op == "voice":
                    assert a.BeatriceBatch_SetTargetSpeaker(h, s, self.voice_map(arg)) == 0
                elif op == "in_gain":
                    assert a.BeatriceBatch_SetInputGain(h, s, float(arg)) == 0
                elif op == "out_gain":
                    assert a.BeatriceBatch_SetOutputGain(h, s, float(arg)) == 0
                else:
                    raise AssertionError(op)
            blk[s, :self.channels * cal.n] = cal.block(k).reshape(-1)
            ns[s] = cal.n
            self.log.append((hd, k, self.c, s))
            hd.k += 1
        self.hip.h2d(C.c_void_p(self.d_in.value + self.c * blk.nbytes), blk)
        before = a.BeatriceBatch_TicksLaunched(h)
        assert a.BeatriceBatch_ProcessBlocksRaggedDevice(h, i32(ns)) == 0
        assert a.BeatriceBatch_ResidentBlocksOwed(h) == min(self.delay, self.c + 1)   # what an undisturbed run owes
        self.ticks.append(a.BeatriceBatch_TicksLaunched(h))
        assert self.ticks[-1] > before
        self.c += 1

    def finish(self):
        """the only drain; then the unbind and one in-order block for every slot that has a caller with a tail"""
        a, h, ch = self.a, self.h, self.channels
        assert a.BeatriceBatch_Synchronize(h) == 0 and a.BeatriceBatch_ResidentBlocksOwed(h) == 0
        out = np.zeros((self.calls, self.B, self.cell), np.float32)
        self.hip.d2h(out, self.d_out)
        self.out = out
        for hd, k, c, s in self.log:
            n = hd.caller.n
            hd.got[k] = out[c, s, :ch * n].reshape(ch, n).copy()
        self.bound_rates = [a.BeatriceBatch_BoundStreamRate(h, s) for s in range(self.B)]
        assert a.BeatriceBatch_BindResidentBlocksRagged(h, None, None, 0, 0, 0) == 0
        assert [a.BeatriceBatch_StreamRate(h, s) for s in range(self.B)] == self.bound_rates and a.BeatriceBatch_BoundStreamQuiescent(h, 0) == -1
        tails = [hd if hd is not None and hd.caller.tail and hd.k == hd.caller.blocks else None for hd in self.heads]
        ns = [hd.caller.n if hd else 0 for hd in tails]
        if any(ns):
            xin = np.concatenate([hd.caller.block(hd.k).reshape(-1) for hd in tails if hd]).astype(np.float32)
            y = np.zeros_like(xin)
            assert a.BeatriceBatch_ProcessBlocksRagged(h, self.bv.fptr(xin), self.bv.fptr(y), ch, i32(ns), 0) == 0
            offs = np.cumsum([0] + [ch * n for n in ns])
            for s, hd in enumerate(tails):
                if hd:
                    hd.got[hd.k] = y[offs[s]:offs[s + 1]].reshape(ch, ns[s]).copy()
        return self

    def close(self):
        self.batch.close()
        self.hip.free(self.d_in)
        self.hip.free(self.d_out)


def quiet(sides, fn, want=0):
    """one of the new calls: it returns `want` and neither a tick nor an output half has run, no rate has changed, in any of `sides`"""
    before = [s.state() for s in sides]
    rc = fn()
    assert rc == want, rc
    after = [s.state() for s in sides]
    for s, b4, aft in zip(sides, before, after):
        assert b4[:2] == aft[:2]
        s.quiet_calls += 1
    return before, after


def header_of(wrapper_blob):
    f = struct.unpack(HEADER, wrapper_blob[:80])
    return dict(rate=f[4], phase_down=f[5], phase_up=f[6], fill=f[7], gains=f[9:13])


def export_pair(side, streams, want=0):
    sb = C.create_string_buffer(len(streams) * side.batch.stream_blob_bytes())
    wb = C.create_string_buffer(len(streams) * BLOB)
    quiet([side], lambda: side.a.BeatriceBatch_ExportBoundStreamsInFlight(side.h, len(streams), i32(streams), C.cast(sb, C.c_void_p), C.cast(wb, C.c_void_p)), want)
    return sb.raw, wb.raw


def import_pair(side, streams, sb, wb, entry_map=None, want=0):
    s_, w_ = C.create_string_buffer(sb, len(sb)), C.create_string_buffer(wb, len(wb))
    em = None if entry_map is None else i32(entry_map)
    return quiet([side], lambda: side.a.BeatriceBatch_ImportBoundStreamsInFlight(side.h, len(streams), i32(streams), C.cast(s_, C.c_void_p), C.cast(w_, C.c_void_p),
                                                                                 em, 0 if em is None else len(entry_map)), want)


def move(src, dst, frm, to, entry_map=None, want=0):
    em = None if entry_map is None else i32(entry_map)
    return quiet([src, dst], lambda: src.a.BeatriceBatch_MoveBoundStreamsInFlight(src.h, dst.h, len(frm), i32(frm), i32(to), em, 0 if em is None else len(entry_map)), want)


def carry(how, src, dst, frm, to, entry_map=None):
    rates = [src.a.BeatriceBatch_BoundStreamRate(src.h, s) for s in frm]
    if how == "move":
        before, after = move(src, dst, frm, to, entry_map)
        before, after = before[1], after[1]
    else:
        sb, wb = export_pair(src, frm)
        before, after = import_pair(dst, to, sb, wb, entry_map)
        before, after = before[0], after[0]
    # the destination slot has the stream's rate, every other stream of it the rate it had
    for t in range(dst.B):
        assert after[2][t] == (rates[to.index(t)] if t in to else before[2][t])


# ---- the walk -------------------------------------------------------------------------------------------------------------------------------
def walk(bv, models, delay, rate, n, how="move", shared=False, channels=1, events=(), permute=False, probe=None, at_boundary=None, seed=7000,
         early=0, do_move=True):
    """The shape of the module docstring.  probe(c, src, dst): called in front of call c of both batches.  at_boundary(src, dst): in front of
    the move.  early: the move is tried that many calls before the boundary instead (and is expected by the caller to be refused: the mover
    then stays out of the destination).  Returns everything."""
    D = delay
    p1, calls = D + 6, 3 * D + 12
    at = p1 + D - early
    made = None
    hip = Hip()
    if shared:
        made = C.c_void_p()
        assert hip.lib.hipStreamCreateWithFlags(C.byref(made), 1) == 0
    voice_map, entry_map, dst_kw = None, None, {}
    if permute:
        t = models.tables
        order, entry_map = [2, 0, 1, 3], [1, 2, 0, 3]   # destination entry i holds the source's entry order[i]; source entry v sits at entry_map[v]
        voice_map = lambda v: entry_map[v]   # noqa: E731
        dst_kw = dict(max_speakers=t.n_speakers + 1, upload_tables=False)
    src = Side(bv, models, [48000.0, rate, 32000.0], calls, channels, hip_stream=made)
    dst = Side(bv, models, [44100.0, 48000.0], calls, channels, hip_stream=made, voice_map=voice_map, bind_rates=[44100.0, LOWEST], **dst_kw)
    res = dict(src=src, dst=dst, moved=False)
    try:
        if permute:
            cb, add, kv = (np.ascontiguousarray(x[order]) for x in (t.codebooks, t.additive, t.kv))
            assert dst.a.BeatriceBatch_SetSpeakerTables(dst.h, t.n_speakers + 1, bv.fptr(cb), bv.fptr(add), bv.fptr(t.formant), bv.fptr(kv)) == 0
            dst.batch.apply_defaults()
            # (every stream starts where a proxy starts: on the source's voice 0, all four blocks installed)
            assert dst.a.BeatriceBatch_SetTargetSpeaker(dst.h, -1, entry_map[0]) == 0 and dst.a.BeatriceBatch_FlushSpeaker(dst.h, -1) == 0
        src.bind()
        dst.bind()
        assert src.delay == D and dst.delay == D
        mover = Caller(rate, n, 2 * D + 12, channels, seed, 1, 1, events)
        heads = dict(src0=src.attach(0, Head(Caller(48000.0, 480, calls, channels, seed + 10, 0, 0))),
                     mover_src=src.attach(1, Head(mover)),
                     src2=src.attach(2, Head(Caller(32000.0, 300, calls, channels, seed + 20, 2, 2))),
                     dst0=dst.attach(0, Head(Caller(44100.0, 300, calls, channels, seed + 30, 2, 1))),
                     first=dst.attach(1, Head(Caller(48000.0, 480, 4, channels, seed + 40, 0, 2, tail=False))))
        res["heads"] = heads
        for c in range(calls):
            if probe is not None:
                probe(c, src, dst)
            if c == at and do_move:
                if at_boundary is not None:
                    at_boundary(src, dst)
                if early == 0:
                    assert src.a.BeatriceBatch_BoundStreamQuiescent(src.h, 1) == 1 and dst.a.BeatriceBatch_BoundStreamQuiescent(dst.h, 1) == 1
                    _, wb = export_pair(src, [1])   # (a question: changes nothing)
                    res["header"] = header_of(wb)
                    carry(how, src, dst, [1], [1], entry_map)
                    heads["mover_dst"] = dst.attach(1, Head(mover, heads["mover_src"].k))
                    res["moved"] = True
            back = c >= p1 + D
            src.call([0, 2] + ([1] if c < p1 or back else []))
            dst.call([0] + ([1] if c < 4 or (back and res["moved"]) else []))
        src.finish()
        dst.finish()
    finally:
        src.close()
        dst.close()
        if made is not None:
            hip.lib.hipStreamDestroy(made)
    return res


def bad_heads(res, model_dir, names=None):
    return {name: hd.differs(model_dir) for name, hd in res["heads"].items() if (names is None or name in names) and hd.differs(model_dir)}


_runs = {}


def once(key, fn):
    if key not in _runs:
        _runs[key] = fn()
    return _runs[key]


# ---- 1. device to device --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True], ids=["own streams", "one caller-made stream"])
@pytest.mark.parametrize("rate,n", MOVERS, ids=MOVER_IDS)
def test_a_bound_stream_moves_device_to_device_and_is_one_proxy(bv, models, model_dir, delay, rate, n, shared):
    res = once(("move", rate, n, shared), lambda: walk(bv, models, delay, rate, n, "move", shared, channels=2 if rate == 44100.0 else 1))
    hdr = res["header"]
    print("mover %g Hz / %d: fill %d, phases %d %d at the move" % (rate, n, hdr["fill"], hdr["phase_down"], hdr["phase_up"]))
    assert res["moved"] and hdr["rate"] == rate
    if (rate, n) in ((44100.0, 300), (48000.0, 64), (32000.0, 300)):
        assert hdr["fill"] != 0
    if rate != 48000.0:   # (at 48 kHz the resampler pair is the identity and has no phase)
        assert hdr["phase_down"] != 0 and hdr["phase_up"] != 0
    assert res["dst"].bound_rates == [44100.0, rate] and res["src"].bound_rates == [48000.0, rate, 32000.0]
    assert res["src"].quiet_calls == 2 and res["dst"].quiet_calls == 1   # (the export that asked for the header, the move)
    # the moved stream has blocks from both batches behind the move, all on the one proxy; so have the neighbours and the slot's first user
    assert len(res["heads"]["mover_dst"].got) == delay + 7 and len(res["heads"]["mover_src"].got) == 2 * delay + 13
    bad = bad_heads(res, model_dir)
    assert not bad, bad


# ---- 2. the blob pair -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,n", MOVERS, ids=MOVER_IDS)
def test_the_same_through_the_blob_pair(bv, models, model_dir, delay, rate, n):
    res = once(("blobs", rate, n), lambda: walk(bv, models, delay, rate, n, "blobs"))
    assert res["moved"] and res["dst"].bound_rates == [44100.0, rate]
    bad = bad_heads(res, model_dir)
    assert not bad, bad


# ---- 3. interchange ---------------------------------------------------------------------------------------------------------------------------
def test_an_in_flight_export_goes_on_in_an_in_order_batch(bv, models, model_dir, delay):
    """ExportBoundStreamsInFlight from P; ImportStreams + ImportStreamWrappers into a batch after ConfigureWrapperRates, which goes on through
    ProcessBlocksRagged.  The source goes on as well."""
    rate, n, more = 44100.0, 441, 6
    taken = {}

    def probe(c, src, dst):
        if c == 2 * delay + 6:
            taken["blobs"] = export_pair(src, [1])
            taken["k"] = src.heads[1].k

    res = walk(bv, models, delay, rate, n, probe=probe, do_move=False)
    mover = res["heads"]["mover_src"].caller
    io = bv.Batch(models, 2)
    try:
        a, h = io.a, io.h
        assert a.BeatriceBatch_ConfigureWrapperRates(h, (C.c_double * 2)(48000.0, 48000.0)) == 0
        assert a.BeatriceBatch_WrapperBlobBytes(h) == BLOB
        io.import_streams([1], taken["blobs"][0])
        io.import_stream_wrappers([1], taken["blobs"][1])
        assert a.BeatriceBatch_StreamRate(h, 1) == rate
        want = proxy_of(model_dir, mover.spec)
        for k in range(taken["k"], taken["k"] + more):
            x = mover.block(k).reshape(-1).astype(np.float32)
            y = np.zeros_like(x)
            assert a.BeatriceBatch_ProcessBlocksRagged(h, bv.fptr(x), bv.fptr(y), 1, i32([0, n]), 0) == 0
            assert np.array_equal(y.reshape(1, n), want[:, k * n:(k + 1) * n]), k
        assert np.abs(want[:, taken["k"] * n:(taken["k"] + more) * n]).max() > 1e-3
    finally:
        io.close()
    bad = bad_heads(res, model_dir)
    assert not bad, bad


def test_a_drained_in_order_export_is_taken_in_flight(bv, models, model_dir, delay):
    """The reverse: the stream runs in order (ProcessBlocksRagged), is exported with the drained pair, and ImportBoundStreamsInFlight takes it
    into the destination slot of a binding that goes on ticking."""
    rate, n, first = 44100.0, 441, 7
    calls = 2 * delay + 10
    mover = Caller(rate, n, first + delay + 6, 1, 7300, 1, 1)
    io = bv.Batch(models, 2)
    dst = Side(bv, models, [44100.0, 48000.0], calls, 1, bind_rates=[44100.0, LOWEST])
    try:
        a, h = io.a, io.h
        assert a.BeatriceBatch_ConfigureWrapperRates(h, (C.c_double * 2)(48000.0, rate)) == 0
        assert a.BeatriceBatch_SetTargetSpeaker(h, 1, 1) == 0 and a.BeatriceBatch_SetVQNumNeighbors(h, 1, 1) == 0
        want = proxy_of(model_dir, mover.spec)
        for k in range(first):
            x = mover.block(k).reshape(-1).astype(np.float32)
            y = np.zeros_like(x)
            assert a.BeatriceBatch_ProcessBlocksRagged(h, bv.fptr(x), bv.fptr(y), 1, i32([0, n]), 0) == 0
            assert np.array_equal(y.reshape(1, n), want[:, k * n:(k + 1) * n]), k
        sb, wb = io.export_streams([1]), io.export_stream_wrappers([1])
        dst.bind()
        d0 = dst.attach(0, Head(Caller(44100.0, 300, calls, 1, 7310, 2, 1)))
        fu = dst.attach(1, Head(Caller(48000.0, 480, 4, 1, 7320, 0, 2, tail=False)))
        md = None
        for c in range(calls):
            if c == delay + 4:
                assert dst.a.BeatriceBatch_BoundStreamQuiescent(dst.h, 1) == 1
                import_pair(dst, [1], sb, wb)
                md = dst.attach(1, Head(mover, first))
            dst.call([0] + ([1] if c < 4 or md is not None else []))
        dst.finish()
        assert dst.bound_rates == [44100.0, rate] and len(md.got) == delay + 7
        for name, hd in (("neighbour", d0), ("first user", fu), ("mover", md)):
            assert not hd.differs(model_dir), (name, hd.differs(model_dir))
    finally:
        io.close()
        dst.close()


# ---- 4. the boundary ----------------------------------------------------------------------------------------------------------------------------
def test_one_call_before_the_rule_is_met_everything_is_refused_with_minus_3(bv, models, model_dir, delay):
    """bound_move_plan.h: at rest once call c + delay has been made.  In front of that call -- the mover's last block was handed in `delay`
    calls ago, one of them still to come -- BoundStreamQuiescent is 0 and move, export and import return -3, as source and as destination
    (source stream 0, which is busy, is no destination either); the batches then equal a twin that never asked.  At the boundary: 1, and
    the move goes through (walk asserts it)."""
    rate, n = 48000.0, 64
    asked = []

    def probe(c, src, dst):
        if c != 2 * delay + 5:
            return
        assert src.a.BeatriceBatch_BoundStreamQuiescent(src.h, 1) == 0 and src.a.BeatriceBatch_BoundStreamQuiescent(src.h, 0) == 0
        assert dst.a.BeatriceBatch_BoundStreamQuiescent(dst.h, 1) == 1 and dst.a.BeatriceBatch_BoundStreamQuiescent(dst.h, 0) == 0
        move(src, dst, [1], [1], want=-3)                 # the source is not at rest
        move(dst, src, [1], [1], want=-3)                 # ... nor is it as a destination
        move(dst, src, [1], [0], want=-3)
        export_pair(src, [1], want=-3)
        export_pair(src, [0, 1], want=-3)
        sb, wb = export_pair(dst, [1])                    # (a pair that is good: only rest can be the reason)
        import_pair(src, [1], sb, wb, want=-3)
        import_pair(dst, [0], sb, wb, want=-3)
        asked.append(c)

    tried = walk(bv, models, delay, rate, n, probe=probe, seed=7400)
    never = walk(bv, models, delay, rate, n, seed=7400)
    assert asked == [2 * delay + 5] and tried["moved"] and never["moved"]
    for side in ("src", "dst"):
        assert np.abs(never[side].out).max() > 1e-3 and np.array_equal(tried[side].out, never[side].out)
        assert tried[side].ticks == never[side].ticks
    bad = bad_heads(tried, model_dir)
    assert not bad, bad


# ---- 5. state in motion -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["move", "blobs"])
def test_gain_ramps_a_speaker_switch_and_an_entry_map_travel(bv, models, model_dir, delay, how):
    """Both gains are set one block before the mover's last block in front of the move (2 dB/ms: -40 dB takes 20 ms, two to three blocks of
    300 samples at 32 kHz, so both ramps are in progress across the move), the voice is switched there as well: at one hop per 1.07 calls
    two of the four key/value blocks are still to come.  The destination holds its tables in another order."""
    k = delay + 4
    events = ((k, "out_gain", -40.0), (k, "in_gain", -40.0), (k, "voice", 2))
    res = walk(bv, models, delay, 32000.0, 300, how, events=events, permute=True, seed=7500)
    g = res["header"]["gains"]   # (in target, in now, out target, out now)
    assert g[0] == -40.0 and g[2] == -40.0 and -40.0 < g[1] < 0.0 and -40.0 < g[3] < 0.0, g
    bad = bad_heads(res, model_dir)
    assert not bad, bad


# ---- 6. pending restart / reset ----------------------------------------------------------------------------------------------------------------
def test_a_pending_restart_on_the_destination_is_cancelled(bv, models, model_dir, delay):
    """RestartStreamInFlight(reset_model = 1) on the destination slot right before the move: the stream that arrives replaces what it would
    have started over -- its next block is the moved stream's next block, not a first block."""
    def at_boundary(src, dst):
        quiet([dst], lambda: dst.a.BeatriceBatch_RestartStreamInFlight(dst.h, 1, 0.0, 1))

    res = walk(bv, models, delay, 44100.0, 441, "move", at_boundary=at_boundary, seed=7600)
    bad = bad_heads(res, model_dir)
    assert res["moved"] and not bad, bad


def test_a_pending_restart_or_reset_on_the_source_refuses_with_minus_3(bv, models, delay):
    calls = delay + 4
    src = Side(bv, models, [48000.0, 44100.0], calls)
    dst = Side(bv, models, [48000.0, 44100.0], calls)
    try:
        src.bind()
        dst.bind()
        for side in (src, dst):
            side.attach(0, Head(Caller(48000.0, 480, calls, 1, 7700, 0, 0)))
            side.attach(1, Head(Caller(44100.0, 441, calls, 1, 7710, 1, 1)))
        for c in range(calls):
            src.call([0] + ([1] if c < 2 else []))
            dst.call([0])
        a = src.a
        assert a.BeatriceBatch_BoundStreamQuiescent(src.h, 1) == 1 and a.BeatriceBatch_BoundStreamQuiescent(dst.h, 1) == 1
        sb, wb = export_pair(src, [1])
        for reset_model in (0, 1):
            assert a.BeatriceBatch_RestartStreamInFlight(src.h, 1, 0.0, reset_model) == 0
            assert a.BeatriceBatch_BoundStreamQuiescent(src.h, 1) == 1     # (at rest by both rules: what refuses is the pending restart)
            move(src, dst, [1], [1], want=-3)
            export_pair(src, [1], want=-3)
            import_pair(src, [1], sb, wb)          # as a destination the slot takes a stream: the restart and the reset are cancelled ...
            export_pair(src, [1])                  # ... and it is a source again
        move(src, dst, [1], [1])
    finally:
        src.close()
        dst.close()


# ---- 7. rates -------------------------------------------------------------------------------------------------------------------------------------
def test_a_rate_the_destination_was_not_sized_for_is_refused(bv, models, delay):
    """A destination bound at 48 kHz with max_samples = 480 (three hops a call at most) is asked to take a 16 kHz stream whose 480-sample
    blocks fire up to five: -1 from the move and from the import, and nothing changes.  (A rate the destination has never held but can
    take -- 96 kHz -- is the third case of tests 1 and 2: the class is added, the neighbours stay on their proxies.)"""
    calls = delay + 4
    src = Side(bv, models, [48000.0, 16000.0], calls, cap=480)
    dst = Side(bv, models, [48000.0, 48000.0], calls, cap=480)
    twin = Side(bv, models, [48000.0, 48000.0], calls, cap=480)
    try:
        for side in (src, dst, twin):
            side.bind()
            side.attach(0, Head(Caller(48000.0, 480, calls, 1, 7800, 0, 0)))
            side.attach(1, Head(Caller(side.rates[1], 480, calls, 1, 7810, 1, 1)))
        for c in range(calls):
            if c == delay + 2:
                assert src.a.BeatriceBatch_BoundStreamQuiescent(src.h, 1) == 1 and dst.a.BeatriceBatch_BoundStreamQuiescent(dst.h, 1) == 1
                before, after = move(src, dst, [1], [1], want=-1)
                assert before == after
                sb, wb = export_pair(src, [1])
                before, after = import_pair(dst, [1], sb, wb, want=-1)
                assert before == after
                move(dst, src, [1], [1])   # (the other way round it fits: only the rate was the reason)
            for side in (src, dst, twin):
                side.call([0] + ([1] if c < 2 or c >= delay + 2 else []))
        for side in (dst, twin):
            side.finish()
        assert np.abs(twin.out).max() > 1e-3 and np.array_equal(dst.out, twin.out) and dst.ticks == twin.ticks
    finally:
        src.close()
        dst.close()
        twin.close()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_change_nothing_and_allocate_nothing(bv, models, delay):
    steps = delay + 8
    other = bv.Batch(models, 2, hops_per_step=2)   # no partner for a move, and no mode P
    got, ran = {}, {}
    try:
        for name in ("asked", "never"):
            src = Side(bv, models, [48000.0, 44100.0, 32000.0], steps)
            dst = Side(bv, models, [48000.0, 44100.0], steps)
            try:
                src.bind()
                dst.bind()
                for side in (src, dst):
                    for s in range(side.B):
                        side.attach(s, Head(Caller(side.rates[s], 300, steps, 1, 7900 + s, s % 3, 1)))   # (vq 1: a batch whose every stream has vq 0 drops the k-NN stage, which drains)
                a = src.a
                size = src.batch.stream_blob_bytes()
                for k in range(steps):
                    if name == "asked" and k in (4, delay + 6):   # source stream 1 and destination stream 0 never hand in a block: at rest throughout
                        good_s, good_w = export_pair(src, [1])
                        out_s, out_w = C.create_string_buffer(2 * size), C.create_string_buffer(2 * BLOB)
                        vp = lambda b: C.cast(C.create_string_buffer(b, len(b)), C.c_void_p)   # noqa: E731
                        ex = lambda n, st, o=out_s, w=out_w: a.BeatriceBatch_ExportBoundStreamsInFlight(   # noqa: E731
                            src.h, n, st, C.cast(o, C.c_void_p) if o is not None else None, C.cast(w, C.c_void_p) if w is not None else None)
                        im = lambda n, st, sb=good_s * 2, wb=good_w * 2, em=None, n_map=0: a.BeatriceBatch_ImportBoundStreamsInFlight(   # noqa: E731
                            dst.h, n, st, vp(sb) if sb is not None else None, vp(wb) if wb is not None else None, em, n_map)
                        mv = lambda n, fr, to_, em=None, n_map=0, s=src.h, d=dst.h: a.BeatriceBatch_MoveBoundStreamsInFlight(s, d, n, fr, to_, em, n_map)   # noqa: E731

                        def damaged(blob, off, xor=0x01):
                            b = bytearray(blob)
                            b[off] ^= xor
                            return bytes(b)

                        def refused():
                            rcs = []
                            for call, B in ((ex, 3), (im, 2)):
                                rcs += [call(0, i32([0])), call(-1, i32([0])), call(B + 1, i32([0, 1, 2, 0])), call(1, None),
                                        call(1, i32([B])), call(1, i32([-1])), call(2, i32([1, 1]))]
                            rcs += [ex(1, i32([1]), None), ex(1, i32([1]), out_s, None), im(1, i32([0]), None), im(1, i32([0]), good_s, None)]
                            rcs += [im(1, i32([0]), damaged(good_s, 0)), im(1, i32([0]), damaged(good_s, 4)), im(1, i32([0]), damaged(good_s, 8, 0x10)),   # magic, version, size
                                    im(1, i32([0]), damaged(good_s, 40)), im(2, i32([0, 1]), good_s + damaged(good_s, 0)),                                   # the check word; the second blob
                                    im(1, i32([0]), good_s, damaged(good_w, 0)), im(1, i32([0]), good_s, damaged(good_w, 4)), im(1, i32([0]), good_s, damaged(good_w, 8, 0x10)),
                                    im(1, i32([0]), good_s, damaged(good_w, 16)), im(1, i32([0]), good_s, damaged(good_w, 32 + 8)),                        # the wrapper's check word, its fill
                                    im(1, i32([0]), good_s, damaged(good_w, 80 + 100)), im(2, i32([0, 1]), good_s * 2, good_w + damaged(good_w, 0)),       # its state; the second blob
                                    im(1, i32([0]), good_s, good_w, i32([0, 1, 2, 3]), -1), im(1, i32([0]), good_s, good_w, None, 4),
                                    im(1, i32([0]), good_s, good_w, i32([0, 1, 2, 3]), 0), im(1, i32([0]), good_s, good_w, i32([4, 1, 2, 3]), 4),
                                    im(1, i32([0]), good_s, good_w, i32([-1, 1, 2, 3]), 4)]
                            rcs += [mv(0, i32([1]), i32([0])), mv(3, i32([0, 1, 2]), i32([0, 1, 0])), mv(1, None, i32([0])), mv(1, i32([1]), None),
                                    mv(1, i32([3]), i32([0])), mv(1, i32([1]), i32([2])), mv(2, i32([1, 1]), i32([0, 1])), mv(2, i32([0, 1]), i32([0, 0])),
                                    mv(1, i32([1]), i32([0]), None, 4), mv(1, i32([1]), i32([0]), i32([0, 1, 2, 3]), 0), mv(1, i32([1]), i32([0]), i32([4, 1, 2, 3]), 4),
                                    mv(1, i32([1]), i32([0]), d=src.h), mv(1, i32([1]), i32([0]), s=None), mv(1, i32([1]), i32([0]), d=None),
                                    mv(1, i32([1]), i32([0]), d=other.h), mv(1, i32([0]), i32([0]), s=other.h)]
                            rcs += [a.BeatriceBatch_BoundStreamQuiescent(src.h, -1), a.BeatriceBatch_BoundStreamQuiescent(src.h, 3), a.BeatriceBatch_BoundStreamQuiescent(None, 0)]
                            return rcs
                        before = (src.state(), dst.state())
                        rcs = refused()
                        assert rcs and set(rcs) == {-1}, rcs
                        if k == 4:   # no staging, no event, no class and no table is made by a refused call
                            free = _free_bytes()
                            for _ in range(50):
                                assert set(refused()) == {-1}
                            assert _free_bytes() == free
                        assert before == (src.state(), dst.state())
                        ran[k] = len(rcs)
                    src.call([0, 2])
                    dst.call([1])
                src.finish()
                dst.finish()
                got[name] = (src.out, dst.out, src.ticks, dst.ticks)
            finally:
                src.close()
                dst.close()
    finally:
        other.close()
    assert sorted(ran) == [4, delay + 6]
    assert np.abs(got["never"][0]).max() > 1e-3
    assert np.array_equal(got["asked"][0], got["never"][0]) and np.array_equal(got["asked"][1], got["never"][1]) and got["asked"][2:] == got["never"][2:]


# ---- 9. mode gating ----------------------------------------------------------------------------------------------------------------------------
def new_calls_refused(batch, partner):
    a, h = batch.a, batch.h
    size, one = batch.stream_blob_bytes(), i32([0])
    sb, wb = C.create_string_buffer(size), C.create_string_buffer(BLOB)
    return [a.BeatriceBatch_BoundStreamQuiescent(h, 0), a.BeatriceBatch_BoundWrapperBlobBytes(h),
            a.BeatriceBatch_ExportBoundStreamsInFlight(h, 1, one, C.cast(sb, C.c_void_p), C.cast(wb, C.c_void_p)),
            a.BeatriceBatch_ImportBoundStreamsInFlight(h, 1, one, C.cast(sb, C.c_void_p), C.cast(wb, C.c_void_p), None, 0),
            a.BeatriceBatch_MoveBoundStreamsInFlight(h, partner.h, 1, one, one, None, 0),
            a.BeatriceBatch_MoveBoundStreamsInFlight(partner.h, h, 1, one, one, None, 0)] == [-1, 0, -1, -1, -1, -1]


@pytest.mark.parametrize("mode", ["in_order", "rates_in_order", "silent_rule_in_order", "stage_pipelining", "resident_io", "tick", "host_streaming",
                                  "blocks48k_around_ticks", "resident_blocks"])
def test_the_new_calls_are_refused_in_every_mode_but_p(bv, product, model_dir, mode):
    """A (with and without rates configured), S, B, C, D, E, F and G: -1 (the size: 0), also with a partner that IS in mode P, and the batch
    goes on to the bit like one that never asked."""
    import test_gpu_mode_matrix as mm
    import wrapperlib
    product = bv.bind_batch(product)
    H, steps = 1, 8
    x16 = np.stack([bv.synth_audio(160 * steps, seed=8800 + s) for s in range(mm.B)]).reshape(mm.B, steps, 160)
    x48 = np.stack([wrapperlib.test_signal(480 * steps * mm.CH, 48000, seed=8900 + s) for s in range(mm.B)]).astype(np.float32).reshape(mm.B, steps, H, mm.CH, 480)
    ns = [441, 480, 320]
    results = []
    partner = mm.Ctx(bv, product, model_dir, H)
    try:
        mm.enter(partner, "resident_blocks_per_stream_clocks")
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
                        assert new_calls_refused(c.batch, partner.batch), (mode, k)
                    if mode == "rates_in_order":
                        xin = np.concatenate([x48[s, k, 0, :, :ns[s]].reshape(-1) for s in range(mm.B)]).astype(np.float32)
                        y = np.zeros_like(xin)
                        assert c.a.BeatriceBatch_ProcessBlocksRagged(c.h, bv.fptr(xin), bv.fptr(y), mm.CH, i32(ns), 0) == 0
                    else:
                        y = mm.step(c, mode, k, x16[:, k], x48[:, k])
                    if y is not None:
                        got.append(np.array(y, copy=True))
                got += mm.finish(c, mode)
                results.append(got)
            finally:
                c.close()
        assert partner.a.BeatriceBatch_BoundStreamQuiescent(partner.h, 0) == 1 and partner.a.BeatriceBatch_BoundWrapperBlobBytes(partner.h) == BLOB
    finally:
        partner.close()
    tried, control = results
    assert len(tried) == len(control) > 0 and max(float(np.abs(y).max()) for y in control) > 1e-3
    for p, q in zip(tried, control):
        assert np.array_equal(p, q)


# ---- 10. leaks ------------------------------------------------------------------------------------------------------------------------------------
def test_thirty_accepted_rounds_do_not_leak(bv, models, delay):
    """Two bindings, no audio: the streams are at rest throughout.  A round = a move there, a blob pair back, at a rate the taker may have
    let go in between (the class comes and goes)."""
    a_side = Side(bv, models, [48000.0, 44100.0, 32000.0], delay + 2)
    b_side = Side(bv, models, [48000.0, 96000.0], delay + 2, bind_rates=[LOWEST, 96000.0])
    try:
        a_side.bind()
        b_side.bind()

        def cycle(i):
            move(a_side, b_side, [1 + i % 2], [i % 2])
            sb, wb = export_pair(b_side, [1 - i % 2])
            import_pair(a_side, [i % 3], sb, wb)

        for i in range(3):
            cycle(i)   # (staging, events, piece tables and the first extra classes are made here)
        before = _free_bytes()
        for i in range(30):
            cycle(i)
        after = _free_bytes()
        print("free device memory: %.1f MB -> %.1f MB" % (before / 2**20, after / 2**20))
        assert before - after <= 8 << 20
    finally:
        a_side.close()
        b_side.close()
