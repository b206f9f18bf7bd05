"""Streams join, leave and move with their own host clocks: BeatriceBatch_SetStreamRate / RestartStreamWrapper / StreamRate and the wrapper
blob of BeatriceBatch_ExportStreamWrappers / ImportStreamWrappers, on batches with clocks per stream (BeatriceBatch_ConfigureWrapperRates /
ProcessBlocksRagged).

Yardstick per stream, at max-abs 0: ONE Proxy of tests/test_host_proxy.py on the oracle core, as in tests/test_gpu_wrapper_ragged.py.  A
migrated stream is one proxy that keeps running; BeatriceBatch_SetStreamRate is BeatriceProxy_SetSampleRate at the same block boundary;
BeatriceBatch_RestartStreamWrapper is SetSampleRate(another rate) followed by SetSampleRate(the rate); a slot turned over adds ResetContext.
Where the oracle has no leg (the refusals) a twin product batch that never asked, compared over the blocks that follow.

CALLS = 22 calls on each side of an event: the deepest model ring has 17 step slots."""
import ctypes as C
import copy
import importlib.util
import os
import struct

import numpy as np
import pytest

import wrapperlib
from test_host_proxy import K_MODEL, K_OUT_GAIN, K_VOICE, K_VQ, Proxy

pytestmark = pytest.mark.gpu
_f32p = C.POINTER(C.c_float)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = 22
FORMS = [(1, False), (2, True)]   # (channels, the shell's silent rule): mono without it, stereo with it
FORM_IDS = ["mono", "stereo, silent rule"]
HEADER = "<IIQQd4i4d"             # csrc/wrapper_blob.h Header: magic, version, size, check, rate, phase_down, phase_up, fill, reserved, 4 gains
BLOB = 80 + 4 * (2 * 257 + 2 * 33 + 480)


@pytest.fixture(scope="module")
def shard():
    spec = importlib.util.spec_from_file_location("bv_shard", os.path.join(REPO, "beatrice-vst_amd", "shard.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def models(bv, product, model_dir):
    m = bv.Models(product, model_dir)
    yield m
    m.close()


# ---- one stream: what it is fed and what happens to it, the same script for the proxy and for the product ------------------------------------
class Spec:
    """rate: the host rate at the start; lens: the block length of every call; events: (call, op, arg) applied BEFORE that call --
    ("voice", v) ("out_gain", dB) ("rate", r) ("restart", another rate) ("reset", None); silent: calls whose block is all zeros."""

    def __init__(self, rate, lens, channels, rule, seed, voice, vq, events=(), silent=()):
        self.rate, self.lens, self.channels, self.rule, self.seed, self.voice, self.vq = rate, tuple(lens), channels, rule, seed, voice, vq
        self.events, self.silent = tuple(events), tuple(silent)

    def key(self):
        return (self.rate, self.lens, self.channels, self.rule, self.seed, self.voice, self.vq, self.events, self.silent)

    def signal(self):
        total = sum(self.lens)
        x = np.stack([(0.6 if c else 1.0) * wrapperlib.test_signal(total, int(self.rate), seed=self.seed + c) for c in range(self.channels)]).astype(np.float32)
        pos = 0
        for k, n in enumerate(self.lens):
            if k in self.silent:
                x[:, pos:pos + n] = 0.0
            pos += n
        return x


_proxy_runs = {}


def proxy_run(model_dir, spec):
    """[channels][sum(lens)] of ONE proxy on the oracle core through the whole script; computed once per script."""
    have = _proxy_runs.get(spec.key())
    if have is not None:
        return have
    x = spec.signal()
    want = np.zeros_like(x)
    p = Proxy(spec.rate)
    assert p.call("SetString", K_MODEL, (model_dir + "/model.toml").encode()) == 0
    assert p.call("SetInt", K_VOICE, spec.voice) == 0
    assert p.call("SetNumber", K_VQ, float(spec.vq)) == 0
    rate, pos = spec.rate, 0
    for k, n in enumerate(spec.lens):
        for at, op, arg in spec.events:
            if at != k:
                continue
            if op == "voice":
                assert p.call("SetInt", K_VOICE, arg) == 0
            elif op == "out_gain":
                assert p.call("SetNumber", K_OUT_GAIN, float(arg)) == 0
            elif op == "rate":
                assert p.call("SetSampleRate", float(arg)) == 0
                rate = arg
            elif op == "restart":
                assert arg != rate and p.call("SetSampleRate", float(arg)) == 0 and p.call("SetSampleRate", float(rate)) == 0
            elif op == "reset":
                assert p.call("ResetContext") == 0
            else:
                raise AssertionError(op)
        sl = slice(pos, pos + n)
        in0 = np.ascontiguousarray(x[0, sl])
        in1 = np.ascontiguousarray(x[1, sl]) if spec.channels == 2 else None
        o0, o1 = np.zeros(n, np.float32), np.zeros(n, np.float32)
        if spec.rule:
            flag = p.call("ProcessChannels", in0.ctypes.data_as(_f32p), in1.ctypes.data_as(_f32p) if in1 is not None else None,
                          o0.ctypes.data_as(_f32p), o1.ctypes.data_as(_f32p) if spec.channels == 2 else None, n)
            assert flag == (1 if k in spec.silent else 0)
        else:
            mono = in0 if spec.channels == 1 else ((in0 + in1) * np.float32(0.5)).astype(np.float32)
            assert p.call("Process", mono.ctypes.data_as(_f32p), o0.ctypes.data_as(_f32p), n) == 0
            o1 = o0
        want[0, sl] = o0
        if spec.channels == 2:
            want[1, sl] = o1
        pos += n
    p.close()
    _proxy_runs[spec.key()] = want
    return want


class Feed:
    """A stream on the product side: where it stands in its script, what it has got back so far.  It is not tied to a batch or a slot."""

    def __init__(self, spec):
        self.spec, self.x = spec, spec.signal()
        self.k = self.pos = 0
        self.got = np.zeros_like(self.x)

    def done(self):
        return self.k >= len(self.spec.lens)

    def before_call(self, batch, slot):
        a, h = batch.a, batch.h
        for at, op, arg in self.spec.events:
            if at != self.k:
                continue
            if op == "voice":
                assert a.BeatriceBatch_SetTargetSpeaker(h, slot, arg) == 0
            elif op == "out_gain":
                assert a.BeatriceBatch_SetOutputGain(h, slot, float(arg)) == 0
            elif op == "rate":
                batch.set_stream_rate(slot, arg)
                assert batch.stream_rate(slot) == arg
            elif op == "restart":
                batch.restart_stream_wrapper(slot)
            elif op == "reset":
                assert a.BeatriceBatch_ResetStream(h, slot) == 0

    def block(self):
        return self.x[:, self.pos:self.pos + self.spec.lens[self.k]]

    def take(self, out):
        n = self.spec.lens[self.k]
        self.got[:, self.pos:self.pos + n] = out
        self.pos += n
        self.k += 1


def start(bv, models, specs):
    """A batch with clocks per stream, stream s set up as tests/test_gpu_wrapper_ragged.py sets its streams up"""
    batch = bv.Batch(models, len(specs))
    a, h = batch.a, batch.h
    for s, sp in enumerate(specs):
        assert a.BeatriceBatch_SetTargetSpeaker(h, s, sp.voice) == 0
        assert a.BeatriceBatch_SetVQNumNeighbors(h, s, sp.vq) == 0
    assert a.BeatriceBatch_ConfigureWrapperRates(h, (C.c_double * len(specs))(*[sp.rate for sp in specs])) == 0
    return batch


def call(bv, batch, feeds, channels, rule, expect=0):
    """One BeatriceBatch_ProcessBlocksRagged: the next block of every feed that has one (None / finished: the slot sits the call out)"""
    live = [f is not None and not f.done() for f in feeds]
    for s, f in enumerate(feeds):
        if live[s]:
            f.before_call(batch, s)
    ns = [f.spec.lens[f.k] if live[s] else 0 for s, f in enumerate(feeds)]
    xin = np.concatenate([np.ascontiguousarray(f.block()).reshape(-1) for s, f in enumerate(feeds) if live[s]]).astype(np.float32)
    out = np.zeros_like(xin)
    assert batch.a.BeatriceBatch_ProcessBlocksRagged(batch.h, bv.fptr(xin), bv.fptr(out), channels, (C.c_int * len(feeds))(*ns), 1 if rule else 0) == expect
    at = 0
    for s, f in enumerate(feeds):
        if live[s]:
            cnt = channels * ns[s]
            f.take(out[at:at + cnt].reshape(channels, ns[s]))
            at += cnt


def same(feed, model_dir, what):
    want = proxy_run(model_dir, feed.spec)
    assert feed.done() and np.abs(want).max() > 1e-3
    d = np.abs(feed.got - want)
    edges = np.cumsum((0,) + feed.spec.lens)
    first = int(np.searchsorted(edges, int(np.argmax(d.max(axis=0) > 0)), side="right")) - 1
    assert np.array_equal(feed.got, want), "%s: max-abs %g, first differing call %d" % (what, d.max(), first)


def header_of(blob):
    return struct.unpack_from(HEADER, blob, 0)


# ---- 1. a stream moves with its host side ------------------------------------------------------------------------------------------------------
AFTER = (441, 512, 300, 441, 330, 512)   # the moved stream's block lengths in its new place: other ones, all of 300 samples or more


def move_specs(channels, rule):
    """Source: three streams at 44.1 / 48 / 32 kHz with blocks of 300 / 512 / 300 samples.  Stream 0 -- the one that moves after CALLS calls --
    has, at the move: a speaker switch made one call earlier (a call of 300 samples at 44.1 kHz is 326 or 327 samples at 48 kHz: at most
    one model hop, so at least three of the four key/value blocks are still to come), and an output gain 40 dB away from its target for
    one call (2 dB/ms: 300 samples at 44.1 kHz move it 13.6 dB).  Its clocks by their own arithmetic (wrapn::to_inner / to_outer, wrapper_plan.h; 44.1 kHz
    is the low side of hi / lo = 160 / 147, so host -> 48 kHz interpolates; both clocks start at hi - 1 = 159): a call of n = 300 samples
    yields m = ((n + 1) x 160 - phase_up - 1) / 147 samples at 48 kHz, 326 or 327, and leaves phase_up = (phase_up + 147 m) mod 160; the way
    back takes (phase_down + 147 m) / 160 = 300 samples and leaves phase_down = (phase_down + 147 m) mod 160.  Over 22 calls that is 7183
    samples at 48 kHz = 14 whole FIFO blocks and a fill of 463 of 480, with both clocks at 60 -- off their start
    value.  The call right after the move is a silent block where the shell's rule is applied."""
    lens0 = (300,) * CALLS + tuple(AFTER[i % len(AFTER)] for i in range(CALLS))
    gain = (((CALLS - 1, "out_gain", -40.0),) if channels == 1 else ((2, "out_gain", -40.0), (CALLS - 1, "out_gain", 0.0)))
    s0 = Spec(44100.0, lens0, channels, rule, 5100, 1, 1, events=((CALLS - 1, "voice", 2),) + gain, silent=(CALLS,) if rule else ())
    s1 = Spec(48000.0, (512,) * (2 * CALLS), channels, rule, 5110, 2, 0)
    s2 = Spec(32000.0, (300,) * (2 * CALLS), channels, rule, 5120, 0, 2, events=((7, "voice", 1),))
    return s0, s1, s2


def dest_specs(channels, rule, before):
    """Destination: two streams at 96 / 48 kHz -- no 44.1 kHz class -- that have run `before` calls at the move (another number than the
    source: its step counter differs)."""
    d0 = Spec(96000.0, (600,) * before, channels, rule, 5200, 0, 0)
    d1 = Spec(48000.0, (480,) * (before + CALLS), channels, rule, 5210, 1, 1, events=((3, "voice", 0),))
    return d0, d1


@pytest.mark.parametrize("channels,rule", FORMS, ids=FORM_IDS)
def test_a_moved_stream_keeps_its_filter_histories_fifo_and_gain_ramp(bv, product, models, model_dir, shard, channels, rule):
    before = CALLS + 3
    results = {}
    for with_wrapper in (True, False):
        s0, s1, s2 = move_specs(channels, rule)
        d0, d1 = dest_specs(channels, rule, before)
        src, dst = start(bv, models, [s0, s1, s2]), start(bv, models, [d0, d1])
        try:
            fs, fd = [Feed(s0), Feed(s1), Feed(s2)], [Feed(d0), Feed(d1)]
            for _ in range(CALLS):
                call(bv, src, fs, channels, rule)
            for _ in range(before):
                call(bv, dst, fd, channels, rule)
            assert fd[0].done() and dst.stream_rate(0) == 96000.0 and src.step_counter() != dst.step_counter()
            if with_wrapper:
                blobs, wblobs = shard.move_streams(src, [0], dst, [0], with_wrapper=True)
                assert len(wblobs) == src.wrapper_blob_bytes() == dst.wrapper_blob_bytes() == BLOB
                _, _, size, _, rate, phase_down, phase_up, fill, _, in_t, in_now, out_t, out_now = header_of(wblobs)
                assert (size, rate, phase_down, phase_up, fill) == (BLOB, 44100.0, 60, 60, 463)   # (the arithmetic above)
                assert out_t == (-40.0 if channels == 1 else 0.0) and 5.0 < abs(out_now - out_t) < 35.0       # the ramp is in mid-flight
                assert src.export_stream_wrappers([0]) == wblobs                                             # the export changed nothing
                assert dst.stream_rate(0) == 44100.0 and dst.export_stream_wrappers([0]) == wblobs            # ... and all of it arrived
            else:
                blobs = shard.move_streams(src, [0], dst, [0])
                assert isinstance(blobs, bytes) and dst.stream_rate(0) == 96000.0
            assert dst.stream_rate(1) == 48000.0 and [src.stream_rate(s) for s in range(3)] == [44100.0, 48000.0, 32000.0]
            stayed = copy.deepcopy(fs[0])   # in the source the stream is still there: it goes on as if nothing had been asked
            fd[0] = fs[0]
            fs[0] = stayed
            for _ in range(CALLS):
                call(bv, dst, fd, channels, rule)
                call(bv, src, fs, channels, rule)
            results[with_wrapper] = (fs, fd)
        finally:
            src.close()
            dst.close()
    fs, fd = results[True]
    same(fd[0], model_dir, "the moved stream, all %d calls" % (2 * CALLS))
    same(fd[1], model_dir, "the destination's other stream")
    same(fs[0], model_dir, "the stream as it went on in the source")
    same(fs[1], model_dir, "source stream 1")
    same(fs[2], model_dir, "source stream 2")
    # the negative control: without the wrapper blob the stream arrives in a slot at 96 kHz with another stream's histories and FIFO
    fs, fd = results[False]
    want = proxy_run(model_dir, fd[0].spec)
    edge = CALLS * 300
    assert np.array_equal(fd[0].got[:, :edge], want[:, :edge]) and not np.array_equal(fd[0].got[:, edge:], want[:, edge:])
    same(fd[1], model_dir, "the destination's other stream (control)")


@pytest.mark.parametrize("channels,rule", FORMS, ids=FORM_IDS)
def test_two_streams_move_crosswise_in_one_call(bv, product, models, model_dir, shard, channels, rule):
    """Source streams 0 and 2 become destination streams 1 and 0: two blobs, two rates the destination lacks (44.1 and 32 kHz), both of the
    destination's own classes (96 and 48 kHz) left without a stream."""
    before = CALLS + 3
    s0, s1, s2 = move_specs(channels, rule)
    d0, d1 = dest_specs(channels, rule, before)
    d1 = Spec(d1.rate, d1.lens[:before], channels, rule, d1.seed, d1.voice, d1.vq, d1.events)
    src, dst = start(bv, models, [s0, s1, s2]), start(bv, models, [d0, d1])
    try:
        fs, fd = [Feed(s0), Feed(s1), Feed(s2)], [Feed(d0), Feed(d1)]
        for _ in range(CALLS):
            call(bv, src, fs, channels, rule)
        for _ in range(before):
            call(bv, dst, fd, channels, rule)
        blobs, wblobs = shard.move_streams(src, [0, 2], dst, [1, 0], with_wrapper=True)
        assert len(blobs) == 2 * src.stream_blob_bytes() and len(wblobs) == 2 * BLOB
        assert [dst.stream_rate(s) for s in range(2)] == [32000.0, 44100.0]
        gone = fd
        fd = [fs[2], fs[0]]
        fs = [None, fs[1], None]
        for _ in range(CALLS):
            call(bv, dst, fd, channels, rule)
            call(bv, src, fs, channels, rule)
    finally:
        src.close()
        dst.close()
    same(fd[1], model_dir, "source stream 0 -> destination stream 1")
    same(fd[0], model_dir, "source stream 2 -> destination stream 0")
    same(fs[1], model_dir, "the source's remaining stream")
    same(gone[0], model_dir, "destination stream 0 until it left")
    same(gone[1], model_dir, "destination stream 1 until it left")


# ---- 2. one stream changes its rate -----------------------------------------------------------------------------------------------------------
def test_one_stream_changes_its_rate_twice_and_the_others_do_not_notice(bv, product, models, model_dir):
    """Classes at the start: 96, 48, 32 kHz.  Stream 1 goes 48 -> 44.1 kHz: a new class, the 48 kHz class is dropped and the 32 kHz class,
    made after it, moves up with its tap offsets while stream 2 is on it.  An equal-rate call is nothing.  Then 44.1 -> 32 kHz: an
    existing class, the 44.1 kHz class is dropped."""
    channels, rule = 1, False
    s0 = Spec(96000.0, (600,) * (3 * CALLS), channels, rule, 5300, 0, 1)
    s1 = Spec(48000.0, (512,) * CALLS + (441,) * CALLS + (320,) * CALLS, channels, rule, 5310, 1, 0,
              events=((9, "out_gain", -12.0), (CALLS, "rate", 44100.0), (CALLS + 5, "rate", 44100.0), (2 * CALLS - 1, "out_gain", 6.0), (2 * CALLS, "rate", 32000.0)))
    s2 = Spec(32000.0, (300,) * (3 * CALLS), channels, rule, 5320, 2, 2, events=((30, "voice", 0),))
    batch = start(bv, models, [s0, s1, s2])
    try:
        feeds = [Feed(s0), Feed(s1), Feed(s2)]
        rates = []
        for k in range(3 * CALLS):
            call(bv, batch, feeds, channels, rule)
            rates.append([batch.stream_rate(s) for s in range(3)])
        assert rates[CALLS - 1] == [96000.0, 48000.0, 32000.0] and rates[CALLS] == [96000.0, 44100.0, 32000.0] and rates[-1] == [96000.0, 32000.0, 32000.0]
    finally:
        batch.close()
    for s, f in enumerate(feeds):
        same(f, model_dir, "stream %d" % s)


# ---- 3. restart, and a slot turned over to a new caller ------------------------------------------------------------------------------------------
def test_a_wrapper_restart_and_a_slot_turned_over(bv, product, models, model_dir):
    """Stream 0: BeatriceBatch_RestartStreamWrapper (the proxy: SetSampleRate(48 kHz), SetSampleRate(44.1 kHz)) with an output gain ramp
    in flight, which goes on.  Stream 2: the slot goes to a new caller -- restart + BeatriceBatch_ResetStream (the proxy: + ResetContext).
    Stream 1 is between them and is not touched."""
    channels, rule = 2, True
    s0 = Spec(44100.0, (300,) * (2 * CALLS), channels, rule, 5400, 1, 1, events=((CALLS - 1, "out_gain", -40.0), (CALLS, "restart", 48000.0)), silent=(CALLS + 1,))
    s1 = Spec(48000.0, (512,) * (2 * CALLS), channels, rule, 5410, 2, 0, events=((CALLS, "voice", 0),))
    s2 = Spec(32000.0, (330,) * (2 * CALLS), channels, rule, 5420, 0, 2, events=((CALLS - 1, "voice", 2), (CALLS, "restart", 48000.0), (CALLS, "reset", None)))
    batch = start(bv, models, [s0, s1, s2])
    try:
        feeds = [Feed(s0), Feed(s1), Feed(s2)]
        for k in range(2 * CALLS):
            call(bv, batch, feeds, channels, rule)
        assert [batch.stream_rate(s) for s in range(3)] == [44100.0, 48000.0, 32000.0]
    finally:
        batch.close()
    for s, f in enumerate(feeds):
        same(f, model_dir, "stream %d" % s)


# ---- 4. refusals change nothing ------------------------------------------------------------------------------------------------------------------
def fnv1a(data):
    h = 1469598103934665603
    for byte in data:
        h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def resealed(blob, **fields):
    """the blob with header fields replaced and a check word that fits: only the batch's own rules can refuse it"""
    names = ("magic", "version", "size", "check", "rate", "phase_down", "phase_up", "fill", "reserved", "in_target", "in_now", "out_target", "out_now")
    h = dict(zip(names, header_of(blob)))
    h.update(fields)
    h["check"] = 0
    body = blob[80:]
    h["check"] = fnv1a(struct.pack(HEADER, *[h[n] for n in names]) + body)
    return struct.pack(HEADER, *[h[n] for n in names]) + body


def new_calls_refused(bv, batch, good):
    """every one of the six new calls, with arguments that are fine where the calls work"""
    a, h = batch.a, batch.h
    one = bv.iptr(np.zeros(1, np.int32))
    out = C.create_string_buffer(BLOB)
    return [a.BeatriceBatch_SetStreamRate(h, 0, 44100.0), a.BeatriceBatch_SetStreamRate(h, 0, 22050.0), a.BeatriceBatch_RestartStreamWrapper(h, 0),
            a.BeatriceBatch_StreamRate(h, 0), a.BeatriceBatch_WrapperBlobBytes(h), a.BeatriceBatch_ExportStreamWrappers(h, 1, one, C.cast(out, C.c_void_p)),
            a.BeatriceBatch_ImportStreamWrappers(h, 1, one, C.cast(C.create_string_buffer(good, BLOB), C.c_void_p))] == [-1, -1, -1, 0.0, 0, -1, -1]


@pytest.fixture(scope="module")
def good_blob(bv, models):
    """a wrapper blob of a 44.1 kHz stream some calls into its life (hi = 160; its FIFO, histories and clocks are not those of a fresh stream)"""
    sp = Spec(44100.0, (300,) * 5, 1, False, 5500, 1, 0, events=((4, "out_gain", -20.0),))
    batch = start(bv, models, [sp])
    try:
        feeds = [Feed(sp)]
        for _ in range(5):
            call(bv, batch, feeds, 1, False)
        blob = batch.export_stream_wrappers([0])
    finally:
        batch.close()
    assert len(blob) == BLOB and header_of(blob)[4] == 44100.0 and any(blob[80:])
    return blob


@pytest.mark.parametrize("mode", ["in_order", "uniform_wrapper", "resident_blocks_per_stream_clocks", "tick"])
def test_the_new_calls_are_refused_outside_their_mode(bv, product, model_dir, good_blob, mode):
    """Before BeatriceBatch_ConfigureWrapperRates, under the uniform BeatriceBatch_ConfigureWrapper, after BeatriceBatch_BindResidentBlocksRagged
    and in tick mode: -1 (0.0, 0), and the batch goes on to the bit like one that never asked."""
    import test_gpu_mode_matrix as mm
    product = bv.bind_batch(product)
    H, B, steps = 1, mm.B, 10
    x16 = np.stack([bv.synth_audio(160 * steps, seed=8800 + s) for s in range(B)]).reshape(B, steps, 160)
    x48 = np.stack([wrapperlib.test_signal(480 * steps * mm.CH, 48000, seed=8900 + s) for s in range(B)]).astype(np.float32).reshape(B, steps, H, mm.CH, 480)
    results = []
    for tries in (True, False):
        c = mm.Ctx(bv, product, model_dir, H)
        try:
            if mode == "uniform_wrapper":
                assert c.a.BeatriceBatch_ConfigureWrapper(c.h, 44100.0) == 0
            else:
                mm.enter(c, mode)
            got = []
            for k in range(steps):
                if tries and k in (1, 4):
                    assert new_calls_refused(bv, c.batch, good_blob), (mode, k)
                if mode == "uniform_wrapper":
                    xin = np.ascontiguousarray(x48[:, k, 0, :, :441])
                    y = np.zeros_like(xin)
                    assert c.a.BeatriceBatch_ProcessBlocks(c.h, bv.fptr(xin), bv.fptr(y), mm.CH, 441) == 0
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


def test_refused_arguments_and_blobs_change_nothing(bv, product, models, good_blob):
    channels, rule, B, calls = 1, False, 3, 30
    specs = [Spec(44100.0, (300,) * calls, channels, rule, 5600, 1, 1, events=((3, "out_gain", -30.0), (16, "out_gain", 0.0))),
             Spec(48000.0, (512,) * calls, channels, rule, 5610, 2, 0),
             Spec(96000.0, (600,) * calls, channels, rule, 5620, 0, 2)]
    i32 = lambda v: bv.iptr(np.ascontiguousarray(v, np.int32))   # noqa: E731
    vp = lambda b: C.cast(C.create_string_buffer(bytes(b), len(b)), C.c_void_p)   # noqa: E731
    nan = float("nan")
    h_names = {"magic": 0, "version": 4, "size": 8, "check": 16, "rate": 24 + 6, "phase_down": 32, "phase_up": 36, "fill": 40, "reserved": 44,
               "in_target": 48 + 6, "in_now": 56 + 6, "out_target": 64 + 6, "out_now": 72 + 6, "state": 80 + 1000, "last byte": BLOB - 1}

    def damaged(off):
        b = bytearray(good_blob)
        b[off] ^= 0x04
        return bytes(b)

    ran = []

    def asks(batch):
        a, h = batch.a, batch.h
        out = C.create_string_buffer(4 * BLOB)
        ex = lambda n, st, dst=out: a.BeatriceBatch_ExportStreamWrappers(h, n, st, C.cast(dst, C.c_void_p) if dst is not None else None)   # noqa: E731
        im = lambda n, st, blob=good_blob * 4: a.BeatriceBatch_ImportStreamWrappers(h, n, st, vp(blob) if blob is not None else None)   # noqa: E731
        for fn in (ex, im):   # bad counts, NULL, bad and duplicate streams
            assert fn(0, i32([0])) == -1 and fn(-1, i32([0])) == -1 and fn(B + 1, i32([0, 1, 2, 0])) == -1
            assert fn(1, None) == -1
            assert fn(1, i32([B])) == -1 and fn(1, i32([-1])) == -1 and fn(2, i32([1, 1])) == -1
        assert ex(1, i32([0]), None) == -1 and im(1, i32([0]), None) == -1
        for s in (-1, B, 1 << 20):
            assert a.BeatriceBatch_SetStreamRate(h, s, 44100.0) == -1 and a.BeatriceBatch_RestartStreamWrapper(h, s) == -1
            assert a.BeatriceBatch_StreamRate(h, s) == 0.0
        for rate in (0.0, nan, 1e9, -44100.0, float("inf")):   # what RateClass::configure refuses
            assert a.BeatriceBatch_SetStreamRate(h, 1, rate) == -1, rate
        for name, off in h_names.items():   # every header field altered (and the state): the format's own checks
            assert im(1, i32([1]), damaged(off)) == -1, name
        assert im(1, i32([1]), good_blob[:BLOB - 16] + bytes(16)) == -1
        for rate in (0.0, nan, 1e9):   # a check word that fits: the batch's rules
            assert im(1, i32([1]), resealed(good_blob, rate=rate)) == -1, rate
        assert im(1, i32([1]), resealed(good_blob, phase_down=160)) == -1 and im(1, i32([1]), resealed(good_blob, phase_up=160)) == -1   # phase = hi
        assert im(1, i32([1]), resealed(good_blob, phase_down=-1)) == -1
        assert im(1, i32([1]), resealed(good_blob, rate=48000.0)) == -1    # the blob's clocks are out of range for hi = 1
        assert im(1, i32([1]), resealed(good_blob, fill=480)) == -1 and im(1, i32([1]), resealed(good_blob, fill=-1)) == -1
        for field in ("in_target", "in_now", "out_target", "out_now"):
            assert im(1, i32([1]), resealed(good_blob, **{field: nan})) == -1, field
        assert im(2, i32([1, 2]), good_blob + damaged(0)) == -1             # a good blob beside a bad one: nothing of the good one lands
        assert im(2, i32([2, 1]), resealed(good_blob, fill=480) + good_blob) == -1
        assert [a.BeatriceBatch_StreamRate(h, s) for s in range(B)] == [44100.0, 48000.0, 96000.0] and a.BeatriceBatch_WrapperBlobBytes(h) == BLOB
        ran.append(1)

    def lands(batch):   # not vacuous: the good blob itself is taken, and is audible in these blocks
        batch.import_stream_wrappers([1], resealed(good_blob))
        assert batch.stream_rate(1) == 44100.0

    got = {}
    for name, change in (("asked", asks), ("never", None), ("landed", lands)):
        batch = start(bv, models, specs)
        try:
            feeds = [Feed(sp) for sp in specs]
            for k in range(calls):
                if change is not None and k in (4, 17):
                    change(batch)
                call(bv, batch, feeds, channels, rule)
            got[name] = np.concatenate([f.got.reshape(-1) for f in feeds])
        finally:
            batch.close()
    assert len(ran) == 2 and np.abs(got["never"]).max() > 1e-3
    assert np.array_equal(got["asked"], got["never"])
    assert not np.array_equal(got["landed"], got["never"])
