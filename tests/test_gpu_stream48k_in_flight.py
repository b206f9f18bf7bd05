"""Mode F (BeatriceBatch_BindResidentIO48k: resident 48 kHz blocks with the tick pipeline between them) without drains:
BeatriceBatch_ResetStreamInFlight travels through the ticks AND through the two halves of the 48 kHz wrapper, and
BeatriceBatch_Stream48kQuiescent / ExportStreams48kInFlight / ImportStreams48kInFlight / MoveStreams48kInFlight move a stream at rest
between two batches that both go on converting blocks.

Yardsticks.  A product TWIN at np.array_equal: the same script with the drained BeatriceBatch_ResetStream, or a batch in which nothing was
asked or moved.  The ORACLE leg: tests/test_gpu_wrapper48k.py's oracle_leg_48k (the ref-pinned host wrapper around an independent oracle
stream; a reset is a new wrapper around a new stream) at the project's bound 1e-4, printed.  For a stream that sits steps out or changes
batches the oracle leg is run on the stream's PRESENT blocks in order, as a batch of one: the shell does not call the core for a block
that sits out, and which batch made a block is nothing the oracle knows about.

The driver (Line) runs S + 14 steps (S = BeatriceBatch_TickStages) on S + 4 slots, so the slot ring wraps; it never calls
BeatriceBatch_Synchronize before the end (that drains): a block about to be overwritten is read back behind a plain device
synchronisation, which waits and changes nothing.  Every step fed asserts BeatriceBatch_TicksLaunched == steps fed."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_mode_matrix as mode_matrix
import wrapperlib
from test_gpu_stream_migration import _free_bytes, models  # noqa: F401
from test_gpu_wrapper48k import oracle_leg_48k
from tick_driver import Hip

pytestmark = pytest.mark.gpu

BOUND = 1e-4
_sig = {}


def i32(v):
    return np.ascontiguousarray(v, np.int32).ctypes.data_as(C.POINTER(C.c_int))


def signal(seed, H):
    """one stream's mono 48 kHz material, [60][H][480]"""
    if (seed, H) not in _sig:
        _sig[(seed, H)] = wrapperlib.test_signal(480 * H * 60, 48000, seed=seed).astype(np.float32).reshape(60, H, 480)
    return _sig[(seed, H)]


class Line:
    """One batch bound to resident 48 kHz blocks, n steps planned in advance.  Stream s consumes its current source (seed, next index) at
    every step it takes part in; with two channels the second carries another signal (distinct=True) or the same one, whose down-mix
    (m + m) * 0.5 is m exactly.  events[k]: callables run before step k is fed; scripts[s](line, s, i) runs before the stream's i-th
    present step."""

    def __init__(self, bv, models, B, H, channels, seeds, n=None, rule=False, distinct=False, drains=False, start_counter=None, stream=None):
        self.bv, self.B, self.H, self.ch, self.rule, self.distinct, self.drains = bv, B, H, channels, rule, distinct, drains
        self.batch = bv.Batch(models, B, hops_per_step=H, start_counter=start_counter)
        self.a, self.h = self.batch.a, self.batch.h
        self.hip = Hip()
        self.S = self.a.BeatriceBatch_TickStages(self.h)
        self.n = self.S + 14 if n is None else n
        self.slots = self.S + 4
        self.out = np.zeros((self.n, B), np.uint8)
        self.sources = {s: [(0, seeds[s], 0)] for s in range(B)}
        self.events, self.scripts = {}, {}
        self.fed = self.base = 0
        self.d_in = self.d_out = None
        self.made_stream = stream
        for s in range(B):   # the settings of every test here: three voices, one k-NN stream
            assert self.a.BeatriceBatch_SetTargetSpeaker(self.h, s, s % 3) == 0
        assert self.a.BeatriceBatch_SetVQNumNeighbors(self.h, B - 1, 2) == 0
        assert self.a.BeatriceBatch_FlushSpeaker(self.h, -1) == 0

    def sit_out(self, s, k0, k1):
        self.out[k0:k1, s] = 1

    def feed_from(self, s, k, seed, idx):
        self.sources[s].append((k, seed, idx))

    def at(self, k, fn):
        self.events.setdefault(k, []).append(fn)

    def start(self):
        B, H, ch = self.B, self.H, self.ch
        self.x = np.zeros((self.n, B, H, ch, 480), np.float32)
        self.took = {s: [] for s in range(B)}   # (step, seed, index) of every present step
        for s in range(B):
            seg = sorted(self.sources[s])
            seed = idx = None
            for k in range(self.n):
                while seg and seg[0][0] <= k:
                    _, seed, idx = seg.pop(0)
                if not self.out[k, s]:
                    self.x[k, s, :, 0] = signal(seed, H)[idx]
                    if ch == 2:
                        self.x[k, s, :, 1] = signal(seed + 5000 if self.distinct else seed, H)[idx]
                    self.took[s].append((k, seed, idx))
                    idx += 1
        self.idx_at = {(k, s): i for s in self.took for i, (k, _, _) in enumerate(self.took[s])}
        self.blk = B * H * ch * 480 * 4
        self.d_in, self.d_out = self.hip.malloc(self.slots * self.blk), self.hip.malloc(self.slots * self.blk)
        assert self.hip.lib.hipMemset(self.d_out, 0, C.c_size_t(self.slots * self.blk)) == 0
        if self.made_stream is not None:
            assert self.a.BeatriceBatch_SetStream(self.h, self.made_stream) == 0
        assert self.a.BeatriceBatch_BindResidentIO48k(self.h, self.d_in, self.d_out, ch, self.slots) == 0
        if self.rule:
            assert self.a.BeatriceBatch_EnableSilentBlockRule(self.h, 1) == 0
        self.y = np.zeros((self.n, B, H, ch, 480), np.float32)
        self.have = np.zeros(self.n, bool)
        return self

    def ticks(self):
        return self.a.BeatriceBatch_TicksLaunched(self.h)

    def _slot(self, k):
        return (k - self.base) % self.slots

    def _collect(self, ks):
        """blocks that have landed: read back behind a device synchronisation (no call of the batch: nothing drains)"""
        assert self.hip.lib.hipDeviceSynchronize() == 0
        for k in ks:
            if not self.have[k]:
                self.hip.d2h(self.y[k], C.c_void_p(self.d_out.value + self._slot(k) * self.blk))
                self.have[k] = True

    def run_to(self, k_end):
        a, h = self.a, self.h
        for k in range(self.fed, k_end):
            for fn in self.events.get(k, ()):   # (first: a re-bind among them restarts the slot count)
                fn(self)
            for s, script in self.scripts.items():
                if (k, s) in self.idx_at:
                    script(self, s, self.idx_at[(k, s)])
            if k - self.base >= self.slots:   # the slot's earlier block landed S + 1 <= slots calls after it was fed
                self._collect([k - self.slots])
            self.hip.h2d(C.c_void_p(self.d_in.value + self._slot(k) * self.blk), self.x[k])
            if self.out[k].any():
                assert a.BeatriceBatch_SetSilentStreams(h, self.out[k].tobytes()) == 0
            assert a.BeatriceBatch_ConvertBlocks48kDevice(h, None, None, self.ch) == 0
            self.fed += 1
            if not self.drains:
                assert self.ticks() == self.fed - self.base, "step %d: %d ticks for %d steps fed" % (k, self.ticks(), self.fed - self.base)
        return self

    def synchronize(self):
        """BeatriceBatch_Synchronize in the middle of a run (a drain: the twin makes the same call)"""
        assert self.a.BeatriceBatch_Synchronize(self.h) == 0
        self._collect(range(max(self.base, self.fed - self.slots), self.fed))

    def rebind(self, unbind_first):
        """leaves F (NULL, NULL) and binds again, or binds again straight away: either way the batch leaves the mode drained, and the
        new binding counts its slots from 0"""
        a, h = self.a, self.h
        if unbind_first:
            assert a.BeatriceBatch_BindResidentIO48k(h, None, None, 0, 0) == 0
            self._collect(range(max(self.base, self.fed - self.slots), self.fed))
            assert a.BeatriceBatch_BindResidentIO48k(h, self.d_in, self.d_out, self.ch, self.slots) == 0
        else:   # (the blocks the re-bind flushes land in the buffers both bindings share)
            assert a.BeatriceBatch_BindResidentIO48k(h, self.d_in, self.d_out, self.ch, self.slots) == 0
            self._collect(range(max(self.base, self.fed - self.slots), self.fed))
        if self.rule:
            assert a.BeatriceBatch_EnableSilentBlockRule(h, 1) == 0
        self.base = self.fed

    def finish(self):
        self.run_to(self.n)
        self.ticks_before_sync = self.ticks()
        assert self.a.BeatriceBatch_Synchronize(self.h) == 0
        self._collect(range(self.n))
        return self

    def heard(self, s, seed):
        """(indices into the seed's material, blocks [..][H][ch][480]) of the steps stream s made on it"""
        rows = [(k, i) for (k, sd, i) in self.took[s] if sd == seed]
        return [i for _, i in rows], self.y[[k for k, _ in rows], s]

    def quiescent(self, s):
        return self.a.BeatriceBatch_Stream48kQuiescent(self.h, s)

    def state(self):
        return (self.ticks(), self.a.BeatriceBatch_StepCounter(self.h), tuple(self.quiescent(s) for s in range(self.B)))

    def close(self):
        self.batch.close()
        for p in (self.d_in, self.d_out):
            if p is not None:
                self.hip.free(p)


def reset(how, s):
    """an event for Line.at: stream s (-1: all) starts over -- in flight, drained, or not at all"""
    def event(ln):
        if how != "never":
            assert (ln.a.BeatriceBatch_ResetStreamInFlight if how == "inflight" else ln.a.BeatriceBatch_ResetStream)(ln.h, s) == 0
    return event


def oracle_blocks(bv, oracle, model_dir, channels, H, x, got, speaker, vq_k, change_step=None):
    """oracle_leg_48k on ONE stream's present blocks in order: x, got [steps][H][ch][480]; change_step(script, i) before its i-th step"""
    steps = len(x)
    xs = np.ascontiguousarray(x.transpose(2, 0, 1, 3).reshape(channels, steps * H * 480))[None]   # [1][ch][blocks * 480]
    blocks = [got[kb // H, kb % H][None] for kb in range(steps * H)]

    def settings(ob):
        ob.a.BeatriceBatch_SetTargetSpeaker(ob.h, 0, speaker)
        ob.a.BeatriceBatch_SetVQNumNeighbors(ob.h, 0, vq_k)
        ob.a.BeatriceBatch_FlushSpeaker(ob.h, 0)

    def change_block(script, kb):
        if change_step is not None and kb % H == 0:
            change_step(script, kb // H)
    _, dev = oracle_leg_48k(bv, oracle, model_dir, 1, channels, xs, steps * H, settings, change_block, blocks, n_pick=1)
    return dev


def differing(p, q):
    return [(k, s) for k in range(len(p)) for s in range(p.shape[1]) if not np.array_equal(p[k, s], q[k, s])]


# ---- 1. reset in flight ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels,H", [(1, 1), (2, 1), (1, 2), (2, 2), (1, 4), (2, 4)])
def test_reset_in_flight_equals_the_drained_twin_and_the_oracle(bv, oracle, product, models, model_dir, channels, H):
    """One stream at steps 6 and S + 3, all streams at step 20: nothing drains, the blocks equal the drained twin's bit for bit and the
    oracle's new streams behind new wrappers, and the blocks still owed at a reset are those of a twin that was never reset."""
    B = 5
    runs = {}
    for how in ("inflight", "drained", "never"):
        ln = Line(bv, models, B, H, channels, [700 + s for s in range(B)], distinct=True, drains=how == "drained")
        try:
            S = ln.S
            ln.at(6, reset(how, 1))
            ln.at(S + 3, reset(how, 3))
            ln.at(20, reset(how, -1))
            ln.start().finish()
            runs[how] = (ln.y.copy(), ln.ticks_before_sync, ln.x.copy(), S)
        finally:
            ln.close()
    y, ticks, x, S = runs["inflight"]
    assert ticks == S + 14                       # one tick per step fed: no reset drained (every reset drains on the parent commit)
    assert runs["drained"][1] > S + 14           # (the twin's did)
    assert np.abs(runs["drained"][0]).max() > 1e-3
    assert differing(y, runs["drained"][0]) == []
    never = runs["never"][0]
    assert all(np.array_equal(y[k, 1], never[k, 1]) for k in range(6))                                   # owed at the reset of step 6: all of them
    assert all(np.array_equal(y[k, s], never[k, s]) for k in range(20) for s in (0, 2, 3, 4))            # owed at step 20: blocks 20 - S .. 19
    assert not np.array_equal(y[6, 1], never[6, 1]) and not np.array_equal(y[20, 0], never[20, 0])       # (and the resets are not no-ops)
    assert not np.array_equal(y[S + 3, 3], never[S + 3, 3])

    def change_block(script, kb):   # (stream = -1 one stream at a time: the leg's wrappers restart with the stream named)
        if kb % H:
            return
        k = kb // H
        for s in ([1] if k == 6 else [3] if k == S + 3 else list(range(B)) if k == 20 else []):
            assert script.a.BeatriceBatch_ResetStream(script.h, s) == 0

    def settings(ob):
        for s in range(B):
            ob.a.BeatriceBatch_SetTargetSpeaker(ob.h, s, s % 3)
        ob.a.BeatriceBatch_SetVQNumNeighbors(ob.h, B - 1, 2)
        ob.a.BeatriceBatch_FlushSpeaker(ob.h, -1)
    n = len(y)
    xs = np.ascontiguousarray(x.transpose(1, 3, 0, 2, 4).reshape(B, channels, n * H * 480))
    got = [y[kb // H, :, kb % H] for kb in range(n * H)]
    sample, dev = oracle_leg_48k(bv, oracle, model_dir, B, channels, xs, n * H, settings, change_block, got)
    print("reset in flight around the 48 kHz wrapper, %d channel(s), H = %d: streams %s vs the oracle max-abs %g" % (channels, H, sample, dev))
    assert dev <= BOUND


# ---- 2. a reset of a stream that sits the step out ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [1, 2])
def test_reset_of_a_stream_that_sits_out_applies_at_its_next_present_step(bv, product, models, H):
    """Rule on, stream 2 flagged at steps 8 .. 10 and reset asked before step 8: it applies at step 11.  The twin calls the drained
    reset right before step 11."""
    B, r = 5, 8
    runs = {}
    for how in ("inflight", "drained"):
        ln = Line(bv, models, B, H, 2, [720 + s for s in range(B)], rule=True, distinct=True, drains=how == "drained")
        try:
            ln.sit_out(2, r, r + 3)
            ln.sit_out(4, 15, 17)
            ln.at(r if how == "inflight" else r + 3, reset(how, 2))
            ln.start().finish()
            runs[how] = (ln.y.copy(), ln.ticks_before_sync, ln.S)
        finally:
            ln.close()
    y, ticks, S = runs["inflight"]
    assert ticks == S + 14 and runs["drained"][1] > S + 14
    assert np.abs(y).max() > 1e-3 and not y[r:r + 3, 2].any()   # (a block that sits out comes back as its own zero down-mix)
    assert differing(y, runs["drained"][0]) == []


# ---- 3. Synchronize, unbind and re-bind in the middle of a travelling reset -------------------------------------------------------------------
@pytest.mark.parametrize("what,after", [("synchronize", 5), ("synchronize", 1), ("unbind", 5), ("unbind", 1), ("rebind", 5), ("rebind", 1),
                                        ("unbind", 0), ("rebind", 0)])
def test_a_drain_in_the_middle_of_a_travelling_reset_carries_it_to_the_end(bv, product, models, what, after):
    """Stream 1 is reset at step 10; `after` steps later the batch is drained by BeatriceBatch_Synchronize, by leaving F or by a re-bind.
    after = 5: the reset's step is still inside the ticks.  after = 1: it is the last step fed, so its output half IS the flush launch.
    after = 0: the reset has been asked and no step has taken it -- leaving the mode applies it, wrapper state included."""
    B, H, r = 5, 2, 10
    runs = {}
    for how in ("inflight", "drained"):
        ln = Line(bv, models, B, H, 1, [740 + s for s in range(B)], drains=True)
        try:
            ln.at(r, reset(how, 1))
            if after == 0:   # (events of a step run in the order given: the reset first)
                ln.at(r, lambda ln: ln.rebind(what == "unbind"))
            else:
                ln.at(r + after, (lambda ln: ln.synchronize()) if what == "synchronize" else (lambda ln: ln.rebind(what == "unbind")))
            ln.start().finish()
            runs[how] = ln.y.copy()
        finally:
            ln.close()
    assert np.abs(runs["drained"]).max() > 1e-3
    assert differing(runs["inflight"], runs["drained"]) == []


# ---- 4 .. 6. the move ----------------------------------------------------------------------------------------------------------------------
N1, FIRST, D = 7, 5, 2   # the stream's steps in the source; the destination slot's own steps before it falls silent; its extra silent steps
SHIFT = 1013             # destination stream's own counter - source stream's: a prime above every ring's slot count


class Pair:
    """Source: mono, 3 streams, stream 1 makes N1 steps (a speaker switch before the last one, so key/value blocks are still to come), then
    sits out.  Destination: stereo, 3 streams, slot 0 makes FIRST steps of its own and sits out; at the move (source: S steps after the
    stream's last, destination: S + D steps after the slot's last) it takes the stream in and makes the stream's next steps."""

    def __init__(self, bv, models, H, moves=True, stream=None, turn_over=False):
        self.src = Line(bv, models, 3, H, 1, [800, 801, 802], rule=True, stream=stream)
        S = self.src.S
        self.dst = Line(bv, models, 3, H, 2, [810, 811, 812], rule=True, stream=stream, start_counter=SHIFT + N1 - FIRST)
        self.S, self.H, self.at_src, self.at_dst = S, H, N1 + S, FIRST + S + D
        self.n2 = self.dst.n - self.at_dst
        self.src.sit_out(1, N1, self.at_src if turn_over else self.src.n)
        if turn_over:
            self.src.feed_from(1, self.at_src, 820, 0)
        self.dst.sit_out(0, FIRST, self.at_dst)
        if moves:
            self.dst.feed_from(0, self.at_dst, 801, N1)
        self.src.scripts[1] = switch_voice

    def start(self):
        self.src.start()
        self.dst.start()
        return self

    def close(self):
        self.src.close()
        self.dst.close()


def switch_voice(ln, s, i):
    if i == N1 - 1:
        assert ln.a.BeatriceBatch_SetTargetSpeaker(ln.h, s, 2) == 0


def carry(how, src, dst, frm, to):
    before = (src.state(), dst.ticks(), dst.a.BeatriceBatch_StepCounter(dst.h))
    if how == "blobs":
        blobs = src.batch.export_streams48k_in_flight(frm)
        assert before[0] == src.state()
        dst.batch.import_streams48k_in_flight(to, blobs)
    else:
        src.batch.move_streams48k_in_flight(dst.batch, frm, to)
    assert before == (src.state(), dst.ticks(), dst.a.BeatriceBatch_StepCounter(dst.h))   # no tick, no clock: nothing drained


_twins = {}


def twins(bv, models, H):
    """the runs in which nothing moves, once per H: the source line (its stream 1 simply goes on after the same silence, on the
    material the destination will feed it) and the destination line (its slot 0 stays silent)"""
    if H not in _twins:
        p = Pair(bv, models, H, moves=False)
        try:
            p.src.out[p.at_src:, 1] = 0
            p.start()
            p.src.finish()
            p.dst.sit_out(0, p.at_dst, p.dst.n)
            p.dst.start().finish()
            _twins[H] = (p.src.y.copy(), p.dst.y.copy(), p.src.x.copy())
        finally:
            p.close()
    return _twins[H]


@pytest.mark.parametrize("H", [1, 4])
def test_the_boundary_is_one_launch_behind_the_last_stage(bv, product, models, H):
    """The stream's last present step fed at tick T: after `stages` ticks, T included, it is at rest in the ticks and NOT around the
    wrapper -- Stream48kQuiescent 0 and -3 from all three calls, as source and as destination, nothing changed; one call later 1, and
    the move goes through.  A slot that never took part is at rest from the first call on."""
    src_y, dst_y, _ = twins(bv, models, H)
    p = Pair(bv, models, H)
    try:
        src, dst, S = p.src, p.dst, p.S
        dst.sit_out(2, 0, dst.n)   # never takes part
        p.start()
        src.run_to(p.at_src - 1)   # ticks - T = S
        dst.run_to(FIRST + S - 1)  # the same for the destination's slot 0
        assert src.quiescent(1) == 0 and dst.quiescent(0) == 0 and dst.quiescent(2) == 1 and src.quiescent(0) == 0
        size = src.batch.stream_blob_bytes()
        buf = C.create_string_buffer(size)
        good = dst.batch.export_streams48k_in_flight([2])
        before = (src.state(), dst.state())
        a = src.a
        rcs = [a.BeatriceBatch_ExportStreams48kInFlight(src.h, 1, i32([1]), C.cast(buf, C.c_void_p)),
               a.BeatriceBatch_ImportStreams48kInFlight(dst.h, 1, i32([0]), C.cast(C.create_string_buffer(good, size), C.c_void_p), None, 0),
               a.BeatriceBatch_MoveStreams48kInFlight(src.h, dst.h, 1, i32([1]), i32([2]), None, 0),    # busy source
               a.BeatriceBatch_MoveStreams48kInFlight(dst.h, src.h, 1, i32([2]), i32([1]), None, 0),    # busy destination
               a.BeatriceBatch_MoveStreams48kInFlight(dst.h, src.h, 2, i32([2, 0]), i32([1, 0]), None, 0)]
        assert rcs == [-3] * 5, rcs
        assert before == (src.state(), dst.state())
        src.run_to(p.at_src)
        assert src.quiescent(1) == 1
        dst.run_to(FIRST + S)
        assert dst.quiescent(0) == 1
        dst.run_to(p.at_dst)
        carry("move", src, dst, [1], [0])
        src.finish()
        dst.finish()
        assert src.ticks_before_sync == src.n and dst.ticks_before_sync == dst.n
        assert np.abs(src.y).max() > 1e-3
        # the source, asked and read, equals the twin that never was (its stream 1 up to the twin's resumption)
        assert all(np.array_equal(src.y[k, s], src_y[k, s]) for k in range(src.n) for s in (0, 2))
        assert all(np.array_equal(src.y[k, 1], src_y[k, 1]) for k in range(p.at_src))
        assert all(np.array_equal(dst.y[k, 1], dst_y[k, 1]) for k in range(dst.n))
        _, moved = dst.heard(0, 801)
        for c in range(2):
            assert np.array_equal(moved[:, :, c], src_y[p.at_src:p.at_src + p.n2, 1, :, 0])
    finally:
        p.close()


@pytest.mark.parametrize("H,how,one_stream", [(1, "blobs", False), (1, "move", False), (1, "blobs", True), (1, "move", True),
                                              (4, "blobs", False), (4, "move", False), (4, "move", True)])
def test_a_moved_stream_goes_on_as_if_it_had_never_moved(bv, oracle, product, models, model_dir, H, how, one_stream):
    """By the blob pair and device to device, each batch on its own stream or both on one the caller made; mono source binding, stereo
    destination binding; the destination stream's own counter SHIFT ahead of the source stream's; a speaker switch right before the
    stream's last step in the source, so key/value blocks are still to come.  The stream's blocks in the destination -- the first one is
    the model output that travelled in the wrapper's FIFO -- equal the twin stream's that never moved and the oracle's; everybody else
    equals the twins that saw no move."""
    src_y, dst_y, src_x = twins(bv, models, H)
    hip, made = C.CDLL("libamdhip64.so"), C.c_void_p()
    if one_stream:
        assert hip.hipStreamCreateWithFlags(C.byref(made), 1) == 0
    p = Pair(bv, models, H, stream=made if one_stream else None)
    try:
        src, dst = p.src, p.dst
        p.start()
        src.run_to(p.at_src)
        dst.run_to(p.at_dst)
        assert src.quiescent(1) == 1 and dst.quiescent(0) == 1
        assert (src.a.BeatriceBatch_StepCounter(src.h) - (p.at_src - N1)) + SHIFT == dst.a.BeatriceBatch_StepCounter(dst.h) - (p.at_dst - FIRST)
        carry(how, src, dst, [1], [0])
        src.finish()
        dst.finish()
        assert src.ticks_before_sync == src.n and dst.ticks_before_sync == dst.n
        idx, moved = dst.heard(0, 801)
        assert idx == list(range(N1, N1 + p.n2)) and np.abs(moved).max() > 1e-3
        for c in range(2):   # the twin stream that never moved: bit for bit, on both channels
            bad = [i for i in range(p.n2) if not np.array_equal(moved[i, :, c], src_y[p.at_src + i, 1, :, 0])]
            assert not bad, "the moved stream's steps %s differ from the twin's" % bad
        assert all(np.array_equal(src.y[k, s], src_y[k, s]) for k in range(src.n) for s in (0, 2))
        assert all(np.array_equal(src.y[k, 1], src_y[k, 1]) for k in range(p.at_src))
        assert all(np.array_equal(dst.y[k, s], dst_y[k, s]) for k in range(dst.n) for s in (1, 2))
        assert all(np.array_equal(dst.y[k, 0], dst_y[k, 0]) for k in range(p.at_dst))
        # the oracle: one stream that simply keeps running, N1 blocks heard in the source and n2 in the destination
        x = np.concatenate([src_x[:N1, 1], src_x[p.at_src:p.at_src + p.n2, 1]])
        got = np.concatenate([src.y[:N1, 1], moved[:, :, :1]])
        dev = oracle_blocks(bv, oracle, model_dir, 1, H, x, got, 1, 0,
                            lambda script, i: i != N1 - 1 or script.a.BeatriceBatch_SetTargetSpeaker(script.h, 0, 2))
        print("moved stream (%s, H = %d, %s) vs the oracle max-abs %g" % (how, H, "one stream" if one_stream else "two streams", dev))
        assert dev <= BOUND
    finally:
        p.close()
        if made:
            hip.hipStreamDestroy(made)


def test_the_source_slot_turned_over_after_the_move_is_a_new_stream(bv, oracle, product, models, model_dir):
    """shard.move_streams(in_flight=True, reset_source=True) on two F batches: the F calls, then BeatriceBatch_ResetStreamInFlight on the
    source slot, which is fed at once as a new stream -- the oracle's new stream behind a new wrapper; neither batch drains."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("bv_shard_48k", os.path.join(os.path.dirname(os.path.abspath(bv.__file__)), "shard.py"))
    shard = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(shard)
    H = 1
    src_y, dst_y, _ = twins(bv, models, H)
    p = Pair(bv, models, H, turn_over=True)
    try:
        src, dst = p.src, p.dst
        p.start()
        src.run_to(p.at_src)
        dst.run_to(p.at_dst)
        before = (src.ticks(), dst.ticks())
        assert shard.move_streams(src.batch, [1], dst.batch, [0], reset_source=True, in_flight=True) is None
        assert before == (src.ticks(), dst.ticks())
        src.finish()
        dst.finish()
        assert src.ticks_before_sync == src.n and dst.ticks_before_sync == dst.n   # no drain in either, the reset included
        _, moved = dst.heard(0, 801)
        for c in range(2):
            assert np.array_equal(moved[:, :, c], src_y[p.at_src:p.at_src + p.n2, 1, :, 0])
        assert all(np.array_equal(src.y[k, s], src_y[k, s]) for k in range(src.n) for s in (0, 2))
        idx, fresh = src.heard(1, 820)
        assert idx == list(range(src.n - p.at_src)) and np.abs(fresh).max() > 1e-3
        dev = oracle_blocks(bv, oracle, model_dir, 1, H, src.x[p.at_src:, 1], fresh, 2, 0)   # (the slot keeps its settings: the voice switched to)
        print("source slot turned over behind the move vs the oracle's new stream max-abs %g" % dev)
        assert dev <= BOUND
    finally:
        p.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def partner(bv, product, models):
    """a batch around resident 48 kHz blocks whose streams are at rest: the other side of a move for a batch in any other mode"""
    ln = Line(bv, models, mode_matrix.B, 1, mode_matrix.CH, [830, 831, 832]).start()
    yield ln
    ln.close()


@pytest.mark.parametrize("mode", ["in_order", "stage_pipelining", "resident_io", "tick", "host_streaming", "resident_blocks",
                                  "resident_blocks_per_stream_clocks", "silent_rule_in_order"])
def test_every_other_mode_refuses_the_four_48k_calls(bv, product, model_dir, partner, mode):
    """A, B, C, D, E, G, P, S (built as tests/test_gpu_mode_matrix.py builds them): -1 -- a move between a D batch and an F batch either
    way round included -- and the batch then equals a twin that never asked."""
    product = bv.bind_batch(product)
    B, CH, H = mode_matrix.B, mode_matrix.CH, 1
    steps = 7 if not mode.startswith("resident_blocks") else 10
    x16 = np.stack([bv.synth_audio(160 * H * steps, seed=8800 + s) for s in range(B)]).reshape(B, steps, H * 160)
    x48 = np.stack([wrapperlib.test_signal(480 * H * steps * CH, 48000, seed=8900 + s) for s in range(B)]).astype(np.float32).reshape(B, steps, H, CH, 480)
    assert partner.quiescent(0) == 1
    results = []
    for tries in (True, False):
        c = mode_matrix.Ctx(bv, product, model_dir, H)
        try:
            mode_matrix.enter(c, mode)
            size = c.batch.stream_blob_bytes()
            got = []
            for k in range(steps):
                if tries and k in (1, 4):
                    a, h = c.a, c.h
                    buf = C.create_string_buffer(size)
                    assert a.BeatriceBatch_Stream48kQuiescent(h, 0) == -1
                    assert a.BeatriceBatch_ExportStreams48kInFlight(h, 1, i32([0]), C.cast(buf, C.c_void_p)) == -1
                    assert a.BeatriceBatch_ImportStreams48kInFlight(h, 1, i32([0]), C.cast(buf, C.c_void_p), None, 0) == -1
                    assert a.BeatriceBatch_MoveStreams48kInFlight(h, partner.h, 1, i32([0]), i32([0]), None, 0) == -1
                    assert a.BeatriceBatch_MoveStreams48kInFlight(partner.h, h, 1, i32([0]), i32([0]), None, 0) == -1
                    assert a.BeatriceBatch_MoveStreamsInFlight(h, partner.h, 1, i32([0]), i32([0]), None, 0) == -1   # (the D calls refuse the F side)
                    assert a.BeatriceBatch_MoveStreamsInFlight(partner.h, h, 1, i32([0]), i32([0]), None, 0) == -1
                y = mode_matrix.step(c, mode, k, x16[:, k], x48[:, k])
                if y is not None:
                    got.append(np.array(y, copy=True))
            got += mode_matrix.finish(c, mode)
            results.append(got)
        finally:
            c.close()
    tried, control = results
    assert len(tried) == len(control) and len(tried) > 0
    assert max(float(np.abs(y).max()) for y in control) > 1e-3
    for p_, q_ in zip(tried, control):
        assert np.array_equal(p_, q_)


def test_bad_arguments_are_refused_and_a_pending_reset_refuses_a_source(bv, product, models):
    """-1: counts, NULL pointers, streams out of range or named twice, a map without a length and the reverse, a mapped index out of
    range, a corrupt blob, src == dst, a NULL batch, other hops per step.  -3: a source stream with a ResetStreamInFlight no step has
    taken; on a destination the import cancels it.  The batches then equal a pair that made only the accepted calls."""
    got = {}
    other = Line(bv, models, 3, 2, 1, [860, 861, 862], rule=True)
    try:
        other.sit_out(1, 0, other.n)
        other.start().run_to(2)
        for name in ("asked", "never"):
            a_ln, b_ln = (Line(bv, models, 3, 1, 1, [840 + 10 * j + s for s in range(3)], rule=True) for j in range(2))
            try:
                for ln in (a_ln, b_ln):
                    ln.sit_out(1, 0, ln.n)
                    ln.start().run_to(3)
                a, ah, bh = a_ln.a, a_ln.h, b_ln.h
                size = a_ln.batch.stream_blob_bytes()
                good = a_ln.batch.export_streams48k_in_flight([1])
                if name == "asked":
                    vp = lambda raw: C.cast(C.create_string_buffer(raw, size), C.c_void_p)   # noqa: E731
                    bad_magic, bad_tail = bytearray(good), bytearray(good)
                    bad_magic[0] ^= 0xFF
                    bad_tail[20] ^= 0x55
                    ex = lambda n, s, p=vp(good): a.BeatriceBatch_ExportStreams48kInFlight(ah, n, s, p)   # noqa: E731
                    im = lambda n, s, p, em=None, nm=0: a.BeatriceBatch_ImportStreams48kInFlight(bh, n, s, p, em, nm)   # noqa: E731
                    mv = lambda n, s, t, em=None, nm=0, x=ah, y=bh: a.BeatriceBatch_MoveStreams48kInFlight(x, y, n, s, t, em, nm)   # noqa: E731
                    before = (a_ln.state(), b_ln.state())
                    rcs = [ex(0, i32([1])), ex(4, i32([0, 1, 2, 1])), ex(1, None), ex(1, i32([1]), None), ex(1, i32([3])), ex(1, i32([-1])), ex(2, i32([1, 1])),
                           im(0, i32([1]), vp(good)), im(1, None, vp(good)), im(1, i32([1]), None), im(1, i32([3]), vp(good)),
                           im(1, i32([1]), vp(bytes(bad_magic))), im(1, i32([1]), vp(bytes(bad_tail))), im(1, i32([1]), vp(good), None, 4),
                           im(1, i32([1]), vp(good), i32([0, 1, 2, 3]), 0), im(1, i32([1]), vp(good), i32([99, 99, 99, 99]), 4),
                           mv(0, i32([1]), i32([1])), mv(1, None, i32([1])), mv(1, i32([1]), None), mv(1, i32([3]), i32([1])), mv(1, i32([1]), i32([3])),
                           mv(2, i32([1, 1]), i32([0, 1])), mv(1, i32([1]), i32([1]), None, 4), mv(1, i32([1]), i32([1]), i32([99, 99, 99, 99]), 4),
                           mv(1, i32([1]), i32([1]), y=ah), mv(1, i32([1]), i32([1]), x=None), mv(1, i32([1]), i32([1]), y=None),
                           mv(1, i32([1]), i32([1]), y=other.h), mv(1, i32([1]), i32([1]), x=other.h),
                           a.BeatriceBatch_Stream48kQuiescent(ah, -1), a.BeatriceBatch_Stream48kQuiescent(ah, 3), a.BeatriceBatch_Stream48kQuiescent(None, 0)]
                    assert set(rcs) == {-1}, rcs
                    assert before == (a_ln.state(), b_ln.state())
                    # a reset no step has taken: -3 on the source, and the quiescence getter still says at rest (what refuses is the reset)
                    assert a.BeatriceBatch_ResetStreamInFlight(ah, 1) == 0 and a_ln.quiescent(1) == 1
                    assert ex(1, i32([1])) == -3 and mv(1, i32([1]), i32([1])) == -3
                    assert before == (a_ln.state(), b_ln.state())
                    # ... cancelled on a destination: stream 1 of `a` takes its own earlier blob back and is NOT reset when it is fed
                    assert a.BeatriceBatch_ImportStreams48kInFlight(ah, 1, i32([1]), vp(good), None, 0) == 0
                    assert ex(1, i32([1])) == 0
                for ln in (a_ln, b_ln):
                    ln.out[6:, 1] = 0   # (stream 1 joins at step 6; its material was planned from index 0)
                    ln.x[6:, 1, :, 0] = signal(ln.sources[1][0][1], 1)[:ln.n - 6]
                    ln.finish()
                    assert ln.ticks_before_sync == ln.n
                got[name] = (a_ln.y.copy(), b_ln.y.copy())
            finally:
                a_ln.close()
                b_ln.close()
    finally:
        other.close()
    assert np.abs(got["never"][0][:, 1]).max() > 1e-3
    assert np.array_equal(got["asked"][0], got["never"][0]) and np.array_equal(got["asked"][1], got["never"][1])


def test_accepted_rounds_do_not_leak(bv, product, models):
    """Three streams a round by all three calls, 30 rounds: device memory is flat within tests/test_gpu_lifecycle.py's 8 MB allowance
    for the allocator's own pools, far below what a staging entry or a blob left behind per round would take."""
    B = 4
    a_ln, b_ln = (Line(bv, models, B, 1, 1 + j, [870 + 10 * j + s for s in range(B)], n=40, rule=True) for j in range(2))
    try:
        for ln in (a_ln, b_ln):
            for s in (1, 2, 3):
                ln.sit_out(s, 0, ln.n)
            ln.start()

        def cycle():
            a_ln.run_to(a_ln.fed + 1)
            b_ln.run_to(b_ln.fed + 1)
            b_ln.batch.import_streams48k_in_flight([3, 1, 2], a_ln.batch.export_streams48k_in_flight([1, 2, 3]))
            b_ln.batch.move_streams48k_in_flight(a_ln.batch, [1, 2, 3], [2, 3, 1])
        for _ in range(3):
            cycle()   # (the piece tables, the staging and the events are made here, once)
        before = _free_bytes()
        for _ in range(30):
            cycle()
        after = _free_bytes()
        print("free device memory: %.1f MB -> %.1f MB, a blob: %.2f MB" % (before / 2**20, after / 2**20, a_ln.batch.stream_blob_bytes() / 2**20))
        assert 30 * 3 * a_ln.batch.stream_blob_bytes() > 2 * (8 << 20)
        assert before - after <= 8 << 20
        a_ln.finish()
        b_ln.finish()
        assert a_ln.ticks_before_sync == a_ln.n and np.abs(a_ln.y[:, 0]).max() > 1e-3
    finally:
        a_ln.close()
        b_ln.close()
