"""The shell's silent-block test on blocks that live on the device (BeatriceBatch_ScanSilentBlocksBegin / End / ScanSilentBlocks /
ScanBoundBlocks48k; csrc/silent_scan.hip, csrc/silent_scan_plan.h).  The yardstick is tests/silent_ref.py, which
tests/test_cpu_silent_scan_abi.py holds against ProcessorProxy::ProcessChannels on the CPU; every comparison here is exact.  Every
device pointer handed to the library is an allocation of this file, large enough for the geometry it is passed with; the refusals
are asked with NULL and bad integers only."""
import ctypes as C

import numpy as np
import pytest

import silent_ref
from tick_driver import Hip, Resident

pytestmark = pytest.mark.gpu

_u8p = C.POINTER(C.c_ubyte)
_i32p = C.POINTER(C.c_int)


def at(p, floats):
    return C.c_void_p(p.value + 4 * floats)


class Dev:
    """Host arrays on the device for the length of a test."""

    def __init__(self):
        self.hip, self.live = Hip(), []

    def put(self, arr, lead=0):
        """The device copy of `arr` (float32, flat), `lead` floats behind the start of an allocation of exactly lead + arr.size floats."""
        a = np.ascontiguousarray(arr, np.float32).reshape(-1)
        host = np.concatenate([np.full(lead, 1.0, np.float32), a])   # (what lies in front of the blocks is loud)
        p = self.hip.malloc(host.nbytes)
        self.live.append(p)
        self.hip.h2d(p, host)
        return at(p, lead)

    def free(self):
        for p in self.live:
            self.hip.free(p)
        self.live = []


@pytest.fixture(scope="module")
def scan_batch(bv, product, model_dir):
    m = bv.Models(product, model_dir)
    batch = bv.Batch(m, 2)
    yield batch
    batch.close()
    m.close()


@pytest.fixture()
def dev():
    d = Dev()
    yield d
    d.free()


def want_flags(cells):
    """cells: [n_cells][J][channels][n] -> uint8 [n_cells][J] by silent_ref."""
    out = np.zeros(cells.shape[:2], np.uint8)
    for c in range(cells.shape[0]):
        for j in range(cells.shape[1]):
            out[c, j] = silent_ref.shell_silent(cells[c, j])
    return out


def scan(batch, p, n_cells, J, channels, n, stride=None, lens=None):
    """BeatriceBatch_ScanSilentBlocks into an array that starts out as neither answer."""
    flags = np.full((n_cells, J), 0xAA, np.uint8)
    la = None if lens is None else np.ascontiguousarray(lens, np.int32)
    rc = batch.a.BeatriceBatch_ScanSilentBlocks(batch.h, p, n_cells, J, channels, n, J * channels * n if stride is None else stride,
                                                None if la is None else la.ctypes.data_as(_i32p), None, flags.ctypes.data_as(_u8p))
    assert rc == 0, rc
    return flags


@pytest.mark.parametrize("J", [1, 4])
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 160, 441, 480, 4088])
def test_edge_table(scan_batch, dev, n, channels, J):
    """Every row of the edge table in every shape, the blocks 16-byte aligned and one float off.  With four blocks per cell a cell
    holds four consecutive rows of the table, so silent and loud blocks sit side by side."""
    rows = silent_ref.edge_table(n, channels)
    R = len(rows)
    cells = np.stack([np.stack([rows[(r + j) % R][1] for j in range(J)]) for r in range(R)])   # [R][J][channels][n]
    want = want_flags(cells)
    assert want.min() == 0 and want.max() == 1
    if J == 1:
        for r, (name, block) in enumerate(rows):
            assert want[r, 0] == silent_ref.shell_silent(block), name
    for lead in (0, 1):
        got = scan(scan_batch, dev.put(cells, lead=lead), R, J, channels, n)
        bad = [(rows[(r + j) % R][0], int(got[r, j]), int(want[r, j])) for r in range(R) for j in range(J) if got[r, j] != want[r, j]]
        assert not bad, "n %d, %d channel(s), %d block(s) per cell, %d float(s) off: (row, got, want) %s" % (n, channels, J, lead, bad[:8])


@pytest.mark.parametrize("n", [480, 441])
def test_every_position(scan_batch, dev, n):
    """Stereo: cell p holds one non-zero sample at flat position p -- no position is skipped; and what lies just in front of a block,
    or just behind it, is never read."""
    N = 2 * n
    cells = np.zeros((N, 1, 2, n), np.float32)
    cells.reshape(N, N)[np.arange(N), np.arange(N)] = 1.0
    for lead in (0, 1):
        p = dev.put(cells, lead=lead)
        got = scan(scan_batch, p, N, 1, 2, n)
        assert not got.any(), "%d float(s) off: positions that were not seen: %s" % (lead, np.flatnonzero(got[:, 0])[:12])
        # the same memory as blocks [2][n_c] with 2 * n_c <= p: the non-zero sample is the first or the second float behind the block
        lens = np.arange(N) // 2
        got = scan(scan_batch, p, N, 1, 2, n, lens=lens)
        assert got.all(), "%d float(s) off: blocks that saw the float behind them: %s" % (lead, np.flatnonzero(got[:, 0] == 0)[:12])
        # ... and one sample longer (where that fits) it is the block's last or last but one
        lens1 = np.minimum(lens + 1, n)
        got = scan(scan_batch, p, N, 1, 2, n, lens=lens1)
        assert not got.any(), "%d float(s) off: positions that were not seen: %s" % (lead, np.flatnonzero(got[:, 0])[:12])
    # silent blocks between loud floats: the float in front of every block and the float behind it are 1.0 (a stride larger than the
    # block).  lead 1 / pad 2: the 4-byte path; lead 4 / pad 4 at n = 480: the 16-byte path
    for lead, pad in ((1, 2), (4, 4)):
        for channels in (1, 2):
            n_cells, stride = 9, channels * n + pad
            mem = np.ones((n_cells, stride), np.float32)
            mem[:, :channels * n] = 0.0
            got = scan(scan_batch, dev.put(mem, lead=lead), n_cells, 1, channels, n, stride=stride)
            assert got.all(), (lead, pad, channels, got[:, 0])
            # the same with per-cell lengths: everything from the block's end on is loud
            lens = np.array([0, 1, 2, 3, n // 2, n - 2, n - 1, n, 5])
            mem = np.ones((n_cells, stride), np.float32)
            for c in range(n_cells):
                mem[c, :channels * lens[c]] = 0.0
            got = scan(scan_batch, dev.put(mem, lead=lead), n_cells, 1, channels, n, stride=stride, lens=lens)
            assert got.all(), (lead, pad, channels, got[:, 0])
    # inside a cell the neighbours are blocks: a silent one between a block whose LAST sample and one whose FIRST sample is loud
    for lead in (0, 1):
        cells = np.zeros((5, 3, 2, n), np.float32)
        cells[:, 0, 1, n - 1] = 1.0
        cells[:, 2, 0, 0] = 1.0
        got = scan(scan_batch, dev.put(cells, lead=lead), 5, 3, 2, n)
        assert np.array_equal(got, np.tile(np.array([0, 1, 0], np.uint8), (5, 1)))


def random_cells(rng, n_cells, J, channels, n, p_silent=0.4):
    cells = rng.standard_normal((n_cells, J, channels, n)).astype(np.float32)
    silent = rng.random((n_cells, J)) < p_silent
    cells[silent] = 0.0
    return cells, silent


def test_layouts_of_the_resident_modes(scan_batch, dev):
    rng = np.random.default_rng(20240)
    slots, B = 3, 5
    # D: [n_slots][B][H * 160], mono, H = 4 hops per cell
    cells, silent = random_cells(rng, slots * B, 4, 1, 160)
    got = scan(scan_batch, dev.put(cells), slots * B, 4, 1, 160)
    assert np.array_equal(got, want_flags(cells)) and np.array_equal(got, silent.astype(np.uint8))
    # F: [n_slots][B][H][channels][480], H = 4, stereo
    cells, silent = random_cells(rng, slots * B, 4, 2, 480)
    got = scan(scan_batch, dev.put(cells), slots * B, 4, 2, 480)
    assert np.array_equal(got, want_flags(cells)) and np.array_equal(got, silent.astype(np.uint8))
    # G: [n_slots][B][channels][n], a 44.1 kHz block
    cells, silent = random_cells(rng, slots * B, 1, 2, 441)
    got = scan(scan_batch, dev.put(cells), slots * B, 1, 2, 441)
    assert np.array_equal(got, want_flags(cells)) and np.array_equal(got, silent.astype(np.uint8))
    # P: [n_slots][B][channels * max_samples], a block [channels][n_c] at the start of its cell; what lies behind it is not the block's
    for channels in (1, 2):
        max_samples = 480
        lens = rng.choice([0, 1, 37, 160, 441, 479, 480], size=slots * B)
        lens[:3] = [0, 480, 441]
        silent = rng.random(slots * B) < 0.4
        mem = rng.standard_normal((slots * B, channels * max_samples)).astype(np.float32)
        blocks = []
        for c in range(slots * B):
            if silent[c]:
                mem[c, :channels * lens[c]] = 0.0
            blocks.append(mem[c, :channels * lens[c]].reshape(channels, lens[c]))
        want = np.array([silent_ref.shell_silent(b) for b in blocks], np.uint8)
        assert np.array_equal(want, (silent | (lens == 0)).astype(np.uint8))
        got = scan(scan_batch, dev.put(mem), slots * B, 1, channels, max_samples, lens=lens)
        assert np.array_equal(got[:, 0], want), (channels, lens, got[:, 0], want)


def test_tickets_and_refusals(scan_batch, dev):
    a, h = scan_batch.a, scan_batch.h
    rng = np.random.default_rng(7)
    geos = [(6, 4, 2, 480), (11, 1, 1, 441), (3, 2, 2, 160), (40, 1, 2, 4)]
    jobs = []
    for n_cells, J, channels, n in geos:
        cells, _ = random_cells(rng, n_cells, J, channels, n)
        jobs.append((dev.put(cells), want_flags(cells), cells))
    tickets = []
    for (p, want, _), (n_cells, J, channels, n) in zip(jobs, geos):
        t = a.BeatriceBatch_ScanSilentBlocksBegin(h, p, n_cells, J, channels, n, J * channels * n, None, None)
        assert t >= 0 and t not in tickets
        tickets.append(t)
    # a fifth is refused and changes nothing: the four still end, in reverse order, each with its own answer
    assert a.BeatriceBatch_ScanSilentBlocksBegin(h, jobs[0][0], 6, 4, 2, 480, 3840, None, None) == -3
    one = np.full((6, 4), 0xAA, np.uint8)
    assert a.BeatriceBatch_ScanSilentBlocks(h, jobs[0][0], 6, 4, 2, 480, 3840, None, None, one.ctypes.data_as(_u8p)) == -3
    assert (one == 0xAA).all()
    spare = np.zeros(64, np.uint8)
    for unknown in (-1, -3, 0, 3, max(tickets) + 4, 0x7fffffff):
        if unknown not in tickets:
            assert a.BeatriceBatch_ScanSilentBlocksEnd(h, unknown, spare.ctypes.data_as(_u8p)) == -1
    assert a.BeatriceBatch_ScanSilentBlocksEnd(h, tickets[0], None) == -1   # (a NULL pointer: the ticket stays out)
    for k in (3, 2, 1, 0):
        n_cells, J = geos[k][:2]
        got = np.full((n_cells, J), 0xAA, np.uint8)
        assert a.BeatriceBatch_ScanSilentBlocksEnd(h, tickets[k], got.ctypes.data_as(_u8p)) == 0
        assert np.array_equal(got, jobs[k][1]), k
        assert a.BeatriceBatch_ScanSilentBlocksEnd(h, tickets[k], got.ctypes.data_as(_u8p)) == -1   # ended: unknown from now on
    # the Python methods over the same calls
    t0 = scan_batch.scan_silent_blocks_begin(jobs[1][0], 11, 1, 1, 441)
    t1 = scan_batch.scan_silent_blocks_begin(jobs[3][0], 40, 1, 2, 4)
    assert np.array_equal(scan_batch.scan_silent_blocks_end(t1), jobs[3][1])
    assert np.array_equal(scan_batch.scan_silent_blocks_end(t0), jobs[1][1])
    with pytest.raises(RuntimeError):
        scan_batch.scan_silent_blocks_end(t0)

    # every refusal of the header's list: -1, nothing enqueued (all four tickets are free afterwards), and a good scan is right
    p, want, _ = jobs[0]   # 6 cells x 4 blocks x stereo x 480
    out = np.full((6, 4), 0xAA, np.uint8)
    f = out.ctypes.data_as(_u8p)
    lens6 = (C.c_int * 6)(480, 0, 1, 480, 7, 9)
    lens_lo = (C.c_int * 6)(480, 0, -1, 480, 7, 9)
    lens_hi = (C.c_int * 6)(480, 0, 1, 481, 7, 9)
    refused = [
        (None, 6, 4, 2, 480, 3840, None),            # a NULL pointer
        (p, 0, 4, 2, 480, 3840, None), (p, -6, 4, 2, 480, 3840, None),
        (p, 6, 0, 2, 480, 3840, None), (p, 6, -4, 2, 480, 3840, None),
        (p, 6, 4, 0, 480, 3840, None), (p, 6, 4, 3, 480, 5760, None), (p, 6, 4, -1, 480, 3840, None),
        (p, 6, 4, 2, 0, 3840, None), (p, 6, 4, 2, -480, 3840, None),
        (p, 1, 1, 1, (1 << 30) + 1, 1 << 31, None),   # (a block longer than the kernel's sample counter is allowed to count)
        (p, 6, 4, 2, 480, 3839, None), (p, 6, 4, 2, 480, 0, None), (p, 6, 4, 2, 480, -3840, None),
        (p, 6, 4, 2, 480, 3840, lens6),              # per-cell lengths with four blocks per cell
        (p, 6, 1, 2, 480, 3840, lens_lo), (p, 6, 1, 2, 480, 3840, lens_hi),
        (p, (1 << 20) + 1, 1, 1, 1, 1, None), (p, 1 << 18, 5, 1, 1, 5, None),   # more than 2^20 blocks
    ]
    for args in refused:
        assert a.BeatriceBatch_ScanSilentBlocksBegin(h, *args, None) == -1, args[1:]
        assert a.BeatriceBatch_ScanSilentBlocks(h, *args, None, f) == -1, args[1:]
    assert a.BeatriceBatch_ScanSilentBlocks(h, p, 6, 4, 2, 480, 3840, None, None, None) == -1   # ... the flags' NULL pointer
    assert (out == 0xAA).all()
    held = [a.BeatriceBatch_ScanSilentBlocksBegin(h, p, 6, 4, 2, 480, 3840, None, None) for _ in range(4)]   # (no refusal took a ticket)
    assert min(held) >= 0 and len(set(held)) == 4
    for t in held:
        assert a.BeatriceBatch_ScanSilentBlocksEnd(h, t, f) == 0
        assert np.array_equal(out, want)
    mem = jobs[0][2].reshape(6, 3840)   # the same cells as one block [2][n_c] at the start of each
    want_ragged = np.array([silent_ref.shell_silent(mem[c, :2 * lens6[c]].reshape(2, lens6[c])) for c in range(6)], np.uint8)
    assert np.array_equal(scan(scan_batch, p, 6, 1, 2, 480, stride=3840, lens=list(lens6))[:, 0], want_ragged)
    # a scan on a stream of the caller's
    st = C.c_void_p()
    assert dev.hip.lib.hipStreamCreateWithFlags(C.byref(st), 1) == 0
    try:
        got = np.full((6, 4), 0xAA, np.uint8)
        assert a.BeatriceBatch_ScanSilentBlocks(h, p, 6, 4, 2, 480, 3840, None, st, got.ctypes.data_as(_u8p)) == 0
        assert np.array_equal(got, want)
    finally:
        assert dev.hip.lib.hipStreamSynchronize(st) == 0
        dev.hip.lib.hipStreamDestroy(st)
    # the bound form is mode F's: refused on a batch in order, and nothing was taken
    sf = np.zeros((1, scan_batch.B), np.uint8)
    assert a.BeatriceBatch_ScanBoundBlocks48k(h, 1, sf.ctypes.data_as(_u8p), None, None) == -1


@pytest.mark.parametrize("H", [1, 4])
def test_a_scan_beside_the_ticks_drains_and_changes_nothing(bv, product, model_dir, H):
    """Two identical batches in plain tick mode over the same input; one scans its input slots between the steps, on the scan's own
    stream, and ends each ticket three steps later, ticks in flight.  Same bits, same number of ticks."""
    B, steps, chunk, lag = 6, (39 if H == 1 else 16), 13, 3
    rng = np.random.default_rng(5 + H)
    x = np.stack([bv.synth_audio(160 * H * steps, seed=8100 + s) for s in range(B)]).reshape(B, steps, H, 160).transpose(1, 0, 2, 3).copy()
    x[rng.random((steps, B, H)) < 0.3] = 0.0     # [steps][B][H][160]
    want_flags_ = np.array([[[silent_ref.shell_silent(x[k, s, hh]) for hh in range(H)] for s in range(B)] for k in range(steps)], np.uint8)
    outs, ticks = {}, {}
    for scanning in (False, True):
        m = bv.Models(product, model_dir)
        batch = bv.Batch(m, B, hops_per_step=H)
        a, h = batch.a, batch.h
        for s in range(B):
            a.BeatriceBatch_SetTargetSpeaker(h, s, s % 3)
        a.BeatriceBatch_FlushSpeaker(h, -1)
        r = Resident(bv, batch, tick=True)
        try:
            got = np.zeros((steps, B, H * 240), np.float32)
            seen = {}
            k0 = 0
            while k0 < steps:
                cnt = min(chunk, steps - k0)
                pending = []

                def before(j, k0=k0, fed=r.fed, pending=pending):
                    if not scanning:
                        return
                    # (the chunk's slots were uploaded before its first step: the blocks are written and visible)
                    slot = (fed + j) % r.slots
                    pending.append((k0 + j, batch.scan_silent_blocks_begin(at(r.d_in, slot * B * H * 160), B, H, 1, 160)))
                    if len(pending) > lag:
                        k, t = pending.pop(0)
                        seen[k] = batch.scan_silent_blocks_end(t)
                    sf = np.zeros((1, B), np.uint8)
                    assert a.BeatriceBatch_ScanBoundBlocks48k(h, 1, sf.ctypes.data_as(_u8p), None, None) == -1   # (not in F)

                got[k0:k0 + cnt] = r.feed([x[k].reshape(B, H * 160) for k in range(k0, k0 + cnt)], before)
                for k, t in pending:
                    seen[k] = batch.scan_silent_blocks_end(t)
                k0 += cnt
            ticks[scanning] = int(a.BeatriceBatch_TicksLaunched(h))
            outs[scanning] = got
            if scanning:
                assert sorted(seen) == list(range(steps))
                for k in range(steps):
                    assert np.array_equal(seen[k], want_flags_[k]), k
            r.leave()
        finally:
            r.free()
            batch.close()
            m.close()
    assert np.abs(outs[False]).max() > 1e-3
    assert np.array_equal(outs[True], outs[False])
    assert ticks[True] == ticks[False] and ticks[True] > 0


@pytest.mark.parametrize("channels,H", [(2, 1), (1, 4), (2, 4)])
def test_silent_48k_blocks_flagged_by_the_scan_alone(bv, product, model_dir, channels, H):
    """tests/test_gpu_tick_ragged.py::test_silent_48k_blocks_per_stream_around_the_tick_pipeline -- its inputs, switches, silent pattern
    and per-stream ProcessorProxy reference -- with one difference: the batch never sees the test's `silent` table.  Its flags come from
    scan_bound_blocks_48k, asked once per uploaded chunk before that chunk's calls."""
    import wrapperlib
    from test_host_proxy import K_MODEL, K_VOICE, K_VQ, Proxy
    _f32p = C.POINTER(C.c_float)
    B, n = 6, 480
    steps = 44 if H == 1 else (26 if H == 2 else 16)
    blocks = steps * H
    x = np.zeros((B, channels, blocks * n), np.float32)
    for s in range(B):
        for c in range(channels):
            x[s, c] = (0.7 if c else 1.0) * wrapperlib.test_signal(blocks * n, 48000, seed=5200 + 5 * s + c)
    silent_steps = ({0: {3, 4, 5, 11}, 1: {0, 1, 9, 20, 21}, 2: set(), 3: set(range(6, 19)), 4: {2, 13, 14, 43}, 5: {30}} if H == 1 else
                    {0: {3, 4, 11}, 1: {0, 1, 9}, 2: set(), 3: set(range(5, 12)), 4: {2, 13, 14, steps - 1}, 5: {7}})
    silent = {s: {st * H + hh for st in ks if st < steps for hh in range(H)} for s, ks in silent_steps.items()}
    for s, ks in silent.items():
        for k in ks:
            x[s, :, k * n:(k + 1) * n] = 0.0
    switch = {0: (3 * H, 2), 1: (8 * H, 0), 3: (5 * H, 1), 4: (13 * H, 2)}
    want = np.zeros_like(x)
    proxy_flags = np.zeros((B, blocks), np.uint8)
    for s in range(B):
        p = Proxy(48000.0)
        assert p.call("SetString", K_MODEL, (model_dir + "/model.toml").encode()) == 0
        p.call("SetInt", K_VOICE, s % 3)
        p.call("SetNumber", K_VQ, float(s % 3))
        for k in range(blocks):
            if s in switch and switch[s][0] == k:
                p.call("SetInt", K_VOICE, switch[s][1])
            sl = slice(k * n, (k + 1) * n)
            in0 = np.ascontiguousarray(x[s, 0, sl])
            in1 = np.ascontiguousarray(x[s, 1, sl]) if channels == 2 else None
            o0, o1 = np.zeros(n, np.float32), np.zeros(n, np.float32)
            flag = p.call("ProcessChannels", in0.ctypes.data_as(_f32p), in1.ctypes.data_as(_f32p) if in1 is not None else None,
                          o0.ctypes.data_as(_f32p), o1.ctypes.data_as(_f32p) if channels == 2 else None, n)
            assert flag == (1 if k in silent[s] else 0)
            proxy_flags[s, k] = flag
            want[s, 0, sl] = o0
            if channels == 2:
                want[s, 1, sl] = o1
        p.close()

    m = bv.Models(product, model_dir)
    batch = bv.Batch(m, B, hops_per_step=H)
    a, h = batch.a, batch.h
    for s in range(B):
        a.BeatriceBatch_SetTargetSpeaker(h, s, s % 3)
        a.BeatriceBatch_SetVQNumNeighbors(h, s, s % 3)
    hip = Hip()
    slots = a.BeatriceBatch_TickStages(h) + 3
    d_in, d_out = hip.malloc(slots * B * H * channels * n * 4), hip.malloc(slots * B * H * channels * n * 4)
    try:
        assert a.BeatriceBatch_BindResidentIO48k(h, d_in, d_out, channels, slots) == 0
        none = np.zeros((1, B), np.uint8)
        for bad in (0, -1, slots + 1):
            assert a.BeatriceBatch_ScanBoundBlocks48k(h, bad, none.ctypes.data_as(_u8p), None, None) == -1
        assert a.BeatriceBatch_ScanBoundBlocks48k(h, 1, None, None, None) == -1
        assert a.BeatriceBatch_EnableSilentBlockRule(h, 1) == 0
        xs = x.reshape(B, channels, steps, H, n).transpose(2, 0, 3, 1, 4)   # [step][B][H][channels][n]: a step's resident slot
        gs = np.zeros_like(xs)
        scanned = np.zeros((B, blocks), np.uint8)
        k0 = 0
        while k0 < steps:
            cnt = min(11, steps - k0)
            buf = np.zeros((slots, B, H, channels, n), np.float32)
            for k in range(k0, k0 + cnt):
                buf[k % slots] = xs[k]
            hip.h2d(d_in, buf)
            step_flags, block_flags = batch.scan_bound_blocks_48k(cnt)   # the chunk's slots, wherever the ring of slots stands
            assert step_flags.shape == (cnt, B) and block_flags.shape == (cnt, B, H)
            assert np.array_equal(step_flags, block_flags.min(axis=2))
            for k in range(k0, k0 + cnt):
                scanned[:, k * H:(k + 1) * H] = block_flags[k - k0]
                for s in range(B):
                    if s in switch and switch[s][0] == k * H:
                        a.BeatriceBatch_SetTargetSpeaker(h, s, switch[s][1])
                if step_flags[k - k0].any():
                    assert a.BeatriceBatch_SetSilentStreams(h, step_flags[k - k0].tobytes()) == 0
                assert a.BeatriceBatch_ConvertBlocks48kDevice(h, None, None, channels) == 0
            assert a.BeatriceBatch_Synchronize(h) == 0
            out = np.zeros((slots, B, H, channels, n), np.float32)
            hip.d2h(out, d_out)
            for k in range(k0, k0 + cnt):
                gs[k] = out[k % slots]
            k0 += cnt
        got = np.ascontiguousarray(gs.transpose(1, 3, 0, 2, 4)).reshape(B, channels, blocks * n)
    finally:
        batch.close()
        m.close()
        hip.free(d_in); hip.free(d_out)
    assert np.array_equal(scanned, proxy_flags), "blocks whose scanned flag is not the proxy's: %s" % np.argwhere(scanned != proxy_flags)[:12].tolist()
    assert np.abs(want).max() > 1e-3
    for s in range(B):
        d = np.abs(got[s] - want[s])
        assert np.array_equal(got[s], want[s]), "stream %d: max-abs %g, first differing block %d" % (s, d.max(), int(np.argmax(d.max(axis=0) > 0)) // n)
