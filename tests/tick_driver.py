"""Drives the product's tick pipeline (BeatriceBatch_EnableTickPipeline over BeatriceBatch_BindResidentIO) from host arrays:
shared by the throughput-mode parity tests and __graft_entry__.smoke().  Test plumbing only (ctypes + libamdhip64 copies)."""
import ctypes as C

import numpy as np


class Hip:
    def __init__(self):
        self.lib = C.CDLL("libamdhip64.so")  # the runtime the product library is linked against

    def malloc(self, nbytes):
        p = C.c_void_p()
        assert self.lib.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
        return p

    def h2d(self, dst, arr):
        assert self.lib.hipMemcpy(dst, arr.ctypes.data_as(C.c_void_p), C.c_size_t(arr.nbytes), 1) == 0

    def d2h(self, arr, src):
        assert self.lib.hipMemcpy(arr.ctypes.data_as(C.c_void_p), src, C.c_size_t(arr.nbytes), 2) == 0

    def free(self, p):
        self.lib.hipFree(p)


class Resident:
    """Resident I/O slots bound to a batch for as long as the object lives, so that a caller can feed a run chunk by chunk and keep the
    binding (and the slot counter: step j since the binding <-> slot j mod slots) between the chunks.  tick=True turns tick mode on
    over the binding, False leaves it at plain resident I/O."""

    def __init__(self, bv, batch, slots=None, tick=True):
        self.hip, self.batch, self.tick = Hip(), batch, tick
        a, h, B, H = batch.a, batch.h, batch.B, batch.H
        self.slots = slots or a.BeatriceBatch_TickStages(h) + 6
        self.d_in, self.d_out = self.hip.malloc(self.slots * B * H * 160 * 4), self.hip.malloc(self.slots * B * H * 240 * 4)
        self.fed = 0
        try:
            assert a.BeatriceBatch_BindResidentIO(h, self.d_in, self.d_out, self.slots) == 0
            if tick:
                assert a.BeatriceBatch_EnableTickPipeline(h, 1) == 0
        except BaseException:
            self.free()
            raise
        self.buf = np.zeros((self.slots, B, H * 160), np.float32)

    def feed(self, inputs, before_step=None):
        """Feeds len(inputs) (<= slots) steps without waiting, drains, and returns their samples [n][B][H * 240].
        before_step(j) runs before the j-th step of this call is fed (settings travel with the step)."""
        a, h, B, H, slots = self.batch.a, self.batch.h, self.batch.B, self.batch.H, self.slots
        n = len(inputs)
        assert n <= slots
        for j in range(n):
            self.buf[(self.fed + j) % slots] = inputs[j]
        self.hip.h2d(self.d_in, self.buf)
        for j in range(n):
            if before_step is not None:
                before_step(j)
            assert a.BeatriceBatch_ConvertFramesDevice(h, None, None) == 0
        assert a.BeatriceBatch_Synchronize(h) == 0
        out = np.zeros((slots, B, H * 240), np.float32)
        self.hip.d2h(out, self.d_out)
        got = np.stack([out[(self.fed + j) % slots] for j in range(n)]) if n else np.zeros((0, B, H * 240), np.float32)
        self.fed += n
        return got

    def leave(self):
        """Back to the in-order chain (streams that have sat steps out come back to the batch's step counter at every drained point)."""
        a, h = self.batch.a, self.batch.h
        if self.tick:
            assert a.BeatriceBatch_EnableTickPipeline(h, 0) == 0
        assert a.BeatriceBatch_BindResidentIO(h, None, None, 0) == 0

    def free(self):
        if self.d_in is not None:
            self.hip.free(self.d_in)
            self.hip.free(self.d_out)
            self.d_in = self.d_out = None


def run_tick(bv, batch, steps, hop_input, change=None, slots=None, chunk=None, leave=True):
    """Feeds `steps` steps through tick mode and returns their samples [steps][B][H * 240] (H = the batch's hops per step).

    hop_input(k) -> [B][H * 160] is step k's input; change(batch, k) runs before step k is fed (settings travel with the step).
    The resident I/O has `slots` slots (default: stages + 6) used round-robin as the library does (step k <-> slot k mod
    slots); steps are fed `chunk` (<= slots) at a time without waiting, then the pipeline is drained and the chunk read back,
    so the ring wraps many times over a long run."""
    r = Resident(bv, batch, slots=slots, tick=True)
    try:
        chunk = min(chunk or r.slots, r.slots)
        got = np.zeros((steps, batch.B, batch.H * 240), np.float32)
        k0 = 0
        while k0 < steps:
            n = min(chunk, steps - k0)
            got[k0:k0 + n] = r.feed([hop_input(k) for k in range(k0, k0 + n)],
                                    (lambda j, k0=k0: change(batch, k0 + j)) if change is not None else None)
            k0 += n
        if leave:
            r.leave()
    finally:
        r.free()
    return got
