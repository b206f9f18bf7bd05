"""ctypes view of the two wrapper libraries: the oracle's C restatement (prefix wo_) and the driver
built from the reference's own headers (prefix ref_, oracle/_ref/libref_wrapper.so)."""
import ctypes as C
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_WRAPPER = os.path.join(REPO, "oracle", "libwrapper_oracle.so")
REF_WRAPPER = os.path.join(REPO, "oracle", "_ref", "libref_wrapper.so")
HOP_FN = C.CFUNCTYPE(None, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p)
_f32p = C.POINTER(C.c_float)


def stub_hop(in160, out240, _user):
    """Deterministic stand-in for the model hop: out[i] = in[(2 i) // 3]."""
    for i in range(240):
        out240[i] = in160[(2 * i) // 3]


class Wrapper:
    def __init__(self, path, prefix):
        self.lib = C.CDLL(path)
        p = prefix
        self.f_fraction = getattr(self.lib, p + "fraction")
        self.f_fraction.argtypes = [C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        self.f_create = getattr(self.lib, p + "create")
        self.f_create.restype, self.f_create.argtypes = C.c_void_p, [C.c_double, HOP_FN, C.c_void_p]
        self.f_destroy = getattr(self.lib, p + "destroy")
        self.f_destroy.argtypes = [C.c_void_p]
        self.f_process = getattr(self.lib, p + "process")
        self.f_process.restype, self.f_process.argtypes = C.c_int, [C.c_void_p, _f32p, _f32p, C.c_int]
        self.f_in_gain = getattr(self.lib, p + "set_input_gain")
        self.f_in_gain.argtypes = [C.c_void_p, C.c_double]
        self.f_out_gain = getattr(self.lib, p + "set_output_gain")
        self.f_out_gain.argtypes = [C.c_void_p, C.c_double]
        # ProcessorCore2::SetSampleRate (processor_core_2.cc:421-429).  A reference library built before the driver had this entry lacks it:
        # has_set_rate is then False and the tests that want it fall back to their recorded results, as where the library is absent
        self.has_set_rate = hasattr(self.lib, p + "set_sample_rate")
        if self.has_set_rate:
            self.f_set_rate = getattr(self.lib, p + "set_sample_rate")
            self.f_set_rate.restype, self.f_set_rate.argtypes = None, [C.c_void_p, C.c_double]
        if prefix == "wo_":   # where a stream stands (the oracle's restatement only): samples waiting in the FIFO; the gains' targets and present values, dB
            self.f_fifo_fill = self.lib.wo_fifo_fill
            self.f_fifo_fill.restype, self.f_fifo_fill.argtypes = C.c_int, [C.c_void_p]
            self.f_gain_state = self.lib.wo_gain_state
            self.f_gain_state.restype, self.f_gain_state.argtypes = None, [C.c_void_p] + [C.POINTER(C.c_double)] * 4
        self.g_create = getattr(self.lib, p + "gain_create")
        self.g_create.restype, self.g_create.argtypes = C.c_void_p, [C.c_double, C.c_double]
        self.g_set = getattr(self.lib, p + "gain_set_target")
        self.g_set.argtypes = [C.c_void_p, C.c_double]
        self.g_process = getattr(self.lib, p + "gain_process")
        self.g_process.argtypes = [C.c_void_p, _f32p, _f32p, C.c_int]
        self.g_destroy = getattr(self.lib, p + "gain_destroy")
        self.g_destroy.argtypes = [C.c_void_p]

    def fraction(self, ratio):
        n, d = C.c_int(0), C.c_int(0)
        self.f_fraction(ratio, C.byref(n), C.byref(d))
        return n.value, d.value

    def run_chain(self, sample_rate, x, block, hop=stub_hop, in_gain_events=(), out_gain_events=()):
        """Stream x through Process() in blocks of `block` samples; gain events = [(sample_index, dB)]."""
        cb = HOP_FN(hop)
        p = self.f_create(float(sample_rate), cb, None)
        x = np.ascontiguousarray(x, np.float32)
        out = np.zeros_like(x)
        pos = 0
        ev_in, ev_out = list(in_gain_events), list(out_gain_events)
        while pos < len(x):
            while ev_in and ev_in[0][0] <= pos:
                self.f_in_gain(p, ev_in.pop(0)[1])
            while ev_out and ev_out[0][0] <= pos:
                self.f_out_gain(p, ev_out.pop(0)[1])
            n = min(block, len(x) - pos)
            rc = self.f_process(p, x[pos:pos + n].ctypes.data_as(_f32p), out[pos:pos + n].ctypes.data_as(_f32p), n)
            assert rc == 0
            pos += n
        self.f_destroy(p)
        return out

    def run_blocks(self, sample_rate, x, blocks, hop=stub_hop, gains=None, rate_at=None):
        """Stream x through Process() in calls of blocks[k] samples.  gains: call -> (input dB or None, output dB or None), set in front
        of that call; rate_at: call -> host rate, SetSampleRate in front of that call (before the gains)."""
        cb = HOP_FN(hop)
        p = self.f_create(float(sample_rate), cb, None)
        x = np.ascontiguousarray(x, np.float32)
        assert len(x) == sum(blocks)
        out = np.zeros_like(x)
        pos = 0
        for k, n in enumerate(blocks):
            if rate_at and k in rate_at:
                self.f_set_rate(p, float(rate_at[k]))
            gin, gout = (gains or {}).get(k, (None, None))
            if gin is not None:
                self.f_in_gain(p, gin)
            if gout is not None:
                self.f_out_gain(p, gout)
            assert self.f_process(p, x[pos:pos + n].ctypes.data_as(_f32p), out[pos:pos + n].ctypes.data_as(_f32p), n) == 0
            pos += n
        self.f_destroy(p)
        return out

    def gain_state(self, p):
        """(input target, input now, output target, output now) in dB"""
        v = [C.c_double(0.0) for _ in range(4)]
        self.f_gain_state(p, *[C.byref(c) for c in v])
        return tuple(c.value for c in v)

    def run_rate_walk(self, x, legs, hop=stub_hop):
        """One processor through a host that changes its rate: legs = [(sample_rate, block, n_samples, input gain dB, output gain dB)];
        before each leg SetSampleRate(rate) (the first leg creates the processor at its rate), then the two gain targets, then the leg's
        samples of x in blocks.  A leg at the rate of the one before it is the reference's no-op."""
        cb = HOP_FN(hop)
        x = np.ascontiguousarray(x, np.float32)
        out = np.zeros_like(x)
        p, pos = None, 0
        for sr, block, n, gin, gout in legs:
            if p is None:
                p = self.f_create(float(sr), cb, None)
            else:
                self.f_set_rate(p, float(sr))
            self.f_in_gain(p, gin)
            self.f_out_gain(p, gout)
            end = pos + n
            while pos < end:
                m = min(block, end - pos)
                assert self.f_process(p, x[pos:pos + m].ctypes.data_as(_f32p), out[pos:pos + m].ctypes.data_as(_f32p), m) == 0
                pos += m
        self.f_destroy(p)
        return out

    def gain_trace(self, sample_rate, x, events, block=97):
        g = self.g_create(float(sample_rate), 0.0)
        x = np.ascontiguousarray(x, np.float32)
        out = np.zeros_like(x)
        pos, ev = 0, list(events)
        while pos < len(x):
            while ev and ev[0][0] <= pos:
                self.g_set(g, ev.pop(0)[1])
            n = min(block, len(x) - pos)
            self.g_process(g, x[pos:pos + n].ctypes.data_as(_f32p), out[pos:pos + n].ctypes.data_as(_f32p), n)
            pos += n
        self.g_destroy(g)
        return out


def oracle_wrapper():
    return Wrapper(ORACLE_WRAPPER, "wo_")


def ref_wrapper():
    return Wrapper(REF_WRAPPER, "ref_") if os.path.exists(REF_WRAPPER) else None


def test_signal(n, sample_rate, seed):
    """Chirp + white noise, amplitude 0.5, from the portable counter-based generator."""
    import sys
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from make_model import Stream
    noise = Stream(0xA0D10 + seed).uniform(n).astype(np.float64)
    t = np.arange(n) / float(sample_rate)
    f0, f1 = 60.0, min(9000.0, 0.45 * sample_rate)
    phase = 2 * np.pi * (f0 * t + 0.5 * (f1 - f0) * t * t / max(t[-1], 1e-9))
    return (0.25 * np.sin(phase) + 0.25 * noise).astype(np.float32)


def vanishing_signal(n, sample_rate, seed):
    """test_signal under an envelope that starts at 1e-30, decays through the whole subnormal range to below 1e-44 (nothing but 0 left
    in float32) over the first 45 % of the run, comes back to 0.3 by 70 % and stays: a tail fading out and a new note."""
    x = test_signal(n, sample_rate, seed).astype(np.float64) / 0.5
    t = np.arange(n) / float(n)
    top = np.log10(0.3)
    log_env = np.where(t < 0.45, -30.0 - 16.5 * t / 0.45, np.where(t < 0.7, -46.5 + (top + 46.5) * (t - 0.45) / 0.25, top))
    return (x * 10.0 ** log_env).astype(np.float32)


def vanishing_gain_events(n):
    """input gain -30 dB from the start; output gain from 0 dB towards -60 dB from the start of the decay, back to 0 dB with the note"""
    return [(0, -30.0)], [(0, -60.0), (int(0.6 * n), 0.0)]
