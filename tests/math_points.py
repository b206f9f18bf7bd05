"""The fixed point set on which MODEL_SPEC 2.1's scalar functions are compared (device against oracle bit for bit in
tests/test_gpu_spec_math.py; oracle against float64 in tests/test_cpu_regimes.py), and ctypes plumbing for the two evaluators.
Test infrastructure only."""
import ctypes as C

import numpy as np

FUNCTIONS = ("exp", "tanh", "gelu", "sigmoid", "log", "lrelu")      # `which` 0..5 of both evaluators; 6..9 = packed exp..sigmoid
LOG2E = np.float32(1.44269504088896341)
CENTRES = [s * v for v in (86.0, 88.0, 43.0, 44.0, 22.0, 9.0) for s in (1.0, -1.0)] + [0.0, 1.0, 1.41421356, 2.0 ** -126]


def _ordinal(bits):
    """float32 bit pattern -> position on the number line (an integer; -0 and +0 coincide)"""
    b = bits.astype(np.int64)
    return np.where(b & 0x80000000, -(b & 0x7fffffff), b)


def _from_ordinal(o):
    return np.where(o < 0, (-o) | 0x80000000, o).astype(np.uint32)


def around(values, ulps):
    """every float32 within `ulps` ulp of each value, as bit patterns"""
    c = _ordinal(np.asarray(values, np.float32).view(np.uint32))
    o = (c[:, None] + np.arange(-ulps, ulps + 1, dtype=np.int64)[None, :]).ravel()
    return _from_ordinal(o[np.abs(o) < 0x7f800000])


def points():
    """Bit patterns, sorted and unique, finite only:
    * every exponent (0 = the subnormals, .. 254) and both signs x 4096 mantissas: 0, 1, 0x7fffff and 4093 seeded ones;
    * every float within 2^16 ulp of +-86, +-88, +-43, +-44, +-22, +-9, 0, 1, 1.41421356 and the smallest normal;
    * 64 ulp either side of every tie of exp's rint, (n + 1/2) / log2e for n = -125 .. 127."""
    rng = np.random.Generator(np.random.PCG64(0x5EC2))
    draw = rng.integers(2, 0x7fffff, 8192)
    _, first = np.unique(draw, return_index=True)
    mant = np.concatenate([[0, 1, 0x7fffff], draw[np.sort(first)][:4093]]).astype(np.uint32)
    assert np.unique(mant).size == 4096
    exps = np.arange(0, 255, dtype=np.uint32)
    grid = ((exps[:, None] << 23) | mant[None, :]).ravel()
    grid = np.concatenate([grid, grid | np.uint32(0x80000000)])
    ties = (np.arange(-125, 128, dtype=np.float64) + 0.5) / float(LOG2E)
    out = np.unique(np.concatenate([grid, around(CENTRES, 1 << 16), around(ties, 64)]))
    return out


def points_for(name, pts=None):
    pts = points() if pts is None else pts
    if name == "log":           # the spec defines log for positive normal arguments only
        return pts[(pts >= 0x00800000) & (pts < 0x7f800000)]
    return pts


def _u32p(a):
    assert a.dtype == np.uint32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def oracle_eval(oracle_abi, which, bits):
    fn = oracle_abi.lib.BeatriceOracle_MathEval
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_uint32)]
    bits = np.ascontiguousarray(bits, np.uint32)
    out = np.zeros_like(bits)
    assert fn(which, _u32p(bits), bits.size, _u32p(out)) == 0
    return out


def device_eval(batch_abi, which, bits):
    bits = np.ascontiguousarray(bits, np.uint32)
    out = np.zeros_like(bits)
    assert batch_abi.BeatriceHip_MathEval(which, _u32p(bits), bits.size, _u32p(out)) == 0
    return out


def oracle_keeps_subnormals(oracle_abi):
    """lrelu(-2^-130) = 0.1f * -2^-130 is a subnormal; a process switched to flush-to-zero (a fast-math library loaded into it can do
    that to the thread) would return -0 here, and the oracle would flush everywhere without a word."""
    x = np.array([-2.0 ** -130], np.float32)
    y = oracle_eval(oracle_abi, 5, x.view(np.uint32)).view(np.float32)
    return x[0] != 0 and y[0] != 0 and abs(float(y[0]) / (0.1 * float(x[0])) - 1.0) < 0.01


# ---- MODEL_SPEC 2.1's mathematical definitions in float64 (the clamp of exp's argument is part of the definition) --------------------
def true_value(name, x32):
    x = x32.astype(np.float64)
    with np.errstate(all="ignore"):
        if name == "exp":
            return np.exp(np.clip(x, -86.0, 88.0))
        if name == "sigmoid":
            return 1.0 / (1.0 + np.exp(np.clip(-x, -86.0, 88.0)))
        if name == "tanh":
            return np.tanh(x)
        if name == "gelu":
            x3 = np.clip(x, -1e60, 1e60) ** 3
            return 0.5 * x * (1.0 + np.tanh(0.7978845608 * (x + 0.044715 * x3)))
        if name == "log":
            return np.log(x)
        return np.where(x > 0, x, 0.1 * x)


def ulp_error(got32, true64):
    """|got - true| in units of float32's spacing at `true` (2^-149 in the subnormal range)"""
    t = np.abs(true64)
    e = np.floor(np.log2(np.maximum(t, 2.0 ** -126)))
    return np.abs(got32.astype(np.float64) - true64) / 2.0 ** (e - 23)
