"""The packed forms of MODEL_SPEC's scalar functions (csrc/spec_math.hip.h: two results per VALU instruction, a shorter
clamp, the integer part of exp's argument from a magic-number add, tanh's quotient without the scaling steps of the
general division) against the scalar definitions the oracle pins -- on the device, for every float32 bit pattern.  And the
device's scalar AND packed functions against oracle/spec_math.h itself, bit for bit, on the fixed point set of
tests/math_points.py (every exponent, the subnormals' neighbours, the clamps, the ties of exp's rint)."""
import ctypes

import numpy as np
import pytest

import math_points as mp

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("which,name", [(0, "exp"), (1, "tanh"), (2, "gelu"), (3, "sigmoid")])
def test_packed_function_equals_scalar_definition_for_every_float(bv, product, which, name):
    abi = bv.bind_batch(product)
    first = ctypes.c_uint(0)
    bad = abi.BeatriceHip_MathSelfTest(which, ctypes.byref(first))
    assert bad == 0, "%s: %d of 2^32 inputs differ, first at bits 0x%08x" % (name, bad, first.value)


@pytest.fixture(scope="module")
def points():
    return mp.points()


@pytest.mark.parametrize("which,name", [(w, n) for w, n in enumerate(mp.FUNCTIONS)] + [(6 + w, n + " (packed)") for w, n in enumerate(mp.FUNCTIONS[:4])])
def test_device_function_equals_oracle_function(bv, product, oracle, points, which, name):
    assert mp.oracle_keeps_subnormals(oracle), "this process flushes subnormals: the oracle cannot be trusted here"
    fn = which if which < 6 else which - 6
    pts = mp.points_for(mp.FUNCTIONS[fn], points)
    want = mp.oracle_eval(oracle, fn, pts)
    got = mp.device_eval(bv.bind_batch(product), which, pts)
    assert np.isfinite(want.view(np.float32)).all()
    bad = np.nonzero(got != want)[0]
    print("%s: %d of %d points differ" % (name, bad.size, pts.size))
    assert bad.size == 0, "%s: %d of %d points differ, first x = 0x%08x: device 0x%08x, oracle 0x%08x" % (
        name, bad.size, pts.size, pts[bad[0]], got[bad[0]], want[bad[0]])
    if which >= 6:      # other partners in the pairs: the same points in reversed order
        assert np.array_equal(mp.device_eval(bv.bind_batch(product), which, pts[::-1].copy()), want[::-1])
