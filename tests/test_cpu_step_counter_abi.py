"""The step counter's test hooks -- BeatriceBatch_SetStepCounter / BeatriceBatch_StepCounter and BeatriceHip_SetHopCount[Legacy] /
BeatriceHip_HopCount[Legacy]: exported by the product library, declared in the header with the wrap value the kernels use, and typed in
the ctypes table (no GPU needed: symbols, prototypes and constants only; tests/test_gpu_counter_wrap.py drives them)."""
import ctypes as C
import inspect
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("BeatriceBatch_SetStepCounter", "BeatriceBatch_StepCounter", "BeatriceHip_SetHopCount", "BeatriceHip_SetHopCountLegacy",
       "BeatriceHip_HopCount", "BeatriceHip_HopCountLegacy")


def test_the_library_exports_the_symbols(bv, product):
    for name in NEW:
        assert hasattr(product.lib, name), name


def test_the_header_declares_the_symbols_and_the_wrap(bv):
    text = open(os.path.join(REPO, "include", "beatrice_batch.h")).read()
    assert "lcm(1..17)" in text and "FRESH" in text      # the header comment states the wrap and the "fresh only" rule
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)   # declarations, not the comments that mention them
    assert re.search(r"\bint\s+BeatriceBatch_SetStepCounter\s*\(\s*BeatriceBatch\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", code)
    assert re.search(r"\bint\s+BeatriceBatch_StepCounter\s*\(\s*const\s+BeatriceBatch\s*\*\s*\w+\s*\)\s*;", code)
    for suffix in ("", "Legacy"):
        assert re.search(r"\bint\s+BeatriceHip_SetHopCount%s\s*\(\s*int\s+\w+\s*,\s*void\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;" % suffix, code)
        assert re.search(r"\bint\s+BeatriceHip_HopCount%s\s*\(\s*int\s+\w+\s*,\s*const\s+void\s*\*\s*\w+\s*\)\s*;" % suffix, code)
    # one wrap: the header's, the kernels' (hop_next) and the Python module's
    wrap = int(re.search(r"#define\s+BEATRICE_HIP_STEP_WRAP\s+(\d+)", code).group(1))
    kernels = open(os.path.join(REPO, "beatrice-vst_amd", "csrc", "kernels_misc.hip.h")).read()
    assert int(re.search(r"#define\s+B_HOP_WRAP\s+(\d+)", kernels).group(1)) == wrap == bv.STEP_WRAP
    lcm = 1
    for i in range(1, 18):
        lcm = lcm * i // __import__("math").gcd(lcm, i)
    assert wrap == lcm and wrap % 3 == 0 and wrap % 4 == 0 and wrap + 2 < 1 << 24      # (the counter + 2 travels in 24 pointer bits, ring.h)


def test_the_ctypes_table_types_the_symbols(bv):
    assert bv._BATCH["BeatriceBatch_SetStepCounter"] == (C.c_int, [C.c_void_p, C.c_int])
    assert bv._BATCH["BeatriceBatch_StepCounter"] == (C.c_int, [C.c_void_p])
    for suffix in ("", "Legacy"):
        assert bv._BATCH["BeatriceHip_SetHopCount" + suffix] == (C.c_int, [C.c_int, C.c_void_p, C.c_int])
        assert bv._BATCH["BeatriceHip_HopCount" + suffix] == (C.c_int, [C.c_int, C.c_void_p])
    assert set(NEW) <= set(bv.ABI_SYMBOLS_BATCH)
    assert callable(bv.Batch.step_counter)
    for cls in (bv.Batch, bv.Stream1, bv.StreamLegacy):
        assert inspect.signature(cls.__init__).parameters["start_counter"].default is None
    for cls in (bv.Stream1, bv.StreamLegacy):
        assert callable(cls.hop_counts)


def test_the_scenario_runner_takes_a_start_counter():
    import scenario as sc
    assert inspect.signature(sc.run_product).parameters["start_counter"].default is None
    assert inspect.signature(sc.compare).parameters["start_counter"].default is None
    assert sc.main(["--seed", "3004", "--start-counter", "12252222"]) == 0      # (without --gpu: the scenario is printed, nothing runs)
