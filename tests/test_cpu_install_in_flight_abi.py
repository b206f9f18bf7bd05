"""BeatriceBatch_InstallSpeakersInFlight / BeatriceBatch_MaxInstallEntries: exported by the product library, declared in the header and
typed in the ctypes table (no GPU needed: symbols and prototypes only)."""
import ctypes as C
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("BeatriceBatch_InstallSpeakersInFlight", "BeatriceBatch_MaxInstallEntries")


def test_the_library_exports_both_symbols(bv, product):
    for name in NEW:
        assert hasattr(product.lib, name), name


def test_the_header_declares_both_symbols():
    text = open(os.path.join(REPO, "include", "beatrice_batch.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)   # declarations, not the comments that mention them
    fp = r"\s*const\s+float\s*\*\s*\w+\s*"
    assert re.search(r"\bint\s+BeatriceBatch_InstallSpeakersInFlight\s*\(\s*BeatriceBatch\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*const\s+int\s*\*\s*\w+\s*,"
                     + fp + "," + fp + "," + fp + r"\)\s*;", text)
    assert re.search(r"\bint\s+BeatriceBatch_MaxInstallEntries\s*\(\s*const\s+BeatriceBatch\s*\*\s*\w+\s*\)\s*;", text)


def test_the_ctypes_table_types_both_symbols(bv):
    i32p, f32p = C.POINTER(C.c_int), C.POINTER(C.c_float)
    assert bv._BATCH["BeatriceBatch_InstallSpeakersInFlight"] == (C.c_int, [C.c_void_p, C.c_int, i32p, f32p, f32p, f32p])
    assert bv._BATCH["BeatriceBatch_MaxInstallEntries"] == (C.c_int, [C.c_void_p])
    assert set(NEW) <= set(bv.ABI_SYMBOLS_BATCH)
