"""BeatriceBatch_InstallSpeakersInFlight / MorphSpeakersInFlight / SpeakerEntryBusy in the wrapper modes F, G and P: the symbols the feature
stands on are exported and typed, and the header says what is now true -- the five modes, the -3 that replaces the drain (no GPU needed:
symbols, prototypes and header text only)."""
import ctypes as C
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("BeatriceBatch_InstallSpeakersInFlight", "BeatriceBatch_MorphSpeakersInFlight", "BeatriceBatch_SpeakerEntryBusy")
READ_BY_THE_TESTS = ("BeatriceBatch_TicksLaunched", "BeatriceBatch_ResidentBlocksOwed", "BeatriceBatch_FlushResidentBlocks",
                     "BeatriceBatch_BindResidentIO48k", "BeatriceBatch_BindResidentBlocks", "BeatriceBatch_BindResidentBlocksRagged")


def header():
    return open(os.path.join(REPO, "include", "beatrice_batch.h")).read()


def comment_before(text, name):
    """The comment block that ends right in front of `int name(`."""
    at = re.search(r"\bint\s+%s\s*\(" % name, text).start()
    start = text.rfind("/*", 0, at)
    assert text.find("*/", start) < at
    return " ".join(text[start:at].replace("*", " ").split())


def test_the_library_exports_the_symbols(bv, product):
    for name in CALLS + READ_BY_THE_TESTS:
        assert hasattr(product.lib, name), name


def test_the_ctypes_table_types_them(bv):
    i32p, f32p = C.POINTER(C.c_int), C.POINTER(C.c_float)
    assert bv._BATCH["BeatriceBatch_InstallSpeakersInFlight"] == (C.c_int, [C.c_void_p, C.c_int, i32p, f32p, f32p, f32p])
    assert bv._BATCH["BeatriceBatch_SpeakerEntryBusy"] == (C.c_int, [C.c_void_p, C.c_int])
    assert set(CALLS + READ_BY_THE_TESTS) <= set(bv.ABI_SYMBOLS_BATCH)


def test_the_prototypes_are_unchanged():
    text = re.sub(r"/\*.*?\*/", " ", header(), flags=re.S)
    fp = r"\s*const\s+float\s*\*\s*\w+\s*"
    assert re.search(r"\bint\s+BeatriceBatch_InstallSpeakersInFlight\s*\(\s*BeatriceBatch\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*const\s+int\s*\*\s*\w+\s*,"
                     + fp + "," + fp + "," + fp + r"\)\s*;", text)
    assert re.search(r"\bint\s+BeatriceBatch_MorphSpeakersInFlight\s*\(\s*BeatriceBatch\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*const\s+int\s*\*\s*\w+\s*,"
                     r"\s*const\s+int\s*\*\s*\w+\s*," + fp + r",\s*int\s+\w+\s*,\s*unsigned\s+\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+BeatriceBatch_SpeakerEntryBusy\s*\(\s*const\s+BeatriceBatch\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", text)


def test_the_comments_of_all_three_name_the_five_modes_and_the_contract_change():
    text = header()
    for name in CALLS:
        c = comment_before(text, name)
        assert "CONTRACT CHANGE" in c and "-3" in c, name
        assert re.search(r"\bF, G and P\b", c), name
    for name in CALLS[:2]:
        c = comment_before(text, name)
        assert "BeatriceBatch_TicksLaunched" in c and "BeatriceBatch_ResidentBlocksOwed" in c, name
        assert "in every other mode" in c, name
    busy = comment_before(text, "BeatriceBatch_SpeakerEntryBusy")
    assert "(b) in D, E, F, G and P" in busy and "speaker_entry_plan.h" in busy and "filling" in busy
    assert "in D and E" not in comment_before(text, "BeatriceBatch_MorphSpeakersInFlight").replace("as in D and E", "")
