"""BeatriceBatch_SetStreamRateInFlight / RestartStreamInFlight / BoundStreamRate: exported by the product library, declared in the header
with footnote 11 of the MODES table, typed in the ctypes table and wrapped by bv.Batch (no GPU needed: symbols, prototypes and texts only)."""
import ctypes as C
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("BeatriceBatch_SetStreamRateInFlight", "BeatriceBatch_RestartStreamInFlight", "BeatriceBatch_BoundStreamRate")


def header():
    return open(os.path.join(REPO, "include", "beatrice_batch.h")).read()


def test_the_library_exports_the_three_symbols(bv, product):
    for name in NEW:
        assert hasattr(product.lib, name), name


def test_the_header_declares_the_three_symbols():
    text = re.sub(r"/\*.*?\*/", " ", header(), flags=re.S)   # declarations, not the comments that mention them
    b, cb, i = r"\s*BeatriceBatch\s*\*\s*\w+\s*", r"\s*const\s+BeatriceBatch\s*\*\s*\w+\s*", r"\s*int\s+\w+\s*"
    d = r"\s*double\s+\w+\s*"
    assert re.search(r"\bint\s+BeatriceBatch_SetStreamRateInFlight\s*\(" + b + "," + i + "," + d + r"\)\s*;", text)
    assert re.search(r"\bint\s+BeatriceBatch_RestartStreamInFlight\s*\(" + b + "," + i + "," + d + "," + i + r"\)\s*;", text)
    assert re.search(r"\bdouble\s+BeatriceBatch_BoundStreamRate\s*\(" + cb + "," + i + r"\)\s*;", text)


def test_the_header_says_where_they_work_and_that_a_new_rate_allocates():
    text = " ".join(header().replace("*", " ").split())
    note = text[text.index("(11)"):]
    note = note[:note.index("Environment variables")]
    for name in NEW:
        assert name.replace("BeatriceBatch_", "") in note, name
    assert '"ProcessBlocksRaggedDevice" says ok' in note and "refused" in note
    doc = text[text.index("INSIDE that binding"):text.index("int BeatriceBatch_SetStreamRateInFlight(")]
    assert "not for an audio thread" in doc and "ALLOCATES" in doc
    assert "BIND WHILE A STREAM OF THE LOWEST RATE YOU EXPECT IS CONFIGURED" in doc
    assert "NOTHING DRAINS" in doc and "-2: HIP or allocation failure; nothing is committed" in doc


def test_the_ctypes_table_types_the_three_symbols(bv):
    vp = C.c_void_p
    assert bv._BATCH["BeatriceBatch_SetStreamRateInFlight"] == (C.c_int, [vp, C.c_int, C.c_double])
    assert bv._BATCH["BeatriceBatch_RestartStreamInFlight"] == (C.c_int, [vp, C.c_int, C.c_double, C.c_int])
    assert bv._BATCH["BeatriceBatch_BoundStreamRate"] == (C.c_double, [vp, C.c_int])
    assert set(NEW) <= set(bv.ABI_SYMBOLS_BATCH)
    for name in ("set_stream_rate_in_flight", "restart_stream_in_flight", "bound_stream_rate"):
        assert callable(getattr(bv.Batch, name))


def test_the_python_wrappers_pass_their_arguments_on(bv):
    class A:
        def __init__(self):
            self.log = []

        def BeatriceBatch_SetStreamRateInFlight(self, h, s, rate):
            self.log.append(("rate", h, s, rate))
            return 0

        def BeatriceBatch_RestartStreamInFlight(self, h, s, rate, reset):
            self.log.append(("restart", h, s, rate, reset))
            return -1 if s == 9 else 0

        def BeatriceBatch_BoundStreamRate(self, h, s):
            return 44100.0

    batch = bv.Batch.__new__(bv.Batch)
    batch.a, batch.h = A(), 7
    batch.set_stream_rate_in_flight(2, 22050)
    batch.restart_stream_in_flight(1)
    batch.restart_stream_in_flight(3, 48000.0, reset_model=True)
    assert batch.a.log == [("rate", 7, 2, 22050.0), ("restart", 7, 1, 0.0, 0), ("restart", 7, 3, 48000.0, 1)]
    assert batch.bound_stream_rate(0) == 44100.0
    try:
        batch.restart_stream_in_flight(9)
    except Exception:
        pass
    else:
        raise AssertionError("a refusal must raise")


def test_the_mode_table_has_no_row_for_them():
    """They are settings gated on the row of ProcessBlocksRaggedDevice: csrc/batch_modes.h keeps the rows of the GPU matrix."""
    text = open(os.path.join(REPO, "beatrice-vst_amd", "csrc", "batch_modes.h")).read()
    for name in NEW:
        assert name.replace("BeatriceBatch_", "") not in text
