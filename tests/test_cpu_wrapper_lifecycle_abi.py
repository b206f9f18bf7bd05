"""BeatriceBatch_SetStreamRate / RestartStreamWrapper / StreamRate / WrapperBlobBytes / ExportStreamWrappers / ImportStreamWrappers:
exported by the product library, declared in the header and typed in the ctypes table; shard.move_streams(with_wrapper=...) on fakes
(no GPU needed: symbols, prototypes and call order only)."""
import ctypes as C
import importlib.util
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("BeatriceBatch_SetStreamRate", "BeatriceBatch_RestartStreamWrapper", "BeatriceBatch_StreamRate", "BeatriceBatch_WrapperBlobBytes",
       "BeatriceBatch_ExportStreamWrappers", "BeatriceBatch_ImportStreamWrappers")


def test_the_library_exports_the_six_symbols(bv, product):
    for name in NEW:
        assert hasattr(product.lib, name), name


def test_the_header_declares_the_six_symbols():
    text = open(os.path.join(REPO, "include", "beatrice_batch.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)   # declarations, not the comments that mention them
    b, cb = r"\s*BeatriceBatch\s*\*\s*\w+\s*", r"\s*const\s+BeatriceBatch\s*\*\s*\w+\s*"
    i, ip = r"\s*int\s+\w+\s*", r"\s*const\s+int\s*\*\s*\w+\s*"
    assert re.search(r"\bint\s+BeatriceBatch_SetStreamRate\s*\(" + b + "," + i + r",\s*double\s+\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+BeatriceBatch_RestartStreamWrapper\s*\(" + b + "," + i + r"\)\s*;", text)
    assert re.search(r"\bdouble\s+BeatriceBatch_StreamRate\s*\(" + cb + "," + i + r"\)\s*;", text)
    assert re.search(r"\bsize_t\s+BeatriceBatch_WrapperBlobBytes\s*\(" + cb + r"\)\s*;", text)
    assert re.search(r"\bint\s+BeatriceBatch_ExportStreamWrappers\s*\(" + b + "," + i + "," + ip + r",\s*void\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+BeatriceBatch_ImportStreamWrappers\s*\(" + b + "," + i + "," + ip + r",\s*const\s+void\s*\*\s*\w+\s*\)\s*;", text)


def test_the_ctypes_table_types_the_six_symbols(bv):
    i32p, vp = C.POINTER(C.c_int), C.c_void_p
    assert bv._BATCH["BeatriceBatch_SetStreamRate"] == (C.c_int, [vp, C.c_int, C.c_double])
    assert bv._BATCH["BeatriceBatch_RestartStreamWrapper"] == (C.c_int, [vp, C.c_int])
    assert bv._BATCH["BeatriceBatch_StreamRate"] == (C.c_double, [vp, C.c_int])
    assert bv._BATCH["BeatriceBatch_WrapperBlobBytes"] == (C.c_size_t, [vp])
    assert bv._BATCH["BeatriceBatch_ExportStreamWrappers"] == (C.c_int, [vp, C.c_int, i32p, vp])
    assert bv._BATCH["BeatriceBatch_ImportStreamWrappers"] == (C.c_int, [vp, C.c_int, i32p, vp])
    assert set(NEW) <= set(bv.ABI_SYMBOLS_BATCH)
    for name in ("set_stream_rate", "restart_stream_wrapper", "stream_rate", "wrapper_blob_bytes", "export_stream_wrappers", "import_stream_wrappers"):
        assert callable(getattr(bv.Batch, name))


def test_the_mode_table_has_no_row_for_them():
    """They are settings gated on the row of ProcessBlocksRagged: csrc/batch_modes.h keeps the rows of the GPU matrix."""
    text = open(os.path.join(REPO, "beatrice-vst_amd", "csrc", "batch_modes.h")).read()
    for name in NEW:
        assert name.replace("BeatriceBatch_", "") not in text


class Fake:
    def __init__(self, log, who):
        self.log, self.who = log, who
        self.a, self.h = self, 7

    def export_streams(self, streams):
        self.log.append((self.who, "export", list(streams)))
        return b"blob"

    def import_streams(self, streams, blobs, entry_map=None):
        self.log.append((self.who, "import", list(streams), blobs, entry_map))

    def export_stream_wrappers(self, streams):
        self.log.append((self.who, "export_wrappers", list(streams)))
        return b"wrap"

    def import_stream_wrappers(self, streams, blobs):
        self.log.append((self.who, "import_wrappers", list(streams), blobs))

    def restart_stream_wrapper(self, s):
        self.log.append((self.who, "restart", s))

    def BeatriceBatch_ResetStream(self, h, s):
        self.log.append((self.who, "reset", h, s))
        return 0

    @staticmethod
    def _check(rc):
        assert rc == 0


def test_move_streams_with_and_without_the_wrapper():
    spec = importlib.util.spec_from_file_location("bv_shard", os.path.join(REPO, "beatrice-vst_amd", "shard.py"))
    shard = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(shard)
    # the default path: exactly what it did before -- the model blob's pair, the blobs returned as they are
    log = []
    src, dst = Fake(log, "src"), Fake(log, "dst")
    assert shard.move_streams(src, [2, 0], dst, [1, 3], entry_map=[1, 0]) == b"blob"
    assert log == [("src", "export", [2, 0]), ("dst", "import", [1, 3], b"blob", [1, 0])]
    del log[:]
    assert shard.move_streams(src, [2], dst, [0], reset_source=True, with_wrapper=False) == b"blob"
    assert log == [("src", "export", [2]), ("dst", "import", [0], b"blob", None), ("src", "reset", 7, 2)]
    # with the wrapper: both exports from the source, then both imports into the destination, in that order; a pair comes back
    del log[:]
    assert shard.move_streams(src, [2, 0], dst, [1, 3], entry_map=[1, 0], with_wrapper=True) == (b"blob", b"wrap")
    assert log == [("src", "export", [2, 0]), ("src", "export_wrappers", [2, 0]), ("dst", "import", [1, 3], b"blob", [1, 0]),
                   ("dst", "import_wrappers", [1, 3], b"wrap")]
    # ... and a source slot that is reset is handed on whole: model state and wrapper
    del log[:]
    shard.move_streams(src, [2], dst, [0], reset_source=True, with_wrapper=True)
    assert log[-2:] == [("src", "reset", 7, 2), ("src", "restart", 2)]
