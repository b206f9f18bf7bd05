"""BeatriceBatch_StreamBlobBytes / BeatriceBatch_ExportStreams / BeatriceBatch_ImportStreams: exported by the product library, declared in
the header and typed in the ctypes table (no GPU needed: symbols and prototypes only)."""
import ctypes as C
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("BeatriceBatch_StreamBlobBytes", "BeatriceBatch_ExportStreams", "BeatriceBatch_ImportStreams")


def test_the_library_exports_the_three_symbols(bv, product):
    for name in NEW:
        assert hasattr(product.lib, name), name


def test_the_header_declares_the_three_symbols():
    text = open(os.path.join(REPO, "include", "beatrice_batch.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)   # declarations, not the comments that mention them
    ip = r"\s*const\s+int\s*\*\s*\w+\s*"
    assert re.search(r"\bsize_t\s+BeatriceBatch_StreamBlobBytes\s*\(\s*const\s+BeatriceBatch\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+BeatriceBatch_ExportStreams\s*\(\s*BeatriceBatch\s*\*\s*\w+\s*,\s*int\s+\w+\s*," + ip + r",\s*void\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+BeatriceBatch_ImportStreams\s*\(\s*BeatriceBatch\s*\*\s*\w+\s*,\s*int\s+\w+\s*," + ip + r",\s*const\s+void\s*\*\s*\w+\s*,"
                     + ip + r",\s*int\s+\w+\s*\)\s*;", text)


def test_the_ctypes_table_types_the_three_symbols(bv):
    i32p = C.POINTER(C.c_int)
    assert bv._BATCH["BeatriceBatch_StreamBlobBytes"] == (C.c_size_t, [C.c_void_p])
    assert bv._BATCH["BeatriceBatch_ExportStreams"] == (C.c_int, [C.c_void_p, C.c_int, i32p, C.c_void_p])
    assert bv._BATCH["BeatriceBatch_ImportStreams"] == (C.c_int, [C.c_void_p, C.c_int, i32p, C.c_void_p, i32p, C.c_int])
    assert set(NEW) <= set(bv.ABI_SYMBOLS_BATCH)
    for name in ("stream_blob_bytes", "export_streams", "import_streams"):
        assert callable(getattr(bv.Batch, name))


def test_shard_has_move_streams():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bv_shard", os.path.join(REPO, "beatrice-vst_amd", "shard.py"))
    shard = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(shard)

    class Fake:
        def __init__(self):
            self.log = []
            self.a, self.h = self, 7

        def export_streams(self, streams):
            self.log.append(("export", list(streams)))
            return b"blob"

        def import_streams(self, streams, blobs, entry_map=None):
            self.log.append(("import", list(streams), blobs, entry_map))

        def BeatriceBatch_ResetStream(self, h, s):
            self.log.append(("reset", h, s))
            return 0

        @staticmethod
        def _check(rc):
            assert rc == 0

    src, dst = Fake(), Fake()
    assert shard.move_streams(src, [2, 0], dst, [1, 3], entry_map=[1, 0]) == b"blob"
    assert src.log == [("export", [2, 0])] and dst.log == [("import", [1, 3], b"blob", [1, 0])]
    shard.move_streams(src, [2], dst, [0], reset_source=True)
    assert src.log[-2:] == [("export", [2]), ("reset", 7, 2)]
