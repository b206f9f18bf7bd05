"""BeatriceBatch_StreamQuiescent / ExportStreamsInFlight / ImportStreamsInFlight / MoveStreamsInFlight: exported by the product library,
declared in the header, typed in the ctypes table, wrapped by Batch, and chosen by shard.move_streams(in_flight=True) (no GPU needed:
symbols, prototypes and fakes only)."""
import ctypes as C
import importlib.util
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("BeatriceBatch_StreamQuiescent", "BeatriceBatch_ExportStreamsInFlight", "BeatriceBatch_ImportStreamsInFlight",
       "BeatriceBatch_MoveStreamsInFlight")


def test_the_library_exports_the_four_symbols(bv, product):
    for name in NEW:
        assert hasattr(product.lib, name), name


def test_the_header_declares_the_four_symbols():
    text = open(os.path.join(REPO, "include", "beatrice_batch.h")).read()
    assert "(12)" in text
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)   # declarations, not the comments that mention them
    ip = r"\s*const\s+int\s*\*\s*\w+\s*"
    bp = r"\s*BeatriceBatch\s*\*\s*\w+\s*"
    assert re.search(r"\bint\s+BeatriceBatch_StreamQuiescent\s*\(\s*const\s+BeatriceBatch\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+BeatriceBatch_ExportStreamsInFlight\s*\(" + bp + r",\s*int\s+\w+\s*," + ip + r",\s*void\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+BeatriceBatch_ImportStreamsInFlight\s*\(" + bp + r",\s*int\s+\w+\s*," + ip + r",\s*const\s+void\s*\*\s*\w+\s*,"
                     + ip + r",\s*int\s+\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+BeatriceBatch_MoveStreamsInFlight\s*\(" + bp + "," + bp + r",\s*int\s+\w+\s*," + ip + "," + ip + "," + ip
                     + r",\s*int\s+\w+\s*\)\s*;", text)


def test_the_ctypes_table_types_the_four_symbols(bv):
    i32p = C.POINTER(C.c_int)
    assert bv._BATCH["BeatriceBatch_StreamQuiescent"] == (C.c_int, [C.c_void_p, C.c_int])
    assert bv._BATCH["BeatriceBatch_ExportStreamsInFlight"] == (C.c_int, [C.c_void_p, C.c_int, i32p, C.c_void_p])
    assert bv._BATCH["BeatriceBatch_ImportStreamsInFlight"] == (C.c_int, [C.c_void_p, C.c_int, i32p, C.c_void_p, i32p, C.c_int])
    assert bv._BATCH["BeatriceBatch_MoveStreamsInFlight"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, i32p, i32p, i32p, C.c_int])
    assert set(NEW) <= set(bv.ABI_SYMBOLS_BATCH)
    for name in ("stream_quiescent", "export_streams_in_flight", "import_streams_in_flight", "move_streams_in_flight"):
        assert callable(getattr(bv.Batch, name))


@pytest.fixture(scope="module")
def shard():
    spec = importlib.util.spec_from_file_location("bv_shard", os.path.join(REPO, "beatrice-vst_amd", "shard.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Fake:
    """A batch that records what is asked of it; `device` is what BeatriceBatch_Device answers."""

    def __init__(self, device):
        self.log, self.device = [], device
        self.a, self.h = self, 7 + device

    def BeatriceBatch_Device(self, h):
        return self.device

    def export_streams(self, streams):
        self.log.append(("export", list(streams)))
        return b"drained"

    def import_streams(self, streams, blobs, entry_map=None):
        self.log.append(("import", list(streams), blobs, entry_map))

    def export_streams_in_flight(self, streams):
        self.log.append(("export_in_flight", list(streams)))
        return b"blob"

    def import_streams_in_flight(self, streams, blobs, entry_map=None):
        self.log.append(("import_in_flight", list(streams), blobs, entry_map))

    def move_streams_in_flight(self, dst, streams, dst_streams, entry_map=None):
        self.log.append(("move_in_flight", dst, list(streams), list(dst_streams), entry_map))

    def BeatriceBatch_ResetStream(self, h, s):
        self.log.append(("reset", h, s))
        return 0

    def BeatriceBatch_ResetStreamInFlight(self, h, s):
        self.log.append(("reset_in_flight", h, s))
        return 0

    @staticmethod
    def _check(rc):
        assert rc == 0


def test_in_flight_on_one_device_is_the_device_to_device_call(shard):
    src, dst = Fake(0), Fake(0)
    assert shard.move_streams(src, [2, 0], dst, [1, 3], entry_map=[1, 0], in_flight=True) is None
    assert src.log == [("move_in_flight", dst, [2, 0], [1, 3], [1, 0])] and dst.log == []
    shard.move_streams(src, [2], dst, [0], reset_source=True, in_flight=True)
    assert src.log[-2:] == [("move_in_flight", dst, [2], [0], None), ("reset_in_flight", 7, 2)] and dst.log == []


def test_in_flight_across_devices_is_the_in_flight_blob_pair(shard):
    src, dst = Fake(0), Fake(1)
    assert shard.move_streams(src, [2, 0], dst, [1, 3], entry_map=[1, 0], reset_source=True, in_flight=True) == b"blob"
    assert src.log == [("export_in_flight", [2, 0]), ("reset_in_flight", 7, 2), ("reset_in_flight", 7, 0)]
    assert dst.log == [("import_in_flight", [1, 3], b"blob", [1, 0])]


def test_the_default_is_the_drained_pair(shard):
    src, dst = Fake(0), Fake(0)
    assert shard.move_streams(src, [2], dst, [0], reset_source=True) == b"drained"
    assert src.log == [("export", [2]), ("reset", 7, 2)] and dst.log == [("import", [0], b"drained", None)]


def test_wrapper_state_does_not_travel_in_flight(shard):
    src, dst = Fake(0), Fake(0)
    with pytest.raises(ValueError):
        shard.move_streams(src, [2], dst, [0], with_wrapper=True, in_flight=True)
    assert src.log == [] and dst.log == []
