"""BeatriceBatch_BoundStreamQuiescent / MoveBoundStreamsInFlight / ExportBoundStreamsInFlight / ImportBoundStreamsInFlight /
BoundWrapperBlobBytes: exported by the product library, declared in the header, typed in the ctypes table, wrapped by Batch, and chosen
by shard.move_bound_streams (no GPU needed: symbols, prototypes and fakes only)."""
import ctypes as C
import importlib.util
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("BeatriceBatch_BoundStreamQuiescent", "BeatriceBatch_MoveBoundStreamsInFlight", "BeatriceBatch_ExportBoundStreamsInFlight",
       "BeatriceBatch_ImportBoundStreamsInFlight", "BeatriceBatch_BoundWrapperBlobBytes")


def test_the_library_exports_the_five_symbols(bv, product):
    for name in NEW:
        assert hasattr(product.lib, name), name


def test_the_header_declares_the_five_symbols():
    text = open(os.path.join(REPO, "include", "beatrice_batch.h")).read()
    assert "(13)" in text
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)   # declarations, not the comments that mention them
    ip = r"\s*const\s+int\s*\*\s*\w+\s*"
    bp = r"\s*BeatriceBatch\s*\*\s*\w+\s*"
    cbp = r"\s*const\s+BeatriceBatch\s*\*\s*\w+\s*"
    vp, cvp = r"\s*void\s*\*\s*\w+\s*", r"\s*const\s+void\s*\*\s*\w+\s*"
    n = r"\s*int\s+\w+\s*"
    assert re.search(r"\bint\s+BeatriceBatch_BoundStreamQuiescent\s*\(" + cbp + "," + n + r"\)\s*;", text)
    assert re.search(r"\bint\s+BeatriceBatch_MoveBoundStreamsInFlight\s*\(" + bp + "," + bp + "," + n + "," + ip + "," + ip + "," + ip + "," + n + r"\)\s*;", text)
    assert re.search(r"\bint\s+BeatriceBatch_ExportBoundStreamsInFlight\s*\(" + bp + "," + n + "," + ip + "," + vp + "," + vp + r"\)\s*;", text)
    assert re.search(r"\bint\s+BeatriceBatch_ImportBoundStreamsInFlight\s*\(" + bp + "," + n + "," + ip + "," + cvp + "," + cvp + "," + ip + "," + n + r"\)\s*;", text)
    assert re.search(r"\bsize_t\s+BeatriceBatch_BoundWrapperBlobBytes\s*\(" + cbp + r"\)\s*;", text)


def test_the_ctypes_table_types_the_five_symbols(bv):
    i32p = C.POINTER(C.c_int)
    assert bv._BATCH["BeatriceBatch_BoundStreamQuiescent"] == (C.c_int, [C.c_void_p, C.c_int])
    assert bv._BATCH["BeatriceBatch_MoveBoundStreamsInFlight"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, i32p, i32p, i32p, C.c_int])
    assert bv._BATCH["BeatriceBatch_ExportBoundStreamsInFlight"] == (C.c_int, [C.c_void_p, C.c_int, i32p, C.c_void_p, C.c_void_p])
    assert bv._BATCH["BeatriceBatch_ImportBoundStreamsInFlight"] == (C.c_int, [C.c_void_p, C.c_int, i32p, C.c_void_p, C.c_void_p, i32p, C.c_int])
    assert bv._BATCH["BeatriceBatch_BoundWrapperBlobBytes"] == (C.c_size_t, [C.c_void_p])
    assert set(NEW) <= set(bv.ABI_SYMBOLS_BATCH)
    for name in ("bound_stream_quiescent", "move_bound_streams_in_flight", "export_bound_streams_in_flight", "import_bound_streams_in_flight",
                 "bound_wrapper_blob_bytes"):
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

    def move_bound_streams_in_flight(self, dst, streams, dst_streams, entry_map=None):
        self.log.append(("move", dst, list(streams), list(dst_streams), entry_map))

    def export_bound_streams_in_flight(self, streams):
        self.log.append(("export", list(streams)))
        return b"blob", b"wrapper"

    def import_bound_streams_in_flight(self, streams, blobs, wrapper_blobs, entry_map=None):
        self.log.append(("import", list(streams), blobs, wrapper_blobs, entry_map))

    def BeatriceBatch_RestartStreamInFlight(self, h, s, rate, reset_model):
        self.log.append(("restart", h, s, rate, reset_model))
        return 0

    @staticmethod
    def _check(rc):
        assert rc == 0


def test_on_one_device_it_is_the_device_to_device_call(shard):
    src, dst = Fake(0), Fake(0)
    assert shard.move_bound_streams(src, [2, 0], dst, [1, 3], entry_map=[1, 0]) is None
    assert src.log == [("move", dst, [2, 0], [1, 3], [1, 0])] and dst.log == []


def test_across_devices_it_is_the_blob_pair(shard):
    src, dst = Fake(0), Fake(1)
    assert shard.move_bound_streams(src, [2, 0], dst, [1, 3], entry_map=[1, 0]) == (b"blob", b"wrapper")
    assert src.log == [("export", [2, 0])] and dst.log == [("import", [1, 3], b"blob", b"wrapper", [1, 0])]


@pytest.mark.parametrize("device", [0, 1])
def test_turn_over_source_restarts_the_source_slots_with_a_model_reset(shard, device):
    src, dst = Fake(0), Fake(device)
    shard.move_bound_streams(src, [2, 0], dst, [1, 3], turn_over_source=True)
    assert src.log[1:] == [("restart", 7, 2, 0.0, 1), ("restart", 7, 0, 0.0, 1)] and len(src.log) == 3
    assert not any(e[0] == "restart" for e in dst.log)


def test_unequal_lists_are_refused_before_anything_is_asked(shard):
    src, dst = Fake(0), Fake(0)
    with pytest.raises(ValueError):
        shard.move_bound_streams(src, [2, 0], dst, [1])
    assert src.log == [] and dst.log == []


def test_move_streams_still_refuses_the_wrapper_in_flight(shard):
    src, dst = Fake(0), Fake(0)
    with pytest.raises(ValueError):
        shard.move_streams(src, [2], dst, [0], with_wrapper=True, in_flight=True)
    assert src.log == [] and dst.log == []
