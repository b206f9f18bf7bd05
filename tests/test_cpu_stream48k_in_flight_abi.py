"""BeatriceBatch_Stream48kQuiescent / ExportStreams48kInFlight / ImportStreams48kInFlight / MoveStreams48kInFlight: exported by the product
library, declared in the header with footnote (14), typed in the ctypes table, wrapped by Batch, refused without a GPU for NULL and
unhealthy batches, and chosen by shard.move_streams(in_flight=True) when both batches convert resident 48 kHz blocks (no GPU needed:
symbols, prototypes and fakes only)."""
import ctypes as C
import importlib.util
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("BeatriceBatch_Stream48kQuiescent", "BeatriceBatch_ExportStreams48kInFlight", "BeatriceBatch_ImportStreams48kInFlight",
       "BeatriceBatch_MoveStreams48kInFlight")


def test_the_library_exports_the_four_symbols(bv, product):
    for name in NEW:
        assert hasattr(product.lib, name), name


def test_the_header_declares_the_four_symbols_and_the_footnotes():
    text = open(os.path.join(REPO, "include", "beatrice_batch.h")).read()
    assert "(14)" in text and "F still is not" not in text
    note12 = text[text.index("(12) not rows"):text.index("(13) not rows")]
    assert "(14)" in note12   # (12) now points at the calls that serve F
    reset = text[text.index("The same reset as a per-stream SETTING"):text.index("int BeatriceBatch_ResetStreamInFlight")]
    assert re.search(r"every other mode \(A, B, C, S, G, P\)", re.sub(r"\s*\n \*\s*", " ", reset))   # F is no longer among the modes that drain
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)   # declarations, not the comments that mention them
    ip = r"\s*const\s+int\s*\*\s*\w+\s*"
    bp = r"\s*BeatriceBatch\s*\*\s*\w+\s*"
    assert re.search(r"\bint\s+BeatriceBatch_Stream48kQuiescent\s*\(\s*const\s+BeatriceBatch\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+BeatriceBatch_ExportStreams48kInFlight\s*\(" + bp + r",\s*int\s+\w+\s*," + ip + r",\s*void\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+BeatriceBatch_ImportStreams48kInFlight\s*\(" + bp + r",\s*int\s+\w+\s*," + ip + r",\s*const\s+void\s*\*\s*\w+\s*,"
                     + ip + r",\s*int\s+\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+BeatriceBatch_MoveStreams48kInFlight\s*\(" + bp + "," + bp + r",\s*int\s+\w+\s*," + ip + "," + ip + "," + ip
                     + r",\s*int\s+\w+\s*\)\s*;", text)


def test_the_ctypes_table_types_the_four_symbols(bv):
    i32p = C.POINTER(C.c_int)
    assert bv._BATCH["BeatriceBatch_Stream48kQuiescent"] == (C.c_int, [C.c_void_p, C.c_int])
    assert bv._BATCH["BeatriceBatch_ExportStreams48kInFlight"] == (C.c_int, [C.c_void_p, C.c_int, i32p, C.c_void_p])
    assert bv._BATCH["BeatriceBatch_ImportStreams48kInFlight"] == (C.c_int, [C.c_void_p, C.c_int, i32p, C.c_void_p, i32p, C.c_int])
    assert bv._BATCH["BeatriceBatch_MoveStreams48kInFlight"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, i32p, i32p, i32p, C.c_int])
    assert set(NEW) <= set(bv.ABI_SYMBOLS_BATCH)
    for name in ("stream48k_quiescent", "export_streams48k_in_flight", "import_streams48k_in_flight", "move_streams48k_in_flight"):
        assert callable(getattr(bv.Batch, name))


def test_null_and_unhealthy_batches_are_refused_without_a_gpu(bv, product):
    """NULL: -1 from the getter and the move, -2 (no healthy batch) from the blob pair, like their siblings in plain tick mode.  A batch
    created from NULL models is not healthy: refused as well, and nothing is touched."""
    a = bv.bind_batch(product)
    one = (C.c_int * 1)(0)
    buf = C.create_string_buffer(64)
    assert a.BeatriceBatch_Stream48kQuiescent(None, 0) == -1
    assert a.BeatriceBatch_ExportStreams48kInFlight(None, 1, one, C.cast(buf, C.c_void_p)) == a.BeatriceBatch_ExportStreamsInFlight(None, 1, one, C.cast(buf, C.c_void_p))
    assert a.BeatriceBatch_ExportStreams48kInFlight(None, 1, one, C.cast(buf, C.c_void_p)) < 0
    assert a.BeatriceBatch_ImportStreams48kInFlight(None, 1, one, C.cast(buf, C.c_void_p), None, 0) < 0
    assert a.BeatriceBatch_MoveStreams48kInFlight(None, None, 1, one, one, None, 0) == -1
    objs = (a.CreatePhoneExtractor(), a.CreatePitchEstimator(), a.CreateWaveformGenerator(), a.CreateEmbeddingSetter())
    sick = a.BeatriceBatch_Create(*objs, 2, 2)   # models that were never read: without a device the batch is not healthy
    try:
        if not a.BeatriceBatch_IsHealthy(sick):
            assert a.BeatriceBatch_Stream48kQuiescent(sick, 0) == -1
            assert a.BeatriceBatch_ExportStreams48kInFlight(sick, 1, one, C.cast(buf, C.c_void_p)) < 0
            assert a.BeatriceBatch_ImportStreams48kInFlight(sick, 1, one, C.cast(buf, C.c_void_p), None, 0) < 0
            assert a.BeatriceBatch_MoveStreams48kInFlight(sick, None, 1, one, one, None, 0) == -1
            assert a.BeatriceBatch_MoveStreams48kInFlight(sick, sick, 1, one, one, None, 0) == -1   # src == dst
            assert buf.raw == b"\0" * 64
    finally:
        a.BeatriceBatch_Destroy(sick)
        for obj, fn in zip(objs, (a.DestroyPhoneExtractor, a.DestroyPitchEstimator, a.DestroyWaveformGenerator, a.DestroyEmbeddingSetter)):
            fn(obj)


@pytest.fixture(scope="module")
def shard():
    spec = importlib.util.spec_from_file_location("bv_shard_48k_abi", os.path.join(REPO, "beatrice-vst_amd", "shard.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Fake:
    """A batch that records what is asked of it; `device` is what BeatriceBatch_Device answers, `around48k` whether it is in mode F
    (the one mode in which BeatriceBatch_Stream48kQuiescent answers 0 or 1)."""

    def __init__(self, device, around48k):
        self.log, self.device, self.around48k = [], device, around48k
        self.a, self.h = self, 7 + device

    def BeatriceBatch_Device(self, h):
        return self.device

    def BeatriceBatch_Stream48kQuiescent(self, h, s):
        return 1 if self.around48k else -1

    def export_streams_in_flight(self, streams):
        self.log.append(("export_in_flight", list(streams)))
        return b"blob"

    def import_streams_in_flight(self, streams, blobs, entry_map=None):
        self.log.append(("import_in_flight", list(streams), blobs, entry_map))

    def move_streams_in_flight(self, dst, streams, dst_streams, entry_map=None):
        self.log.append(("move_in_flight", dst, list(streams), list(dst_streams), entry_map))

    def export_streams48k_in_flight(self, streams):
        self.log.append(("export48k_in_flight", list(streams)))
        return b"blob48k"

    def import_streams48k_in_flight(self, streams, blobs, entry_map=None):
        self.log.append(("import48k_in_flight", list(streams), blobs, entry_map))

    def move_streams48k_in_flight(self, dst, streams, dst_streams, entry_map=None):
        self.log.append(("move48k_in_flight", dst, list(streams), list(dst_streams), entry_map))

    def BeatriceBatch_ResetStreamInFlight(self, h, s):
        self.log.append(("reset_in_flight", h, s))
        return 0

    @staticmethod
    def _check(rc):
        assert rc == 0


def test_two_batches_around_48k_blocks_on_one_device_take_the_48k_move(shard):
    src, dst = Fake(0, True), Fake(0, True)
    assert shard.move_streams(src, [2, 0], dst, [1, 3], entry_map=[1, 0], reset_source=True, in_flight=True) is None
    assert src.log == [("move48k_in_flight", dst, [2, 0], [1, 3], [1, 0]), ("reset_in_flight", 7, 2), ("reset_in_flight", 7, 0)] and dst.log == []


def test_two_batches_around_48k_blocks_across_devices_take_the_48k_blob_pair(shard):
    src, dst = Fake(0, True), Fake(1, True)
    assert shard.move_streams(src, [2], dst, [1], in_flight=True) == b"blob48k"
    assert src.log == [("export48k_in_flight", [2])] and dst.log == [("import48k_in_flight", [1], b"blob48k", None)]


@pytest.mark.parametrize("src_f,dst_f", [(False, False), (True, False), (False, True)])
def test_plain_and_mixed_modes_ask_the_plain_calls_as_before(shard, src_f, dst_f):
    """(one batch in each mode: the plain calls are asked and the library refuses them, as before)"""
    src, dst = Fake(0, src_f), Fake(0, dst_f)
    shard.move_streams(src, [2], dst, [0], in_flight=True)
    assert src.log == [("move_in_flight", dst, [2], [0], None)] and dst.log == []
