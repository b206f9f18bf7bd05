"""Cost of moving streams between two bindings with clocks per stream without a drain (BeatriceBatch_MoveBoundStreamsInFlight and the
blob pair), beside the drained route it replaces: Synchronize, unbind, ExportStreams / ExportStreamWrappers, ImportStreams /
ImportStreamWrappers, bind again -- the only way the state of a stream in mode P could change batch before.

Two batches of --streams streams at 48 kHz / 480-sample blocks; the upper half of each runs a call before every timed move so that the
tick pipeline is full, the lower half never hands in a block and is at rest.  Prints one JSON line.

  python tools/bound_stream_move_timing.py [--streams 64] [--repeats 30]"""
import argparse
import ctypes as C
import importlib.util
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=30)
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("beatrice_vst_amd", os.path.join(REPO, "beatrice-vst_amd", "__init__.py"))
    bv = importlib.util.module_from_spec(spec)
    sys.modules["beatrice_vst_amd"] = bv
    spec.loader.exec_module(bv)
    import make_model
    from tick_driver import Hip

    d = tempfile.mkdtemp(prefix="bound_move_model")
    make_model.make_model(d, n_speakers=3)
    product = bv.bind_batch(bv.load_product())
    models = bv.Models(product, d)
    hip = Hip()
    B, n, slots = a.streams, 480, 64
    i32 = lambda v: (C.c_int * len(v))(*v)   # noqa: E731

    class Side:
        def __init__(self):
            self.batch = bv.Batch(models, B)
            self.a, self.h = self.batch.a, self.batch.h
            self.bytes = slots * B * n * 4
            self.d_in, self.d_out = hip.malloc(self.bytes), hip.malloc(self.bytes)
            x = (0.1 * np.random.default_rng(1).standard_normal(slots * B * n)).astype(np.float32)
            hip.h2d(self.d_in, x)
            assert self.a.BeatriceBatch_ConfigureWrapperRates(self.h, (C.c_double * B)(*([48000.0] * B))) == 0
            self.bind()
            self.ns = i32([0] * (B // 2) + [n] * (B - B // 2))

        def bind(self):
            assert self.a.BeatriceBatch_BindResidentBlocksRagged(self.h, self.d_in, self.d_out, 1, n, slots) == 0

        def unbind(self):
            assert self.a.BeatriceBatch_BindResidentBlocksRagged(self.h, None, None, 0, 0, 0) == 0

        def call(self):
            assert self.a.BeatriceBatch_ProcessBlocksRaggedDevice(self.h, self.ns) == 0

    src, dst = Side(), Side()
    delay = src.a.BeatriceBatch_ResidentBlocksDelay(src.h)
    for _ in range(delay + 4):
        src.call()
        dst.call()
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert hip.lib.hipEventCreate(C.byref(ev0)) == 0 and hip.lib.hipEventCreate(C.byref(ev1)) == 0
    dst_stream = C.c_void_p(src.a.BeatriceBatch_GetStream(dst.h))
    res = {"streams_per_batch": B, "delay_calls": delay, "repeats": a.repeats}

    def timed(fn, device=True):
        host, dev = [], []
        for _ in range(a.repeats):
            src.call()
            dst.call()
            if device:
                assert hip.lib.hipEventRecord(ev0, dst_stream) == 0
            t0 = time.perf_counter()
            fn()
            host.append((time.perf_counter() - t0) * 1e6)
            if device:
                assert hip.lib.hipEventRecord(ev1, dst_stream) == 0 and hip.lib.hipEventSynchronize(ev1) == 0
                ms = C.c_float(0)
                assert hip.lib.hipEventElapsedTime(C.byref(ms), ev0, ev1) == 0
                dev.append(ms.value * 1e3)
        out = {"host_us_median": round(statistics.median(host), 1), "host_us_min": round(min(host), 1), "host_us_max": round(max(host), 1)}
        if device:
            out["device_us_median"] = round(statistics.median(dev), 1)
        return out

    for k in (1, 16):
        idx = i32(list(range(k)))
        res["move_%d" % k] = timed(lambda: src.batch._check(src.a.BeatriceBatch_MoveBoundStreamsInFlight(src.h, dst.h, k, idx, idx, None, 0)))

        def pair(k=k):
            sb, wb = src.batch.export_bound_streams_in_flight(list(range(k)))
            dst.batch.import_bound_streams_in_flight(list(range(k)), sb, wb)
        res["blob_pair_%d" % k] = timed(pair)

        def drained(k=k):
            streams = list(range(k))
            assert src.a.BeatriceBatch_Synchronize(src.h) == 0 and dst.a.BeatriceBatch_Synchronize(dst.h) == 0
            src.unbind()
            dst.unbind()
            sb, wb = src.batch.export_streams(streams), src.batch.export_stream_wrappers(streams)
            dst.batch.import_streams(streams, sb)
            dst.batch.import_stream_wrappers(streams, wb)
            src.bind()
            dst.bind()
        res["drained_%d" % k] = timed(drained, device=False)
        for _ in range(delay + 4):   # (the drained route leaves both pipelines empty: refill before the next measurement)
            src.call()
            dst.call()
    assert src.a.BeatriceBatch_Synchronize(src.h) == 0 and dst.a.BeatriceBatch_Synchronize(dst.h) == 0
    print(json.dumps(res))


if __name__ == "__main__":
    main()
