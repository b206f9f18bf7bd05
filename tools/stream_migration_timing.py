#!/usr/bin/env python3
"""What moving streams between batches costs (BeatriceBatch_ExportStreams / BeatriceBatch_ImportStreams).

Three kinds of child process, each under its own `timeout` (after a child that faulted, hung or timed out nothing more is started):
  sizes    bytes of one stream's blob at 1, 2 and 4 hops per step, beside BeatriceBatch_StateBytes / B (the blob is that plus the previous
           bin, the 48 kHz wrapper's history, padding, and a header + settings part);
  drained  two 256-stream batches with nothing in flight: wall time of one Export and of one Import of n = 1 and n = 16 streams (the
           median of several calls; the first call, which allocates the staging pair, is made before the timing);
  ticks    the same calls on batches in full tick mode (every stage holding a step), where the call begins with the drain: beside it the
           wall time of a bare BeatriceBatch_Synchronize from the same full pipeline, so that the drain's share can be read off.
One JSON line per child, then a summary.

    python tools/stream_migration_timing.py [--hops 4] [--n 1 16] [--out FILE]
"""
import argparse
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, REPEATS = 256, 7
FAULT_CODES = {124, 134, 137, 139}


def load_pkg():
    spec = importlib.util.spec_from_file_location("beatrice_vst_amd", os.path.join(REPO, "beatrice-vst_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["beatrice_vst_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def med(v):
    return round(statistics.median(v), 4)


def child(kind, H, ns):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import make_model
    from tick_driver import Resident
    bv = load_pkg()
    product = bv.bind_batch(bv.load_product())
    with tempfile.TemporaryDirectory() as d:
        make_model.make_model(d, n_speakers=3)
        m = bv.Models(product, d)
        res = {"kind": kind, "streams": B}
        if kind == "sizes":
            for hh in (1, 2, 4):
                batch = bv.Batch(m, B, hops_per_step=hh)
                res["H%d" % hh] = {"blob_bytes": batch.stream_blob_bytes(),
                                   "state_bytes_per_stream": int(batch.a.BeatriceBatch_StateBytes(batch.h)) // B}
                batch.close()
        else:
            res["hops_per_step"] = H
            src, dst = bv.Batch(m, B, hops_per_step=H), bv.Batch(m, B, hops_per_step=H)
            rs = rd = None
            try:
                if kind == "ticks":
                    rs, rd = Resident(bv, src, slots=64, tick=True), Resident(bv, dst, slots=64, tick=True)
                    sig = np.stack([bv.synth_audio(160 * H * 64, seed=300 + s) for s in range(16)]).reshape(16, 64, H * 160)
                    for r in (rs, rd):
                        r.buf[:] = np.ascontiguousarray(sig[np.arange(B) % 16].transpose(1, 0, 2))
                        r.hip.h2d(r.d_in, r.buf)
                    stages = src.a.BeatriceBatch_TickStages(src.h)
                    res["tick_stages"] = stages

                    def fill(batch):
                        for _ in range(stages + 2):
                            assert batch.a.BeatriceBatch_ConvertFramesDevice(batch.h, None, None) == 0
                else:
                    x = np.zeros((B, H * 160), np.float32)
                    for batch in (src, dst):
                        batch.convert(x)

                    def fill(batch):
                        assert batch.a.BeatriceBatch_Synchronize(batch.h) == 0

                def timed(batch, call):
                    fill(batch)
                    t0 = time.perf_counter()
                    out = call()
                    return 1e3 * (time.perf_counter() - t0), out

                t_end = time.perf_counter() + 1.0   # device warm-up: a second of the batches' own steps, drained
                while time.perf_counter() < t_end:
                    for batch in (src, dst):
                        fill(batch)
                        assert batch.a.BeatriceBatch_Synchronize(batch.h) == 0
                if kind == "ticks":
                    res["drain_alone_ms"] = med([timed(src, lambda: src.a.BeatriceBatch_Synchronize(src.h))[0] for _ in range(REPEATS)])
                for n in ns:
                    streams = [(5 * i + 1) % B for i in range(n)]
                    blobs = src.export_streams(streams)   # (staging for min(n, 16) blobs is made here)
                    dst.import_streams(streams, blobs)
                    ex, im = [], []
                    for _ in range(REPEATS):
                        ms, blobs = timed(src, lambda: src.export_streams(streams))
                        ex.append(ms)
                        im.append(timed(dst, lambda: dst.import_streams(streams, blobs))[0])
                    res["n%d" % n] = {"export_ms": med(ex), "import_ms": med(im), "export_ms_all": [round(v, 4) for v in ex],
                                      "import_ms_all": [round(v, 4) for v in im], "bytes": len(blobs)}
            finally:
                for r in (rs, rd):
                    if r is not None:
                        r.free()
                src.close()
                dst.close()
        m.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--hops", type=int, default=4, help="hops per step of the timed batches")
    ap.add_argument("--n", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--timeout", type=int, default=150, help="seconds per child")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.hops, a.n)
    rows = []
    for kind in ("sizes", "drained", "ticks"):
        p = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", kind,
                            "--hops", str(a.hops), "--n"] + [str(n) for n in a.n], stdout=subprocess.PIPE, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode != 0 or not lines:
            print("%s: exit status %d -- stopping here" % (kind, p.returncode), flush=True)
            return 1 if (p.returncode in FAULT_CODES or p.returncode < 0) else 2
        print(lines[-1], flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(lines[-1] + "\n")
        rows.append(json.loads(lines[-1]))
    for r in rows:
        if r["kind"] == "sizes":
            for hh in (1, 2, 4):
                v = r["H%d" % hh]
                print("H = %d: blob %d bytes, state per stream %d bytes (+%d)" % (hh, v["blob_bytes"], v["state_bytes_per_stream"],
                                                                                 v["blob_bytes"] - v["state_bytes_per_stream"]))
        else:
            for n in a.n:
                v = r["n%d" % n]
                print("%-8s n = %2d: export %.3f ms, import %.3f ms%s" % (r["kind"], n, v["export_ms"], v["import_ms"],
                                                                        ", drain alone %.3f ms" % r["drain_alone_ms"] if "drain_alone_ms" in r else ""))
    return 0


if __name__ == "__main__":
    sys.exit(main())
