#!/usr/bin/env python3
"""What moving streams between two TICKING batches costs, by the three ways there are: the drained pair (shard.move_streams: both batches
drain, relevel and refill), the in-flight blob pair (BeatriceBatch_ExportStreamsInFlight / ImportStreamsInFlight) and the
device-to-device call (BeatriceBatch_MoveStreamsInFlight).

Two 256-stream batches in full tick mode (every stage holding a step) with the silent-block rule; the 16 streams that may move sit every
step out, so they are at rest while everyone else is busy -- the situation of a scheduler that consolidates batches.  Child processes,
each under its own `timeout` (after a child that faulted, hung or timed out nothing more is started):
  calls    wall time of one move of n = 1 and n = 16 streams by each way (the median of several; the first call of each way, which makes
           its staging, is made before the timing);
  run      frames per second of a 300-step run of both batches that moves 16 streams every 50 steps, one child per way (and one that
           moves nothing).
One JSON line per child, then a summary.

    python tools/stream_move_in_flight_timing.py [--hops 4] [--n 1 16] [--out FILE]
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
B, REPEATS, MOVERS, STEPS, EVERY = 256, 7, 16, 300, 50
FAULT_CODES = {124, 134, 137, 139}
WAYS = ("drained", "blobs", "device")


def load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def med(v):
    return round(statistics.median(v), 4)


def child(kind, H, ns):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import make_model
    from tick_driver import Resident
    bv = load("beatrice_vst_amd", os.path.join(REPO, "beatrice-vst_amd", "__init__.py"))
    shard = load("bv_shard", os.path.join(REPO, "beatrice-vst_amd", "shard.py"))
    product = bv.bind_batch(bv.load_product())
    movers = [(5 * i + 1) % B for i in range(MOVERS)]
    flags = np.zeros(B, np.uint8)
    flags[movers] = 1
    with tempfile.TemporaryDirectory() as d:
        make_model.make_model(d, n_speakers=3)
        m = bv.Models(product, d)
        res = {"kind": kind, "streams": B, "hops_per_step": H}
        src, dst = bv.Batch(m, B, hops_per_step=H), bv.Batch(m, B, hops_per_step=H)
        rs = rd = None
        try:
            rs, rd = Resident(bv, src, slots=64, tick=True), Resident(bv, dst, slots=64, tick=True)
            sig = np.stack([bv.synth_audio(160 * H * 64, seed=300 + s) for s in range(16)]).reshape(16, 64, H * 160)
            for r in (rs, rd):
                r.buf[:] = np.ascontiguousarray(sig[np.arange(B) % 16].transpose(1, 0, 2))
                r.hip.h2d(r.d_in, r.buf)
            stages = src.a.BeatriceBatch_TickStages(src.h)
            res["tick_stages"] = stages
            for batch in (src, dst):
                assert batch.a.BeatriceBatch_EnableSilentBlockRule(batch.h, 1) == 0

            def feed(batch, steps):
                for _ in range(steps):
                    assert batch.a.BeatriceBatch_SetSilentStreams(batch.h, flags.tobytes()) == 0
                    assert batch.a.BeatriceBatch_ConvertFramesDevice(batch.h, None, None) == 0

            def move(way, frm, to, n):
                if way == "drained":
                    shard.move_streams(frm, movers[:n], to, movers[:n])
                elif way == "blobs":
                    to.import_streams_in_flight(movers[:n], frm.export_streams_in_flight(movers[:n]))
                else:
                    frm.move_streams_in_flight(to, movers[:n], movers[:n])

            t_end = time.perf_counter() + 1.0   # device warm-up: a second of the batches' own steps, drained
            while time.perf_counter() < t_end:
                for batch in (src, dst):
                    feed(batch, stages + 2)
                    assert batch.a.BeatriceBatch_Synchronize(batch.h) == 0
            if kind == "calls":
                for n in ns:
                    row = {}
                    for way in WAYS:
                        move(way, src, dst, n)   # (staging, events and piece tables are made here)
                        ms = []
                        for i in range(REPEATS):
                            feed(src, stages + 2)   # both pipelines full, the movers at rest
                            feed(dst, stages + 2)
                            frm, to = (src, dst) if i % 2 == 0 else (dst, src)
                            t0 = time.perf_counter()
                            move(way, frm, to, n)
                            ms.append(1e3 * (time.perf_counter() - t0))
                        row[way + "_ms"] = med(ms)
                        row[way + "_ms_all"] = [round(v, 4) for v in ms]
                    res["n%d" % n] = row
            else:
                way = kind[len("run_"):]
                for batch in (src, dst):
                    assert batch.a.BeatriceBatch_Synchronize(batch.h) == 0
                t0 = time.perf_counter()
                for k in range(STEPS):
                    if way != "none" and k > 0 and k % EVERY == 0:
                        frm, to = (src, dst) if (k // EVERY) % 2 else (dst, src)
                        move(way, frm, to, MOVERS)
                    feed(src, 1)
                    feed(dst, 1)
                for batch in (src, dst):
                    assert batch.a.BeatriceBatch_Synchronize(batch.h) == 0
                wall = time.perf_counter() - t0
                res.update(steps=STEPS, moves=(STEPS - 1) // EVERY if way != "none" else 0, wall_ms=round(1e3 * wall, 2),
                           frames_per_s=round(2 * (B - MOVERS) * H * STEPS / wall, 1),
                           ticks=[int(b.a.BeatriceBatch_TicksLaunched(b.h)) for b in (src, dst)])
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
    for kind in ("calls", "run_none") + tuple("run_" + w for w in WAYS):
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
        if r["kind"] == "calls":
            for n in a.n:
                v = r["n%d" % n]
                print("n = %2d: drained %.3f ms, blob pair in flight %.3f ms, device to device %.3f ms" % (n, v["drained_ms"], v["blobs_ms"], v["device_ms"]))
        else:
            print("%-12s %d steps, %d moves of %d: %.1f frames/s (%.1f ms, ticks %s)" % (r["kind"], r["steps"], r["moves"], MOVERS, r["frames_per_s"],
                                                                                    r["wall_ms"], r["ticks"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
