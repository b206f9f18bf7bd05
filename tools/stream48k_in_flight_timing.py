#!/usr/bin/env python3
"""What a stream's reset and a stream's move cost around the resident 48 kHz blocks (mode F, BeatriceBatch_BindResidentIO48k), nothing
drained (BeatriceBatch_ResetStreamInFlight; BeatriceBatch_ExportStreams48kInFlight / ImportStreams48kInFlight / MoveStreams48kInFlight).

Child processes, each under its own `timeout` (after a child that faulted, hung or timed out nothing more is started):
  reset    64 stereo streams, four blocks per step: a run of 240 steps with BeatriceBatch_ResetStreamInFlight of one stream every 20
           steps, and the same run without; wall time and ticks launched of both, the difference per reset.  With --parent-lib the
           same child once more on that build (there the call in F is the drained reset), for the comparison.
  calls    two 256-stream batches, the silent-block rule on, the 16 streams that may move sitting every step out (at rest while everyone
           else is busy): wall time of one move of n = 1 and n = 16 streams by the blob pair and device to device (the median of
           several; the first call of each way, which makes its staging, is made before the timing) -- the situation and the sizes of
           tools/stream_move_in_flight_timing.py, whose figures for plain tick mode stand beside these.
One JSON line per child, then a summary.

    python tools/stream48k_in_flight_timing.py [--parent-lib PATH] [--n 1 16] [--out FILE]
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
REPEATS, MOVERS = 7, 16
RESET_B, RESET_H, RESET_STEPS, RESET_EVERY = 64, 4, 240, 20
FAULT_CODES = {124, 134, 137, 139}


def load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


class Bound:
    """a batch bound to `slots` resident 48 kHz slots filled once with sounding material"""

    def __init__(self, bv, hip, batch, channels, slots):
        import wrapperlib
        self.batch, self.hip, self.ch = batch, hip, channels
        B, H = batch.B, batch.H
        n = slots * B * H * channels * 480
        self.d_in, self.d_out = hip.malloc(4 * n), hip.malloc(4 * n)
        sig = np.stack([wrapperlib.test_signal(480 * 64, 48000, seed=400 + s) for s in range(16)]).astype(np.float32)
        buf = np.resize(sig[np.arange(B) % 16], (B, H * channels * 480 * slots)).reshape(B, slots, H * channels * 480)
        hip.h2d(self.d_in, np.ascontiguousarray(buf.transpose(1, 0, 2)))
        assert batch.a.BeatriceBatch_BindResidentIO48k(batch.h, self.d_in, self.d_out, channels, slots) == 0

    def feed(self, steps, flags=None):
        a, h = self.batch.a, self.batch.h
        for _ in range(steps):
            if flags is not None:
                assert a.BeatriceBatch_SetSilentStreams(h, flags) == 0
            assert a.BeatriceBatch_ConvertBlocks48kDevice(h, None, None, self.ch) == 0

    def sync(self):
        assert self.batch.a.BeatriceBatch_Synchronize(self.batch.h) == 0

    def free(self):
        self.hip.free(self.d_in)
        self.hip.free(self.d_out)


def child(kind, ns):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import make_model
    from tick_driver import Hip
    bv = load("beatrice_vst_amd", os.path.join(REPO, "beatrice-vst_amd", "__init__.py"))
    product = bv.bind_batch(bv.load_product())
    hip = Hip()
    with tempfile.TemporaryDirectory() as d:
        make_model.make_model(d, n_speakers=3)
        m = bv.Models(product, d)
        res = {"kind": kind, "lib": os.environ.get("BEATRICE_HIP_LIB", "this build")}
        bound = []
        try:
            if kind == "reset":
                batch = bv.Batch(m, RESET_B, hops_per_step=RESET_H)
                ln = Bound(bv, hip, batch, 2, 64)
                bound.append(ln)
                stages = batch.a.BeatriceBatch_TickStages(batch.h)
                t_end = time.perf_counter() + 1.0   # device warm-up
                while time.perf_counter() < t_end:
                    ln.feed(stages + 2)
                    ln.sync()
                rows = {}
                for with_resets in (False, True, False, True, False, True):
                    ln.sync()
                    t0_ticks = batch.a.BeatriceBatch_TicksLaunched(batch.h)
                    t0 = time.perf_counter()
                    for k in range(RESET_STEPS):
                        if with_resets and k % RESET_EVERY == RESET_EVERY // 2:
                            assert batch.a.BeatriceBatch_ResetStreamInFlight(batch.h, (7 * k) % RESET_B) == 0
                        ln.feed(1)
                    ticks = batch.a.BeatriceBatch_TicksLaunched(batch.h) - t0_ticks   # (before the final drain)
                    ln.sync()
                    rows.setdefault(with_resets, []).append((1e3 * (time.perf_counter() - t0), int(ticks)))
                n_resets = RESET_STEPS // RESET_EVERY
                plain, reset = (statistics.median(w for w, _ in rows[v]) for v in (False, True))
                res.update(streams=RESET_B, hops_per_step=RESET_H, channels=2, tick_stages=stages, steps=RESET_STEPS, resets=n_resets,
                           wall_ms_without=round(plain, 3), wall_ms_with=round(reset, 3), us_per_reset=round(1e3 * (reset - plain) / n_resets, 1),
                           ticks_without=rows[False][0][1], ticks_with=rows[True][0][1],
                           ticks_added_per_reset=round((rows[True][0][1] - rows[False][0][1]) / n_resets, 2),
                           wall_ms_all={"without": [round(w, 3) for w, _ in rows[False]], "with": [round(w, 3) for w, _ in rows[True]]})
            else:
                B, H = 256, 4
                movers = [(5 * i + 1) % B for i in range(MOVERS)]
                flags = np.zeros(B, np.uint8)
                flags[movers] = 1
                flags = flags.tobytes()
                src, dst = (Bound(bv, hip, bv.Batch(m, B, hops_per_step=H), 2, 48) for _ in range(2))
                bound += [src, dst]
                stages = src.batch.a.BeatriceBatch_TickStages(src.batch.h)
                for ln in (src, dst):
                    assert ln.batch.a.BeatriceBatch_EnableSilentBlockRule(ln.batch.h, 1) == 0
                t_end = time.perf_counter() + 1.0
                while time.perf_counter() < t_end:
                    for ln in (src, dst):
                        ln.feed(stages + 2, flags)
                        ln.sync()

                def move(way, frm, to, n):
                    if way == "blobs":
                        to.batch.import_streams48k_in_flight(movers[:n], frm.batch.export_streams48k_in_flight(movers[:n]))
                    else:
                        frm.batch.move_streams48k_in_flight(to.batch, movers[:n], movers[:n])
                res.update(streams=B, hops_per_step=H, channels=2, tick_stages=stages, blob_bytes=src.batch.stream_blob_bytes())
                for n in ns:
                    row = {}
                    for way in ("blobs", "device"):
                        src.feed(stages + 2, flags)
                        dst.feed(stages + 2, flags)
                        move(way, src, dst, n)   # (staging, events and piece tables are made here)
                        ms = []
                        for i in range(REPEATS):
                            src.feed(stages + 2, flags)   # both pipelines full, the movers at rest
                            dst.feed(stages + 2, flags)
                            frm, to = (src, dst) if i % 2 == 0 else (dst, src)
                            t0 = time.perf_counter()
                            move(way, frm, to, n)
                            ms.append(1e3 * (time.perf_counter() - t0))
                        row[way + "_ms"] = round(statistics.median(ms), 4)
                        row[way + "_ms_all"] = [round(v, 4) for v in ms]
                    res["n%d" % n] = row
                for ln in (src, dst):
                    ln.sync()
        finally:
            for ln in bound:
                ln.batch.close()
                ln.free()
        m.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--parent-lib", default=None, help="a build of the parent commit's library: the `reset` child once more on it")
    ap.add_argument("--timeout", type=int, default=150, help="seconds per child")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.n)
    runs = [("reset", None), ("calls", None)] + ([("reset", a.parent_lib)] if a.parent_lib else [])
    for kind, lib in runs:
        env = dict(os.environ)
        if lib:
            env["BEATRICE_HIP_LIB"] = os.path.abspath(lib)
        p = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", kind, "--n"] + [str(n) for n in a.n],
                           stdout=subprocess.PIPE, text=True, env=env)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode != 0 or not lines:
            print("%s: exit status %d -- stopping here" % (kind, p.returncode), flush=True)
            return 1 if (p.returncode in FAULT_CODES or p.returncode < 0) else 2
        print(lines[-1], flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(lines[-1] + "\n")
        r = json.loads(lines[-1])
        if kind == "reset":
            print("reset (%s): %d resets in %d steps: %.1f us and %.2f ticks added per reset (%.2f ms against %.2f ms)" % (
                r["lib"], r["resets"], r["steps"], r["us_per_reset"], r["ticks_added_per_reset"], r["wall_ms_with"], r["wall_ms_without"]), flush=True)
        else:
            for n in a.n:
                v = r["n%d" % n]
                print("n = %2d: blob pair in flight %.3f ms, device to device %.3f ms" % (n, v["blobs_ms"], v["device_ms"]), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
