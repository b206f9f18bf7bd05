#!/usr/bin/env python3
"""What putting new voices into a running batch costs a server in tick mode: 256 streams, four hops per step, the pipeline full, n = 1, 8
and the per-call cap of table entries written at once.

For every n, in a child process of its own (each under its own `timeout`; after a child that faulted, hung or timed out nothing more
is started):
  (i)   HIP-event time of the launches of ONE BeatriceBatch_InstallSpeakersInFlight call of n entries, between two events on the batch's
        stream with the pipeline full (the stream runs in order, so the ticks queued in front of the first event are not counted);
  (ii)  host time inside that call (the copy into pinned staging and the two launches), the median of several calls;
  (iii) wall time of 20 steps + drain with one such call before step 10;
  (iv)  the same with n drained BeatriceBatch_UpdateSpeaker calls instead (--drained-lib: another build of the library, e.g. the parent
        commit's, which has no in-flight call) -- their drain and the refill of the pipeline are inside the figure;
and, measured in the same child, the time of one full tick launch (BeatriceBatch_TimeTickLaunch) and the wall time of 20 steps + drain
with no call at all, so that every figure can be read as a multiple of a tick.  One JSON line per child, then a summary table.

    python tools/install_in_flight_timing.py [--drained-lib PATH] [--n 1 8 16] [--out FILE]
"""
import argparse
import ctypes as C
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
N_REAL, B, H, STEPS, CALL_AT, REPEATS = 8, 256, 4, 20, 10, 5
FAULT_CODES = {124, 134, 137, 139}


def load_pkg():
    spec = importlib.util.spec_from_file_location("beatrice_vst_amd", os.path.join(REPO, "beatrice-vst_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["beatrice_vst_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def child(n, how):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import make_model
    from tick_driver import Resident
    bv = load_pkg()
    product = bv.bind_batch(bv.load_product())
    with tempfile.TemporaryDirectory() as d:
        make_model.make_model(d, n_speakers=N_REAL)
        m = bv.Models(product, d)
        t = m.tables
        batch = bv.Batch(m, B, max_speakers=N_REAL + n, hops_per_step=H)
        a, h = batch.a, batch.h
        # the voices: the model's own speakers' tables, rotated; no stream is ever moved onto the entries, so they stay free
        pick = (np.arange(n) + 1) % N_REAL
        cb, add, kv = (np.ascontiguousarray(x[pick]) for x in (t.codebooks, t.additive, t.kv))
        entries = np.arange(N_REAL, N_REAL + n, dtype=np.int32)
        for s in range(B):
            assert a.BeatriceBatch_SetTargetSpeaker(h, s, s % N_REAL) == 0
        assert a.BeatriceBatch_FlushSpeaker(h, -1) == 0
        r = Resident(bv, batch, slots=64, tick=True)
        try:
            sig = np.stack([bv.synth_audio(160 * H * 64, seed=300 + s) for s in range(16)]).reshape(16, 64, H * 160)
            r.buf[:] = np.ascontiguousarray(sig[np.arange(B) % 16].transpose(1, 0, 2))
            r.hip.h2d(r.d_in, r.buf)

            def steps(k):
                for _ in range(k):
                    assert a.BeatriceBatch_ConvertFramesDevice(h, None, None) == 0

            def sync():
                assert a.BeatriceBatch_Synchronize(h) == 0

            def install():
                if how == "inflight":
                    rc = a.BeatriceBatch_InstallSpeakersInFlight(h, n, bv.iptr(entries), bv.fptr(cb), bv.fptr(add), bv.fptr(kv))
                    assert rc == 0, rc
                else:
                    for i in range(n):
                        rc = a.BeatriceBatch_UpdateSpeaker(h, int(entries[i]), bv.fptr(cb[i]), bv.fptr(add[i]), bv.fptr(kv[i]))
                        assert rc == 0, rc

            t_end = time.perf_counter() + 1.0   # device warm-up as bench.py's: a second of the workload's own steps, drained
            while time.perf_counter() < t_end:
                steps(64)
                sync()
            stages = a.BeatriceBatch_TickStages(h)
            steps(stages + 2)
            us, fl, by = C.c_float(0), C.c_double(0), C.c_double(0)
            for _ in range(3):
                assert a.BeatriceBatch_TimeTickLaunch(h, 64, C.byref(us), C.byref(fl), C.byref(by)) == 0
            sync()
            res = {"n": n, "how": how, "library": os.path.relpath(product.path, REPO),
                   "streams": B, "hops_per_step": H, "tick_stages": stages, "tick_launch_us": round(us.value, 2)}

            def wall(call):
                sync()
                t0 = time.perf_counter()
                steps(CALL_AT)
                if call is not None:
                    call()
                steps(STEPS - CALL_AT)
                sync()
                return 1e3 * (time.perf_counter() - t0)

            install()   # (the first call allocates the staging ring)
            sync()
            res["wall_ms_20_steps_no_call"] = round(min(wall(None) for _ in range(REPEATS)), 4)
            if how == "inflight":   # (i), (ii): the pipeline full, the call between a pair of events on the batch's stream
                hip = r.hip.lib
                stream = C.c_void_p(a.BeatriceBatch_GetStream(h))
                e0, e1 = C.c_void_p(), C.c_void_p()
                assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
                dev, host = [], []
                for _ in range(REPEATS):
                    sync()
                    steps(stages + 2)
                    assert hip.hipEventRecord(e0, stream) == 0
                    t0 = time.perf_counter()
                    install()
                    host.append(1e3 * (time.perf_counter() - t0))
                    assert hip.hipEventRecord(e1, stream) == 0
                    assert hip.hipEventSynchronize(e1) == 0
                    ms = C.c_float(0)
                    assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
                    dev.append(ms.value)
                res["call_device_ms"] = round(statistics.median(dev), 4)
                res["call_device_ms_all"] = [round(x, 4) for x in dev]
                res["call_host_ms"] = round(statistics.median(host), 4)
                res["call_host_ms_all"] = [round(x, 4) for x in host]
                hip.hipEventDestroy(e0)
                hip.hipEventDestroy(e1)
            walls = [wall(install) for _ in range(REPEATS)]
            res["wall_ms_20_steps_one_install"] = round(min(walls), 4)
            res["wall_ms_20_steps_one_install_all"] = [round(x, 4) for x in walls]
            res["ticks_launched"] = a.BeatriceBatch_TicksLaunched(h)
            r.leave()
        finally:
            r.free()
        batch.close()
        m.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, nargs="+", default=[1, 8, 16])
    ap.add_argument("--drained-lib", default=None, help="library for the drained runs (default: the same build)")
    ap.add_argument("--timeout", type=int, default=150, help="seconds per child")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--child", nargs=2, metavar=("N", "HOW"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(int(a.child[0]), a.child[1])
    rows = []
    for n in a.n:
        for how in ("inflight", "drained"):
            env = dict(os.environ)
            if how == "drained" and a.drained_lib:
                env["BEATRICE_HIP_LIB"] = os.path.abspath(a.drained_lib)
            p = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", str(n), how],
                               env=env, stdout=subprocess.PIPE, text=True)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
            if p.returncode != 0 or not lines:
                print("n = %d, %s: exit status %d -- stopping here" % (n, how, p.returncode), flush=True)
                return 1 if (p.returncode in FAULT_CODES or p.returncode < 0) else 2
            print(lines[-1], flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(lines[-1] + "\n")
            rows.append(json.loads(lines[-1]))
    print("%4s %9s %10s %14s %14s %14s %16s" % ("n", "how", "tick us", "(i) device ms", "(ii) host ms", "20 steps ms", "with install ms"))
    for r in rows:
        print("%4d %9s %10.1f %14s %14s %14.3f %16.3f" % (r["n"], r["how"], r["tick_launch_us"], r.get("call_device_ms", "-"), r.get("call_host_ms", "-"),
                                                       r["wall_ms_20_steps_no_call"], r["wall_ms_20_steps_one_install"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
