#!/usr/bin/env python3
"""What moving morph weights costs a server in tick mode: 256 streams, four hops per step, n = 1, 16, 64 table entries moved at once.

For every n, in a child process of its own (each under its own `timeout`; after a child that faulted, hung or timed out nothing more
is started):
  (i)   HIP-event time of the device work of ONE BeatriceBatch_MorphSpeakersInFlight call of n entries (an empty pipeline around it);
  (ii)  wall time of 20 steps + drain with one such call before step 10;
  (iii) the same with n drained BeatriceBatch_MorphSpeakerStaged calls instead (--drained-lib: another build of the library, e.g. the
        parent commit's, which has no in-flight call);
and, measured in the same child, the time of one full tick launch (BeatriceBatch_TimeTickLaunch) and the wall time of 20 steps + drain
with no morph at all, so that every figure can be read as a multiple of a tick.  One JSON line per child, then a summary table.

    python tools/morph_in_flight_timing.py [--drained-lib PATH] [--n 1 16 64] [--out FILE]
"""
import argparse
import ctypes as C
import importlib.util
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_REAL, B, H, STEPS, CALL_AT = 8, 256, 4, 20, 10
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
    rng = np.random.Generator(np.random.PCG64(4242))
    with tempfile.TemporaryDirectory() as d:
        make_model.make_model(d, n_speakers=N_REAL)
        m = bv.Models(product, d)
        batch = bv.Batch(m, B, max_speakers=N_REAL + 2 * n, hops_per_step=H)
        a, h = batch.a, batch.h
        w = rng.random((3, n, N_REAL)).astype(np.float32) + np.float32(0.05)
        sets = [list(range(N_REAL, N_REAL + n)), list(range(N_REAL + n, N_REAL + 2 * n))]
        for s in range(B):
            assert a.BeatriceBatch_SetTargetSpeaker(h, s, s % N_REAL) == 0
        for i, e in enumerate(sets[0]):   # stream i morphs on entry sets[0][i]; the timed calls move it to and fro between the two sets
            assert a.BeatriceBatch_MorphSpeaker(h, e, bv.fptr(np.ascontiguousarray(w[0, i])), N_REAL, 7) == 0
            assert a.BeatriceBatch_SetTargetSpeaker(h, i, e) == 0
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

            def move(slots, froms, wts):
                if how == "inflight":
                    rc = a.BeatriceBatch_MorphSpeakersInFlight(h, n, bv.iptr(np.array(slots, np.int32)), bv.iptr(np.array(froms, np.int32)),
                                                               bv.fptr(np.ascontiguousarray(wts)), N_REAL, 7)
                    assert rc == 0, rc
                else:
                    for i in range(n):
                        rc = a.BeatriceBatch_MorphSpeakerStaged(h, slots[i], froms[i], bv.fptr(np.ascontiguousarray(wts[i])), N_REAL, 7)
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

            res["wall_ms_20_steps_no_morph"] = round(min(wall(None) for _ in range(3)), 4)
            if how == "inflight":   # (i): the call's two launches between a pair of events on the batch's stream, nothing else in flight
                hip = r.hip.lib
                stream = C.c_void_p(a.BeatriceBatch_GetStream(h))
                e0, e1 = C.c_void_p(), C.c_void_p()
                assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
                sync()
                assert hip.hipEventRecord(e0, stream) == 0
                move(sets[1], sets[0], w[1])
                assert hip.hipEventRecord(e1, stream) == 0
                assert hip.hipEventSynchronize(e1) == 0
                ms = C.c_float(0)
                assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
                res["call_device_ms"] = round(ms.value, 4)
                hip.hipEventDestroy(e0)
                hip.hipEventDestroy(e1)
            else:
                move(sets[1], sets[0], w[1])
            steps(8)   # the moved streams install their new blocks (eight hops), then the drain frees the entries they left
            sync()
            res["wall_ms_20_steps_one_move"] = round(wall(lambda: move(sets[0], sets[1], w[2])), 4)
            res["ticks_launched"] = a.BeatriceBatch_TicksLaunched(h)
            r.leave()
        finally:
            r.free()
        batch.close()
        m.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, nargs="+", default=[1, 16, 64])
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
    print("%4s %9s %10s %14s %14s %14s" % ("n", "how", "tick us", "(i) call ms", "20 steps ms", "with a move ms"))
    for r in rows:
        print("%4d %9s %10.1f %14s %14.3f %14.3f" % (r["n"], r["how"], r["tick_launch_us"], r.get("call_device_ms", "-"),
                                                    r["wall_ms_20_steps_no_morph"], r["wall_ms_20_steps_one_move"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
