#!/usr/bin/env python3
"""What a new voice costs a server in the wrapper modes around the ticks: 256 streams, F (BindResidentIO48k, four hops per step) and P
(BindResidentBlocksRagged, four rates, 10 ms blocks), the pipeline full, ONE BeatriceBatch_InstallSpeakersInFlight call of one entry.

For every mode and library, in a child process of its own (each under its own `timeout`; after a child that faulted, hung or timed out
nothing more is started):
  (i)   host time inside the call, the median of several calls;
  (ii)  the gap the call leaves on the batch's stream: HIP-event time between an event recorded in front of the call and one behind it,
        with the pipeline full (the stream runs in order, so the work queued in front of the first event is not counted; where the call
        drains, the drain's ticks and the wait are inside the figure);
  (iii) wall time of 40 calls + a final synchronisation with one install before call 20, and with none.
--drained-lib names another build of the library (the parent commit's, in which the call drains in F and P) for a second set of children.

    python tools/speaker_in_flight_wrapper_timing.py [--drained-lib PATH] [--modes F P] [--out FILE]
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
N_REAL, B, CALLS, CALL_AT, REPEATS = 8, 256, 40, 20, 5
RATES = [16000.0, 44100.0, 48000.0, 96000.0]
FAULT_CODES = {124, 134, 137, 139}


def load_pkg():
    spec = importlib.util.spec_from_file_location("beatrice_vst_amd", os.path.join(REPO, "beatrice-vst_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["beatrice_vst_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def child(mode, label):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import make_model
    from tick_driver import Hip
    bv = load_pkg()
    product = bv.bind_batch(bv.load_product())
    H = 4 if mode == "F" else 1
    with tempfile.TemporaryDirectory() as d:
        make_model.make_model(d, n_speakers=N_REAL)
        m = bv.Models(product, d)
        t = m.tables
        batch = bv.Batch(m, B, max_speakers=N_REAL + 1, hops_per_step=H)
        a, h = batch.a, batch.h
        cb, add, kv = (np.ascontiguousarray(x[1:2]) for x in (t.codebooks, t.additive, t.kv))
        entries = np.array([N_REAL], np.int32)      # no stream is ever moved onto the entry, so it stays free
        for s in range(B):
            assert a.BeatriceBatch_SetTargetSpeaker(h, s, s % N_REAL) == 0
        assert a.BeatriceBatch_FlushSpeaker(h, -1) == 0
        stages = a.BeatriceBatch_TickStages(h)
        hip = Hip()
        rng = np.random.default_rng(5)
        if mode == "F":
            slots = 64
            buf = (0.1 * rng.standard_normal((slots, B, H, 1, 480))).astype(np.float32)
            d_in, d_out = hip.malloc(buf.nbytes), hip.malloc(buf.nbytes)
            hip.h2d(d_in, buf)
            assert a.BeatriceBatch_BindResidentIO48k(h, d_in, d_out, 1, slots) == 0
            step = lambda: a.BeatriceBatch_ConvertBlocks48kDevice(h, None, None, 1)   # noqa: E731
        else:
            rates = [RATES[s % 4] for s in range(B)]
            ns = (C.c_int * B)(*[int(r / 100) for r in rates])
            cap, slots = 960, 3 * stages
            buf = (0.1 * rng.standard_normal((slots, B, cap))).astype(np.float32)
            d_in, d_out = hip.malloc(buf.nbytes), hip.malloc(buf.nbytes)
            hip.h2d(d_in, buf)
            assert a.BeatriceBatch_ConfigureWrapperRates(h, (C.c_double * B)(*rates)) == 0
            assert a.BeatriceBatch_BindResidentBlocksRagged(h, d_in, d_out, 1, cap, slots) == 0
            step = lambda: a.BeatriceBatch_ProcessBlocksRaggedDevice(h, ns)   # noqa: E731

        def steps(k):
            for _ in range(k):
                assert step() == 0

        def sync():
            assert a.BeatriceBatch_Synchronize(h) == 0

        def install():
            rc = a.BeatriceBatch_InstallSpeakersInFlight(h, 1, bv.iptr(entries), bv.fptr(cb), bv.fptr(add), bv.fptr(kv))
            assert rc == 0, rc

        t_end = time.perf_counter() + 1.0   # device warm-up: a second of the workload's own calls, drained
        while time.perf_counter() < t_end:
            steps(32)
            sync()
        install()   # (the first call allocates the staging ring)
        sync()
        res = {"mode": mode, "library": label, "streams": B, "hops_per_step": H, "tick_stages": stages}

        def wall(call):
            sync()
            t0 = time.perf_counter()
            steps(CALL_AT)
            if call is not None:
                call()
            steps(CALLS - CALL_AT)
            sync()
            return 1e3 * (time.perf_counter() - t0)

        res["wall_ms_40_calls_no_install"] = round(min(wall(None) for _ in range(REPEATS)), 4)
        stream = C.c_void_p(a.BeatriceBatch_GetStream(h))
        e0, e1 = C.c_void_p(), C.c_void_p()
        assert hip.lib.hipEventCreate(C.byref(e0)) == 0 and hip.lib.hipEventCreate(C.byref(e1)) == 0
        gap, host, moved = [], [], []
        for _ in range(REPEATS):
            sync()
            steps(stages + 2)
            before = a.BeatriceBatch_TicksLaunched(h)
            assert hip.lib.hipEventRecord(e0, stream) == 0
            t0 = time.perf_counter()
            install()
            host.append(1e3 * (time.perf_counter() - t0))
            assert hip.lib.hipEventRecord(e1, stream) == 0
            assert hip.lib.hipEventSynchronize(e1) == 0
            moved.append(a.BeatriceBatch_TicksLaunched(h) - before)
            ms = C.c_float(0)
            assert hip.lib.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
            gap.append(ms.value)
        res["call_host_ms"] = round(statistics.median(host), 4)
        res["call_host_ms_all"] = [round(x, 4) for x in host]
        res["stream_gap_ms"] = round(statistics.median(gap), 4)
        res["stream_gap_ms_all"] = [round(x, 4) for x in gap]
        res["ticks_launched_by_the_call"] = moved
        walls = [wall(install) for _ in range(REPEATS)]
        res["wall_ms_40_calls_one_install"] = round(min(walls), 4)
        res["wall_ms_40_calls_one_install_all"] = [round(x, 4) for x in walls]
        hip.lib.hipEventDestroy(e0)
        hip.lib.hipEventDestroy(e1)
        sync()
        batch.close()
        m.close()
        hip.free(d_in)
        hip.free(d_out)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--modes", nargs="+", default=["F", "P"])
    ap.add_argument("--drained-lib", default=None, help="a second library (the parent commit's build) for a second set of children")
    ap.add_argument("--timeout", type=int, default=120, help="seconds per child")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--child", nargs=2, metavar=("MODE", "LABEL"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1])
    rows = []
    for mode in a.modes:
        for label in ("this build", "drained-lib") if a.drained_lib else ("this build",):
            env = dict(os.environ)
            if label == "drained-lib":
                env["BEATRICE_HIP_LIB"] = os.path.abspath(a.drained_lib)
            p = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", mode, label],
                               env=env, stdout=subprocess.PIPE, text=True)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
            if p.returncode != 0 or not lines:
                print("%s, %s: exit status %d -- stopping here" % (mode, label, p.returncode), flush=True)
                return 1 if (p.returncode in FAULT_CODES or p.returncode < 0) else 2
            print(lines[-1], flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(lines[-1] + "\n")
            rows.append(json.loads(lines[-1]))
    print("%4s %12s %13s %14s %16s %18s %8s" % ("mode", "library", "(i) host ms", "(ii) gap ms", "40 calls ms", "with install ms", "ticks"))
    for r in rows:
        print("%4s %12s %13.4f %14.4f %16.3f %18.3f %8s" % (r["mode"], r["library"], r["call_host_ms"], r["stream_gap_ms"],
                                                            r["wall_ms_40_calls_no_install"], r["wall_ms_40_calls_one_install"],
                                                            r["ticks_launched_by_the_call"][0]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
