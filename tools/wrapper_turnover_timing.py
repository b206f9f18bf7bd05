#!/usr/bin/env python3
"""Host time of one BeatriceBatch_RestartStreamInFlight / SetStreamRateInFlight inside a binding with clocks per stream: the shape
bench.py times as clocks_per_stream_four_rates (256 streams at 44.1 / 48 / 96 / 32 kHz, 10 ms blocks, cells of 960 samples), the
pipeline full.  The calls neither launch nor wait, so what is timed is the host clock around the call itself, between two calls of
BeatriceBatch_ProcessBlocksRaggedDevice:
  known rate   BeatriceBatch_RestartStreamInFlight(s, 0.0, 0): a few stores
  turn-over    the same with reset_model = 1: + the marks of BeatriceBatch_ResetStreamInFlight and BeatriceBatch_FlushSpeaker's tile rebuild
               (the first one also builds the in-flight reset's ring table: reported apart)
  held rate    BeatriceBatch_SetStreamRateInFlight to a rate another stream is on
  new rate     BeatriceBatch_SetStreamRateInFlight to a rate the binding has no class for: the rate's two tap tables are computed (32 hi + 1
               sinc / Hann values each), placed, and go up with one async copy; the first of them replaces the tap buffer by a longer one
One JSON line.

    python tools/wrapper_turnover_timing.py
"""
import ctypes as C
import importlib.util
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, CAP = 256, 960
RATES = [(44100.0, 441), (48000.0, 480), (96000.0, 960), (32000.0, 320)]
NEW = [37800.0, 44056.0, 47952.0, 50000.0, 64000.0, 88200.0, 176400.0, 192000.0]   # (none needs more hops per call than 32 kHz does)


def load_pkg():
    spec = importlib.util.spec_from_file_location("beatrice_vst_amd", os.path.join(REPO, "beatrice-vst_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["beatrice_vst_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import make_model
    from tick_driver import Hip
    bv = load_pkg()
    product = bv.bind_batch(bv.load_product())
    hip = Hip()
    with tempfile.TemporaryDirectory() as d:
        make_model.make_model(d, n_speakers=3)
        m = bv.Models(product, d)
        batch = bv.Batch(m, B)
        a, h = batch.a, batch.h
        assert a.BeatriceBatch_FlushSpeaker(h, -1) == 0
        assert a.BeatriceBatch_ConfigureWrapperRates(h, (C.c_double * B)(*[RATES[s % 4][0] for s in range(B)])) == 0
        stages = a.BeatriceBatch_TickStages(h)
        slots = stages + 8
        nbytes = slots * B * CAP * 4
        d_in, d_out = hip.malloc(nbytes), hip.malloc(nbytes)
        assert hip.lib.hipMemset(d_in, 0, C.c_size_t(nbytes)) == 0
        assert a.BeatriceBatch_BindResidentBlocksRagged(h, d_in, d_out, 1, CAP, slots) == 0
        ns = (C.c_int * B)(*[RATES[s % 4][1] for s in range(B)])

        def calls(k):
            for _ in range(k):
                assert a.BeatriceBatch_ProcessBlocksRaggedDevice(h, ns) == 0

        def timed(fn, *args):
            calls(2)   # (the pipeline stays full; every timed call stands between two calls)
            t0 = time.perf_counter()
            rc = fn(h, *args)
            dt = 1e6 * (time.perf_counter() - t0)
            assert rc == 0, (args, rc)
            return dt

        calls(stages + 4)
        res = {"streams": B, "tick_stages": stages}
        known = [timed(a.BeatriceBatch_RestartStreamInFlight, 4 * i, 0.0, 0) for i in range(21)]
        first_turn = timed(a.BeatriceBatch_RestartStreamInFlight, 1, 0.0, 1)
        turn = [timed(a.BeatriceBatch_RestartStreamInFlight, 4 * i + 1, 0.0, 1) for i in range(1, 22)]
        held = [timed(a.BeatriceBatch_SetStreamRateInFlight, 4 * i + 2, 48000.0) for i in range(21)]
        fresh = [timed(a.BeatriceBatch_SetStreamRateInFlight, 4 * i + 3, rate) for i, rate in enumerate(NEW)]
        ticks = a.BeatriceBatch_TicksLaunched(h)
        assert a.BeatriceBatch_RestartStreamInFlight(h, 0, 0.0, 0) == 0
        assert a.BeatriceBatch_TicksLaunched(h) == ticks
        assert a.BeatriceBatch_Synchronize(h) == 0
        med = lambda v: round(statistics.median(v), 2)   # noqa: E731
        res.update({"known_rate_us": med(known), "known_rate_us_min_max": [round(min(known), 2), round(max(known), 2)],
                    "turn_over_us": med(turn), "turn_over_us_min_max": [round(min(turn), 2), round(max(turn), 2)], "first_turn_over_us": round(first_turn, 2),
                    "held_rate_us": med(held), "held_rate_us_min_max": [round(min(held), 2), round(max(held), 2)],
                    "new_rate_us": {str(rate): round(us, 2) for rate, us in zip(NEW, fresh)}, "new_rate_us_median": med(fresh)})
        assert a.BeatriceBatch_BindResidentBlocksRagged(h, None, None, 0, 0, 0) == 0
        batch.close()
        m.close()
        hip.free(d_in)
        hip.free(d_out)
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
