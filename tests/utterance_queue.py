"""Continuous batching of utterances on one tick-mode batch (test helper and measurement script, not a test file).

A seeded list of utterances (16 kHz float, different lengths, each with its own target speaker) goes through the streams of a batch
in plain tick mode over resident I/O: a stream takes the next utterance from the queue when its current one ends (the last step padded
with zeros to H hops), every new utterance starts with BeatriceBatch_SetTargetSpeaker + BeatriceBatch_ResetStreamInFlight, streams with
nothing left sit the steps out (the silent-block rule's flags), and every utterance's 24 kHz output is collected from the slots
BeatriceBatch_TickStages() - 1 steps later.  in_flight=False uses the drained BeatriceBatch_ResetStream instead (the comparison).

As a script: python tests/utterance_queue.py --streams 256 --hops-per-step 4 --utterances 2000 --min-hops 100 --max-hops 600 [--drained]
prints one JSON line with frames/s, steps, ticks launched and the host's time per step."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tick_driver import Hip  # noqa: E402


def make_queue(bv, n, min_hops, max_hops, n_speakers, seed=1):
    """[(audio [hops * 160], speaker)], seeded; cheap noise for long queues, bv.synth_audio for short ones."""
    rng = np.random.default_rng(seed)
    q = []
    for i in range(n):
        hops = int(rng.integers(min_hops, max_hops + 1))
        if n <= 64:
            audio = bv.synth_audio(160 * hops, seed=seed * 1000 + i)
        else:
            audio = (0.1 * rng.standard_normal(160 * hops)).astype(np.float32)
        q.append((np.ascontiguousarray(audio, np.float32), int(rng.integers(0, n_speakers))))
    return q


def run_queue(bv, batch, queue, in_flight=True, collect=True):
    """-> (outputs: one [hops * 240] array per utterance (None unless collect), stats dict)"""
    a, h, B, H = batch.a, batch.h, batch.B, batch.H
    hip = Hip()
    stages = a.BeatriceBatch_TickStages(h)
    slots, chunk = 2 * stages + 8, stages + 4   # a step's input slot stays untouched for `stages` further steps; outputs are read before they are overwritten
    d_in, d_out = hip.malloc(slots * B * H * 160 * 4), hip.malloc(slots * B * H * 240 * 4)
    reset = a.BeatriceBatch_ResetStreamInFlight if in_flight else a.BeatriceBatch_ResetStream
    outputs = [np.zeros(len(x) // 160 * 240, np.float32) if collect else None for x, _ in queue]
    cur = [None] * B           # per stream: [utterance, hops done]
    nxt, done_utts = 0, 0
    where = {}                 # step -> [(stream, utterance, first hop, hops)]
    fed, collected, host_s, resets = 0, 0, 0.0, 0
    buf = np.zeros((slots, B, H * 160), np.float32)
    out = np.zeros((slots, B, H * 240), np.float32)
    try:
        assert a.BeatriceBatch_BindResidentIO(h, d_in, d_out, slots) == 0
        assert a.BeatriceBatch_EnableTickPipeline(h, 1) == 0
        assert a.BeatriceBatch_EnableSilentBlockRule(h, 1) == 0
        stream = a.BeatriceBatch_GetStream(h)

        def gather(upto):   # the steps below `upto` have left the pipeline
            nonlocal collected
            if collected >= upto:
                return
            hip.d2h(out, d_out)
            for u in range(collected, upto):
                for s, i, h0, n in where.pop(u):
                    if collect:
                        outputs[i][h0 * 240:(h0 + n) * 240] = out[u % slots, s, :n * 240]
            collected = upto

        t_start = time.perf_counter()
        while done_utts < len(queue):
            plan = []   # this chunk's steps: (new utterances [(stream, speaker)], flags)
            for j in range(chunk):
                starts, flags, rows = [], bytearray(B), []
                for s in range(B):
                    if cur[s] is None and nxt < len(queue):
                        cur[s] = [nxt, 0]
                        starts.append((s, queue[nxt][1]))
                        nxt += 1
                    if cur[s] is None:
                        flags[s] = 1
                        buf[(fed + j) % slots, s] = 0.0
                        continue
                    i, h0 = cur[s]
                    x = queue[i][0]
                    n = min(H, len(x) // 160 - h0)
                    row = buf[(fed + j) % slots, s]
                    row[:n * 160] = x[h0 * 160:(h0 + n) * 160]
                    row[n * 160:] = 0.0
                    rows.append((s, i, h0, n))
                    cur[s][1] += n
                    if cur[s][1] >= len(x) // 160:
                        cur[s] = None
                        done_utts += 1
                if not rows:
                    break
                where[fed + j] = rows
                plan.append((starts, bytes(flags)))
            hip.h2d(d_in, buf)
            t0 = time.perf_counter()
            for starts, flags in plan:
                for s, spk in starts:
                    assert a.BeatriceBatch_SetTargetSpeaker(h, s, spk) == 0
                    assert reset(h, s) == 0
                    resets += 1
                if any(flags):
                    assert a.BeatriceBatch_SetSilentStreams(h, flags) == 0
                assert a.BeatriceBatch_ConvertFramesDevice(h, None, None) == 0
            host_s += time.perf_counter() - t0
            fed += len(plan)
            assert hip.lib.hipStreamSynchronize(C.c_void_p(stream)) == 0   # waits for the ticks enqueued; drains nothing
            gather(max(0, fed - (stages - 1)))
        ticks = a.BeatriceBatch_TicksLaunched(h)
        assert a.BeatriceBatch_Synchronize(h) == 0   # the final drain
        ticks_end = a.BeatriceBatch_TicksLaunched(h)
        elapsed = time.perf_counter() - t_start
        gather(fed)
        assert a.BeatriceBatch_EnableTickPipeline(h, 0) == 0
        assert a.BeatriceBatch_EnableSilentBlockRule(h, 0) == 0
        assert a.BeatriceBatch_BindResidentIO(h, None, None, 0) == 0
    finally:
        hip.free(d_in)
        hip.free(d_out)
    hops = sum(len(x) // 160 for x, _ in queue)
    stats = dict(in_flight=bool(in_flight), streams=B, hops_per_step=H, utterances=len(queue), hops=hops, steps=fed, resets=resets,
                 ticks_before_final_drain=int(ticks), ticks=int(ticks_end), tick_stages=int(stages), seconds=elapsed,
                 frames_per_s=hops / elapsed, host_work_us_per_step=1e6 * host_s / max(fed, 1))
    return outputs, stats


def main():
    import argparse
    import importlib.util
    import tempfile
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--hops-per-step", type=int, default=4)
    ap.add_argument("--utterances", type=int, default=2000)
    ap.add_argument("--min-hops", type=int, default=100)
    ap.add_argument("--max-hops", type=int, default=600)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--drained", action="store_true", help="BeatriceBatch_ResetStream instead of BeatriceBatch_ResetStreamInFlight")
    args = ap.parse_args()
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("beatrice_vst_amd", os.path.join(repo, "beatrice-vst_amd", "__init__.py"))
    bv = importlib.util.module_from_spec(spec)
    sys.modules["beatrice_vst_amd"] = bv
    spec.loader.exec_module(bv)
    sys.path.insert(0, os.path.join(repo, "tools"))
    import make_model
    with tempfile.TemporaryDirectory() as d:
        make_model.make_model(d, n_speakers=3)
        m = bv.Models(bv.load_product(), d)
        batch = bv.Batch(m, args.streams, hops_per_step=args.hops_per_step)
        queue = make_queue(bv, args.utterances, args.min_hops, args.max_hops, 3, seed=args.seed)
        _, stats = run_queue(bv, batch, queue, in_flight=not args.drained, collect=False)
        batch.close()
        m.close()
    print(json.dumps(stats))


if __name__ == "__main__":
    main()
