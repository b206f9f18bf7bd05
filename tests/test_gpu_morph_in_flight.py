"""BeatriceBatch_MorphSpeakersInFlight: many morph entries in one call, and in tick mode / host streaming without draining the pipeline
(csrc/morph.hip sph_mean_batched_kernel + morph_project_kernel; csrc/batch.hip entry_busy).  Everything at max-abs 0: the batched
kernels against the single-entry ones (BeatriceBatch_MorphSpeaker), a TWIN batch on which the same script uses the drained
BeatriceBatch_MorphSpeaker / BeatriceBatch_MorphSpeakerStaged one call per entry, and reference streams driven through the reference's
timeline with the embeddings read back from the device."""
import numpy as np
import pytest

from test_gpu_morph_device import model_dir8  # noqa: F401  (fixture: the 8-speaker synthetic model)
from tick_driver import Resident

pytestmark = pytest.mark.gpu

SHAPES = [(7, 70, 1), (7, 70, 2), (40, 64, 4)]
N, S, SEED = 8, 16, 77           # real speakers, table entries (8 + 8), lottery seed
KNN_STREAM, SILENT_STREAM, SIT_OUT = 1, 1, (30, 31, 32)

# the four weight vectors of test_morphed_embeddings_match_host, and one with every weight below the 0.01 threshold (no active point)
W_HOST = np.array([[0.2, 0.5, 0.3, 0, 0, 0, 0, 0],
                   [0.05, 0.3, 0.005, 0.2, 0.1, 0.15, 0.1, 0.1],
                   [0, 0, 0, 1.0, 0, 0, 0, 0],
                   [0.125] * 8,
                   [0.005] * 8], np.float32)
W_A = np.array([[0.5, 0.0, 0.3, 0.2, 0, 0, 0, 0], [0.1, 0.0, 0.45, 0.0, 0.25, 0.2, 0, 0], [0, 0.25, 0, 0.25, 0, 0.25, 0, 0.25]], np.float32)   # step 5
W_B = np.array([[0.0, 0.6, 0.0, 0.0, 0.1, 0.3, 0, 0], [0.7, 0.0, 0.0, 0.0, 0.0, 0.0, 0.2, 0.1]], np.float32)                             # step 12
W_C = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.5, 0.5]], np.float32)                                                                # step 14
W_D = np.array([[0.3, 0.3, 0.0, 0.0, 0.4, 0.0, 0.0, 0.0]], np.float32)                                                                # the reuse of entry 8


def i32(v):
    return np.ascontiguousarray(v, np.int32)


class Api:
    """What a script sees: morph(slots, from_slots, weights) as ONE in-flight call, or as the drained single-entry calls one per entry."""

    def __init__(self, bv, batch, how):
        self.bv, self.a, self.h, self.B, self.how = bv, batch.a, batch.h, batch.B, how

    def morph(self, slots, froms, w):
        bv, a, h = self.bv, self.a, self.h
        w = np.ascontiguousarray(w, np.float32)
        if self.how == "inflight":
            return a.BeatriceBatch_MorphSpeakersInFlight(h, len(slots), bv.iptr(i32(slots)), bv.iptr(i32(froms)), bv.fptr(w), w.shape[1], SEED)
        for i, (slot, frm) in enumerate(zip(slots, froms)):
            wi = np.ascontiguousarray(w[i])
            rc = (a.BeatriceBatch_MorphSpeaker(h, slot, bv.fptr(wi), w.shape[1], SEED) if frm < 0 else
                  a.BeatriceBatch_MorphSpeakerStaged(h, slot, frm, bv.fptr(wi), w.shape[1], SEED))
            assert rc == 0, (slot, frm, rc)
        return 0

    def busy(self, e):
        return self.a.BeatriceBatch_SpeakerEntryBusy(self.h, e)

    def move(self, streams, speakers):
        assert self.a.BeatriceBatch_SetTargetSpeakers(self.h, len(streams), self.bv.iptr(i32(streams)), self.bv.iptr(i32(speakers))) == 0


def inputs(bv, B, steps, H, seed=9700):
    return np.stack([bv.synth_audio(160 * H * steps, seed=seed + s) for s in range(B)]).reshape(B, steps, H * 160).copy()


def settings(api, knn=True):
    for s in range(api.B):
        assert api.a.BeatriceBatch_SetTargetSpeaker(api.h, s, s % N) == 0
    if knn:
        assert api.a.BeatriceBatch_SetVQNumNeighbors(api.h, KNN_STREAM, 2) == 0
    assert api.a.BeatriceBatch_FlushSpeaker(api.h, -1) == 0


def script(api, k, reuse_at):
    """Streams 0, 1, 2 morph: 0 over entries 8 -> 11 -> 13, 1 (the k-NN stream) over 9 -> 12, 2 on 10 and, once entry 8 is free, on 8 again."""
    if k == 5:
        assert api.morph([8, 9, 10], [-1, -1, -1], W_A) == 0
        api.move([0, 1, 2], [8, 9, 10])
    if k == 12:
        assert api.morph([11, 12], [8, 9], W_B) == 0
    if k == 14:
        assert api.morph([13], [11], W_C) == 0     # restarts stream 0's four-hop wait
    if k == 20 and api.how == "inflight":
        assert api.morph([8], [10], W_D) == -3      # (the twin never asks)
    if k == reuse_at:
        assert api.morph([8], [10], W_D) == 0


def last_step_naming(entry, H, steps):
    """The last step in which stream 0 -- the only stream ever on entry 8 before its reuse -- names `entry`, from the reference's
    per-hop protocol (processor_core_2.cc:51-177, 179-181): one pending key/value block installed per hop once the wait is over."""
    target, add, kv, count, delay, last = 0, 0, [0] * 4, 4, 0, -1
    for k in range(steps):
        if k == 5:
            target, add, count, delay = 8, 8, 0, 0
        if k in (12, 14):
            target = add = {12: 11, 14: 13}[k]
            count, delay = 0, 4
        for _ in range(H):
            if delay > 0:
                delay -= 1
            elif count < 4:
                kv[count] = target
                count += 1
            if entry in [target, add] + kv:
                last = k
    return last


def run_script(bv, product, model_dir, B, steps, H, how, rule=False, knn=True, reuse_at=None, read_entries=()):
    """-> dict(out [steps][B][H * 240], ticks before the final drain, polls {step: SpeakerEntryBusy(8) before it}, reuse_at, stages, emb)"""
    x = inputs(bv, B, steps, H)
    m = bv.Models(product, model_dir)
    batch = bv.Batch(m, B, max_speakers=S, hops_per_step=H)
    a, h = batch.a, batch.h
    api = Api(bv, batch, how)
    settings(api, knn)
    r = Resident(bv, batch, slots=steps + 2, tick=True)
    res = dict(polls={}, reuse_at=reuse_at, stages=a.BeatriceBatch_TickStages(h), emb={})
    try:
        if rule:
            assert a.BeatriceBatch_EnableSilentBlockRule(h, 1) == 0
        for k in range(steps):
            r.buf[k] = x[:, k]
        r.hip.h2d(r.d_in, r.buf)
        for k in range(steps):
            if how == "inflight":
                res["polls"][k] = api.busy(8)
                if k > 20 and res["reuse_at"] is None and res["polls"][k] == 0:
                    res["reuse_at"] = k
            script(api, k, res["reuse_at"])
            if rule and k in SIT_OUT:
                assert a.BeatriceBatch_SetSilentStreams(h, bytes(1 if s == SILENT_STREAM else 0 for s in range(B))) == 0
            assert a.BeatriceBatch_ConvertFramesDevice(h, None, None) == 0
        res["ticks"] = a.BeatriceBatch_TicksLaunched(h)
        assert a.BeatriceBatch_Synchronize(h) == 0
        out = np.zeros((r.slots, B, H * 240), np.float32)
        r.hip.d2h(out, r.d_out)
        res["out"] = out[:steps].copy()
        if read_entries:
            # entry 8 was rewritten on the way: its first contents once more, into a free entry (the kernels are deterministic)
            assert api.morph([14], [-1], W_A[:1]) == 0
            for e in read_entries:
                add, kv = np.zeros(bv.HID, np.float32), np.zeros((bv.KV_LEN, bv.KV_CH), np.float32)
                assert a.BeatriceBatch_GetSpeakerEmbeddings(h, e, bv.fptr(add), bv.fptr(kv)) == 0
                res["emb"][e] = (add, kv)
        r.leave()
    finally:
        r.free()
    batch.close()
    m.close()
    return res


def differing(got, want, streams, steps, absent=None):
    return [(s, k, float(np.abs(got[k, s] - want[k, s]).max())) for s in streams for k in range(steps)
            if not (absent and k in absent.get(s, ())) and not np.array_equal(got[k, s], want[k, s])]


def test_one_call_computes_what_five_single_entry_calls_compute(bv, product, model_dir8):
    """In-order mode (the call drains like the single-entry ones): embeddings of every entry and 12 hops of streams placed on them."""
    B, hops = 6, 12
    slots = [8, 9, 10, 11, 12]
    audio = inputs(bv, B, hops, 1, seed=9900)
    m = bv.Models(product, model_dir8)

    def run(how):
        batch = bv.Batch(m, B, max_speakers=S)
        a, h = batch.a, batch.h
        api = Api(bv, batch, how)
        assert api.morph(slots, [-1] * 5, W_HOST) == 0
        emb = []
        for e in slots:
            add, kv = np.zeros(bv.HID, np.float32), np.zeros((bv.KV_LEN, bv.KV_CH), np.float32)
            assert a.BeatriceBatch_GetSpeakerEmbeddings(h, e, bv.fptr(add), bv.fptr(kv)) == 0
            emb.append((add, kv))
        api.move(list(range(5)), slots)                      # stream 5 stays on a real speaker
        assert a.BeatriceBatch_SetVQNumNeighbors(h, 1, 2) == 0
        assert a.BeatriceBatch_FlushSpeaker(h, -1) == 0
        out = np.stack([batch.convert(np.ascontiguousarray(audio[:, k])) for k in range(hops)])
        batch.close()
        return emb, out

    emb, out = run("inflight")
    emb1, out1 = run("drained")
    m.close()
    for e, (x, y) in zip(slots, zip(emb, emb1)):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]), "entry %d: max-abs %g / %g" % (
            e, float(np.abs(x[0] - y[0]).max()), float(np.abs(x[1] - y[1]).max()))
    assert np.abs(emb[0][1]).max() > 0.1 and not emb[4][0].any() and not emb[4][1].any()   # (no active point: zeros)
    assert np.abs(out1).max() > 0.05
    assert np.array_equal(out, out1), "12 hops on the entries: max-abs %g" % float(np.abs(out - out1).max())


@pytest.mark.parametrize("rule", [False, True], ids=["plain", "silent-rule"])
@pytest.mark.parametrize("B,steps,H", SHAPES)
def test_morphs_in_flight_equal_the_drained_twin(bv, product, model_dir8, B, steps, H, rule):
    got = run_script(bv, product, model_dir8, B, steps, H, "inflight", rule=rule)
    assert got["reuse_at"] is not None, "entry 8 never became free: %s" % got["polls"]
    twin = run_script(bv, product, model_dir8, B, steps, H, "drained", rule=rule, reuse_at=got["reuse_at"])
    absent = {SILENT_STREAM: set(SIT_OUT)} if rule else None
    assert np.abs(twin["out"]).max() > 0.05
    print("in flight vs the drained twin: max-abs %g; entry 8 reused before step %d" % (float(np.abs(got["out"] - twin["out"]).max()), got["reuse_at"]))
    bad = differing(got["out"], twin["out"], range(B), steps, absent)
    assert not bad, "in flight vs the drained twin, (stream, step, max-abs): %s" % bad[:12]
    # nothing drained: as many tick launches as steps fed; every drained call costs more
    assert got["ticks"] == steps
    assert twin["ticks"] > steps
    # entry 8 stays busy while the last step that named it is inside the pipeline, and not much longer
    last, stages, polls = last_step_naming(8, H, steps), got["stages"], got["polls"]
    assert last >= 13 and all(polls[k] == 1 for k in range(5 + 1, last + 1))   # (named by stream 0's settings)
    assert all(polls[k] == 1 for k in range(last + 1, last + stages)), "busy for TickStages() - 1 steps after step %d: %s" % (last, polls)
    assert got["reuse_at"] <= last + stages + 1, "free no later than TickStages() + 1 steps after step %d: %s" % (last, polls)


def test_morphs_in_flight_follow_the_reference_timeline(bv, oracle, product, model_dir8):
    """k-NN off (no lottery in the way): one reference stream per morphing stream, driven through the reference's protocol
    (processor_core_2.cc:51-177) with the embeddings the device computed -- additive embedding on the hop of the call, the old key/value
    blocks for four more hops, then one new block per hop; a call inside the wait restarts it."""
    B, steps, H = SHAPES[0]
    got = run_script(bv, product, model_dir8, B, steps, H, "inflight", knn=False, read_entries=(8, 9, 10, 11, 12, 13, 14))
    emb, reuse_at = got["emb"], got["reuse_at"]
    assert reuse_at is not None
    # stream -> [(step, entry whose embeddings arrive, staged?)]; 14 holds entry 8's first contents
    plan = {0: [(5, 14, False), (12, 11, True), (14, 13, True)], 1: [(5, 9, False), (12, 12, True)], 2: [(5, 10, False), (reuse_at, 8, True)]}
    x = inputs(bv, B, steps, H)
    mo = bv.Models(oracle, model_dir8)
    for s, events in plan.items():
        st = bv.Stream1(mo, speaker=s % N, vq_k=0)
        register_at = None
        for k in range(steps):
            for at, e, staged in events:
                if at != k:
                    continue
                st.a.SetAdditiveSpeakerEmbedding(mo.embed, bv.fptr(emb[e][0]), st.ec, st.wc)
                register_at = (k + 4 if staged else k, e)
            if register_at is not None and register_at[0] == k:   # Stream1.hop installs one block per hop from here
                st.a.RegisterKeyValueSpeakerEmbedding(mo.embed, bv.fptr(emb[register_at[1]][1]), st.ec)
                st.kv_count = 0
                register_at = None
            want = st.hop(x[s, k])
            assert np.array_equal(got["out"][k, s], want), "stream %d step %d vs the reference timeline: max-abs %g" % (
                s, k, float(np.abs(got["out"][k, s] - want).max()))
        st.close()
    mo.close()
    assert np.abs(got["out"][:, :3]).max() > 0.05


def test_morphs_in_flight_in_host_streaming(bv, product, model_dir8):
    """Mode E: the step-5 and step-12 actions between BeatriceBatch_StreamFrames calls, against an in-order twin with the drained calls."""
    B, steps, H = 7, 60, 1
    x = inputs(bv, B, steps, H, seed=9800)
    m = bv.Models(product, model_dir8)

    twin = bv.Batch(m, B, max_speakers=S)
    api = Api(bv, twin, "drained")
    settings(api)
    ref = []
    for k in range(steps):
        if k in (5, 12):
            script(api, k, None)
        ref.append(twin.convert(np.ascontiguousarray(x[:, k])))
    twin.close()
    ref = np.stack(ref)

    batch = bv.Batch(m, B, max_speakers=S)
    a, h = batch.a, batch.h
    api = Api(bv, batch, "inflight")
    settings(api)
    assert a.BeatriceBatch_EnableHostStreaming(h, 1) == 0
    out = np.zeros((B, H * 240), np.float32)
    got = []
    for k in range(steps):
        if k in (5, 12):
            script(api, k, None)
        rc = a.BeatriceBatch_StreamFrames(h, bv.fptr(np.ascontiguousarray(x[:, k])), bv.fptr(out))
        assert rc in (0, 1)
        if rc == 1:
            got.append(out.copy())
    assert a.BeatriceBatch_TicksLaunched(h) == steps   # nothing drained on the way
    while True:
        rc = a.BeatriceBatch_StreamFlush(h, bv.fptr(out))
        assert rc in (0, 1)
        if rc == 0:
            break
        got.append(out.copy())
    assert a.BeatriceBatch_EnableHostStreaming(h, 0) == 0
    batch.close()
    m.close()
    got = np.stack(got)
    assert got.shape == ref.shape and np.abs(ref).max() > 0.05
    bad = differing(got, ref, range(B), steps)
    assert not bad, "host streaming vs the in-order twin, (stream, step, max-abs): %s" % bad[:12]


def test_refused_calls_change_nothing(bv, product, model_dir8):
    B, steps, H = 7, 24, 1
    w2 = np.ascontiguousarray(W_B)

    def run(ask):
        x = inputs(bv, B, steps, H)
        m = bv.Models(product, model_dir8)
        batch = bv.Batch(m, B, max_speakers=S)
        a, h = batch.a, batch.h
        api = Api(bv, batch, "inflight")
        settings(api)

        def call(n, slots, froms, w=w2, n_weights=N):
            return a.BeatriceBatch_MorphSpeakersInFlight(h, n, bv.iptr(i32(slots)), bv.iptr(i32(froms)), bv.fptr(w) if w is not None else None, n_weights, 999)

        r = Resident(bv, batch, slots=steps + 12, tick=True)   # (>= TickStages() + 1)
        try:
            for k in range(steps):
                r.buf[k] = x[:, k]
            r.hip.h2d(r.d_in, r.buf)
            for k in range(steps):
                if k == 5:
                    script(api, k, None)
                if ask and k in (3, 9, 10):
                    many = list(range(N, S)) + [N]
                    assert call(0, [11], [-1]) == -1 and call(-1, [11], [-1]) == -1 and call(S + 1, many * 2, [-1] * (2 * len(many))) == -1
                    assert call(1, [11], [-1], n_weights=0) == -1 and call(1, [11], [-1], n_weights=257) == -1 and call(1, [11], [-1], w=None) == -1
                    assert call(1, [15], [-1], w=np.zeros((1, 13), np.float32), n_weights=13) == -1      # more weights than speakers in the table
                    assert call(1, [N - 1], [-1]) == -1 and call(1, [S], [-1]) == -1 and call(1, [-1], [-1]) == -1
                    assert call(2, [11, 11], [-1, -1]) == -1                                               # a slot twice
                    assert call(2, [11, 12], [4, 4]) == -1                                                 # a from_slot twice
                    assert call(1, [11], [S]) == -1 and call(1, [11], [-2]) == -1                          # a from_slot out of range
                    assert call(1, [11], [11]) == -1 and call(2, [11, 12], [12, -1]) == -1                 # its own slot; another pair's slot
                    if k > 5:
                        assert call(1, [8], [-1]) == -3 and call(2, [11, 9], [4, -1]) == -3                # entries streams are on
                        assert api.busy(8) == 1 and api.busy(11) == 0
                    assert api.busy(-1) == -1 and api.busy(S) == -1
                assert a.BeatriceBatch_ConvertFramesDevice(h, None, None) == 0
            ticks = a.BeatriceBatch_TicksLaunched(h)
            assert a.BeatriceBatch_Synchronize(h) == 0
            out = np.zeros((r.slots, B, H * 240), np.float32)
            r.hip.d2h(out, r.d_out)
            r.leave()
        finally:
            r.free()
        batch.close()
        m.close()
        return out[:steps].copy(), ticks

    got, ticks = run(True)
    never, ticks_never = run(False)
    assert np.abs(never).max() > 0.05
    assert np.array_equal(got, never)
    assert ticks == ticks_never == steps


def test_an_entry_is_free_right_after_a_synchronize(bv, product, model_dir8):
    """Rule (b) ends with a drain: once no stream's settings name the entry, BeatriceBatch_Synchronize frees it."""
    B, steps, H = 7, 18, 1
    x = inputs(bv, B, steps, H)
    m = bv.Models(product, model_dir8)
    batch = bv.Batch(m, B, max_speakers=S)
    a, h = batch.a, batch.h
    api = Api(bv, batch, "inflight")
    settings(api)
    r = Resident(bv, batch, slots=steps + 12, tick=True)   # (>= TickStages() + 1)
    try:
        for k in range(steps):
            r.buf[k] = x[:, k]
        r.hip.h2d(r.d_in, r.buf)
        for k in range(steps):
            if k == 2:
                assert api.morph([8], [-1], W_A[:1]) == 0
                api.move([0], [8])
            if k == 8:
                assert api.morph([11], [8], W_C) == 0
            assert a.BeatriceBatch_ConvertFramesDevice(h, None, None) == 0
        # stream 0 installed entry 11's last block in step 15: no setting names entry 8, but steps that did are inside the pipeline
        assert a.BeatriceBatch_TicksLaunched(h) == steps and steps - 15 < a.BeatriceBatch_TickStages(h)
        assert api.busy(8) == 1
        assert a.BeatriceBatch_Synchronize(h) == 0
        assert api.busy(8) == 0 and api.busy(11) == 1
        assert api.morph([8], [-1], W_D) == 0
        r.leave()
    finally:
        r.free()
    batch.close()
    m.close()
