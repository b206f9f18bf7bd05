"""BeatriceBatch_InstallSpeakersInFlight: new voices into table entries in one call, and in tick mode / host streaming without draining the
pipeline (csrc/install.hip install_entries_kernel + csrc/morph.hip morph_project_kernel; csrc/batch.hip entry_busy).  Everything at
max-abs 0 against two yardsticks: twin A, a batch on which the same script calls the drained BeatriceBatch_UpdateSpeaker once per entry,
and twin B, a batch whose table held the voices in those entries from the start (BeatriceBatch_SetSpeakerTables with 16 entries).

The voices V[0..7] are the 8-speaker synthetic model's own tables with the speaker axis rotated by one and the codebook rows reversed.  A
codebook is heard only under k-NN, so in every script a stream on an installed entry has BeatriceBatch_SetVQNumNeighbors(.., 2)."""
import ctypes as C

import numpy as np
import pytest

import wrapperlib
from test_gpu_morph_device import model_dir8  # noqa: F401  (fixture: the 8-speaker synthetic model)
from tick_driver import Hip, Resident

pytestmark = pytest.mark.gpu

SHAPES = [(7, 70, 1), (7, 70, 2), (40, 64, 4)]
N, S, SEED = 8, 16, 77           # real speakers, table entries (8 + 8), lottery seed
KNN_STREAM, SILENT_STREAM, SIT_OUT = 1, 1, (30, 31, 32)


def i32(v):
    return np.ascontiguousarray(v, np.int32)


class Voices:
    def __init__(self, t):
        self.cb = np.ascontiguousarray(np.roll(t.codebooks[:N], 1, axis=0)[:, ::-1])
        self.add = np.ascontiguousarray(np.roll(t.additive[:N], 1, axis=0))
        self.kv = np.ascontiguousarray(np.roll(t.kv[:N], 1, axis=0))
        assert not np.array_equal(self.cb[1], t.codebooks[1]) and not np.array_equal(self.add[3], self.add[4])


class Api:
    """What a script sees: install(entries, voices) as ONE in-flight call, or as the drained BeatriceBatch_UpdateSpeaker one per entry."""

    def __init__(self, bv, batch, how):
        self.bv, self.batch, self.a, self.h, self.B, self.how = bv, batch, batch.a, batch.h, batch.B, how
        self.v = Voices(batch.m.tables)

    def install(self, entries, voices, raw=False):
        bv, a, h, v = self.bv, self.a, self.h, self.v
        if self.how == "inflight":
            cb, add, kv = v.cb[voices].copy(), v.add[voices].copy(), v.kv[voices].copy()
            rc = a.BeatriceBatch_InstallSpeakersInFlight(h, len(entries), bv.iptr(i32(entries)), bv.fptr(cb), bv.fptr(add), bv.fptr(kv))
            for x in (cb, add, kv):
                x[...] = np.nan     # the call has copied them out
            return rc
        if self.how == "preloaded":   # twin B: the entries hold their voices already
            return 0
        for e, i in zip(entries, voices):
            assert a.BeatriceBatch_UpdateSpeaker(h, e, bv.fptr(v.cb[i]), bv.fptr(v.add[i]), bv.fptr(v.kv[i])) == 0
        return 0

    def morph(self, slot, w):
        bv, a, h = self.bv, self.a, self.h
        w = np.ascontiguousarray(w, np.float32)
        if self.how == "inflight":
            return a.BeatriceBatch_MorphSpeakersInFlight(h, 1, bv.iptr(i32([slot])), bv.iptr(i32([-1])), bv.fptr(w), len(w), SEED)
        return a.BeatriceBatch_MorphSpeaker(h, slot, bv.fptr(w), len(w), SEED)

    def busy(self, e):
        return self.a.BeatriceBatch_SpeakerEntryBusy(self.h, e)

    def move(self, streams, speakers):
        assert self.a.BeatriceBatch_SetTargetSpeakers(self.h, len(streams), self.bv.iptr(i32(streams)), self.bv.iptr(i32(speakers))) == 0

    def embeddings(self, e):
        add, kv = np.zeros(self.bv.HID, np.float32), np.zeros((self.bv.KV_LEN, self.bv.KV_CH), np.float32)
        assert self.a.BeatriceBatch_GetSpeakerEmbeddings(self.h, e, self.bv.fptr(add), self.bv.fptr(kv)) == 0
        return add, kv


def make_batch(bv, m, B, H=1, placed=None):
    """A 16-entry batch on the model's tables; placed {entry: voice}: twin B, whose table holds those voices from the start."""
    if placed is None:
        return bv.Batch(m, B, max_speakers=S, hops_per_step=H)
    t, v = m.tables, Voices(m.tables)
    cb, add, kv = np.zeros((S,) + t.codebooks.shape[1:], np.float32), np.zeros((S, bv.HID), np.float32), np.zeros((S,) + t.kv.shape[1:], np.float32)
    cb[:N], add[:N], kv[:N] = t.codebooks[:N], t.additive[:N], t.kv[:N]
    for e, i in placed.items():
        cb[e], add[e], kv[e] = v.cb[i], v.add[i], v.kv[i]
    batch = bv.Batch(m, B, max_speakers=S, hops_per_step=H, upload_tables=False)
    assert batch.a.BeatriceBatch_SetSpeakerTables(batch.h, S, bv.fptr(cb), bv.fptr(add), bv.fptr(t.formant), bv.fptr(kv)) == 0
    batch.apply_defaults()
    return batch


def inputs(bv, B, steps, H, seed=9700):
    return np.stack([bv.synth_audio(160 * H * steps, seed=seed + s) for s in range(B)]).reshape(B, steps, H * 160).copy()


def settings(api, speakers=None):
    for s in range(api.B):
        assert api.a.BeatriceBatch_SetTargetSpeaker(api.h, s, speakers[s] if speakers else s % N) == 0
    assert api.a.BeatriceBatch_SetVQNumNeighbors(api.h, KNN_STREAM, 2) == 0
    assert api.a.BeatriceBatch_FlushSpeaker(api.h, -1) == 0


def run_ticks(bv, product, model_dir, B, steps, H, how, script, state=None, rule=False, speakers=None, mode="D", after=None):
    """Feeds `steps` steps through tick mode (mode "C": plain resident I/O) with script(api, k, state) before step k.
    -> state with out [steps][B][H * 240], ticks (before the final drain), stages, and what `after(api, state)` adds once drained."""
    x = inputs(bv, B, steps, H)
    m = bv.Models(product, model_dir)
    batch = make_batch(bv, m, B, H)
    a, h = batch.a, batch.h
    api = Api(bv, batch, how)
    settings(api, speakers)
    st = dict(state or {})
    st["stages"] = a.BeatriceBatch_TickStages(h)
    r = Resident(bv, batch, slots=max(steps + 2, st["stages"] + 4), tick=mode == "D")
    try:
        if rule:
            assert a.BeatriceBatch_EnableSilentBlockRule(h, 1) == 0
        for k in range(steps):
            r.buf[k] = x[:, k]
        r.hip.h2d(r.d_in, r.buf)
        for k in range(steps):
            script(api, k, st)
            if rule and k in SIT_OUT:
                assert a.BeatriceBatch_SetSilentStreams(h, bytes(1 if s == SILENT_STREAM else 0 for s in range(B))) == 0
            assert a.BeatriceBatch_ConvertFramesDevice(h, None, None) == 0
        st["ticks"] = a.BeatriceBatch_TicksLaunched(h)
        assert a.BeatriceBatch_Synchronize(h) == 0
        out = np.zeros((r.slots, B, H * 240), np.float32)
        r.hip.d2h(out, r.d_out)
        st["out"] = out[:steps].copy()
        if after:
            after(api, st)
        r.leave()
    finally:
        r.free()
    batch.close()
    m.close()
    return st


def differing(got, want, streams, steps, absent=None):
    return [(s, k, float(np.abs(got[k, s] - want[k, s]).max())) for s in streams for k in range(steps)
            if not (absent and k in absent.get(s, ())) and not np.array_equal(got[k, s], want[k, s])]


# ---- 1. the kernels, in order ------------------------------------------------------------------------------------------------------
def test_installs_in_order_equal_both_twins(bv, product, model_dir8):
    """Mode A (the call drains like BeatriceBatch_UpdateSpeaker): n = 1, n = 3 on non-adjacent entries, n = the cap over all eight free
    entries (rewriting the four already written with other voices); the raw tables read back; 12 steps of k-NN streams on the entries."""
    B, hops = 3, 12
    audio = inputs(bv, B, hops, 1, seed=9900)
    m = bv.Models(product, model_dir8)
    final = {8 + i: i for i in range(8)}
    rounds = [(8, 9, 10), (11, 12, 13), (14, 15, 8)]     # the entries the three streams sit on, four steps each

    def run(how):
        batch = make_batch(bv, m, B, placed=final if how == "preloaded" else None)
        a, h = batch.a, batch.h
        api = Api(bv, batch, how)
        if how == "inflight":
            cap = a.BeatriceBatch_MaxInstallEntries(h)
            assert cap == 16
        assert api.install([15], [0]) == 0
        assert api.install([9, 12, 14], [2, 3, 5]) == 0
        emb = {}
        if how != "preloaded":
            emb = {("early", e): api.embeddings(e) for e in (15, 9, 12, 14)}
        assert api.install(list(range(8, 16)), list(range(8))) == 0
        emb.update({e: api.embeddings(e) for e in range(8, 16)})
        for s in range(B):
            assert a.BeatriceBatch_SetVQNumNeighbors(h, s, 2) == 0
        out = []
        for k in range(hops):
            if k % 4 == 0:
                api.move(list(range(B)), list(rounds[k // 4]))
                assert a.BeatriceBatch_FlushSpeaker(h, -1) == 0
            out.append(batch.convert(np.ascontiguousarray(audio[:, k])))
        batch.close()
        return emb, np.stack(out)

    emb, out = run("inflight")
    emb_a, out_a = run("drained")
    emb_b, out_b = run("preloaded")
    v = Voices(m.tables)
    m.close()
    for (key, i) in [(("early", 15), 0), (("early", 9), 2), (("early", 12), 3), (("early", 14), 5)] + [(8 + i, i) for i in range(8)]:
        assert np.array_equal(emb[key][0], v.add[i]) and np.array_equal(emb[key][1], v.kv[i]), "entry %s does not hold voice %d" % (key, i)
        assert np.array_equal(emb_a[key][0], v.add[i]) and np.array_equal(emb_a[key][1], v.kv[i])
    assert np.abs(out_a).max() > 0.05
    print("in order: max-abs vs twin A %g, vs twin B %g" % (float(np.abs(out - out_a).max()), float(np.abs(out - out_b).max())))
    assert np.array_equal(out_a, out_b), "the twins disagree: max-abs %g" % float(np.abs(out_a - out_b).max())
    assert np.array_equal(out, out_a), "12 steps on the entries vs twin A: max-abs %g" % float(np.abs(out - out_a).max())
    assert np.array_equal(out, out_b), "12 steps on the entries vs twin B: max-abs %g" % float(np.abs(out - out_b).max())


# ---- 2., 3. in flight ----------------------------------------------------------------------------------------------------------------
def script(api, k, st):
    """Streams 0, 1 (the k-NN stream) and 2 go onto the new entries 8, 9, 10; stream 0 leaves 8 again, and once 8 is free it is written a
    second time and stream 2 moves onto it."""
    if api.how == "inflight":
        st.setdefault("polls", {})[k] = api.busy(8)
        if k > 20 and st.get("reuse_at") is None and st["polls"][k] == 0 and st.get("reuse", True):
            st["reuse_at"] = k
    if k == 5:
        assert api.install([8, 9, 10], [0, 1, 2]) == 0
        api.move([0, 1, 2], [8, 9, 10])
    if k == 12:
        api.move([0], [3])
    if k == 20 and api.how == "inflight":
        assert api.install([8], [5]) == -3      # (the twins never ask)
    if k == st.get("reuse_at"):
        assert api.install([8], [5]) == 0
        api.move([2], [8])


def last_step_naming_8(H, steps):
    """The last step in which stream 0 -- the only stream on entry 8 before its reuse -- names it, from the reference's per-hop protocol
    (processor_core_2.cc:431-466, 179-181): a switch takes the codebook and additive embedding at once and one key/value block per hop."""
    target, kv, count, last = 0, [0] * 4, 4, -1
    for k in range(steps):
        if k in (5, 12):
            target, count = {5: 8, 12: 3}[k], 0
        for _ in range(H):
            if count < 4:
                kv[count] = target
                count += 1
            if 8 in [target] + kv:
                last = k
    return last


def check_in_flight(bv, product, model_dir, B, steps, H, rule):
    got = run_ticks(bv, product, model_dir, B, steps, H, "inflight", script, rule=rule)
    assert got.get("reuse_at") is not None, "entry 8 never became free: %s" % got["polls"]
    twin = run_ticks(bv, product, model_dir, B, steps, H, "drained", script, state={"reuse_at": got["reuse_at"]}, rule=rule)
    absent = {SILENT_STREAM: set(SIT_OUT)} if rule else None
    assert np.abs(twin["out"]).max() > 0.05
    last, stages, polls = last_step_naming_8(H, steps), got["stages"], got["polls"]
    print("in flight vs the drained twin: max-abs %g; entry 8 last named in step %d, %d stages, reused before step %d; ticks %d (twin %d)" % (
        float(np.abs(got["out"] - twin["out"]).max()), last, stages, got["reuse_at"], got["ticks"], twin["ticks"]))
    bad = differing(got["out"], twin["out"], range(B), steps, absent)
    assert not bad, "in flight vs the drained twin, (stream, step, max-abs): %s" % bad[:12]
    # nothing drained: as many tick launches as steps fed; every drained call costs more
    assert got["ticks"] == steps
    assert twin["ticks"] > steps
    # entry 8 is busy while stream 0's settings name it and while the last step that did is inside the pipeline: that step was fed by
    # tick `last` and leaves the last stage TickStages() ticks on, so the poll before step last + TickStages() is the first to see it free
    assert all(polls[k] == 0 for k in range(5 + 1)) and all(polls[k] == 1 for k in range(5 + 1, last + stages)), polls
    assert got["reuse_at"] == last + stages, "first free step %d, predicted %d + %d: %s" % (got["reuse_at"], last, stages, polls)


@pytest.mark.parametrize("B,steps,H", SHAPES)
def test_installs_in_flight_equal_the_drained_twin(bv, product, model_dir8, B, steps, H):
    check_in_flight(bv, product, model_dir8, B, steps, H, rule=False)


def test_installs_in_flight_under_the_silent_block_rule(bv, product, model_dir8):
    """The same with the rule on and the k-NN stream, which sits on the new entry 9, sitting steps 30-32 out."""
    B, steps, H = SHAPES[0]
    check_in_flight(bv, product, model_dir8, B, steps, H, rule=True)


def test_installs_in_flight_in_host_streaming(bv, product, model_dir8):
    """Mode E: the script between BeatriceBatch_StreamFrames calls, against twin B on BeatriceBatch_ConvertFrames (every entry is written
    once: 40 steps end before entry 8 could be free again)."""
    B, steps, H = 7, 40, 1
    x = inputs(bv, B, steps, H, seed=9800)
    m = bv.Models(product, model_dir8)

    twin = make_batch(bv, m, B, placed={8: 0, 9: 1, 10: 2})
    api = Api(bv, twin, "preloaded")
    settings(api)
    ref = []
    for k in range(steps):
        script(api, k, {})
        ref.append(twin.convert(np.ascontiguousarray(x[:, k])))
    twin.close()
    ref = np.stack(ref)

    batch = make_batch(bv, m, B)
    a, h = batch.a, batch.h
    api = Api(bv, batch, "inflight")
    settings(api)
    assert a.BeatriceBatch_EnableHostStreaming(h, 1) == 0
    stages = a.BeatriceBatch_TickStages(h)
    out = np.zeros((B, H * 240), np.float32)
    got, st = [], {"reuse": False}
    for k in range(steps):
        script(api, k, st)
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
    assert all(st["polls"][k] == 1 for k in range(6, min(steps, last_step_naming_8(H, steps) + stages)))
    bad = differing(got, ref, range(B), steps)
    assert not bad, "host streaming vs twin B, (stream, step, max-abs): %s" % bad[:12]


# ---- 4. with morphs ------------------------------------------------------------------------------------------------------------------
W_M = np.array([0.4, 0.0, 0.35, 0.0, 0.0, 0.25, 0.0, 0.0], np.float32)    # entry 10: speaker 2 among the lottery's candidates
W_N = np.array([0.0, 0.0, 0.6, 0.0, 0.0, 0.0, 0.4, 0.0], np.float32)      # entry 11, over the NEW speaker 2
NOT_ON_2 = [0, 1, 3, 4, 5, 6, 7]


def morph_script(api, k, st):
    inflight = api.how == "inflight"
    if k == 3:
        if inflight:
            assert api.busy(2) == 0
        assert api.morph(10, W_M) == 0
        if inflight:
            assert api.busy(2) == 0              # listed by a morph nothing names yet
        api.move([KNN_STREAM], [10])
        if inflight:
            assert api.busy(2) == 1              # ... and now a stream is on that morph
    if inflight and 3 < k and st.get("free_at") is None:
        busy10, busy2 = api.busy(10), api.busy(2)
        assert busy2 == busy10, "step %d: entry 2 busy %d, morph entry 10 busy %d" % (k, busy2, busy10)
        if busy10 == 1 and k in (4, 9, 11, 20):
            assert api.install([2], [3]) == -3 and api.install([12, 2], [3, 4]) == -3     # nothing changes: the twin never asks
        if busy10 == 0:
            st["free_at"] = k
    if k == 10:
        api.move([KNN_STREAM], [6])
    if k == st.get("free_at"):
        assert api.install([2], [3]) == 0
        assert api.morph(11, W_N) == 0           # in the same gap: reads the new raw rows of entry 2
        api.move([0, KNN_STREAM], [2, 11])


def test_a_morph_keeps_its_candidates_busy(bv, product, model_dir8):
    B, steps, H = 7, 64, 1

    def after(api, st):
        st["emb"] = {e: api.embeddings(e) for e in (2, 10, 11)}

    got = run_ticks(bv, product, model_dir8, B, steps, H, "inflight", morph_script, speakers=NOT_ON_2, after=after)
    assert got.get("free_at") is not None and got["free_at"] > 10 + got["stages"] - 1, got.get("free_at")
    twin = run_ticks(bv, product, model_dir8, B, steps, H, "drained", morph_script, state={"free_at": got["free_at"]}, speakers=NOT_ON_2, after=after)
    assert got["ticks"] == steps and twin["ticks"] > steps
    v = Voices(bv.SpeakerTables(product, model_dir8))
    assert np.array_equal(got["emb"][2][0], v.add[3]) and np.array_equal(got["emb"][2][1], v.kv[3])
    for e in (2, 10, 11):
        for x, y in zip(got["emb"][e], twin["emb"][e]):
            assert np.array_equal(x, y), "entry %d read back: max-abs %g" % (e, float(np.abs(x - y).max()))
    assert np.abs(got["emb"][11][1]).max() > 0.1
    print("with morphs: entry 2 free before step %d; max-abs vs twin A %g" % (got["free_at"], float(np.abs(got["out"] - twin["out"]).max())))
    assert np.abs(twin["out"]).max() > 0.05
    bad = differing(got["out"], twin["out"], range(B), steps)
    assert not bad, "with morphs vs twin A, (stream, step, max-abs): %s" % bad[:12]


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refused_calls_change_nothing(bv, product, model_dir8):
    B, steps, H = 7, 24, 1

    def asking(api, k, st):
        if k == 5:
            script(api, k, st)
        if not st["ask"] or k not in (3, 9, 10):
            return
        bv_, a, h, v = api.bv, api.a, api.h, api.v
        cap = a.BeatriceBatch_MaxInstallEntries(h)

        def call(n, entries, cb=v.cb, add=v.add, kv=v.kv):
            p = [bv_.fptr(np.ascontiguousarray(np.resize(t, (max(n, 1),) + t.shape[1:]))) if t is not None else None for t in (cb, add, kv)]
            return a.BeatriceBatch_InstallSpeakersInFlight(h, n, bv_.iptr(i32(entries)) if entries is not None else None, *p)

        assert call(0, [11]) == -1 and call(-1, [11]) == -1 and call(cap + 1, list(range(cap + 1))) == -1
        assert call(1, None) == -1 and call(1, [11], cb=None) == -1 and call(1, [11], add=None) == -1 and call(1, [11], kv=None) == -1
        assert call(1, [S]) == -1 and call(1, [-1]) == -1 and call(2, [11, S]) == -1
        assert call(2, [11, 11]) == -1 and call(3, [12, 11, 12]) == -1                        # an entry twice
        assert call(1, [3]) == -3 and call(2, [11, 4]) == -3                                  # entries streams are on
        if k > 5:
            assert call(1, [8]) == -3 and call(3, [11, 12, 9]) == -3
            assert api.busy(8) == 1
        assert api.busy(11) == 0 and api.busy(12) == 0

    got = run_ticks(bv, product, model_dir8, B, steps, H, "inflight", asking, state={"ask": True, "reuse": False})
    never = run_ticks(bv, product, model_dir8, B, steps, H, "inflight", asking, state={"ask": False, "reuse": False})
    assert np.abs(never["out"]).max() > 0.05
    assert np.array_equal(got["out"], never["out"])
    assert got["ticks"] == never["ticks"] == steps


# ---- 6. the other modes drain and agree ----------------------------------------------------------------------------------------------
def install_at_3(api, k, st=None):
    if k == 3:
        assert api.install([9, 12], [1, 4]) == 0
        api.move([KNN_STREAM, 2], [9, 12])


def run_mode(bv, product, model_dir, mode, how):
    B, steps, CH = 3, 8, 1
    if mode == "C":
        return run_ticks(bv, product, model_dir, B, steps, 1, how, install_at_3, mode="C")["out"]
    m = bv.Models(product, model_dir)
    batch = make_batch(bv, m, B)
    a, h = batch.a, batch.h
    api = Api(bv, batch, how)
    settings(api)
    try:
        if mode == "B":
            x = inputs(bv, B, steps, 1)
            assert a.BeatriceBatch_EnablePipelining(h, 2) == 0
            out = []
            for k in range(steps):
                install_at_3(api, k)
                out.append(batch.convert(np.ascontiguousarray(x[:, k])))
            return np.stack(out)
        assert mode == "F"
        hip = Hip()
        slots = max(steps + 2, a.BeatriceBatch_TickStages(h) + 4)
        x48 = np.stack([wrapperlib.test_signal(480 * steps * CH, 48000, seed=8900 + s) for s in range(B)]).astype(np.float32).reshape(B, steps, 1, CH, 480)
        buf = np.zeros((slots, B, 1, CH, 480), np.float32)
        buf[:steps] = x48.transpose(1, 0, 2, 3, 4)
        d_in, d_out = hip.malloc(buf.nbytes), hip.malloc(buf.nbytes)
        try:
            hip.h2d(d_in, buf)
            assert hip.lib.hipMemset(d_out, 0, C.c_size_t(buf.nbytes)) == 0
            assert a.BeatriceBatch_BindResidentIO48k(h, d_in, d_out, CH, slots) == 0
            for k in range(steps):
                install_at_3(api, k)
                assert a.BeatriceBatch_ConvertBlocks48kDevice(h, None, None, CH) == 0
            assert a.BeatriceBatch_Synchronize(h) == 0
            out = np.zeros_like(buf)
            hip.d2h(out, d_out)
            batch.close()      # (with the slots still allocated)
        finally:
            hip.free(d_in)
            hip.free(d_out)
        return out[:steps].copy()
    finally:
        batch.close()
        m.close()


@pytest.mark.parametrize("mode", ["B", "C", "F"])
def test_other_modes_drain_and_agree(bv, product, model_dir8, mode):
    got = run_mode(bv, product, model_dir8, mode, "inflight")
    twin = run_mode(bv, product, model_dir8, mode, "drained")
    assert np.abs(twin).max() > 0.05
    assert np.array_equal(got, twin), "mode %s vs twin A: max-abs %g" % (mode, float(np.abs(got - twin).max()))


# ---- 7. the staging ring comes round -------------------------------------------------------------------------------------------------
def test_more_calls_than_ring_entries(bv, product, model_dir8):
    """Eleven one-entry calls between consecutive ticks (the ring has four entries, so one is claimed while the device may still be
    behind); every call's arrays are overwritten with NaN as soon as it returns (Api.install).  Entry 13 is heard from step 8 on, entries
    8 and 10 -- written twice -- from step 16 on."""
    B, steps, H = 3, 40, 1
    voice_of = lambda c: (3 * c + 1) % 8     # noqa: E731  (calls 0..5 -> entries 8..13, calls 6..10 -> entries 8..12 again, other voices)

    def rotate(api, k, st):
        if 2 <= k <= 7:
            assert api.install([8 + (k - 2)], [voice_of(k - 2)]) == 0
        if k == 8:
            api.move([2], [13])
        if 9 <= k <= 13:
            assert api.install([8 + (k - 9)], [voice_of(k - 3)]) == 0
        if k == 16:
            api.move([0, KNN_STREAM], [8, 10])

    def after(api, st):
        st["emb"] = {e: api.embeddings(e) for e in range(8, 14)}

    got = run_ticks(bv, product, model_dir8, B, steps, H, "inflight", rotate, after=after)
    twin = run_ticks(bv, product, model_dir8, B, steps, H, "drained", rotate, after=after)
    assert got["ticks"] == steps
    v = Voices(bv.SpeakerTables(product, model_dir8))
    for e in range(8, 14):
        i = voice_of(5) if e == 13 else voice_of(6 + e - 8)
        assert np.array_equal(got["emb"][e][0], v.add[i]) and np.array_equal(got["emb"][e][1], v.kv[i]), "entry %d does not hold voice %d" % (e, i)
        assert np.array_equal(twin["emb"][e][0], v.add[i])
    assert np.abs(twin["out"]).max() > 0.05
    bad = differing(got["out"], twin["out"], range(B), steps)
    assert not bad, "ring reuse vs twin A, (stream, step, max-abs): %s" % bad[:12]
