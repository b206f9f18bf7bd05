"""Object lifecycle: contexts and batches can be created and destroyed for ever
without leaking device memory (the reference host destroys and re-creates its four contexts on every
ResetContext, processor_core_2.cc:258-266)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _free_bytes():
    """hipMemGetInfo through the HIP runtime the product library itself is linked against"""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    assert hip.hipDeviceSynchronize() == 0
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_contexts_do_not_leak(bv, product, model_dir):
    m = bv.Models(product, model_dir)
    x = bv.synth_audio(160 * 2, seed=3)

    def cycle():
        s = bv.Stream1(m, speaker=1, vq_k=2)
        for h in range(2):
            s.hop(x[h * 160:(h + 1) * 160])
        s.close()

    for _ in range(3):
        cycle()  # warm up allocator pools and the codebook cache
    before = _free_bytes()
    for _ in range(40):
        cycle()
    after = _free_bytes()
    m.close()
    print("free device memory: %.1f MB -> %.1f MB" % (before / 2**20, after / 2**20))
    assert before - after <= 8 << 20


def test_batches_do_not_leak(bv, product, model_dir):
    m = bv.Models(product, model_dir)
    n = m.tables.n_speakers
    w = np.array([0.5, 0.3, 0.2], np.float32)

    def cycle(i):
        batch = bv.Batch(m, 48, hops_per_step=(1, 2, 4, 8)[i % 4])
        assert batch.a.BeatriceBatch_MorphSpeaker(batch.h, n, bv.fptr(w), n, i) == 0
        batch.a.BeatriceBatch_SetTargetSpeaker(batch.h, 0, n)
        x = np.zeros((48, batch.H * 160), np.float32)
        batch.convert(x)
        batch.convert(x)
        batch.close()

    for i in range(4):
        cycle(i)
    before = _free_bytes()
    for i in range(24):
        cycle(i)
    after = _free_bytes()
    m.close()
    print("free device memory: %.1f MB -> %.1f MB" % (before / 2**20, after / 2**20))
    assert before - after <= 8 << 20


def test_wrapper_bindings_around_the_ticks_do_not_leak(bv, product, model_dir):
    """The resident-block wrappers around the tick pipeline (uniform clocks at 1 / 2 / 4 hops per step, clocks per stream): bound, run,
    unbound or destroyed while still bound, for ever."""
    import ctypes as C
    from tick_driver import Hip
    m = bv.Models(product, model_dir)
    hip = Hip()
    B, block = 8, 441

    def cycle(i):
        H = (1, 2, 4, 1)[i % 4]
        ragged = i % 4 == 3
        batch = bv.Batch(m, B, hops_per_step=H)
        a, h = batch.a, batch.h
        if ragged:
            assert a.BeatriceBatch_ConfigureWrapperRates(h, (C.c_double * B)(*([44100.0, 48000.0] * (B // 2)))) == 0
            slots = a.BeatriceBatch_TickStages(h) + 4
        else:
            assert a.BeatriceBatch_ConfigureWrapper(h, 44100.0) == 0
            slots = a.BeatriceBatch_ResidentBlocksDelayFor(h, block) + 4
        d_in, d_out = hip.malloc(slots * B * 480 * 4), hip.malloc(slots * B * 480 * 4)
        assert hip.lib.hipMemset(d_in, 0, C.c_size_t(slots * B * 480 * 4)) == 0
        if ragged:
            assert a.BeatriceBatch_BindResidentBlocksRagged(h, d_in, d_out, 1, 480, slots) == 0
            for _ in range(6):
                assert a.BeatriceBatch_ProcessBlocksRaggedDevice(h, (C.c_int * B)(*([441, 480] * (B // 2)))) == 0
        else:
            assert a.BeatriceBatch_BindResidentBlocks(h, d_in, d_out, 1, block, slots) == 0
            for _ in range(6):
                assert a.BeatriceBatch_ProcessBlocksDevice(h, None, None, 1, block) == 0
        assert a.BeatriceBatch_Synchronize(h) == 0
        if i % 2 == 0:   # every other batch is destroyed while still bound
            assert (a.BeatriceBatch_BindResidentBlocksRagged(h, None, None, 0, 0, 0) if ragged else a.BeatriceBatch_BindResidentBlocks(h, None, None, 0, 0, 0)) == 0
        batch.close()
        hip.free(d_in)
        hip.free(d_out)

    for i in range(4):
        cycle(i)
    before = _free_bytes()
    for i in range(16):
        cycle(i)
    after = _free_bytes()
    m.close()
    print("free device memory: %.1f MB -> %.1f MB" % (before / 2**20, after / 2**20))
    assert before - after <= 8 << 20


def test_every_other_mode_does_not_leak(bv, product, model_dir):
    """The owners the tests above do not reach: stage streams (EnablePipelining(3)), host streaming, the 48 kHz wrapper around the ticks,
    the silent-block rule in order with a flagged block, tick mode with streams that sit steps out (the per-stream counters), the
    per-stream-clock wrapper in order, and FlushResidentBlocks at two hops per step (its block of zeros).  One cycle = every mode once;
    every other batch of a mode is destroyed while still in it."""
    import ctypes as C
    from tick_driver import Hip
    m = bv.Models(product, model_dir)
    hip = Hip()
    B = 8

    def stage_streams(batch, leave):
        assert batch.a.BeatriceBatch_EnablePipelining(batch.h, 3) == 0
        x = np.zeros((B, 160), np.float32)
        batch.convert(x)
        batch.convert(x)
        if leave:
            assert batch.a.BeatriceBatch_EnablePipelining(batch.h, 0) == 0

    def host_streaming(batch, leave):
        a, h = batch.a, batch.h
        assert a.BeatriceBatch_EnableHostStreaming(h, 1) == 0
        x, out = np.zeros((B, 160), np.float32), np.zeros((B, 240), np.float32)
        for _ in range(a.BeatriceBatch_HostStreamDelay(h) + 4):
            assert a.BeatriceBatch_StreamFrames(h, bv.fptr(x), bv.fptr(out)) in (0, 1)
        if leave:
            while a.BeatriceBatch_StreamFlush(h, bv.fptr(out)) == 1:
                pass
            assert a.BeatriceBatch_EnableHostStreaming(h, 0) == 0

    def resident_48k(batch, leave):
        a, h = batch.a, batch.h
        slots = a.BeatriceBatch_TickStages(h) + 2
        nbytes = slots * B * 480 * 4
        d_in, d_out = hip.malloc(nbytes), hip.malloc(nbytes)
        assert hip.lib.hipMemset(d_in, 0, C.c_size_t(nbytes)) == 0
        assert a.BeatriceBatch_BindResidentIO48k(h, d_in, d_out, 1, slots) == 0
        for _ in range(6):
            assert a.BeatriceBatch_ConvertBlocks48kDevice(h, None, None, 1) == 0
        assert a.BeatriceBatch_Synchronize(h) == 0
        if leave:
            assert a.BeatriceBatch_BindResidentIO48k(h, None, None, 0, 0) == 0
        return d_in, d_out

    def silent_rule_in_order(batch, leave):
        a, h = batch.a, batch.h
        assert a.BeatriceBatch_EnableSilentBlockRule(h, 1) == 0
        x = np.full((B, 1, 480), 0.25, np.float32)
        x[0] = 0.0   # stream 0's block is silent by the shell's rule
        for _ in range(3):
            batch.convert48k(x, 1)
        if leave:
            assert a.BeatriceBatch_EnableSilentBlockRule(h, 0) == 0

    def ticks_with_streams_sitting_out(batch, leave):
        a, h = batch.a, batch.h
        slots = a.BeatriceBatch_TickStages(h) + 2
        d_in, d_out = hip.malloc(slots * B * 160 * 4), hip.malloc(slots * B * 240 * 4)
        assert hip.lib.hipMemset(d_in, 0, C.c_size_t(slots * B * 160 * 4)) == 0
        assert a.BeatriceBatch_BindResidentIO(h, d_in, d_out, slots) == 0
        assert a.BeatriceBatch_EnableTickPipeline(h, 1) == 0
        assert a.BeatriceBatch_EnableSilentBlockRule(h, 1) == 0
        for k in range(6):
            assert a.BeatriceBatch_SetSilentStreams(h, bytes([1 if s == k % B else 0 for s in range(B)])) == 0
            assert a.BeatriceBatch_ConvertFramesDevice(h, None, None) == 0
        assert a.BeatriceBatch_Synchronize(h) == 0
        if leave:
            assert a.BeatriceBatch_EnableTickPipeline(h, 0) == 0
            assert a.BeatriceBatch_BindResidentIO(h, None, None, 0) == 0
        return d_in, d_out

    def per_stream_clocks_in_order(batch, leave):
        a, h = batch.a, batch.h
        assert a.BeatriceBatch_ConfigureWrapperRates(h, (C.c_double * B)(*([44100.0, 48000.0] * (B // 2)))) == 0
        ns = [441, 480] * (B // 2)
        xin = np.full(sum(ns), 0.25, np.float32)
        out = np.zeros_like(xin)
        for _ in range(3):
            assert a.BeatriceBatch_ProcessBlocksRagged(h, bv.fptr(xin), bv.fptr(out), 1, (C.c_int * B)(*ns), 0) == 0

    def flush_at_two_hops(batch, leave):
        a, h = batch.a, batch.h
        block = 441
        assert a.BeatriceBatch_ConfigureWrapper(h, 44100.0) == 0
        slots = a.BeatriceBatch_ResidentBlocksDelayFor(h, block) + 4
        d_in, d_out = hip.malloc(slots * B * 480 * 4), hip.malloc(slots * B * 480 * 4)
        assert hip.lib.hipMemset(d_in, 0, C.c_size_t(slots * B * 480 * 4)) == 0
        assert a.BeatriceBatch_BindResidentBlocks(h, d_in, d_out, 1, block, slots) == 0
        for _ in range(5):
            assert a.BeatriceBatch_ProcessBlocksDevice(h, None, None, 1, block) == 0
        assert a.BeatriceBatch_FlushResidentBlocks(h) == 0
        assert a.BeatriceBatch_ResidentBlocksOwed(h) == 0
        if leave:
            assert a.BeatriceBatch_BindResidentBlocks(h, None, None, 0, 0, 0) == 0
        return d_in, d_out

    kinds = [(stage_streams, 1), (host_streaming, 1), (resident_48k, 1), (silent_rule_in_order, 1), (ticks_with_streams_sitting_out, 1),
             (per_stream_clocks_in_order, 1), (flush_at_two_hops, 2)]

    def cycle(i):
        for j, (run, H) in enumerate(kinds):
            batch = bv.Batch(m, B, hops_per_step=H)
            mine = run(batch, (i + j) % 2 == 0)
            batch.close()
            for p in mine or ():
                hip.free(p)

    for i in range(4):
        cycle(i)
    before = _free_bytes()
    for i in range(8):
        cycle(i)
    after = _free_bytes()
    m.close()
    print("free device memory: %.1f MB -> %.1f MB" % (before / 2**20, after / 2**20))
    assert before - after <= 8 << 20


def test_unhealthy_objects_fail_softly(bv, product, model_dir):
    """Calls on objects that could not be built must not crash: error code from the batch, zeros from the
    void per-hop calls ('Errors')."""
    a = bv.bind_batch(product)
    empty_phone, empty_pitch = a.CreatePhoneExtractor(), a.CreatePitchEstimator()      # never loaded
    empty_wave, empty_embed = a.CreateWaveformGenerator(), a.CreateEmbeddingSetter()
    b = a.BeatriceBatch_Create(empty_phone, empty_pitch, empty_wave, empty_embed, 4, 2)
    assert a.BeatriceBatch_IsHealthy(b) == 0
    x = np.ones((4, 160), np.float32)
    y = np.ones((4, 240), np.float32)
    assert a.BeatriceBatch_ConvertFrames(b, bv.fptr(x), bv.fptr(y)) == -2
    assert a.BeatriceBatch_SetTargetSpeaker(b, 0, 0) == -2
    a.BeatriceBatch_Destroy(b)
    pc = a.CreatePhoneContext1()
    out = np.ones(bv.PHONE_CH, np.float32)
    a.ExtractPhone1(empty_phone, bv.fptr(x[0]), bv.fptr(out), pc)   # model not loaded: silence, no crash
    assert not out.any()
    a.DestroyPhoneContext1(pc)
    a.DestroyPhoneExtractor(empty_phone); a.DestroyPitchEstimator(empty_pitch)
    a.DestroyWaveformGenerator(empty_wave); a.DestroyEmbeddingSetter(empty_embed)
