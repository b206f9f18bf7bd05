"""beatrice-vst_amd -- MI355X-native Beatrice 2 (rc.0) per-hop voice-conversion path.

The product is the C-ABI shared library ``csrc/libbeatrice_hip.so`` (hand-written HIP for gfx950,
declared in ``include/beatrice_abi.h`` + ``include/beatrice_batch.h``).  This Python module is
plumbing only: ctypes prototypes for that ABI, used by the tests, ``bench.py`` and
``__graft_entry__.py``.  The directory name contains a hyphen, so import it by path:

    import importlib.util, sys
    spec = importlib.util.spec_from_file_location("beatrice_vst_amd", ".../beatrice-vst_amd/__init__.py")

There is deliberately NO CPU fallback here: ``load_product()`` raises if the HIP library is
missing or cannot be loaded.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
# (BEATRICE_HIP_LIB: another build of the same library, for A/B measurements of kernel variants)
PRODUCT_LIB = os.environ.get("BEATRICE_HIP_LIB") or os.path.join(HERE, "csrc", "libbeatrice_hip.so")

IN_HOP, OUT_HOP = 160, 240
PHONE_CH, HID, PITCH_BINS = 128, 256, 448
CODEBOOK, KV_LEN, KV_CH, N_BLOCKS = 512, 384, 128, 4
STEP_WRAP = 12252240  # BEATRICE_HIP_STEP_WRAP (include/beatrice_batch.h): the step / hop counter wraps to 0 after STEP_WRAP - 1

_f32p = C.POINTER(C.c_float)
_i32p = C.POINTER(C.c_int)
_u8p = C.POINTER(C.c_ubyte)
_vp = C.c_void_p

# name -> (restype, argtypes) for the rc0 generation (include/beatrice_abi.h)
_RC0 = {
    "CreatePhoneExtractor": (_vp, []), "DestroyPhoneExtractor": (None, [_vp]),
    "CreatePhoneContext1": (_vp, []), "DestroyPhoneContext1": (None, [_vp]),
    "CreatePitchEstimator": (_vp, []), "DestroyPitchEstimator": (None, [_vp]),
    "CreatePitchContext1": (_vp, []), "DestroyPitchContext1": (None, [_vp]),
    "CreateWaveformGenerator": (_vp, []), "DestroyWaveformGenerator": (None, [_vp]),
    "CreateWaveformContext1": (_vp, []), "DestroyWaveformContext1": (None, [_vp]),
    "CreateEmbeddingSetter": (_vp, []), "DestroyEmbeddingSetter": (None, [_vp]),
    "CreateEmbeddingContext": (_vp, []), "DestroyEmbeddingContext": (None, [_vp]),
    "ReadPhoneExtractorParameters": (C.c_int, [_vp, C.c_char_p]),
    "ReadPitchEstimatorParameters": (C.c_int, [_vp, C.c_char_p]),
    "ReadWaveformGeneratorParameters": (C.c_int, [_vp, C.c_char_p]),
    "ReadEmbeddingSetterParameters": (C.c_int, [_vp, C.c_char_p]),
    "ReadNSpeakers": (C.c_int, [C.c_char_p, _i32p]),
    "ReadSpeakerEmbeddings": (C.c_int, [C.c_char_p, _f32p, _f32p, _f32p, _f32p]),
    "SetVQNumNeighbors": (None, [_vp, C.c_int]),
    "SetMinQuantizedPitch": (None, [_vp, C.c_int]),
    "SetMaxQuantizedPitch": (None, [_vp, C.c_int]),
    "ExtractPhone1": (None, [_vp, _f32p, _f32p, _vp]),
    "EstimatePitch1": (None, [_vp, _f32p, _i32p, _f32p, _vp]),
    "GenerateWaveform1": (None, [_vp, _f32p, _i32p, _f32p, _f32p, _vp]),
    "SetCodebook": (None, [_vp, _f32p]),
    "SetAdditiveSpeakerEmbedding": (None, [_vp, _f32p, _vp, _vp]),
    "SetFormantShiftEmbedding": (None, [_vp, _f32p, _vp, _vp]),
    "RegisterKeyValueSpeakerEmbedding": (None, [_vp, _f32p, _vp]),
    "SetKeyValueSpeakerEmbedding": (None, [_vp, C.c_int, _vp, _vp]),
}
ABI_SYMBOLS_RC0 = ["Beatrice20rc0_" + n for n in _RC0]
_LEGACY = ["CreatePhoneExtractor", "DestroyPhoneExtractor", "CreatePhoneContext1",
           "DestroyPhoneContext1", "CreatePitchEstimator", "DestroyPitchEstimator",
           "CreatePitchContext1", "DestroyPitchContext1", "CreateWaveformGenerator",
           "DestroyWaveformGenerator", "CreateWaveformContext1", "DestroyWaveformContext1",
           "ReadPhoneExtractorParameters", "ReadPitchEstimatorParameters",
           "ReadWaveformGeneratorParameters", "ReadNSpeakers", "ReadSpeakerEmbeddings",
           "ExtractPhone1", "SetMinQuantizedPitch", "SetMaxQuantizedPitch", "EstimatePitch1",
           "GenerateWaveform1"]
ABI_SYMBOLS_LEGACY = [g + "_" + n for g in ("Beatrice20a2", "Beatrice20b1") for n in _LEGACY]


# legacy generations (include/beatrice_abi.h: Beatrice20a2_*, Beatrice20b1_*): 256-d phone vector, 384 pitch bins, the speaker
# vector handed to GenerateWaveform1 per hop (reference lib/beatricelib/beatrice.h:39-203)
LEGACY_PHONE_CH, LEGACY_PITCH_BINS = 256, 384
_LEGACY_SIG = {
    "CreatePhoneExtractor": (_vp, []), "DestroyPhoneExtractor": (None, [_vp]),
    "CreatePhoneContext1": (_vp, []), "DestroyPhoneContext1": (None, [_vp]),
    "CreatePitchEstimator": (_vp, []), "DestroyPitchEstimator": (None, [_vp]),
    "CreatePitchContext1": (_vp, []), "DestroyPitchContext1": (None, [_vp]),
    "CreateWaveformGenerator": (_vp, []), "DestroyWaveformGenerator": (None, [_vp]),
    "CreateWaveformContext1": (_vp, []), "DestroyWaveformContext1": (None, [_vp]),
    "ReadPhoneExtractorParameters": (C.c_int, [_vp, C.c_char_p]),
    "ReadPitchEstimatorParameters": (C.c_int, [_vp, C.c_char_p]),
    "ReadWaveformGeneratorParameters": (C.c_int, [_vp, C.c_char_p]),
    "ReadNSpeakers": (C.c_int, [C.c_char_p, _i32p]),
    "ReadSpeakerEmbeddings": (C.c_int, [C.c_char_p, _f32p]),
    "ExtractPhone1": (None, [_vp, _f32p, _f32p, _vp]),
    "SetMinQuantizedPitch": (None, [_vp, C.c_int]),
    "SetMaxQuantizedPitch": (None, [_vp, C.c_int]),
    "EstimatePitch1": (None, [_vp, _f32p, _i32p, _f32p, _vp]),
    "GenerateWaveform1": (None, [_vp, _f32p, _i32p, _f32p, _f32p, _f32p, _vp]),
}


def fptr(a):
    assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_f32p)


def iptr(a):
    assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_i32p)


class Abi:
    """Typed view of any shared library exporting the Beatrice20rc0_* C-ABI."""

    def __init__(self, path):
        if not os.path.exists(path):
            raise FileNotFoundError("beatrice library not built: %s" % path)
        self.path = path
        self.lib = C.CDLL(path, mode=C.RTLD_LOCAL)
        for name, (res, args) in _RC0.items():
            fn = getattr(self.lib, "Beatrice20rc0_" + name)
            fn.restype, fn.argtypes = res, args
            setattr(self, name, fn)


class AbiLegacy:
    """Typed view of a library's Beatrice20a2_* or Beatrice20b1_* entry points (generation = "20a2" | "20b1")."""

    def __init__(self, path, generation="20b1"):
        if not os.path.exists(path):
            raise FileNotFoundError("beatrice library not built: %s" % path)
        self.path, self.generation = path, generation
        self.lib = C.CDLL(path, mode=C.RTLD_LOCAL)
        for name, (res, args) in _LEGACY_SIG.items():
            fn = getattr(self.lib, "Beatrice%s_%s" % (generation, name))
            fn.restype, fn.argtypes = res, args
            setattr(self, name, fn)


class ModelsLegacy:
    """The five files of a legacy package, read as the reference's ProcessorCore0 / 1 read them
    (reference src/common/processor_core_1.cc:165-216)."""

    def __init__(self, abi, model_dir):
        self.abi = abi
        self.phone, self.pitch, self.wave = abi.CreatePhoneExtractor(), abi.CreatePitchEstimator(), abi.CreateWaveformGenerator()
        for obj, fn, name in ((self.phone, abi.ReadPhoneExtractorParameters, "phone_extractor.bin"),
                              (self.pitch, abi.ReadPitchEstimatorParameters, "pitch_estimator.bin"),
                              (self.wave, abi.ReadWaveformGeneratorParameters, "waveform_generator.bin")):
            err = fn(obj, os.path.join(model_dir, name).encode())
            if err:
                raise RuntimeError("%s: Beatrice_ErrorCode %d" % (name, err))
        n = C.c_int(0)
        path = os.path.join(model_dir, "speaker_embeddings.bin").encode()
        err = abi.ReadNSpeakers(path, C.byref(n))
        if err:
            raise RuntimeError("ReadNSpeakers error %d" % err)
        self.n_speakers = n.value
        self.speakers = np.zeros((self.n_speakers + 1, HID), np.float32)      # + the morph slot, as the reference keeps it
        err = abi.ReadSpeakerEmbeddings(path, fptr(self.speakers))
        self.formant = np.zeros((9, HID), np.float32)
        err = err or abi.ReadSpeakerEmbeddings(os.path.join(model_dir, "formant_shift_embeddings.bin").encode(), fptr(self.formant))
        if err:
            raise RuntimeError("ReadSpeakerEmbeddings error %d" % err)

    def close(self):
        a = self.abi
        a.DestroyPhoneExtractor(self.phone)
        a.DestroyPitchEstimator(self.pitch)
        a.DestroyWaveformGenerator(self.wave)


def set_hop_count(fn, contexts, counter):
    """The hop counters of a new stream's (phone, pitch, waveform) contexts through BeatriceHip_SetHopCount[Legacy] (kind 1, 2, 3)."""
    fn.restype, fn.argtypes = C.c_int, [C.c_int, _vp, C.c_int]
    for kind, ctx in enumerate(contexts, 1):
        if fn(kind, ctx, counter) != 0:
            raise RuntimeError("hop counter %d refused (context kind %d)" % (counter, kind))


def get_hop_counts(fn, contexts):
    fn.restype, fn.argtypes = C.c_int, [C.c_int, _vp]
    return tuple(int(fn(kind, ctx)) for kind, ctx in enumerate(contexts, 1))


class StreamLegacy:
    """One stream through a legacy generation's per-hop protocol (reference src/common/processor_core_1.cc:50-143):
    phone, pitch, the host's pitch transform (clamped to [1, 383]), speaker vector = speaker + formant-shift row."""

    def __init__(self, models, speaker=0, formant_index=4, min_q=1, max_q=LEGACY_PITCH_BINS - 1, start_counter=None):
        self.m, self.a = models, models.abi
        a = self.a
        self.pc, self.tc, self.wc = a.CreatePhoneContext1(), a.CreatePitchContext1(), a.CreateWaveformContext1()
        if start_counter is not None:  # test hook, product library only (BeatriceHip_SetHopCountLegacy)
            set_hop_count(a.lib.BeatriceHip_SetHopCountLegacy, (self.pc, self.tc, self.wc), start_counter)
        self.speaker, self.formant_index = speaker, formant_index
        self.pitch_params = {}
        a.SetMinQuantizedPitch(self.tc, min_q)
        a.SetMaxQuantizedPitch(self.tc, max_q)

    def hop_counts(self):
        return get_hop_counts(self.a.lib.BeatriceHip_HopCountLegacy, (self.pc, self.tc, self.wc))

    def hop(self, x160, return_all=False):
        a, m = self.a, self.m
        x = np.ascontiguousarray(x160, np.float32)
        phone = np.zeros(LEGACY_PHONE_CH, np.float32)
        a.ExtractPhone1(m.phone, fptr(x), fptr(phone), self.pc)
        q = np.zeros(1, np.int32)
        feat = np.zeros(4, np.float32)
        a.EstimatePitch1(m.pitch, fptr(x), iptr(q), fptr(feat), self.tc)
        q2 = np.array([min(pitch_transform(int(q[0]), **self.pitch_params), LEGACY_PITCH_BINS - 1)], np.int32)
        spk = np.ascontiguousarray(m.speakers[self.speaker] + m.formant[self.formant_index])      # float32 add, as the host does
        out = np.zeros(OUT_HOP, np.float32)
        a.GenerateWaveform1(m.wave, fptr(phone), iptr(q2), fptr(feat), fptr(spk), fptr(out), self.wc)
        if return_all:
            return out, phone, int(q[0]), feat, int(q2[0]), spk
        return out

    def close(self):
        a = self.a
        a.DestroyPhoneContext1(self.pc)
        a.DestroyPitchContext1(self.tc)
        a.DestroyWaveformContext1(self.wc)


def load_product():
    """The HIP library.  Raises (never falls back) when it is not built or not loadable."""
    return Abi(PRODUCT_LIB)


class SpeakerTables:
    """Caller-owned embedding tables, shaped as the reference host keeps them
    (reference src/common/processor_core_2.cc:335-351: n_speakers+1 slots, last = morph result)."""

    def __init__(self, abi, model_dir):
        path = os.path.join(model_dir, "speaker_embeddings.bin").encode()
        n = C.c_int(0)
        err = abi.ReadNSpeakers(path, C.byref(n))
        if err:
            raise RuntimeError("ReadNSpeakers error %d" % err)
        self.n_speakers = n.value
        s = self.n_speakers + 1
        self.codebooks = np.zeros((s, CODEBOOK, PHONE_CH), np.float32)
        self.additive = np.zeros((s, HID), np.float32)
        self.formant = np.zeros((9, HID), np.float32)
        self.kv = np.zeros((s, KV_LEN, KV_CH), np.float32)
        err = abi.ReadSpeakerEmbeddings(path, fptr(self.codebooks), fptr(self.additive),
                                        fptr(self.formant), fptr(self.kv))
        if err:
            raise RuntimeError("ReadSpeakerEmbeddings error %d" % err)


class Models:
    def __init__(self, abi, model_dir):
        self.abi = abi
        self.phone = abi.CreatePhoneExtractor()
        self.pitch = abi.CreatePitchEstimator()
        self.wave = abi.CreateWaveformGenerator()
        self.embed = abi.CreateEmbeddingSetter()
        for obj, fn, name in ((self.phone, abi.ReadPhoneExtractorParameters, "phone_extractor.bin"),
                              (self.pitch, abi.ReadPitchEstimatorParameters, "pitch_estimator.bin"),
                              (self.wave, abi.ReadWaveformGeneratorParameters, "waveform_generator.bin"),
                              (self.embed, abi.ReadEmbeddingSetterParameters, "embedding_setter.bin")):
            err = fn(obj, os.path.join(model_dir, name).encode())
            if err:
                raise RuntimeError("%s: Beatrice_ErrorCode %d" % (name, err))
        self.tables = SpeakerTables(abi, model_dir)

    def close(self):
        a = self.abi
        a.DestroyPhoneExtractor(self.phone)
        a.DestroyPitchEstimator(self.pitch)
        a.DestroyWaveformGenerator(self.wave)
        a.DestroyEmbeddingSetter(self.embed)


def pitch_transform(q, avg=52.0, intonation=1.0, shift=0.0, correction=0.0, ctype=0):
    """Host pitch math between EstimatePitch1 and GenerateWaveform1, in double precision
    (restates reference src/common/processor_core_2.cc:190-252)."""
    import math
    per = 8.0
    t = avg + (float(q) - avg) * intonation + per * shift
    if correction != 0.0:
        if ctype == 0:
            near = (math.floor(t / per) + 0.5) * per
            d = (t - near) * (2.0 / per)
            t = near if abs(d) < 1e-4 else near + d * math.pow(abs(d), -correction) * (per / 2.0)
        else:
            # C++ std::round: half away from zero
            tt = t / per
            near = (math.floor(tt + 0.5) if tt >= 0 else -math.floor(-tt + 0.5)) * per
            d = (t - near) * (2.0 / per)
            if correction > 1 - 1e-4:
                t = near
            elif d >= 0.0:
                t = near + math.pow(d, 1.0 / (1.0 - correction)) * (per / 2.0)
            else:
                t = near - math.pow(-d, 1.0 / (1.0 - correction)) * (per / 2.0)
    r = math.floor(t + 0.5) if t >= 0 else -math.floor(-t + 0.5)
    return int(min(max(int(r), 1), PITCH_BINS - 1))


class Stream1:
    """One stream through the 1-stream C-ABI with the reference's per-hop call protocol
    (reference src/common/processor_core_2.cc:181-255 and :431-466)."""

    def __init__(self, models, speaker=0, formant_index=4, vq_k=0, min_q=1, max_q=383, start_counter=None):
        self.m, a = models, models.abi
        self.a = a
        self.pc, self.tc = a.CreatePhoneContext1(), a.CreatePitchContext1()
        self.wc, self.ec = a.CreateWaveformContext1(), a.CreateEmbeddingContext()
        if start_counter is not None:  # test hook, product library only: the new contexts' hop counters (BeatriceHip_SetHopCount)
            set_hop_count(a.lib.BeatriceHip_SetHopCount, (self.pc, self.tc, self.wc), start_counter)
        self.kv_count = N_BLOCKS
        self.pitch_params = {}
        self.set_target_speaker(speaker)
        while self.set_kv_block():
            pass
        self.set_formant_index(formant_index)
        a.SetMinQuantizedPitch(self.tc, min_q)
        a.SetMaxQuantizedPitch(self.tc, max_q)
        a.SetVQNumNeighbors(self.pc, vq_k)

    def hop_counts(self):
        """The hop counters of the (phone, pitch, waveform) contexts' next hops (product library only, BeatriceHip_HopCount)."""
        return get_hop_counts(self.a.lib.BeatriceHip_HopCount, (self.pc, self.tc, self.wc))

    def set_target_speaker(self, s):
        t, a = self.m.tables, self.a
        a.SetCodebook(self.pc, fptr(t.codebooks[s]))
        a.SetAdditiveSpeakerEmbedding(self.m.embed, fptr(t.additive[s]), self.ec, self.wc)
        a.RegisterKeyValueSpeakerEmbedding(self.m.embed, fptr(t.kv[s]), self.ec)
        self.kv_count = 0

    def set_formant_index(self, idx):
        self.a.SetFormantShiftEmbedding(self.m.embed, fptr(self.m.tables.formant[idx]), self.ec, self.wc)

    def set_kv_block(self):
        if self.kv_count < N_BLOCKS:
            self.a.SetKeyValueSpeakerEmbedding(self.m.embed, self.kv_count, self.ec, self.wc)
            self.kv_count += 1
            return True
        return False

    def hop(self, x160, return_all=False):
        a = self.a
        x = np.ascontiguousarray(x160, np.float32)
        self.set_kv_block()
        phone = np.zeros(PHONE_CH, np.float32)
        a.ExtractPhone1(self.m.phone, fptr(x), fptr(phone), self.pc)
        q = np.zeros(1, np.int32)
        feat = np.zeros(4, np.float32)
        a.EstimatePitch1(self.m.pitch, fptr(x), iptr(q), fptr(feat), self.tc)
        q2 = np.array([pitch_transform(int(q[0]), **self.pitch_params)], np.int32)
        out = np.zeros(OUT_HOP, np.float32)
        a.GenerateWaveform1(self.m.wave, fptr(phone), iptr(q2), fptr(feat), fptr(out), self.wc)
        if return_all:
            return out, phone, int(q[0]), feat, int(q2[0])
        return out

    def close(self):
        a = self.a
        a.DestroyPhoneContext1(self.pc)
        a.DestroyPitchContext1(self.tc)
        a.DestroyWaveformContext1(self.wc)
        a.DestroyEmbeddingContext(self.ec)


def synth_audio(n_samples, seed=0, sr=16000, silence_gap=False):
    """Deterministic voiced-like test signal: gliding band-limited saw,
    4 Hz syllable envelope, low-level noise.  silence_gap: 0.5 s of digital silence from 0.1 s on (the survey's
    "10 % of the streams contain 0.5 s digital silence gaps"; the harness converts them like anything else)."""
    rng = np.random.Generator(np.random.PCG64(0xBEA7 + seed))
    t = np.arange(n_samples) / sr
    period = 2.0 + 2.0 * rng.random()
    f0 = 90.0 * (400.0 / 90.0) ** (0.5 - 0.5 * np.cos(2 * np.pi * t / period + rng.random() * 6.28))
    ph = 2 * np.pi * np.cumsum(f0) / sr
    x = np.zeros(n_samples)
    for h in range(1, 20):
        x += np.sin(h * ph) / h * (h * f0 < 0.45 * sr)
    env = 0.55 + 0.45 * np.sin(2 * np.pi * 4.0 * t + rng.random() * 6.28)
    x = 0.3 * x / 1.8 * env + 0.0316 * 0.3 * rng.standard_normal(n_samples)
    if silence_gap:
        x[int(0.1 * sr):int(0.6 * sr)] = 0.0
    return x.astype(np.float32)


# ------------------------------------------------------------------------------------------------
# Batched extension ABI (include/beatrice_batch.h)
# ------------------------------------------------------------------------------------------------
_BATCH = {
    "BeatriceHip_LoadPhoneExtractorFromMemory": (C.c_int, [_vp, _vp, C.c_size_t]),
    "BeatriceHip_LoadPitchEstimatorFromMemory": (C.c_int, [_vp, _vp, C.c_size_t]),
    "BeatriceHip_LoadWaveformGeneratorFromMemory": (C.c_int, [_vp, _vp, C.c_size_t]),
    "BeatriceHip_LoadEmbeddingSetterFromMemory": (C.c_int, [_vp, _vp, C.c_size_t]),
    "BeatriceHip_SetDevice": (C.c_int, [C.c_int]),
    "BeatriceHip_GetDevice": (C.c_int, []),
    "BeatriceBatch_Device": (C.c_int, [_vp]),
    "BeatriceHip_MathSelfTest": (C.c_longlong, [C.c_int, C.POINTER(C.c_uint)]),
    "BeatriceHip_MathEval": (C.c_int, [C.c_int, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_uint32)]),
    "BeatriceHip_InvalidateCodebook": (None, [_vp, _vp]),
    "BeatriceHip_InjectTeamTimeout": (C.c_int, [_vp]),
    "BeatriceHip_InjectTeamTimeoutPhone": (C.c_int, [_vp]),
    "BeatriceHip_InjectTeamTimeoutPitch": (C.c_int, [_vp]),
    "BeatriceHip_PitchSpeculation": (C.c_int, [_vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "BeatriceBatch_InjectTeamTimeout": (C.c_int, [_vp]),
    "BeatriceBatch_SetStepCounter": (C.c_int, [_vp, C.c_int]),
    "BeatriceBatch_StepCounter": (C.c_int, [_vp]),
    "BeatriceHip_SetHopCount": (C.c_int, [C.c_int, _vp, C.c_int]),
    "BeatriceHip_SetHopCountLegacy": (C.c_int, [C.c_int, _vp, C.c_int]),
    "BeatriceHip_HopCount": (C.c_int, [C.c_int, _vp]),
    "BeatriceHip_HopCountLegacy": (C.c_int, [C.c_int, _vp]),
    "BeatriceHip_ModelBlob": (C.c_int, [C.c_int, _vp, C.c_int, C.POINTER(_vp), C.POINTER(C.c_size_t)]),
    "BeatriceHip_ModelBlobReady": (C.c_int, [C.c_int, _vp]),
    "BeatriceBatch_Create": (_vp, [_vp, _vp, _vp, _vp, C.c_int, C.c_int]),
    "BeatriceBatch_CreateBlock": (_vp, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int]),
    "BeatriceBatch_HopsPerStep": (C.c_int, [_vp]),
    "BeatriceBatch_StateBytes": (C.c_size_t, [_vp]),
    "BeatriceBatch_Destroy": (None, [_vp]),
    "BeatriceBatch_IsHealthy": (C.c_int, [_vp]),
    "BeatriceBatch_NumStreams": (C.c_int, [_vp]),
    "BeatriceBatch_SetSpeakerTables": (C.c_int, [_vp, C.c_int, _f32p, _f32p, _f32p, _f32p]),
    "BeatriceBatch_BindResidentIO48k": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int]),
    "BeatriceBatch_EnableHostStreaming": (C.c_int, [_vp, C.c_int]),
    "BeatriceBatch_HostStreamDelay": (C.c_int, [_vp]),
    "BeatriceBatch_StreamFrames": (C.c_int, [_vp, _f32p, _f32p]),
    "BeatriceBatch_StreamFlush": (C.c_int, [_vp, _f32p]),
    "BeatriceBatch_SpeakerTablesDevice": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_size_t)]),
    "BeatriceBatch_ProjectSpeakerTables": (C.c_int, [_vp, C.c_int]),
    "BeatriceBatch_UpdateSpeaker": (C.c_int, [_vp, C.c_int, _f32p, _f32p, _f32p]),
    "BeatriceBatch_SeedLottery": (C.c_int, [_vp, C.c_int, C.c_uint]),
    "BeatriceBatch_MorphSpeaker": (C.c_int, [_vp, C.c_int, _f32p, C.c_int, C.c_uint]),
    "BeatriceBatch_EnableSilentBlockRule": (C.c_int, [_vp, C.c_int]),
    "BeatriceBatch_SetSilentStreams": (C.c_int, [_vp, C.c_char_p]),
    "BeatriceBatch_ScanSilentBlocksBegin": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, _i32p, _vp]),
    "BeatriceBatch_ScanSilentBlocksEnd": (C.c_int, [_vp, C.c_int, _u8p]),
    "BeatriceBatch_ScanSilentBlocks": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, _i32p, _vp, _u8p]),
    "BeatriceBatch_ScanBoundBlocks48k": (C.c_int, [_vp, C.c_int, _u8p, _u8p, _vp]),
    "BeatriceBatch_BindResidentBlocks": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int]),
    "BeatriceBatch_ResidentBlocksDelay": (C.c_int, [_vp]),
    "BeatriceBatch_ResidentBlocksDelayFor": (C.c_int, [_vp, C.c_int]),
    "BeatriceBatch_ResidentBlocksOwed": (C.c_int, [_vp]),
    "BeatriceBatch_FlushResidentBlocks": (C.c_int, [_vp]),
    "BeatriceBatch_BindResidentBlocksRagged": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int]),
    "BeatriceBatch_ProcessBlocksRaggedDevice": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "BeatriceBatch_MorphSpeakerStaged": (C.c_int, [_vp, C.c_int, C.c_int, _f32p, C.c_int, C.c_uint]),
    "BeatriceBatch_MorphSpeakersInFlight": (C.c_int, [_vp, C.c_int, _i32p, _i32p, _f32p, C.c_int, C.c_uint]),
    "BeatriceBatch_SpeakerEntryBusy": (C.c_int, [_vp, C.c_int]),
    "BeatriceBatch_InstallSpeakersInFlight": (C.c_int, [_vp, C.c_int, _i32p, _f32p, _f32p, _f32p]),
    "BeatriceBatch_MaxInstallEntries": (C.c_int, [_vp]),
    "BeatriceBatch_GetSpeakerEmbeddings": (C.c_int, [_vp, C.c_int, _f32p, _f32p]),
    "BeatriceBatch_SetTargetSpeaker": (C.c_int, [_vp, C.c_int, C.c_int]),
    "BeatriceBatch_SetTargetSpeakers": (C.c_int, [_vp, C.c_int, _i32p, _i32p]),
    "BeatriceBatch_FlushSpeaker": (C.c_int, [_vp, C.c_int]),
    "BeatriceBatch_SetFormantShift": (C.c_int, [_vp, C.c_int, C.c_double]),
    "BeatriceBatch_SetVQNumNeighbors": (C.c_int, [_vp, C.c_int, C.c_int]),
    "BeatriceBatch_SetMinSourcePitch": (C.c_int, [_vp, C.c_int, C.c_double]),
    "BeatriceBatch_SetMaxSourcePitch": (C.c_int, [_vp, C.c_int, C.c_double]),
    "BeatriceBatch_SetPitchShift": (C.c_int, [_vp, C.c_int, C.c_double]),
    "BeatriceBatch_SetAverageSourcePitch": (C.c_int, [_vp, C.c_int, C.c_double]),
    "BeatriceBatch_SetIntonationIntensity": (C.c_int, [_vp, C.c_int, C.c_double]),
    "BeatriceBatch_SetPitchCorrection": (C.c_int, [_vp, C.c_int, C.c_double]),
    "BeatriceBatch_SetPitchCorrectionType": (C.c_int, [_vp, C.c_int, C.c_int]),
    "BeatriceBatch_ResetStream": (C.c_int, [_vp, C.c_int]),
    "BeatriceBatch_ResetStreamInFlight": (C.c_int, [_vp, C.c_int]),
    "BeatriceBatch_TicksLaunched": (C.c_longlong, [_vp]),
    "BeatriceBatch_StreamBlobBytes": (C.c_size_t, [_vp]),
    "BeatriceBatch_ExportStreams": (C.c_int, [_vp, C.c_int, _i32p, _vp]),
    "BeatriceBatch_ImportStreams": (C.c_int, [_vp, C.c_int, _i32p, _vp, _i32p, C.c_int]),
    "BeatriceBatch_StreamQuiescent": (C.c_int, [_vp, C.c_int]),
    "BeatriceBatch_ExportStreamsInFlight": (C.c_int, [_vp, C.c_int, _i32p, _vp]),
    "BeatriceBatch_ImportStreamsInFlight": (C.c_int, [_vp, C.c_int, _i32p, _vp, _i32p, C.c_int]),
    "BeatriceBatch_MoveStreamsInFlight": (C.c_int, [_vp, _vp, C.c_int, _i32p, _i32p, _i32p, C.c_int]),
    "BeatriceBatch_Stream48kQuiescent": (C.c_int, [_vp, C.c_int]),
    "BeatriceBatch_ExportStreams48kInFlight": (C.c_int, [_vp, C.c_int, _i32p, _vp]),
    "BeatriceBatch_ImportStreams48kInFlight": (C.c_int, [_vp, C.c_int, _i32p, _vp, _i32p, C.c_int]),
    "BeatriceBatch_MoveStreams48kInFlight": (C.c_int, [_vp, _vp, C.c_int, _i32p, _i32p, _i32p, C.c_int]),
    "BeatriceBatch_ConvertFrames": (C.c_int, [_vp, _f32p, _f32p]),
    "BeatriceBatch_ConvertFramesDevice": (C.c_int, [_vp, _vp, _vp]),
    "BeatriceBatch_ConvertBlocks48k": (C.c_int, [_vp, _f32p, _f32p, C.c_int]),
    "BeatriceBatch_ConvertBlocks48kDevice": (C.c_int, [_vp, _vp, _vp, C.c_int]),
    "BeatriceBatch_ConfigureWrapper": (C.c_int, [_vp, C.c_double]),
    "BeatriceBatch_SetInputGain": (C.c_int, [_vp, C.c_int, C.c_double]),
    "BeatriceBatch_SetOutputGain": (C.c_int, [_vp, C.c_int, C.c_double]),
    "BeatriceBatch_ProcessBlocks": (C.c_int, [_vp, _f32p, _f32p, C.c_int, C.c_int]),
    "BeatriceBatch_ProcessBlocksDevice": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int]),
    "BeatriceBatch_MaxWrapperBlock": (C.c_int, [_vp]),
    "BeatriceBatch_ConfigureWrapperRates": (C.c_int, [_vp, C.POINTER(C.c_double)]),
    "BeatriceBatch_ProcessBlocksRagged": (C.c_int, [_vp, _vp, _vp, C.c_int, C.POINTER(C.c_int), C.c_int]),
    "BeatriceBatch_SetStreamRate": (C.c_int, [_vp, C.c_int, C.c_double]),
    "BeatriceBatch_RestartStreamWrapper": (C.c_int, [_vp, C.c_int]),
    "BeatriceBatch_StreamRate": (C.c_double, [_vp, C.c_int]),
    "BeatriceBatch_WrapperBlobBytes": (C.c_size_t, [_vp]),
    "BeatriceBatch_ExportStreamWrappers": (C.c_int, [_vp, C.c_int, _i32p, _vp]),
    "BeatriceBatch_ImportStreamWrappers": (C.c_int, [_vp, C.c_int, _i32p, _vp]),
    "BeatriceBatch_SetStreamRateInFlight": (C.c_int, [_vp, C.c_int, C.c_double]),
    "BeatriceBatch_RestartStreamInFlight": (C.c_int, [_vp, C.c_int, C.c_double, C.c_int]),
    "BeatriceBatch_BoundStreamRate": (C.c_double, [_vp, C.c_int]),
    "BeatriceBatch_BoundStreamQuiescent": (C.c_int, [_vp, C.c_int]),
    "BeatriceBatch_MoveBoundStreamsInFlight": (C.c_int, [_vp, _vp, C.c_int, _i32p, _i32p, _i32p, C.c_int]),
    "BeatriceBatch_ExportBoundStreamsInFlight": (C.c_int, [_vp, C.c_int, _i32p, _vp, _vp]),
    "BeatriceBatch_ImportBoundStreamsInFlight": (C.c_int, [_vp, C.c_int, _i32p, _vp, _vp, _i32p, C.c_int]),
    "BeatriceBatch_BoundWrapperBlobBytes": (C.c_size_t, [_vp]),
    "BeatriceBatch_Synchronize": (C.c_int, [_vp]),
    "BeatriceBatch_BindResidentIO": (C.c_int, [_vp, _vp, _vp, C.c_int]),
    "BeatriceBatch_SetStream": (C.c_int, [_vp, _vp]),
    "BeatriceBatch_GetStream": (_vp, [_vp]),
    "BeatriceBatch_EnableGraph": (C.c_int, [_vp, C.c_int]),
    "BeatriceBatch_EnablePipelining": (C.c_int, [_vp, C.c_int]),
    "BeatriceBatch_GetWaveStream": (_vp, [_vp]),
    "BeatriceBatch_EnableTickPipeline": (C.c_int, [_vp, C.c_int]),
    "BeatriceBatch_TickStages": (C.c_int, [_vp]),
    "BeatriceBatch_TimeTickLaunch": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "BeatriceBatch_Prepare": (C.c_int, [_vp]),
    "BeatriceBatch_DeviceInput": (_vp, [_vp]),
    "BeatriceBatch_DeviceOutput": (_vp, [_vp]),
    "BeatriceBatch_GetIntermediates": (C.c_int, [_vp, _f32p, _i32p, _i32p, _f32p]),
    "BeatriceBatch_TimeSteps": (C.c_int, [_vp, C.c_int, _f32p]),
    "BeatriceBatch_ProfileKernels": (C.c_int, [_vp, C.c_int, C.c_int, C.c_char_p, _i32p,
                                               C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
}
ABI_SYMBOLS_BATCH = list(_BATCH)


def bind_batch(abi):
    """Attach typed prototypes of the batched extension to an Abi (product library only)."""
    if getattr(abi, "_batch_bound", False):
        return abi
    for name, (res, args) in _BATCH.items():
        if os.environ.get("BEATRICE_HIP_LIB") and not hasattr(abi.lib, name):
            continue   # an older build of the library loaded for an A/B measurement: it simply lacks the newer entry points
        fn = getattr(abi.lib, name)
        fn.restype, fn.argtypes = res, args
        setattr(abi, name, fn)
    abi._batch_bound = True
    return abi


class Batch:
    """B concurrent streams on one GPU through include/beatrice_batch.h.

    hops_per_step = 1: one 10 ms hop per step (real time).  2 or 4: block mode, every step converts that
    many consecutive hops per stream (in [B][H*160] -> out [B][H*240]), same results as single hops."""

    def __init__(self, models, n_streams, max_speakers=None, hops_per_step=1, upload_tables=True, start_counter=None):
        self.m = models
        self.a = bind_batch(models.abi)
        t = models.tables if upload_tables else None
        self.B = n_streams
        self.H = hops_per_step
        self._scans = {}  # ticket -> (n_cells, blocks_per_cell) of the scans begun and not ended (scan_silent_blocks_begin)
        if t is None and max_speakers is None:
            raise ValueError("Batch(upload_tables=False) needs max_speakers: without host tables the table size is unknown")
        ms = max_speakers or (t.n_speakers + 1)
        if hops_per_step == 1:
            self.h = self.a.BeatriceBatch_Create(models.phone, models.pitch, models.wave, models.embed, n_streams, ms)
        else:
            self.h = self.a.BeatriceBatch_CreateBlock(models.phone, models.pitch, models.wave, models.embed, n_streams, ms,
                                                      hops_per_step)
        if not self.a.BeatriceBatch_IsHealthy(self.h):
            raise RuntimeError("BeatriceBatch_Create failed (no GPU / HIP error)")
        if start_counter is not None:  # test hook: the new batch's step counter (BeatriceBatch_SetStepCounter)
            self._check(self.a.BeatriceBatch_SetStepCounter(self.h, start_counter))
        if not upload_tables:  # the caller fills the device tables itself (shard.share_speaker_tables)
            return
        self._check(self.a.BeatriceBatch_SetSpeakerTables(self.h, t.n_speakers + 1, fptr(t.codebooks), fptr(t.additive),
                                                          fptr(t.formant), fptr(t.kv)))
        self.apply_defaults()

    def apply_defaults(self):
        # reference host defaults (processor_core_2.h:103-113): speaker 0 with all K/V blocks installed
        self._check(self.a.BeatriceBatch_SetTargetSpeaker(self.h, -1, 0))
        self._check(self.a.BeatriceBatch_FlushSpeaker(self.h, -1))
        self._check(self.a.BeatriceBatch_SetMinSourcePitch(self.h, -1, 33.125))
        self._check(self.a.BeatriceBatch_SetMaxSourcePitch(self.h, -1, 80.875))

    @staticmethod
    def _check(rc):
        if rc != 0:
            raise RuntimeError("BeatriceBatch call failed: %d" % rc)

    def step_counter(self):
        """The step counter of the next step (the host's mirror, BeatriceBatch_StepCounter)."""
        return int(self.a.BeatriceBatch_StepCounter(self.h))

    def convert(self, x):
        x = np.ascontiguousarray(x, np.float32)
        assert x.shape == (self.B, self.H * IN_HOP)
        out = np.zeros((self.B, self.H * OUT_HOP), np.float32)
        self._check(self.a.BeatriceBatch_ConvertFrames(self.h, fptr(x), fptr(out)))
        return out

    def convert48k(self, x, channels):
        """x: [B][channels][480] planar float @48 kHz -> same shape (device-side wrapper, configs[4])."""
        x = np.ascontiguousarray(x, np.float32)
        assert x.shape == (self.B, channels, 480)
        out = np.zeros_like(x)
        self._check(self.a.BeatriceBatch_ConvertBlocks48k(self.h, fptr(x), fptr(out), channels))
        return out

    def intermediates(self):
        shape = (self.B,) if self.H == 1 else (self.B, self.H)
        phone = np.zeros(shape + (PHONE_CH,), np.float32)
        q_raw = np.zeros(shape, np.int32)
        q = np.zeros(shape, np.int32)
        feat = np.zeros(shape + (4,), np.float32)
        self._check(self.a.BeatriceBatch_GetIntermediates(self.h, fptr(phone), iptr(q_raw), iptr(q), fptr(feat)))
        return phone, q_raw, q, feat

    def time_steps(self, steps):
        ms = C.c_float(0)
        self._check(self.a.BeatriceBatch_TimeSteps(self.h, steps, C.byref(ms)))
        return ms.value

    def profile_kernels(self, repeats=10, max_entries=96):
        """[{name, launches, mean_us, flops, bytes}] for one hop (BeatriceBatch_ProfileKernels)."""
        names = C.create_string_buffer(64 * max_entries)
        launches = (C.c_int * max_entries)()
        us = (C.c_double * max_entries)()
        fl = (C.c_double * max_entries)()
        by = (C.c_double * max_entries)()
        n = self.a.BeatriceBatch_ProfileKernels(self.h, repeats, max_entries, names, launches, us, fl, by)
        if n < 0:
            raise RuntimeError("BeatriceBatch_ProfileKernels failed: %d" % n)
        rows = []
        for i in range(n):
            nm = names.raw[64 * i:64 * (i + 1)].split(b"\0")[0].decode()
            rows.append(dict(name=nm, launches=launches[i], mean_us=us[i], flops=fl[i], bytes=by[i]))
        return rows

    def stream_blob_bytes(self):
        """Bytes of one stream's blob (the same for every stream of this batch)."""
        return int(self.a.BeatriceBatch_StreamBlobBytes(self.h))

    def export_streams(self, streams):
        """The state and settings of `streams` as len(streams) blobs back to back (BeatriceBatch_ExportStreams): bytes that
        import_streams of another batch of the same library build and hops per step takes.  Drains; changes nothing."""
        idx = np.ascontiguousarray(streams, np.int32).reshape(-1)
        buf = C.create_string_buffer(max(1, len(idx) * self.stream_blob_bytes()))
        self._check(self.a.BeatriceBatch_ExportStreams(self.h, len(idx), iptr(idx), C.cast(buf, _vp)))
        return buf.raw[:len(idx) * self.stream_blob_bytes()]

    def import_streams(self, streams, blobs, entry_map=None):
        """Blob i of `blobs` (export_streams' bytes) becomes stream streams[i] of this batch (BeatriceBatch_ImportStreams).
        entry_map[i]: the table entry of this batch that holds what entry i of the source batch held (None: the same entries)."""
        idx = np.ascontiguousarray(streams, np.int32).reshape(-1)
        if len(blobs) != len(idx) * self.stream_blob_bytes():
            raise ValueError("import_streams: %d bytes for %d streams of %d bytes each" % (len(blobs), len(idx), self.stream_blob_bytes()))
        em = None if entry_map is None else np.ascontiguousarray(entry_map, np.int32).reshape(-1)
        buf = C.create_string_buffer(bytes(blobs), max(1, len(blobs)))
        self._check(self.a.BeatriceBatch_ImportStreams(self.h, len(idx), iptr(idx), C.cast(buf, _vp),
                                                       None if em is None else iptr(em), 0 if em is None else len(em)))

    def stream_quiescent(self, stream):
        """In plain tick mode: True when no step the stream took part in is inside the pipeline (BeatriceBatch_StreamQuiescent),
        which is when the in-flight calls below take it."""
        rc = int(self.a.BeatriceBatch_StreamQuiescent(self.h, int(stream)))
        if rc < 0:
            raise RuntimeError("BeatriceBatch_StreamQuiescent failed: %d" % rc)
        return rc == 1

    def export_streams_in_flight(self, streams):
        """export_streams' bytes of streams that are quiescent, without draining (BeatriceBatch_ExportStreamsInFlight): waits for the
        ticks already enqueued and its own copy, launches no tick, changes nothing.  Not for an audio thread."""
        idx = np.ascontiguousarray(streams, np.int32).reshape(-1)
        buf = C.create_string_buffer(max(1, len(idx) * self.stream_blob_bytes()))
        self._check(self.a.BeatriceBatch_ExportStreamsInFlight(self.h, len(idx), iptr(idx), C.cast(buf, _vp)))
        return buf.raw[:len(idx) * self.stream_blob_bytes()]

    def import_streams_in_flight(self, streams, blobs, entry_map=None):
        """import_streams into streams that are quiescent, in front of the next tick and without waiting
        (BeatriceBatch_ImportStreamsInFlight); each is turned to its own counter."""
        idx = np.ascontiguousarray(streams, np.int32).reshape(-1)
        if len(blobs) != len(idx) * self.stream_blob_bytes():
            raise ValueError("import_streams_in_flight: %d bytes for %d streams of %d bytes each" % (len(blobs), len(idx), self.stream_blob_bytes()))
        em = None if entry_map is None else np.ascontiguousarray(entry_map, np.int32).reshape(-1)
        buf = C.create_string_buffer(bytes(blobs), max(1, len(blobs)))
        self._check(self.a.BeatriceBatch_ImportStreamsInFlight(self.h, len(idx), iptr(idx), C.cast(buf, _vp),
                                                               None if em is None else iptr(em), 0 if em is None else len(em)))

    def move_streams_in_flight(self, dst, streams, dst_streams, entry_map=None):
        """Quiescent streams of this batch go on as dst_streams of `dst`, a batch on the same device, ring to ring on the device
        (BeatriceBatch_MoveStreamsInFlight): no blob, no host wait.  This batch is unchanged."""
        idx, to = (np.ascontiguousarray(v, np.int32).reshape(-1) for v in (streams, dst_streams))
        if len(idx) != len(to):
            raise ValueError("move_streams_in_flight: %d source streams, %d destination streams" % (len(idx), len(to)))
        em = None if entry_map is None else np.ascontiguousarray(entry_map, np.int32).reshape(-1)
        self._check(self.a.BeatriceBatch_MoveStreamsInFlight(self.h, dst.h, len(idx), iptr(idx), iptr(to),
                                                             None if em is None else iptr(em), 0 if em is None else len(em)))

    def stream48k_quiescent(self, stream):
        """Around the resident 48 kHz blocks (BeatriceBatch_BindResidentIO48k): True when no step the stream took part in is inside
        the pipeline AND the wrapper launch that emits its last block has been enqueued (BeatriceBatch_Stream48kQuiescent), which is
        when the in-flight calls below take it: one call later than stream_quiescent in plain tick mode."""
        rc = int(self.a.BeatriceBatch_Stream48kQuiescent(self.h, int(stream)))
        if rc < 0:
            raise RuntimeError("BeatriceBatch_Stream48kQuiescent failed: %d" % rc)
        return rc == 1

    def export_streams48k_in_flight(self, streams):
        """export_streams_in_flight for a batch bound to resident 48 kHz blocks (BeatriceBatch_ExportStreams48kInFlight): the same
        bytes, the 48 kHz wrapper's state of the stream among them.  Not for an audio thread."""
        idx = np.ascontiguousarray(streams, np.int32).reshape(-1)
        buf = C.create_string_buffer(max(1, len(idx) * self.stream_blob_bytes()))
        self._check(self.a.BeatriceBatch_ExportStreams48kInFlight(self.h, len(idx), iptr(idx), C.cast(buf, _vp)))
        return buf.raw[:len(idx) * self.stream_blob_bytes()]

    def import_streams48k_in_flight(self, streams, blobs, entry_map=None):
        """import_streams_in_flight for a batch bound to resident 48 kHz blocks (BeatriceBatch_ImportStreams48kInFlight)."""
        idx = np.ascontiguousarray(streams, np.int32).reshape(-1)
        if len(blobs) != len(idx) * self.stream_blob_bytes():
            raise ValueError("import_streams48k_in_flight: %d bytes for %d streams of %d bytes each" % (len(blobs), len(idx), self.stream_blob_bytes()))
        em = None if entry_map is None else np.ascontiguousarray(entry_map, np.int32).reshape(-1)
        buf = C.create_string_buffer(bytes(blobs), max(1, len(blobs)))
        self._check(self.a.BeatriceBatch_ImportStreams48kInFlight(self.h, len(idx), iptr(idx), C.cast(buf, _vp),
                                                                  None if em is None else iptr(em), 0 if em is None else len(em)))

    def move_streams48k_in_flight(self, dst, streams, dst_streams, entry_map=None):
        """move_streams_in_flight between two batches bound to resident 48 kHz blocks on one device
        (BeatriceBatch_MoveStreams48kInFlight): the stream's next block in `dst` is the block it would have got here."""
        idx, to = (np.ascontiguousarray(v, np.int32).reshape(-1) for v in (streams, dst_streams))
        if len(idx) != len(to):
            raise ValueError("move_streams48k_in_flight: %d source streams, %d destination streams" % (len(idx), len(to)))
        em = None if entry_map is None else np.ascontiguousarray(entry_map, np.int32).reshape(-1)
        self._check(self.a.BeatriceBatch_MoveStreams48kInFlight(self.h, dst.h, len(idx), iptr(idx), iptr(to),
                                                                None if em is None else iptr(em), 0 if em is None else len(em)))

    def set_stream_rate(self, stream, rate):
        """One stream's SetSampleRate (BeatriceBatch_SetStreamRate): its resampler pair and FIFO restart at `rate`, its gains keep
        their state; an equal rate does nothing.  No other stream changes."""
        self._check(self.a.BeatriceBatch_SetStreamRate(self.h, int(stream), float(rate)))

    def restart_stream_wrapper(self, stream):
        """The same restart at the stream's present rate (BeatriceBatch_RestartStreamWrapper); with BeatriceBatch_ResetStream it
        turns the slot over to a new caller."""
        self._check(self.a.BeatriceBatch_RestartStreamWrapper(self.h, int(stream)))

    def stream_rate(self, stream):
        """The stream's host rate (0.0 on a batch without clocks per stream)."""
        return float(self.a.BeatriceBatch_StreamRate(self.h, int(stream)))

    def set_stream_rate_in_flight(self, stream, rate):
        """One stream's SetSampleRate inside a binding with clocks per stream (BeatriceBatch_SetStreamRateInFlight): nothing drains,
        the owed blocks come out at the old rate, no other stream changes.  A rate the binding has not had allocates: not for an
        audio thread."""
        self._check(self.a.BeatriceBatch_SetStreamRateInFlight(self.h, int(stream), float(rate)))

    def restart_stream_in_flight(self, stream, rate=0.0, reset_model=False):
        """The same restart, also at the present rate (rate = 0.0); reset_model: the stream's next present step is the first step
        of a new stream -- the slot is turned over to a new caller (BeatriceBatch_RestartStreamInFlight)."""
        self._check(self.a.BeatriceBatch_RestartStreamInFlight(self.h, int(stream), float(rate), 1 if reset_model else 0))

    def bound_stream_rate(self, stream):
        """The stream's host rate inside a binding with clocks per stream (0.0 anywhere else)."""
        return float(self.a.BeatriceBatch_BoundStreamRate(self.h, int(stream)))

    def bound_stream_quiescent(self, stream):
        """Inside a binding with clocks per stream: True when the stream is at rest by both rules -- no step of it inside the ticks, the
        output half of every call it handed a block in launched (BeatriceBatch_BoundStreamQuiescent) -- which is when the three calls below
        take it: after BeatriceBatch_ResidentBlocksDelay() calls it sat out."""
        rc = int(self.a.BeatriceBatch_BoundStreamQuiescent(self.h, int(stream)))
        if rc < 0:
            raise RuntimeError("BeatriceBatch_BoundStreamQuiescent failed: %d" % rc)
        return rc == 1

    def bound_wrapper_blob_bytes(self):
        """Bytes of one stream's wrapper blob inside a binding with clocks per stream (0 anywhere else)."""
        return int(self.a.BeatriceBatch_BoundWrapperBlobBytes(self.h))

    def move_bound_streams_in_flight(self, dst, streams, dst_streams, entry_map=None):
        """Streams at rest in this binding go on as dst_streams of `dst`, a batch bound the same way on the same device, with model
        state, settings, wrapper state, rate, clocks and gain ramps (BeatriceBatch_MoveBoundStreamsInFlight): no blob, no host wait, no
        drain.  This batch is unchanged.  A rate `dst` does not hold allocates: not for an audio thread."""
        idx, to = (np.ascontiguousarray(v, np.int32).reshape(-1) for v in (streams, dst_streams))
        if len(idx) != len(to):
            raise ValueError("move_bound_streams_in_flight: %d source streams, %d destination streams" % (len(idx), len(to)))
        em = None if entry_map is None else np.ascontiguousarray(entry_map, np.int32).reshape(-1)
        self._check(self.a.BeatriceBatch_MoveBoundStreamsInFlight(self.h, dst.h, len(idx), iptr(idx), iptr(to),
                                                                  None if em is None else iptr(em), 0 if em is None else len(em)))

    def export_bound_streams_in_flight(self, streams):
        """(stream blobs, wrapper blobs) of streams at rest in this binding, without draining (BeatriceBatch_ExportBoundStreamsInFlight):
        the bytes of export_streams and export_stream_wrappers.  Waits for its own copies; changes nothing."""
        idx = np.ascontiguousarray(streams, np.int32).reshape(-1)
        ns, nw = len(idx) * self.stream_blob_bytes(), len(idx) * self.bound_wrapper_blob_bytes()
        sbuf, wbuf = C.create_string_buffer(max(1, ns)), C.create_string_buffer(max(1, nw))
        self._check(self.a.BeatriceBatch_ExportBoundStreamsInFlight(self.h, len(idx), iptr(idx), C.cast(sbuf, _vp), C.cast(wbuf, _vp)))
        return sbuf.raw[:ns], wbuf.raw[:nw]

    def import_bound_streams_in_flight(self, streams, blobs, wrapper_blobs, entry_map=None):
        """Blob pair i becomes stream streams[i] of this binding, in front of its next block and without waiting
        (BeatriceBatch_ImportBoundStreamsInFlight); the blobs of either export, bound or in order."""
        idx = np.ascontiguousarray(streams, np.int32).reshape(-1)
        if len(blobs) != len(idx) * self.stream_blob_bytes() or len(wrapper_blobs) != len(idx) * self.bound_wrapper_blob_bytes():
            raise ValueError("import_bound_streams_in_flight: %d + %d bytes for %d streams of %d + %d bytes each" %
                             (len(blobs), len(wrapper_blobs), len(idx), self.stream_blob_bytes(), self.bound_wrapper_blob_bytes()))
        em = None if entry_map is None else np.ascontiguousarray(entry_map, np.int32).reshape(-1)
        sbuf = C.create_string_buffer(bytes(blobs), max(1, len(blobs)))
        wbuf = C.create_string_buffer(bytes(wrapper_blobs), max(1, len(wrapper_blobs)))
        self._check(self.a.BeatriceBatch_ImportBoundStreamsInFlight(self.h, len(idx), iptr(idx), C.cast(sbuf, _vp), C.cast(wbuf, _vp),
                                                                    None if em is None else iptr(em), 0 if em is None else len(em)))

    def wrapper_blob_bytes(self):
        """Bytes of one stream's wrapper blob (0 where export_stream_wrappers / import_stream_wrappers are refused)."""
        return int(self.a.BeatriceBatch_WrapperBlobBytes(self.h))

    def export_stream_wrappers(self, streams):
        """The any-rate wrapper's state of `streams` -- rate, resampler clocks, FIFO, gain clocks, filter histories -- as
        len(streams) wrapper blobs back to back (BeatriceBatch_ExportStreamWrappers).  Drains; changes nothing."""
        idx = np.ascontiguousarray(streams, np.int32).reshape(-1)
        size = self.wrapper_blob_bytes()
        buf = C.create_string_buffer(max(1, len(idx) * size))
        self._check(self.a.BeatriceBatch_ExportStreamWrappers(self.h, len(idx), iptr(idx), C.cast(buf, _vp)))
        return buf.raw[:len(idx) * size]

    def import_stream_wrappers(self, streams, blobs):
        """Wrapper blob i of `blobs` becomes the wrapper state of stream streams[i] (BeatriceBatch_ImportStreamWrappers); a rate
        this batch has no class for gets one."""
        idx = np.ascontiguousarray(streams, np.int32).reshape(-1)
        if len(blobs) != len(idx) * self.wrapper_blob_bytes():
            raise ValueError("import_stream_wrappers: %d bytes for %d streams of %d bytes each" % (len(blobs), len(idx), self.wrapper_blob_bytes()))
        buf = C.create_string_buffer(bytes(blobs), max(1, len(blobs)))
        self._check(self.a.BeatriceBatch_ImportStreamWrappers(self.h, len(idx), iptr(idx), C.cast(buf, _vp)))

    def scan_silent_blocks_begin(self, d_blocks, n_cells, blocks_per_cell, channels, n_samples, cell_stride=None, cell_samples=None,
                                 hip_stream=None):
        """Enqueues the shell's silent-block test over device-resident blocks (BeatriceBatch_ScanSilentBlocksBegin) and returns its
        ticket for scan_silent_blocks_end.  d_blocks: a device pointer; cell_stride in floats (None: the cells back to back);
        cell_samples: per-cell lengths (blocks_per_cell = 1).  Up to four tickets may be out; changes nothing of the batch."""
        if cell_stride is None:
            cell_stride = blocks_per_cell * channels * n_samples
        lens = None if cell_samples is None else np.ascontiguousarray(cell_samples, np.int32).reshape(-1)
        if lens is not None and len(lens) != n_cells:
            raise ValueError("scan_silent_blocks: %d lengths for %d cells" % (len(lens), n_cells))
        t = self.a.BeatriceBatch_ScanSilentBlocksBegin(self.h, d_blocks, n_cells, blocks_per_cell, channels, n_samples, cell_stride,
                                                       None if lens is None else iptr(lens), hip_stream)
        if t < 0:
            raise RuntimeError("BeatriceBatch_ScanSilentBlocksBegin failed: %d" % t)
        self._scans[t] = (n_cells, blocks_per_cell)
        return t

    def scan_silent_blocks_end(self, ticket):
        """Waits for that ticket's scan alone and returns its flags, uint8 [n_cells, blocks_per_cell] (1 = silent)."""
        shape = self._scans.pop(ticket, None)   # (the library gives the ticket up whether the wait succeeds or not)
        if shape is None:
            raise RuntimeError("scan_silent_blocks_end: unknown ticket %r" % (ticket,))
        flags = np.zeros(shape, np.uint8)
        self._check(self.a.BeatriceBatch_ScanSilentBlocksEnd(self.h, ticket, flags.ctypes.data_as(_u8p)))
        return flags

    def scan_silent_blocks(self, d_blocks, n_cells, blocks_per_cell, channels, n_samples, cell_stride=None, cell_samples=None, hip_stream=None):
        """Begin + End: uint8 [n_cells, blocks_per_cell], 1 where every sample of a block's down-mix equals 0.0f."""
        return self.scan_silent_blocks_end(self.scan_silent_blocks_begin(d_blocks, n_cells, blocks_per_cell, channels, n_samples, cell_stride,
                                                                         cell_samples, hip_stream))

    def scan_bound_blocks_48k(self, n_calls, hip_stream=None):
        """With BeatriceBatch_BindResidentIO48k bound: (step_flags uint8 [n_calls, B], block_flags uint8 [n_calls, B, H]) of the slots the
        next n_calls calls will read; step_flags[k] is what BeatriceBatch_SetSilentStreams takes before the k-th of them."""
        step = np.zeros((n_calls, self.B), np.uint8)
        block = np.zeros((n_calls, self.B, self.H), np.uint8)
        self._check(self.a.BeatriceBatch_ScanBoundBlocks48k(self.h, n_calls, step.ctypes.data_as(_u8p), block.ctypes.data_as(_u8p), hip_stream))
        return step, block

    def close(self):
        if self.h:
            self.a.BeatriceBatch_Destroy(self.h)
            self.h = None
