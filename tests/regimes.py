"""Model packages and drive signals for the numeric regimes that tools/make_model.py's defaults never reach (test
infrastructure; tests/test_cpu_regimes.py witnesses them with the float64 restatement, tests/test_gpu_regimes.py compares HIP
with the oracle in them bit for bit).

Every package is make_model's own package (same seeds, same tensor order, same model.toml) with some tensors edited
before writing.  Every scale factor is a power of two, so an edit is exact in float32.

hot -- saturating activations.  Factors (HOT; legacy packages HOT_LEGACY):
    phone residual convs x32, x8, x4, x4; pitch GRU W_ih x16; pitch logits Linear x8; every tensor of the four wave blocks
    (c1, c2, q, o) x4; first ConvT of the upsampler x2^-11 (legacy: x2^-13), which brings the PCM back out of tanh's saturation.
    Witnessed by the float64 restatement over 24 hops of synth_audio(seed 2024), speaker 1, formant row 6:
      attention rows with a term s_j - max s < -86:   24 of 24 in each of the four blocks
      gelu arguments beyond |x| > 5, wave block convs:  55 %, 94 %, 99 %, 100 %;  phone residual convs: 40 %, 83 %, 95 %, 98 %
      GRU gate arguments: phone [-2758, 2423], pitch [-80.8, 76.2]  (sigmoid rounds to 0 / 1 beyond +-17)
      f0 rounds to 1.0f in 4 hops;  every output finite;  PCM: 0.0 % at |pcm| >= 0.999, rms 0.54  (legacy: 0.0 %, rms 0.52)
    (x4 on the block tensors alone gives 99.7 % of the PCM at +-1; x2^-6 on the first ConvT still 83 %, x2^-10 5.6 %.)

vanishing -- subnormal values.  Every bias is zero; factors (VANISHING): first front conv of the phone extractor x2^-20; the wave
    generator's input side -- phone Linear, PitchEmb, W_f, the additive and formant projections, the K and V projections of
    every block -- x2^-126 (these WEIGHTS are subnormal themselves, and keep what bits fit); the last conv x2^124, so that the
    PCM is audible and a wrong bit upstream is seen; codebook row i x(1 + (511 - i) / 512), so that the k-NN search has a margin
    when the phone vector vanishes.  Drive: vanishing_audio -- 1e-30 at hop 0, below 1e-44 (then 0) by hop 10, 0.3 from hop 16.
    Witnessed (share of a layer's input values v with 0 < |v| < 2^-126, best hop): phone front convs 100 %, residual convs
    96-100 %, GRU input 72 %, output Linear 57 %; wave blocks c1 64-78 %, c2 97-100 %, q 62-75 %, o 100 %; upsampler 80-100 %;
    FFT input 79 %, frame-energy partials 100 %.  The phone extractor's layers are in the normal range in hop 0 and from hop 12
    on; the wave generator's values straddle 2^-126 in every hop (they hang on the embeddings, not on the level of the audio).
    In float32 the phone GRU's candidate tanh is exactly 0 below 2^-25 (MODEL_SPEC 2.5), so there the output Linear sees exact
    zeros where the restatement sees subnormals.  The legacy generator gets its speaker vector from the host, unscaled: the
    legacy variant reaches the regime in the phone extractor and the pitch front only.

ties -- exact ties (MODEL_SPEC 2.4).  Rows TIE_ROWS = 0, 6, 7, 70, 306, 511 of every speaker's codebook are one row, the float64
    restatement's mean raw phone vector over the drive (xor-distance 1 inside one wave; + 64 and + 300 in other waves; the two
    ends); its distance lies in -55 .. 11 over the hops, the nearest other row's in 65 .. 117.  Columns and biases
    TIE_BINS = 40, 41, 104, 240 of the logits Linear are one column (j and j + 64: one lane, two slots; the others: other lanes) with
    bias 64, against other logits of at most 11.8: the four hold the maximum in every hop, f0 = 1/4.
"""
import os
import sys

import numpy as np

import spec_numpy as sn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import make_model as mm  # noqa: E402

HOPS = 24
N_SPEAKERS = 3
SUBNORMAL = 2.0 ** -126

# ---- positions in make_model's tensor lists (MODEL_SPEC section 5 order) -------------------------------------------------------
PH_FRONT_W, PH_RES_W = [0, 2, 4, 6, 8], [10, 12, 14, 16]
PH_WIH, PH_WHH, PH_WO = 18, 19, 22
PH_BIAS = [1, 3, 5, 7, 9, 11, 13, 15, 17, 20, 21, 23]
PI_P1_W, PI_RES_W, PI_WIH, PI_WHH, PI_WO, PI_BO, PI_V = 2, [4, 6], 8, 9, 12, 13, 14
PI_BIAS = [3, 5, 7, 10, 11, 13, 15]
WG_WI, WG_BI, WG_PITCH_EMB, WG_WF = 0, 1, 2, 3


def wg_block(i, which):
    """position of block i's tensor: c1 (dilated conv), c2 (1x1), q, o; weights (their biases follow at + 1)"""
    return 4 + 8 * i + 2 * ("c1", "c2", "q", "o").index(which)


def wg_up(s, which):
    """position of upsampler stage s's tensor: t (polyphase ConvT), a (res d=1), b (res d=3); weights"""
    return 36 + 6 * s + 2 * ("t", "a", "b").index(which)


WG_FIN_W = 60
WG_BIAS = [1] + [wg_block(i, w) + 1 for i in range(4) for w in ("c1", "c2", "q", "o")] + \
          [wg_up(s, w) + 1 for s in range(4) for w in ("t", "a", "b")] + [61]
ES_ADD_W, ES_FRM_W = 0, 2


def es_kv(i, which):
    return 4 + 4 * i + 2 * ("k", "v").index(which)


ES_BIAS = [1, 3] + [es_kv(i, w) + 1 for i in range(4) for w in ("k", "v")]
# legacy generations: the waveform generator has no attention half (c1, c2 per block), the rest of the order is the same
LWG_BLOCK = {(i, w): 4 + 4 * i + 2 * ("c1", "c2").index(w) for i in range(4) for w in ("c1", "c2")}


def lwg_up(s, which):
    return 20 + 6 * s + 2 * ("t", "a", "b").index(which)


LWG_FIN_W = 44
LWG_BIAS = [1] + [LWG_BLOCK[i, w] + 1 for i in range(4) for w in ("c1", "c2")] + \
           [lwg_up(s, w) + 1 for s in range(4) for w in ("t", "a", "b")] + [45]

SEED, LEGACY_SEED = 0x20C0, 0x20B1


def default_tensors(n_speakers=N_SPEAKERS, seed=SEED):
    """make_model.make_model's tensors, by file name, as lists that may be edited in place"""
    out = {}
    for name, fn in (("phone_extractor", mm.phone_extractor), ("pitch_estimator", mm.pitch_estimator),
                     ("waveform_generator", mm.waveform_generator), ("embedding_setter", mm.embedding_setter)):
        out[name] = fn(mm.Stream(seed + mm.KIND[name]))
    out["speaker_embeddings"] = mm.speaker_embeddings(mm.Stream(seed + mm.KIND["speaker_embeddings"]), n_speakers)
    return out


def default_legacy_tensors(seed=LEGACY_SEED):
    out = {}
    for name, fn in (("phone_extractor", mm.legacy_phone_extractor), ("pitch_estimator", mm.legacy_pitch_estimator),
                     ("waveform_generator", mm.legacy_waveform_generator)):
        out[name] = fn(mm.Stream(seed + mm.LEGACY_KIND[name]))
    return out


def write_package(out_dir, tensors, n_speakers=N_SPEAKERS, seed=SEED):
    """make_model's package (model.toml and every file), then the edited tensor files over it"""
    mm.make_model(out_dir, n_speakers=n_speakers, seed=seed)
    for name, t in tensors.items():
        mm.write_file(os.path.join(out_dir, name + ".bin"), name, t)
    return out_dir


def write_legacy_package(out_dir, tensors, n_speakers=N_SPEAKERS, seed=LEGACY_SEED, version="2.0.0-beta.1"):
    mm.make_model_legacy(out_dir, n_speakers=n_speakers, seed=seed, version=version)
    for name, t in tensors.items():
        mm.write_legacy_file(os.path.join(out_dir, name + ".bin"), name, t)
    return out_dir


def scale(tensors, positions, factor):
    m, e = np.frexp(factor)
    assert m == 0.5, "scale factors are powers of two: the edit must be exact"
    for p in ([positions] if isinstance(positions, int) else positions):
        before = tensors[p]
        tensors[p] = (before * np.float32(factor)).astype(np.float32)
        normal = np.abs(tensors[p]) >= SUBNORMAL    # (a weight scaled into the subnormal range keeps what bits fit there)
        assert np.array_equal(tensors[p].astype(np.float64)[normal], (before.astype(np.float64) * factor)[normal]), "inexact scaling"


def zero(tensors, positions):
    for p in positions:
        tensors[p] = np.zeros_like(tensors[p])


# ---- hot ---------------------------------------------------------------------------------------------------------------
HOT = dict(phone_res=(32.0, 8.0, 4.0, 4.0), phone_wih=1.0, pitch_wih=16.0, pitch_wo=8.0, block=4.0, up0_t=2.0 ** -11)


def _hot_common(t, wg_pos, f=HOT):
    for p, factor in zip(PH_RES_W, f["phone_res"]):
        scale(t["phone_extractor"], p, factor)
    scale(t["phone_extractor"], PH_WIH, f["phone_wih"])
    scale(t["pitch_estimator"], PI_WIH, f["pitch_wih"])
    scale(t["pitch_estimator"], PI_WO, f["pitch_wo"])
    scale(t["waveform_generator"], wg_pos, f["block"])


def hot_tensors(f=HOT):
    t = default_tensors()
    _hot_common(t, [wg_block(i, w) for i in range(4) for w in ("c1", "c2", "q", "o")], f)
    scale(t["waveform_generator"], wg_up(0, "t"), f["up0_t"])
    return t


HOT_LEGACY = dict(HOT, up0_t=2.0 ** -13)     # (no attention half to average the blocks' output: the generator runs hotter)


def hot_legacy_tensors(f=HOT_LEGACY):
    t = default_legacy_tensors()
    _hot_common(t, [LWG_BLOCK[i, w] for i in range(4) for w in ("c1", "c2")], f)
    scale(t["waveform_generator"], lwg_up(0, "t"), f["up0_t"])
    return t


# ---- vanishing ---------------------------------------------------------------------------------------------------------
VANISHING = dict(phone_in=2.0 ** -20, wave_in=2.0 ** -126, wave_kv=2.0 ** -126, fin=2.0 ** 124)


def vanishing_tensors(f=VANISHING):
    t = default_tensors()
    zero(t["phone_extractor"], PH_BIAS)
    zero(t["pitch_estimator"], PI_BIAS)
    zero(t["waveform_generator"], WG_BIAS)
    zero(t["embedding_setter"], ES_BIAS)
    scale(t["phone_extractor"], PH_FRONT_W[0], f["phone_in"])
    scale(t["waveform_generator"], [WG_WI, WG_PITCH_EMB, WG_WF], f["wave_in"])
    scale(t["embedding_setter"], [ES_ADD_W, ES_FRM_W], f["wave_in"])
    scale(t["embedding_setter"], [es_kv(i, w) for i in range(4) for w in ("k", "v")], f["wave_kv"])
    scale(t["waveform_generator"], WG_FIN_W, f["fin"])
    # a vanishing phone vector is equally far from every unit-norm codebook row: spread the norms (row i times 1 + (511 - i) / 512), so that
    # the k-NN choice has a margin there and can be compared with the restatement
    sp = t["speaker_embeddings"]
    for s in range(N_SPEAKERS):
        cb = sp[1 + 3 * s].reshape(sn.CODEBOOK, sn.PHONE_CH).astype(np.float64)
        sp[1 + 3 * s] = (cb * (1.0 + np.arange(sn.CODEBOOK)[::-1, None] / 512.0)).astype(np.float32)
    return t


def vanishing_legacy_tensors(f=VANISHING):
    """(the legacy generator takes its speaker vector from the host per hop, unscaled: only the phone extractor, the pitch front and
    the wrapper see the vanishing signal there; the generator's input side is scaled down as far as its own tensors reach)"""
    t = default_legacy_tensors()
    zero(t["phone_extractor"], PH_BIAS)
    zero(t["pitch_estimator"], PI_BIAS)
    zero(t["waveform_generator"], LWG_BIAS)
    scale(t["phone_extractor"], PH_FRONT_W[0], f["phone_in"])
    return t


def vanishing_audio(bv, hops=HOPS, seed=7):
    """A tail that decays from 1e-30 through the whole subnormal range to below 1e-44 (where float32 has nothing left but 0),
    comes back up to 0.3 and stays there: values enter and leave the subnormal range in both directions."""
    n = hops * sn.IN_HOP
    x = bv.synth_audio(n, seed=seed).astype(np.float64) / 0.3
    t = np.arange(n) / float(sn.IN_HOP)                       # in hops
    down, up = 10.0, 16.0                                      # the bottom is reached after 10 hops, 0.3 again after 16
    log_env = np.where(t < down, -30.0 + (-46.5 + 30.0) * t / down,
                       np.where(t < up, -46.5 + (np.log10(0.3) + 46.5) * (t - down) / (up - down), np.log10(0.3)))
    return (x * 10.0 ** log_env).astype(np.float32)


# ---- ties --------------------------------------------------------------------------------------------------------------
TIE_ROWS = (0, 6, 7, 70, 306, 511)     # copies of one codebook row: 6^7 = 1 (same wave), 6+64, 6+300 (other waves), the ends
TIE_BINS = (40, 41, 104, 240)          # duplicated logit columns: j, j+1 (next lane), j+64 (same lane, next slot), j+200
TIES = dict(codebook_gain=1.0, logit_bias=64.0)


def ties_tensors(bv, phone_mean=None, f=TIES):
    """phone_mean: the float64 restatement's mean raw phone vector over the drive signal (tests pass it in; None computes it)"""
    t = default_tensors()
    if phone_mean is None:
        phone_mean = ties_phone_mean(bv)
    row = (np.asarray(phone_mean, np.float64) * f["codebook_gain"]).astype(np.float32)
    sp = t["speaker_embeddings"]
    for s in range(N_SPEAKERS):
        cb = sp[1 + 3 * s].reshape(sn.CODEBOOK, sn.PHONE_CH).copy()
        cb[list(TIE_ROWS)] = row
        sp[1 + 3 * s] = cb
    pi = t["pitch_estimator"]
    wo = pi[PI_WO].reshape(128, sn.BINS).copy()
    bo = pi[PI_BO].copy()
    j = TIE_BINS[0]
    bo[j] = np.float32(f["logit_bias"])
    for c in TIE_BINS[1:]:
        wo[:, c], bo[c] = wo[:, j], bo[j]
    pi[PI_WO], pi[PI_BO] = wo.ravel(), bo
    return t


def ties_audio(bv, hops=HOPS):
    return bv.synth_audio(hops * sn.IN_HOP, seed=2024)


def ties_phone_mean(bv):
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        write_package(d, default_tensors())
        _, raw, _ = sn.PhoneExtractor(d)(ties_audio(bv))
    return raw.mean(0)


REGIMES = {"hot": hot_tensors, "vanishing": vanishing_tensors, "ties": ties_tensors}
LEGACY_REGIMES = {"hot": hot_legacy_tensors, "vanishing": vanishing_legacy_tensors}


def regime_audio(bv, regime, hops=HOPS, seed=2024):
    if regime == "vanishing":
        return vanishing_audio(bv, hops, seed=seed)
    return bv.synth_audio(hops * sn.IN_HOP, seed=seed)


# ---- witnesses: the float64 restatement, end to end, with every probe recorded -----------------------------------------------
def restate(model_dir, audio, speaker=1, formant_index=4, vq_k=0, wave=True):
    """-> (rec, out): the probes of one end-to-end float64 run and its outputs (wave=False: without the generator, pcm None)"""
    raw = open(os.path.join(model_dir, "speaker_embeddings.bin"), "rb").read()
    flat = np.frombuffer(raw, "<f4", offset=16).astype(np.float64)
    per = sn.CODEBOOK * sn.PHONE_CH + sn.HID + sn.KV_LEN * sn.KV_CH
    formant = flat[:9 * sn.HID].reshape(9, sn.HID)
    base = 9 * sn.HID + speaker * per
    cb = flat[base:base + sn.CODEBOOK * sn.PHONE_CH].reshape(sn.CODEBOOK, sn.PHONE_CH)
    add = flat[base + sn.CODEBOOK * sn.PHONE_CH:][:sn.HID]
    kv = flat[base + sn.CODEBOOK * sn.PHONE_CH + sn.HID:][:sn.KV_LEN * sn.KV_CH].reshape(sn.KV_LEN, sn.KV_CH)
    with sn.recording() as rec, np.errstate(all="ignore"):
        phone, raw_phone, dist = sn.PhoneExtractor(model_dir)(audio, codebook=cb, k=vq_k)
        bins, feat, logits = sn.PitchEstimator(model_dir)(audio, 1, sn.BINS - 1)
        pcm = sn.WaveformGenerator(model_dir)(phone, bins, feat, add, formant[formant_index], kv) if wave else None
    return rec, dict(phone=phone, raw_phone=raw_phone, dist=dist, bins=bins, feat=feat, logits=logits, pcm=pcm)


def per_hop(a, hops=HOPS):
    """a probe's rows grouped by the hop they belong to: [hops][...]"""
    a = np.asarray(a)
    return a.reshape(hops, -1)


def subnormal_share(a, hops=HOPS):
    """per hop, the share of values v with 0 < |v| < 2^-126"""
    v = np.abs(per_hop(a, hops))
    return ((v > 0) & (v < SUBNORMAL)).mean(1)


# the inputs of every GEMM layer of the phone extractor (the GRU's recurrent product included) and of the wave generator's blocks
# (both operands of the two attention products included), upsampler and last conv.  Not here: the generator's input Linear, whose
# input is the phone vector itself -- at least 2^-25 where it is not 0 (MODEL_SPEC 2.5), or a codebook mean -- and the pitch
# estimator's layers, which sit behind log(|X|^2 + 1e-5).
GEMM_INPUTS = ["phone.F%d.in" % i for i in range(5)] + ["phone.R%d.in" % i for i in range(4)] + \
              ["phone.gru.in", "phone.gru.h.in", "phone.out.in"] + \
              ["wave.B%d.%s.in" % (i, w) for i in range(4) for w in ("c1", "c2", "q", "o")] + \
              ["wave.B%d.att.%s" % (i, w) for i in range(4) for w in ("q", "k", "v")] + \
              ["wave.U%d.%s.in" % (s, w) for s in range(4) for w in ("t", "a", "b")] + ["wave.fin.in"]
PHONE_LAYERS = [n for n in GEMM_INPUTS if n.startswith("phone.")]


# ---- packages and drives shared by the CPU and the GPU tests -------------------------------------------------------------------
def package(bv, regime, out_dir, legacy=False):
    if legacy:
        return write_legacy_package(out_dir, LEGACY_REGIMES[regime]())
    return write_package(out_dir, ties_tensors(bv) if regime == "ties" else REGIMES[regime]())


def drive(bv, abi, model_dir, audio, change=None, **stream):
    """One stream through the 1-stream ABI of `abi` (oracle or product), every intermediate kept per hop.
    change(stream1, hop) runs before each hop."""
    m = bv.Models(abi, model_dir)
    st = bv.Stream1(m, **stream)
    outs = []
    for h in range(audio.size // sn.IN_HOP):
        if change is not None:
            change(st, h)
        outs.append(st.hop(audio[h * sn.IN_HOP:(h + 1) * sn.IN_HOP], return_all=True))
    st.close()
    tables = m.tables
    m.close()
    return dict(pcm=np.concatenate([o[0] for o in outs]), phone=np.stack([o[1] for o in outs]), q=np.array([o[2] for o in outs]),
                feat=np.stack([o[3] for o in outs]), tables=tables)


def drive_legacy(bv, abi_legacy, model_dir, audio, **stream):
    m = bv.ModelsLegacy(abi_legacy, model_dir)
    st = bv.StreamLegacy(m, **stream)
    outs = [st.hop(audio[h * sn.IN_HOP:(h + 1) * sn.IN_HOP], return_all=True) for h in range(audio.size // sn.IN_HOP)]
    st.close()
    m.close()
    return dict(pcm=np.concatenate([o[0] for o in outs]), phone=np.stack([o[1] for o in outs]), q=np.array([o[2] for o in outs]),
                feat=np.stack([o[3] for o in outs]), spk=np.stack([o[5] for o in outs]))
