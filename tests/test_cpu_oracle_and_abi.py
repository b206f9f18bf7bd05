"""CPU-side checks: oracle vs its committed self-test vector, file-reader error codes on both
libraries, host pitch math known answers, and that the product library loads and exports every
symbol declared in include/*.h (no compute call is made: there is no GPU here)."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")


def test_oracle_matches_core_selftest_vector(bv, oracle, model_dir):
    g = np.load(os.path.join(GOLD, "core_selftest.npz"))
    m = bv.Models(oracle, model_dir)
    assert m.tables.n_speakers == int(g["speakers"][0])
    s = bv.Stream1(m, speaker=0, vq_k=2)
    x = g["audio"]
    for i in range(16):
        if i == 6:
            s.set_target_speaker(2)
        o, ph, q, f, _ = s.hop(x[i * 160:(i + 1) * 160], return_all=True)
        assert q == int(g["q"][i])
        assert np.array_equal(ph, g["phone"][i])
        assert np.array_equal(f, g["feat"][i])
        assert np.array_equal(o, g["out"][i])
    s.close()
    m.close()


def test_streaming_state_is_per_context(bv, oracle, model_dir):
    """Two contexts on one model are independent; a fresh context reproduces the first hops."""
    m = bv.Models(oracle, model_dir)
    x = bv.synth_audio(160 * 6, seed=11)
    a, b = bv.Stream1(m, speaker=1), bv.Stream1(m, speaker=1)
    outs_a = [a.hop(x[i * 160:(i + 1) * 160]) for i in range(6)]
    b.hop(np.zeros(160, np.float32))  # perturb b's history
    outs_b = [b.hop(x[i * 160:(i + 1) * 160]) for i in range(6)]
    c = bv.Stream1(m, speaker=1)
    outs_c = [c.hop(x[i * 160:(i + 1) * 160]) for i in range(6)]
    assert all(np.array_equal(p, q) for p, q in zip(outs_a, outs_c))
    assert not np.array_equal(outs_a[0], outs_b[0])
    for s in (a, b, c):
        s.close()
    m.close()


def _reader_cases(tmp_path, model_dir):
    src = open(os.path.join(model_dir, "phone_extractor.bin"), "rb").read()
    cases = {}
    for name, data in (("small", src[:-4]), ("large", src + b"\0\0\0\0"), ("tiny", src[:8]),
                       ("magic", b"XXXX" + src[4:]), ("kind", src[:4] + struct.pack("<I", 3) + src[8:])):
        p = tmp_path / (name + ".bin")
        p.write_bytes(data)
        cases[name] = str(p).encode()
    cases["missing"] = str(tmp_path / "nope.bin").encode()
    return cases


def _check_reader_errors(bv, abi, tmp_path, model_dir):
    c = _reader_cases(tmp_path, model_dir)
    obj = abi.CreatePhoneExtractor()
    # reference lib/beatricelib/beatrice.h:30-37
    assert abi.ReadPhoneExtractorParameters(obj, c["missing"]) == 1  # kFileOpenError
    assert abi.ReadPhoneExtractorParameters(obj, c["small"]) == 2    # kFileTooSmall
    assert abi.ReadPhoneExtractorParameters(obj, c["tiny"]) == 2
    assert abi.ReadPhoneExtractorParameters(obj, c["large"]) == 3    # kFileTooLarge
    assert abi.ReadPhoneExtractorParameters(obj, c["magic"]) == 4    # kInvalidFileSize
    assert abi.ReadPhoneExtractorParameters(obj, c["kind"]) == 4
    abi.DestroyPhoneExtractor(obj)
    spk = open(os.path.join(model_dir, "speaker_embeddings.bin"), "rb").read()
    bad = tmp_path / "spk_bad.bin"
    n_floats = (len(spk) - 16) // 4 - 100
    bad.write_bytes(spk[:8] + struct.pack("<II", 1, n_floats) + spk[16:16 + 4 * n_floats])
    n = C.c_int(-1)
    assert abi.ReadNSpeakers(str(bad).encode(), C.byref(n)) == 4     # not a whole number of speakers
    assert abi.ReadNSpeakers(os.path.join(model_dir, "speaker_embeddings.bin").encode(), C.byref(n)) == 0 and n.value == 3


def test_reader_error_codes_oracle(bv, oracle, tmp_path, model_dir):
    _check_reader_errors(bv, oracle, tmp_path, model_dir)


def test_reader_error_codes_product(bv, product, tmp_path, model_dir):
    """Validation happens before any device work, so the error paths run without a GPU."""
    _check_reader_errors(bv, product, tmp_path, model_dir)


def _declared_symbols():
    names = set()
    for hdr in ("beatrice_abi.h", "beatrice_batch.h"):
        text = open(os.path.join(REPO, "include", hdr)).read()
        names.update(re.findall(r"\b(BeatriceBatch_[A-Za-z0-9]+|BeatriceHip_[A-Za-z0-9]+)\s*\(", text))
    return names


def test_product_exports_every_declared_symbol(bv, product):
    lib = product.lib
    missing = [s for s in bv.ABI_SYMBOLS_RC0 + bv.ABI_SYMBOLS_LEGACY + sorted(_declared_symbols()) if not hasattr(lib, s)]
    assert not missing, missing
    assert set(bv.ABI_SYMBOLS_BATCH) == _declared_symbols()  # python prototypes cover the whole batch header
    assert len(bv.ABI_SYMBOLS_RC0) == 33 and len(bv.ABI_SYMBOLS_LEGACY) == 44


def test_host_library_exports_every_declared_symbol():
    """include/beatrice_host.h (the C view of the ProcessorCore2 / ProcessorProxy mirrors) vs libbeatrice_host.so."""
    text = open(os.path.join(REPO, "include", "beatrice_host.h")).read()
    names = set(re.findall(r"\b(Beatrice(?:Host|Proxy)_[A-Za-z0-9]+)\s*\(", text))
    assert len(names) >= 40
    lib = C.CDLL(os.path.join(REPO, "beatrice-vst_amd", "host", "libbeatrice_host.so"))
    missing = [s for s in sorted(names) if not hasattr(lib, s)]
    assert not missing, missing
    # and the other way round: no undeclared BeatriceHost_/BeatriceProxy_ export
    import subprocess
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(REPO, "beatrice-vst_amd", "host", "libbeatrice_host.so")]).decode()
    exported = set(re.findall(r"\b(Beatrice(?:Host|Proxy)_[A-Za-z0-9]+)\b", out))
    assert exported == names, sorted(exported ^ names)


_C_TYPE_WORDS = {"void", "char", "short", "int", "long", "float", "double", "signed", "unsigned", "const", "volatile", "struct", "enum"}


def _param_type(decl):
    """`const float* input` -> `const float*`: the type of a parameter (or a return type), without the parameter's name and without a
    qualifier of the parameter itself, which is not part of the function's type (`T* const` -> `T*`, `const int` -> `int`)."""
    tok = re.findall(r"\w+|\*", decl)
    if len(tok) > 1 and re.match(r"\w", tok[-1]) and tok[-1] not in _C_TYPE_WORDS and tok[-2] not in ("struct", "enum"):
        tok = tok[:-1]
    if tok[-1:] == ["const"]:
        tok = tok[:-1]
    elif "*" not in tok:
        tok = [t for t in tok if t != "const"]
    return " ".join(tok).replace(" *", "*")


def _abi_view(header, compiler, std):
    """What a caller binds from a beatricelib header, as `compiler` reads it in `std`: {function: its type as
    `return(param,...)`}, {typedef name: `struct tag` / `enum tag`} and {error code: value}."""
    import subprocess
    text = subprocess.check_output([compiler, std, "-E", "-P", "-x", "c" if compiler == "gcc" else "c++", header]).decode()
    text = " ".join(text.split())
    funcs, typedefs, codes = {}, {}, {}
    for st in re.split(r"[;{}]", text):
        m = re.fullmatch(r"\s*(.*?)\b(Beatrice20(?:a2|b1|rc0)_\w+)\s*\((.*)\)\s*", st)
        if m:
            funcs[m.group(2)] = "%s(%s)" % (_param_type(m.group(1)), ",".join(_param_type(p) for p in m.group(3).split(",")))
    for kind, tag, alias in re.findall(r"typedef (struct|enum) (\w+)\s*(?:\{[^}]*\})?\s*(\w+)\s*;", text):
        typedefs[alias] = kind + " " + tag
    value = -1
    for e in re.search(r"enum Beatrice_ErrorCode\s*\{([^}]*)\}", text).group(1).split(","):
        name, _, v = e.strip().partition("=")
        if name:
            value = int(v) if v.strip() else value + 1
            codes[name.strip()] = value
    return funcs, typedefs, codes


def _fingerprint(function_type):
    import hashlib
    return hashlib.sha256(function_type.encode()).hexdigest()[:16] if function_type is not None else None


def _reference_abi():
    """The reference header's C-ABI, recorded with _abi_view (tests/golden/reference_abi.json: names, a fingerprint of every
    function's type, typedefs, error codes)."""
    import json
    return json.load(open(os.path.join(GOLD, "reference_abi.json")))


def test_declarations_match_reference_header():
    """Every function name the reference header declares is declared by ours, and no other."""
    want = set(_reference_abi()["functions"])
    have = set(_abi_view(os.path.join(REPO, "include", "beatrice_abi.h"), "gcc", "-std=c11")[0])
    assert want == have and len(want) == 77, sorted(want ^ have)


def test_legacy_generations_link_and_decline(product):
    """20a2/20b1 are link stubs: readers fail (host falls back to 'unloaded'), per-hop calls give silence."""
    lib = product.lib
    for g in ("Beatrice20a2", "Beatrice20b1"):
        create = getattr(lib, g + "_CreatePhoneExtractor")
        create.restype = C.c_void_p
        obj = create()
        read = getattr(lib, g + "_ReadPhoneExtractorParameters")
        read.argtypes = [C.c_void_p, C.c_char_p]
        assert read(obj, b"/nonexistent") == 1
        destroy = getattr(lib, g + "_DestroyPhoneExtractor")
        destroy.argtypes = [C.c_void_p]
        destroy(obj)


def test_pitch_transform_known_answers(bv):
    """processor_core_2.cc:190-252 cannot be compiled here (toml11 absent), so the restatements are
    checked against values derived by hand from that code."""
    import wrapperlib
    wo = C.CDLL(wrapperlib.ORACLE_WRAPPER)
    wo.wo_pitch_transform.argtypes = [C.c_int] + [C.c_double] * 4 + [C.c_int]

    def both(q, **kw):
        a = bv.pitch_transform(q, **kw)
        b = wo.wo_pitch_transform(q, kw.get("avg", 52.0), kw.get("intonation", 1.0), kw.get("shift", 0.0),
                                  kw.get("correction", 0.0), kw.get("ctype", 0))
        assert a == b, (q, kw, a, b)
        return a

    for q in (1, 100, 447):
        assert both(q) == q                               # identity at defaults
    assert both(100, shift=12.0) == 196                   # 8 bins per semitone
    assert both(440, shift=24.0) == 447 and both(5, shift=-24.0) == 1  # clamp to [1, 447]
    assert both(100, intonation=0.0) == 52                # collapses onto average_source_pitch
    assert both(100, intonation=2.0) == 148
    assert both(101, correction=1.0, ctype=1) == 104      # snap to nearest semitone (13*8)
    assert both(99, correction=1.0, ctype=1) == 96
    # type 0 pushes away from the midpoint (100 = 12.5 semitones) toward the semitones
    assert both(101, correction=1.0, ctype=0) == 104 and both(99, correction=1.0, ctype=0) == 96
    assert both(100, correction=0.5, ctype=0) == 100      # |x| < 1e-4 stays on the midpoint
    for q in range(1, 448, 7):                            # monotone pull toward the semitone for type 1
        for p in (0.3, 0.7):
            t = both(q, correction=p, ctype=1)
            near = round(q / 8.0) * 8
            assert abs(t - near) <= abs(q - near)


def test_product_without_gpu_emits_silence_not_crash(bv, product, model_dir):
    """Boundary rule: void entry points never fail -- on an internal HIP error
    (here: no device) they leave zeros.  Readers still validate files; a valid file cannot be uploaded
    without a device and reports kFileOpenError.  Skipped when a GPU is present."""
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("GPU present: covered by the gpu-marked parity tests")
    except ImportError:
        pass
    pe = product.CreatePhoneExtractor()
    rc = product.ReadPhoneExtractorParameters(pe, os.path.join(model_dir, "phone_extractor.bin").encode())
    assert rc == 1  # upload impossible -> the model stays unloaded
    pc, tc, wc, ec = (product.CreatePhoneContext1(), product.CreatePitchContext1(), product.CreateWaveformContext1(),
                      product.CreateEmbeddingContext())
    x = np.ones(160, np.float32)
    phone = np.full(128, 7.0, np.float32)
    product.ExtractPhone1(pe, bv.fptr(x), bv.fptr(phone), pc)
    assert not phone.any()
    q = np.full(1, 99, np.int32)
    feat = np.full(4, 7.0, np.float32)
    pt = product.CreatePitchEstimator()
    product.EstimatePitch1(pt, bv.fptr(x), bv.iptr(q), bv.fptr(feat), tc)
    assert q[0] == 1 and not feat.any()
    wg = product.CreateWaveformGenerator()
    out = np.full(240, 7.0, np.float32)
    product.GenerateWaveform1(wg, bv.fptr(phone), bv.iptr(q), bv.fptr(feat), bv.fptr(out), wc)
    assert not out.any()
    product.SetVQNumNeighbors(pc, 3)
    product.SetMinQuantizedPitch(tc, 5)
    bv.bind_batch(product)
    es = product.CreateEmbeddingSetter()
    b = product.BeatriceBatch_Create(pe, pt, wg, es, 4, 2)
    assert product.BeatriceBatch_IsHealthy(b) == 0
    assert product.BeatriceBatch_SetTargetSpeaker(b, 0, 0) == -2
    product.BeatriceBatch_Destroy(b)
    for obj, fn in ((pc, product.DestroyPhoneContext1), (tc, product.DestroyPitchContext1), (wc, product.DestroyWaveformContext1),
                    (ec, product.DestroyEmbeddingContext), (pe, product.DestroyPhoneExtractor), (pt, product.DestroyPitchEstimator),
                    (wg, product.DestroyWaveformGenerator), (es, product.DestroyEmbeddingSetter)):
        fn(obj)


def test_model_toml_has_the_schema_the_reference_reader_asks_for(model_dir):
    """model.toml next to the five .bin files: every key that reference src/common/model_config.h:73-136 looks up
    (a missing one makes its reader throw), the rc0 version string (:25-35), voice ids contiguous from 0."""
    import os
    import tomli
    with open(os.path.join(model_dir, "model.toml"), "rb") as f:
        doc = tomli.load(f)
    assert doc["model"]["version"] == "2.0.0-rc.0"
    assert isinstance(doc["model"]["name"], str) and isinstance(doc["model"]["description"], str)
    ids = sorted(int(k) for k in doc["voice"])
    assert ids == list(range(len(ids))) and len(ids) >= 1
    for k in ids:
        v = doc["voice"][str(k)]
        assert isinstance(v["name"], str) and v["name"] and isinstance(v["description"], str)
        assert 0.0 <= float(v["average_pitch"]) <= 128.0
        assert isinstance(v["portrait"]["path"], str) and isinstance(v["portrait"]["description"], str)


@pytest.mark.parametrize("compiler,std", [("gcc", "-std=c11"), ("g++", "-std=c++20")])
def test_prototypes_agree_with_reference_header(tmp_path, compiler, std):
    """Types, not just names: every prototype of our header, as `compiler` reads it in `std`, has the type the reference header
    gives that function (return and parameter types, against the fingerprints recorded from the reference header), the opaque
    types are the reference's typedefs, and the error codes have its values.  A translation unit that takes the address of all
    77 functions compiles cleanly and refers to them by their plain C names (C linkage, in C++ too)."""
    import subprocess
    ref = _reference_abi()
    header = os.path.join(REPO, "include", "beatrice_abi.h")
    funcs, typedefs, codes = _abi_view(header, compiler, std)
    bad = {k: funcs.get(k) for k, fp in ref["functions"].items() if _fingerprint(funcs.get(k)) != fp}
    assert not bad, bad
    assert {k: typedefs.get(k) for k in ref["typedefs"]} == ref["typedefs"]
    assert codes == ref["error_codes"] and len(codes) == 5
    src = tmp_path / ("tu.c" if compiler == "gcc" else "tu.cc")
    src.write_text('#include "beatrice_abi.h"\nvoid* const fns[] = {%s};\n' % ", ".join("(void*)&" + k for k in sorted(ref["functions"])))
    obj = tmp_path / "tu.o"
    out = subprocess.run([compiler, std, "-c", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"), str(src), "-o", str(obj)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    undefined = set(subprocess.check_output(["nm", "-u", str(obj)]).decode().split())
    assert set(ref["functions"]) <= undefined, sorted(set(ref["functions"]) - undefined)[:5]
    # and the check has teeth: one changed argument type must be caught
    ours = open(header).read()
    broken = ours.replace("void G##_SetMinQuantizedPitch(G##_PitchContext1* ctx, int min_quantized_pitch);",
                          "void G##_SetMinQuantizedPitch(G##_PitchContext1* ctx, long min_quantized_pitch);")
    assert broken != ours
    (tmp_path / "broken.h").write_text(broken)
    funcs = _abi_view(str(tmp_path / "broken.h"), compiler, std)[0]
    assert {k for k, fp in ref["functions"].items() if _fingerprint(funcs.get(k)) != fp} == \
        {"Beatrice20%s_SetMinQuantizedPitch" % g for g in ("a2", "b1", "rc0")}
