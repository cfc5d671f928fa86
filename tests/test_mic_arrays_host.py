"""Microphone arrays of 2 to 8 channels (include/css_mi355_array.h; csrc/mvdr.hip as a template over the microphone count), the
part that needs no GPU: the header, the library and the binding table agree, the descriptor is laid out as the C compiler lays it
out, css_blob_num_floats accepts num_mics 1 .. 8, the Python layer takes and refuses `num_mics` as described, every instantiation
of the MVDR kernels compiles without scratch, and tests/array_reference.py is backend_reference at C = 7 and lies inside its own
bounds at every C."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT, pkg
import array_reference as A
import backend_reference as R

CSRC = os.path.join(ROOT, "notsofar1-challenge_amd", "csrc")
HEADER = "css_mi355_array.h"
OTHERS = ("css_mi355.h", "css_mi355_rate.h", "css_mi355_preview.h", "css_mi355_preview_handoff.h", "css_mi355_encoder.h",
          "css_mi355_window.h", "css_mi355_present_window.h", "css_mi355_frontend.h", "css_mi355_session_handoff.h",
          "css_mi355_stream_out.h", "css_mi355_backend.h")
NAMES = ("css_mvdr_array_host",)
DESC_INT32 = ("form", "C", "F", "S", "T", "hop", "nseg", "use_mvdr", "n_sets", "reserved")
DESC_FLOAT = ("mask_floor", "reserved_f")
DESC_INT64 = ("seg_lo", "stft_frames", "T_ld", "mask_ld", "x_floats", "mask_floats", "override_bytes", "scm_doubles", "bfw_doubles",
              "sep_floats")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)


def test_header_library_and_binding_agree():
    L = pkg("_lib")
    lib = L.load()
    text = _header()
    assert '#include "css_mi355.h"' in text
    declared = re.findall(r"\bint\s+(css_\w+)\s*\(", text)
    assert sorted(declared) == sorted(NAMES) == sorted(L.ARRAY_SIGNATURES)
    tables = [getattr(L, n) for n in dir(L) if n.startswith("SIGNATURES")]       # (the eleven tables of the other headers)
    assert len(tables) == 11 and not any(set(L.ARRAY_SIGNATURES) & set(t) for t in tables)
    assert len(L.SIGNATURES) == 85
    for other in OTHERS:
        body = open(os.path.join(ROOT, "include", other)).read()
        for name in NAMES + ("CssMvdrArrayDesc", "CssMvdrArraySet", "CSS_ARRAY_MAX_SETS"):
            assert not re.search(rf"\b{name}\b", body), f"{name} belongs to {HEADER} alone"
    fn = lib.css_mvdr_array_host      # (AttributeError: the library does not export it)
    params = re.search(r"\bcss_mvdr_array_host\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
    restype, argtypes = L.ARRAY_SIGNATURES["css_mvdr_array_host"]
    assert restype is C.c_int and fn.restype is C.c_int and list(fn.argtypes) == list(argtypes) and len(argtypes) == len(params) == 8
    assert argtypes[0] is C.c_void_p and argtypes[1] is C.POINTER(L.CssMvdrArrayDesc) and all("*" in p for p in params[1:])
    macros = {k: int(v) for k, v in re.findall(r"#define\s+(CSS_ARRAY_\w+)\s+(\d+)", text)}
    assert macros == {"CSS_ARRAY_MAX_SETS": 16, "CSS_ARRAY_MIN_MICS": L.ARRAY_MIN_MICS, "CSS_ARRAY_MAX_MICS": L.ARRAY_MAX_MICS}
    assert (L.ARRAY_MIN_MICS, L.ARRAY_MAX_MICS) == (2, 8)
    # css_mvdr_host keeps its own header; the Makefile rebuilds the unit on the new one
    assert "css_mvdr_host" in open(os.path.join(ROOT, "include", "css_mi355_backend.h")).read() and "css_mvdr_host" not in declared
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^build/api_backend\.o build_asan/api_backend\.o:.*\.\./\.\./include/css_mi355_array\.h", mk, flags=re.M)
    assert re.search(r"^build/mvdr\.o build_asan/mvdr\.o:.*scm_walk\.inc", mk, flags=re.M)


def test_struct_layout_is_the_compilers():
    """sizeof / offsetof of CssMvdrArrayDesc and CssMvdrArraySet from a compiled probe against the ctypes mirrors"""
    L = pkg("_lib")
    body = re.search(r"typedef struct CssMvdrArrayDesc \{(.*?)\} CssMvdrArrayDesc;", _header(), flags=re.S).group(1)
    members = [m.strip() for part in body.split(";") if part.strip() for m in re.sub(r"^\s*\w+\s+", "", part.strip()).split(",")]
    names = list(DESC_INT32 + DESC_FLOAT + DESC_INT64) + ["sets"]
    assert members == names[:-1] + ["sets[CSS_ARRAY_MAX_SETS]"]
    T, TS = L.CssMvdrArrayDesc, L.CssMvdrArraySet
    assert [n for n, _ in T._fields_] == names and [n for n, _ in TS._fields_] == ["seg_lo", "nseg", "scm_off", "bfw_off"]
    src = ('#include <stddef.h>\n#include <stdio.h>\n#include "css_mi355_array.h"\nint main(void) {\n'
           '    printf("%zu %zu", sizeof(CssMvdrArraySet), sizeof(CssMvdrArrayDesc));\n' +
           "".join(f'    printf(" %zu", offsetof(CssMvdrArrayDesc, {n}));\n' for n in names) + "    return 0;\n}\n")
    with tempfile.TemporaryDirectory() as d:
        c_file, exe = os.path.join(d, "probe.c"), os.path.join(d, "probe")
        open(c_file, "w").write(src)
        cc = "/opt/rocm/lib/llvm/bin/clang" if os.path.exists("/opt/rocm/lib/llvm/bin/clang") else "cc"
        subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), c_file, "-o", exe], check=True,
                       capture_output=True, timeout=120)
        got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.split()]
    want = [32, 128 + 16 * 32] + [4 * i for i in range(12)] + [48 + 8 * i for i in range(10)] + [128]
    assert got == [C.sizeof(TS), C.sizeof(T)] + [getattr(T, n).offset for n in names] == want
    # the same members as css_mvdr_host's descriptor: one body serves both entries (csrc/api_backend.hip)
    assert [(n, t) for n, t in T._fields_[:-1]] == [(n, t) for n, t in L.CssMvdrDesc._fields_[:-1]] and C.sizeof(T) == C.sizeof(L.CssMvdrDesc)


def test_null_handle_is_refused():
    L = pkg("_lib")
    d = L.CssMvdrArrayDesc(form=0, C=4)
    assert L.load().css_mvdr_array_host(None, C.byref(d), None, None, None, None, None, None) == L.CSS_ERR_INVALID_ARG


def test_blob_size_for_every_microphone_count():
    L, w = pkg("_lib"), pkg("weights")
    size = lambda desc: L.load().css_blob_num_floats(C.byref(L.make_desc(desc)))
    for c in range(2, 9):
        desc = w.ModelDesc(num_mics=c, in_features=257 * c)
        assert size(desc) == w.blob_num_floats(desc) > 0, c
    assert size(w.ModelDesc(num_mics=1, in_features=257)) == w.blob_num_floats(w.ModelDesc.sc_v1())
    for c in (0, 9):
        assert size(w.ModelDesc(num_mics=c, in_features=257 * 4)) == -1, c
    assert size(w.ModelDesc(num_mics=1, in_features=257 * 4)) == -1      # (pairs need a second microphone)


def _cfg(ipd_index):
    S = pkg("separator")
    cfg = S.ConformerCssCfg()
    cfg.extractor_conf.ipd_index = ipd_index
    cfg.nnet_conf.in_features = 257 * (1 + len(S.ipd_pairs(ipd_index)))
    return cfg


def test_desc_from_cfg_takes_and_refuses_num_mics():
    S = pkg("separator")
    pairs3 = "1,0;2,0;3,0"
    assert S.desc_from_cfg(_cfg(pairs3)).num_mics == 7                     # the default stays: the NOTSOFAR array where the pairs fit it
    assert S.desc_from_cfg(S.ConformerCssCfg()).num_mics == 7
    for c in (4, 5, 6, 7, 8):
        d = S.desc_from_cfg(_cfg(pairs3), num_mics=c)
        assert (d.num_mics, d.in_features) == (c, 257 * 4)
    for bad in (3, 1, 0, 9, -4):                                           # does not exceed pair index 3; outside 1 .. 8
        with pytest.raises(ValueError, match="num_mics"):
            S.desc_from_cfg(_cfg(pairs3), num_mics=bad)
    assert S.desc_from_cfg(_cfg(""), num_mics=1).num_mics == 1 == S.desc_from_cfg(_cfg("")).num_mics
    with pytest.raises(ValueError, match="num_mics"):
        S.desc_from_cfg(_cfg(""), num_mics=4)                             # no pairs: a single-channel model


def test_separator_and_state_dict_take_num_mics():
    S, w = pkg("separator"), pkg("weights")
    for c in (2, 4, 8):
        desc = w.ModelDesc(num_mics=c, in_features=257 * c, num_blocks=1)
        st = w.portable_state_dict(desc, 3)
        assert w.ModelDesc.from_state_dict(st).num_mics == 7               # a state dict does not say: the default stays
        assert w.ModelDesc.from_state_dict(st, num_mics=c) == desc
        sep = S.HipSeparator(st, None, num_mics=c)
        assert sep.desc == desc and sep.blob.size == w.blob_num_floats(desc)
        assert S.HipSeparator(st, None).desc.num_mics == 7
        with pytest.raises(ValueError, match="num_mics"):
            S.HipSeparator(st, None, num_mics=1)
        with pytest.raises(ValueError, match="num_mics"):
            S.HipSeparator(st, None, num_mics=9)
    sc = w.portable_state_dict(w.ModelDesc.sc_v1(), 0)
    assert w.ModelDesc.from_state_dict(sc, num_mics=1).num_mics == 1
    with pytest.raises(ValueError, match="num_mics"):
        w.ModelDesc.from_state_dict(sc, num_mics=4)
    cfg = _cfg("1,0;2,0;3,0")
    cfg.nnet_conf.conformer_conf.num_blocks = 1
    desc = S.desc_from_cfg(cfg, num_mics=4)
    assert S.HipSeparator(w.portable_state_dict(desc, 3), cfg, num_mics=4).desc == desc and desc.num_mics == 4


def test_wav_file_counts():
    W = pkg("wavio")
    for n in range(2, 9):
        W.check_mic_count(n, True)
    W.check_mic_count(1, False)
    for n, mc in ((1, True), (9, True), (0, True), (2, False), (7, False)):
        with pytest.raises(AssertionError):
            W.check_mic_count(n, mc)


# ---- the kernels' resources -------------------------------------------------------------------------------------------------------

def test_every_instantiation_compiles_without_scratch():
    """mvdr.hip for gfx950 with the Makefile's own flags; the compiler's resource report of every instantiation: the three tile
    forms and the any-length form of the covariances, the solve and the beamformer, at each of the seven microphone counts"""
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, flags=re.M).group(1)
    flags = [f.replace("$(ARCH)", arch) for f in re.search(r"^CXXFLAGS\s*\?=\s*(.*)$", text, flags=re.M).group(1).split()]
    assert arch == "gfx950" and "-O3" in flags
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
                                                                 "-I" + CSRC, os.path.join(CSRC, "mvdr.hip"), "-o", os.path.join(d, "mvdr.o")],
                             capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    usage, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"remark: +([^:]+): (\d+)", line)
        if m and name:
            usage[name][m.group(1).strip()] = int(m.group(2))
    want = []
    for c in range(2, 9):
        want += [f"scm_kernelILi{c}ELi4ELi192E", f"scm_kernelILi{c}ELi4ELi256E", f"scm_kernelILi{c}ELi8ELi512E", f"scm_long_kernelILi{c}E",
                 f"mvdr_solve_multi_kernelILi{c}E", f"beamform_kernelILi{c}E"]
    for kernel in want:
        mine = {k: v for k, v in usage.items() if kernel in k}
        assert len(mine) == 1, (kernel, sorted(usage))
        (k, v), = mine.items()
        print(kernel, {q: v[q] for q in ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")})
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
    # the 7-microphone rows are the ones the kernels had before the template
    seven = {k: next(v for n, v in usage.items() if k in n) for k in want if "Li7E" in k}
    assert [seven[k]["VGPRs"] for k in sorted(seven)] == [70, 256, 242, 242, 242, 50], {k: seven[k]["VGPRs"] for k in sorted(seven)}
    assert seven["mvdr_solve_multi_kernelILi7E"]["AGPRs"] == 36 and seven["scm_long_kernelILi7E"]["LDS Size [bytes/block]"] == 11264


# ---- the reference's own checks ---------------------------------------------------------------------------------------------------

def _same(a, b):
    """the same values of the same type, signs of zeros included (not the bytes: a longdouble has six bytes of padding)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    parts = ((a.real, b.real), (a.imag, b.imag)) if np.iscomplexobj(a) else ((a, b),)
    return all(np.array_equal(x, y, equal_nan=True) and np.array_equal(np.signbit(x), np.signbit(y)) for x, y in parts)


def test_reference_at_seven_is_backend_reference():
    """values and bounds, bit for bit (longdouble and float64)"""
    assert A.npack(7) == R.NPACK and A.pairs(7) == R.PAIRS and A.solve_g(7) == R.SOLVE_G
    for c in [c for c in R.scm_cases() if c["name"] in ("T65", "T186", "T193_tied", "pairs_S3", "T255_all_equal_index", "T600_all_equal")]:
        X, M, ov = R.scm_case_arrays(c)
        assert _same(X, A.planes(c["planes"], 7, c["F"], c["T_ld"], c["stft_frames"], c["seed"])), c["name"]
        for seg in range(c["seg_lo"], c["seg_lo"] + c["nseg"]):
            for long_path in (False, True):
                args = (X, c["F"], c["stft_frames"], M, c["S"], c["T"], c["hop"], seg, ov, long_path)
                (p0, b0), (p1, b1) = R.scm(*args), A.scm(*args)
                assert _same(p0, p1) and _same(b0, b1), (c["name"], seg, long_path)
    for c in [c for c in R.solve_cases() if c["name"] in ("well_T64_x1", "well_T186_x1000", "quiet_ref_S2", "silent_S3", "rank3", "pivot_S1")]:
        scm = R.solve_case_scm(c)[0]
        assert _same(scm, A.covariances(c["family"], 7, c["S"], c["F"], c["seed"], c["T"], c["scale"], c["winners_n"])), c["name"]
        (w0, b0), (w1, b1) = R.solve(scm, c["S"], c["F"]), A.solve(scm, c["S"], c["F"], 7)
        assert _same(w0, w1) and _same(b0, b1), c["name"]
        assert _same(R.unpack(scm), A.unpack(scm, 7))
    c = {c["name"]: c for c in R.scm_cases()}["T65"]
    X, M, _ = R.scm_case_arrays(c)
    rng = np.random.default_rng(5)
    W = (rng.standard_normal((c["S"], c["F"], 7)) + 1j * rng.standard_normal((c["S"], c["F"], 7))) / 7
    for seg in range(c["seg_lo"], c["seg_lo"] + c["nseg"]):
        args = (X, c["F"], c["stft_frames"], M, c["S"], c["T"], c["hop"], seg, 0.05)
        assert all(_same(a, b) for a, b in zip(R.beamform(*args, W), A.beamform(*args, W)))
        assert _same(R.beamform_plain(*args), A.beamform_plain(*args))


def _ratio(err, bound):
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    return float(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300)).max())


@pytest.mark.parametrize("C_", A.CS)
def test_float64_evaluation_lies_inside_the_bound(C_):
    """the same formulas in float64 (numpy's own summation order) against the longdouble values: covariances, solve, beamformer"""
    worst = [0.0, 0.0, 0.0]
    for c in [c for c in A.scm_cases() if c["C"] == C_][:6] or [A.scm_case(f"C{C_}", C_, 186, 3, 2, 2, 0, 93, 1, 0, "random", "gaussian", None, 50 + C_)]:
        X, M, ov = A.scm_case_arrays(c)
        for seg in range(c["seg_lo"], c["seg_lo"] + c["nseg"]):
            args = (X, c["F"], c["stft_frames"], M, c["S"], c["T"], c["hop"], seg, ov)
            phi, bound = A.scm(*args)
            phi64, _ = A.scm(*args, dtype=np.float64)
            worst[0] = max(worst[0], _ratio(np.abs(phi64.astype(R.LD) - phi), bound))
    for fam, scale in (("well", 1.0), ("well", 1e3), ("quiet_ref", 1.0)):
        scm = A.covariances(fam, C_, 2, 3, 60 + C_, 64, scale)
        W, bound = A.solve(scm, 2, 3, C_)
        W64, _ = A.solve(scm, 2, 3, C_, dtype=np.float64, want_bound=False)
        j = A.judged(W, bound)
        worst[1] = max(worst[1], _ratio(np.where(j[..., None], np.abs(W64.astype(R.CLD) - W).astype(np.float64), 0.0), bound))
    c = A.scm_case("b", C_, 17, 2, 3, 2, 0, 9, 1, 0, "random", "gaussian", None, 70 + C_)
    X, M, _ = A.scm_case_arrays(c)
    rng = np.random.default_rng(C_)
    W = (rng.standard_normal((2, 3, C_)) + 1j * rng.standard_normal((2, 3, C_))) / C_
    for seg in (0, 1):
        ref, bound = A.beamform(X, 3, c["stft_frames"], M, 2, 17, 9, seg, 0.05, W)
        worst[2] = max(worst[2], _ratio(np.abs(ref.astype(np.float32).astype(np.float64) - ref), bound))
    print(f"C = {C_}: float64 against longdouble, worst error / bound: covariances {worst[0]:.3f}, solve {worst[1]:.4f}, "
          f"beamformer (one rounding to float32) {worst[2]:.3f}")
    assert max(worst) <= 1.0, worst


def test_complete_solve_families_are_judged_by_the_reference():
    """every system of the families marked complete has a bound of at most 1e-9 max |W| (the project's JUDGED), on the segments the
    GPU test uploads; the other families are judged at least somewhere or nowhere, as the conditioning has it"""
    for c in A.solve_cases():
        scm = A.solve_case_scm(c, 3)
        for seg in range(3):
            W, bound = A.solve(scm[seg], c["S"], c["F"], c["C"])
            assert np.isfinite(bound).all() or not c["complete"], c["name"]
            if c["complete"]:
                assert A.judged(W, bound).all(), (c["name"], seg, float((bound.max(axis=-1) / np.abs(W).max(axis=-1)).max()))
