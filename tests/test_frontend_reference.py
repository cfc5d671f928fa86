"""tests/frontend_reference.py on the CPU, on the inputs tests/test_hip_frontend_kernels.py gives the kernels:
  (a) the float64 references agree with oracle/css_oracle.py (stft and features in float64);
  (b) the bounds are reachable: the same formulas in numpy's float32 arithmetic stay inside every bound (the analysis both as a
      float32 radix-4 evaluation and as the float32 direct sum);
  (c) the bounds are not vacuous: each deliberate mistake moves some output by at least 10 times its bound (analysis, features)
      or changes a bit (the exact kernels).
The reference tests need no GPU and no library; the first two tests pin include/css_mi355_frontend.h against the library and
its binding, as tests/test_encoder_reference.py pins the encoder header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import css_oracle as O
import frontend_reference as R
from conftest import ROOT, pkg

CSRC = os.path.join(ROOT, "notsofar1-challenge_amd", "csrc")
HEADER = "css_mi355_frontend.h"
OTHERS = ("css_mi355.h", "css_mi355_rate.h", "css_mi355_preview.h", "css_mi355_preview_handoff.h", "css_mi355_encoder.h",
          "css_mi355_window.h", "css_mi355_present_window.h")
NAMES = ("css_analysis_host", "css_features_host", "css_synthesis_tail_host", "css_pcm_edges_host")
DESCS = ("CssAnalysisDesc", "CssFeaturesDesc", "CssSynthesisTailDesc", "CssPcmEdgesDesc")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)


def test_header_library_and_binding_agree():
    L = pkg("_lib")
    lib = L.load()
    text = _header()
    assert '#include "css_mi355.h"' in text
    declared = re.findall(r"\bint\s+(css_\w+)\s*\(", text)
    assert sorted(declared) == sorted(NAMES) == sorted(L.SIGNATURES_FRONTEND)
    assert not set(L.SIGNATURES_FRONTEND) & (set(L.SIGNATURES) | set(L.SIGNATURES_RATE) | set(L.SIGNATURES_PREVIEW) |
                                             set(L.SIGNATURES_PREVIEW_HANDOFF) | set(L.SIGNATURES_ENCODER) |
                                             set(L.SIGNATURES_WINDOW) | set(L.SIGNATURES_PRESENT))
    assert len(L.SIGNATURES) == 85
    others = [open(os.path.join(ROOT, "include", f)).read() for f in OTHERS]
    for name in NAMES + DESCS:
        for other in others:
            assert not re.search(rf"\b{name}\b", other), f"{name} belongs to {HEADER} alone"
    kinds = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "CssFeatureCfg": L.CssFeatureCfg}
    for name in NAMES:
        params = re.search(rf"\b{name}\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
        restype, argtypes = L.SIGNATURES_FRONTEND[name]
        fn = getattr(lib, name)
        assert restype is C.c_int and len(argtypes) == len(params), name
        assert fn.restype is C.c_int and list(fn.argtypes) == list(argtypes)       # load() applied the eighth table
        assert all("*" in p or p.split()[0] == "css_handle_t" for p in params), name
    for desc in DESCS:   # the header's fields in the header's order, with the header's types
        body = re.search(rf"typedef struct {desc} \{{(.*?)\}} {desc};", text, flags=re.S).group(1)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                kind, names = decl.split(None, 1)
                for n in names.split(","):
                    arr = re.fullmatch(r"(\w+)\[(\d+)\]", n.strip())
                    fields.append((arr.group(1), kinds[kind] * int(arr.group(2))) if arr else (n.strip(), kinds[kind]))
        assert fields == list(getattr(L, desc)._fields_), desc
    assert C.sizeof(L.CssAnalysisDesc) == 64 and L.CssAnalysisDesc.x_stride.offset == 24
    assert C.sizeof(L.CssFeaturesDesc) == 80 + C.sizeof(L.CssFeatureCfg) and L.CssFeaturesDesc.T_ld.offset == 32
    assert C.sizeof(L.CssSynthesisTailDesc) == 40 + 11 * 8 + 2 * 64 * 8 and L.CssSynthesisTailDesc.T_frames.offset == 40
    assert C.sizeof(L.CssPcmEdgesDesc) == 24 + 8 * 8 and L.CssPcmEdgesDesc.n.offset == 24
    deps = re.findall(r"^build(?:_asan)?/%\.o:.*$", open(os.path.join(CSRC, "Makefile")).read(), flags=re.M)
    assert len(deps) == 2 and all(f"../../include/{hd}" in d for d in deps for hd in OTHERS + (HEADER,))
    srcs = re.search(r"^SRCS\s*:=(.*)$", open(os.path.join(CSRC, "Makefile")).read(), flags=re.M).group(1).split()
    assert "api_frontend.hip" in srcs


def test_null_handle_and_null_descriptor_are_refused():
    L = pkg("_lib")
    lib = L.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    x = np.full(1024, 3.0, np.float32)
    out = np.full(1024, 7.0, np.float32)
    peak = np.full(4, 9, np.uint32)
    assert lib.css_analysis_host(None, C.byref(L.CssAnalysisDesc()), p(x), p(out), None) == L.CSS_ERR_INVALID_ARG
    assert lib.css_features_host(None, C.byref(L.CssFeaturesDesc()), p(x), None, p(x), p(x), p(out)) == L.CSS_ERR_INVALID_ARG
    assert lib.css_synthesis_tail_host(None, C.byref(L.CssSynthesisTailDesc()), p(x), p(out)) == L.CSS_ERR_INVALID_ARG
    assert lib.css_pcm_edges_host(None, C.byref(L.CssPcmEdgesDesc()), p(x), p(out), p(peak)) == L.CSS_ERR_INVALID_ARG
    assert lib.css_analysis_host(None, None, None, None, None) == L.CSS_ERR_INVALID_ARG
    assert (out == 7.0).all() and (peak == 9).all()


# ---- analysis -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C_", sorted(R.ANALYSIS_FAMILIES))
@pytest.mark.parametrize("window", (0, 1))
def test_analysis_tie_reach_and_mutations(C_, window):
    x = R.analysis_samples(C_)
    T = R.ANALYSIS_FRAMES
    ref, bound = R.analysis(x, 0, T, window), R.analysis_bound(x, 0, T, window)
    # (a) the table's window is the float32 rounding of the oracle's; with the oracle's float64 Hann window the two direct sums agree
    assert (R.bits(R.window_table(0)) == R.bits(O.hann_periodic(512, np.float64).astype(np.float32))).all()
    assert (R.bits(R.window_table(1)) == R.bits(np.sqrt(O.hann_periodic(512, np.float32)) / np.float32(16))).all()
    mine = R.analysis(x, 0, T, window, win=None if window else O.hann_periodic(512, np.float64))
    o = np.moveaxis(O.stft(x[:, :256 * (T - 1) + 512].T.astype(np.float64), dtype=np.float64,
                           window="sqrt_hann" if window else "hann"), 2, 0)
    o = np.concatenate([o.real, o.imag], axis=1)
    assert np.abs(o - mine).max() <= 1e-13 * np.abs(o).max()
    assert (ref[:, 257] == 0).all() and (ref[:, 513] == 0).all() and not np.signbit(ref[:, [257, 513]]).any()
    # sub-ranges are the same numbers (to the order of the float64 sums), and NaN outside a range is never touched
    for t_lo, t_hi in R.ANALYSIS_RANGES:
        sub = R.analysis(R.analysis_input(x, t_lo, t_hi), t_lo, t_hi, window)
        assert np.abs(sub - ref[:, :, t_lo:t_hi]).max() <= 1e-12 * np.abs(ref).max()
    # (b) both float32 evaluations stay inside the bound (a zero bound -- the all-zero channel -- means an exact zero)
    for name, y in (("radix-4", R.analysis_radix4_f32(x, 0, T, window)), ("direct", R.analysis(x, 0, T, window, dtype=np.float32))):
        err = np.abs(y - ref)
        assert (err <= bound).all(), (name, float((err / np.maximum(bound, 1e-300)).max()))
    # (c) the mistakes
    for mut in ("sym_hann", "frame_t1"):
        r = np.abs(R.analysis(x, 0, T - 1, window, mut=mut) - ref[:, :, :T - 1]) / np.maximum(bound[:, :, :T - 1], 1e-300)
        assert r.max() >= 10.0, (mut, float(r.max()))
    if C_ == 7:
        assert np.any(R.bits(R.analysis(x, 0, T, window, dtype=np.float32, mut="nyq_im")[:, 513]) != 0)
        assert not np.any(R.bits(R.analysis(x, 0, T, window, dtype=np.float32)[:, [257, 513]]))


# ---- features -------------------------------------------------------------------------------------------------------------------

def _segments(c):
    return range(c["seg_lo"], c["seg_lo"] + c["nseg"])


def _ref(c, s, **kw):
    return R.features(c["X"], c["stft_frames"], s, c["T"], c["hop"], c["opts"], c["bias"], c["scale"], **kw)


@pytest.mark.parametrize("T", R.FEATURE_T_TUNED + R.FEATURE_T_LONG)
def test_features_tie_reach_and_conditioning(T):
    for k in range(len(R.FEATURE_FAMILIES)):
        c = R.feature_case(T, k)
        n_un = n_all = 0
        for s in _segments(c):
            y, bound, d_ang = _ref(c, s, bound=True)
            assert np.isfinite(y).all(), c["name"]
            judged = d_ang <= R.UNCOND
            n_un += int((~judged).sum())
            n_all += judged.size
            # (a) the oracle in float64.  Its atan2(+0, negative) is +pi where the kernel's convention is CSS_PHASE_NEG_REAL, 1.5e-7
            #     from -pi: the IPD columns of a bin that is real and negative in some frame (every bin stands alone) are left out
            if T <= 192:
                re, im, _ = R._segment(c["X"], c["stft_frames"], s, T, c["hop"])
                plain = ~((im == 0) & (re < 0)).any(axis=(0, 2))
                tied = judged & np.concatenate([np.ones(R.F, bool)] + [plain] * len(c["opts"]["pairs"]))[None, :]
                o = R.oracle_features(O, c["X"], c["stft_frames"], s, T, c["hop"], c["opts"], c["bias"], c["scale"])
                e = R.feature_error(o, y, c["scale"], c["opts"])
                assert e[tied].max(initial=0.0) <= 1e-9 and tied.mean() > 0.9 * judged.mean(), (c["name"], s, float(e[tied].max()))
            # (b) float32 numpy
            e = R.feature_error(_ref(c, s, dtype=np.float32), y, c["scale"], c["opts"])
            assert (e[judged] <= bound[judged]).all(), (c["name"], s, float((e[judged] / bound[judged]).max()))
        # the float64 reference alone meets the cap on unconditioned elements
        if c["family"] != "constant_difference":
            assert n_un <= 0.01 * n_all, (c["name"], n_un, n_all)


def _mutation_ratio(mut, want):
    """the largest |mutated - reference| / bound over the judged elements of the cases `want` selects"""
    worst = 0.0
    for T in (64, 65, 186, 191):
        for k in range(len(R.FEATURE_FAMILIES)):
            c = R.feature_case(T, k)
            if not want(c):
                continue
            for s in _segments(c):
                y, bound, d_ang = _ref(c, s, bound=True)
                judged = d_ang <= R.UNCOND
                e = R.feature_error(_ref(c, s, mut=mut), y, c["scale"], c["opts"])
                worst = max(worst, float((e[judged] / bound[judged]).max(initial=0.0)))
    return worst


@pytest.mark.parametrize("mut, want", [
    ("var_T", lambda c: c["opts"]["mvn"] and c["family"] == "gaussian"),
    ("valid_only", lambda c: c["opts"]["mvn"] and 2 <= c["stft_frames"] - (c["seg_lo"] + c["nseg"] - 1) * c["hop"] < c["T"]),
    ("swap_lr", lambda c: bool(c["opts"]["pairs"]) and c["family"] in ("gaussian", "magnitudes")),
    ("v2_as_v3", lambda c: bool(c["opts"]["pairs"]) and c["opts"]["norm"] and c["opts"]["version"] == 2),
    ("cos_first", lambda c: bool(c["opts"]["pairs"]) and c["opts"]["cos"] and c["opts"]["norm"]),
    ("pi_plus", lambda c: bool(c["opts"]["pairs"]) and c["opts"]["norm"] and c["opts"]["version"] == 3 and c["family"] == "negative_real"),
])
def test_feature_mistakes_are_caught(mut, want):
    r = _mutation_ratio(mut, want)
    assert r >= 10.0, (mut, r)


# ---- the exact kernels ----------------------------------------------------------------------------------------------------------

def test_level_gain_and_overlap_add():
    assert [float(R.level_gain(w)) for w in R.LEVELS] == [1.0, 1.0, 2.0 ** 100, 2.0 ** 19, 1.0, 2.0 ** -16, 1.0]
    changed = {"newest_first": 0, "ignore_f_hi": 0}
    for c in R.ola_cases():
        G = R.ola_input(c)
        args = (c["B"], c["T_frames"], c["hop"], c["L"], c["q_lo"], c["q_hi"], c["f_lo"], c["f_hi"], c["out_ld"], c["out_q0"])
        n = c["B"] * c["out_ld"] + 64
        out = R.wave_ola(G, R.canary(n), *args, c["level"])
        # against the definition in float64: every frame of the window added at its place, times 2^e
        want = np.zeros((c["B"], (c["T_frames"] + 4) * c["hop"] + c["L"]))
        g = G.reshape(c["B"], c["T_frames"], c["L"]).astype(np.float64)
        for t in range(c["f_lo"], c["f_hi"]):
            want[:, t * c["hop"]:t * c["hop"] + c["L"]] += g[:, t]
        want = want / float(R.level_gain(c["level"]))
        lo, hi = c["q_lo"] * c["hop"], min(c["q_hi"] * c["hop"], c["out_q0"] * c["hop"] + c["out_ld"])
        got = out[:c["B"] * c["out_ld"]].reshape(c["B"], -1)
        at = (c["q_lo"] - c["out_q0"]) * c["hop"]
        assert np.allclose(got[:, at:at + hi - lo], want[:, lo:hi], rtol=1e-5, atol=1e-6 / float(R.level_gain(c["level"]))), c
        own = np.zeros((c["B"], c["out_ld"]), bool)
        own[:, at:at + hi - lo] = True
        assert (R.bits(got)[~own] == R.CANARY).all() and (R.bits(out[c["B"] * c["out_ld"]:]) == R.CANARY).all(), c
        for mut in changed:
            changed[mut] += int(np.any(R.bits(R.wave_ola(G, R.canary(n), *args, c["level"], mut=mut)) != R.bits(out)))
    assert changed["newest_first"] and changed["ignore_f_hi"], changed
    # newest first changes bits only where four frames meet: (512, 128)
    for c in R.ola_cases():
        if (c["L"], c["hop"]) == (512, 256) and c["level"] is None:
            args = (c["B"], c["T_frames"], c["hop"], c["L"], c["q_lo"], c["q_hi"], c["f_lo"], c["f_hi"], c["out_ld"], c["out_q0"])
            a = R.wave_ola(R.ola_input(c), R.canary(c["B"] * c["out_ld"]), *args, None)
            b = R.wave_ola(R.ola_input(c), R.canary(c["B"] * c["out_ld"]), *args, None, mut="newest_first")
            assert (R.bits(a) == R.bits(b)).all()            # (a two-term float sum commutes)


def test_join_rows_and_pcm_models():
    for c in R.join_cases():
        rs = np.random.RandomState(c["seed"])
        g = rs.standard_normal(c["world"] * c["S"] * c["ld"]).astype(np.float32)
        out = R.join_shards(g, R.canary(c["S"] * c["out_ld"]), c["ld"], c["t_lo"], c["t_hi"], c["S"], c["hop"], c["n_out"], c["out_ld"])
        out = out.reshape(c["S"], c["out_ld"])
        assert (R.bits(out[:, c["n_out"]:]) == R.CANARY).all()
        want = np.zeros((c["S"], c["n_out"]))                      # the definition in float64: every rank that holds the block
        g3 = g.reshape(c["world"], c["S"], c["ld"]).astype(np.float64)
        held = np.zeros(c["n_out"], int)
        for k, (lo, hi) in enumerate(zip(c["t_lo"], c["t_hi"])):
            if hi > lo:
                a, b = lo * c["hop"], min((hi + 1) * c["hop"], c["n_out"])
                want[:, a:b] += g3[k, :, :b - a]
                held[a:b] += 1
        assert np.allclose(out[:, :c["n_out"]], want, rtol=1e-6, atol=1e-6) and held.max() == min(c["world"], 2) and held.min() == 1
    rows = R.planes_to_rows(np.arange(2 * 6 * 5, dtype=np.float32), R.canary(2 * 5 * 8 + 3), 2, 6, 5, 8).copy()
    assert rows[8 + 2] == 1 * 5 + 1 + 1 * 5 and (rows[6:8] == 0).all() and (R.bits(rows[-3:]) == R.CANARY).all()
    # de-interleave: split rows decode to the float32 rows
    rs = np.random.RandomState(3)
    n, C_, n_pad = 257, 7, 320
    pcm = rs.standard_normal((n, C_)).astype(np.float32)
    for i_lo, i_hi in R.pcm_ranges(n, n_pad):
        plain = R.channel_major(pcm, R.canary(C_ * n_pad), n, C_, n_pad, i_lo, i_hi).reshape(C_, n_pad)
        split = R.channel_major(pcm, R.canary(C_ * n_pad), n, C_, n_pad, i_lo, i_hi, 1).reshape(C_, n_pad)
        assert (R.bits(plain[:, :i_lo]) == R.CANARY).all() and (R.bits(plain[:, i_hi:]) == R.CANARY).all()
        want = np.zeros((C_, n_pad), np.float32)
        want[:, :n] = pcm.T
        assert (plain[:, i_lo:i_hi] == want[:, i_lo:i_hi]).all()
        if i_hi > i_lo:
            zeroed = np.where(np.isnan(plain), 0, plain)
            dec = R.split_decode(split)
            assert np.abs(dec[:, i_lo:i_hi] - zeroed[:, i_lo:i_hi]).max() <= R.SPLIT_ST * np.abs(zeroed).max() + R.SPLIT_FLOOR
    assert R.pcm16_scale(np.array([-32768, 32767, 1], np.int16)).tolist() == [-1.0, 32767 / 32768, 2.0 ** -15]
    # peaks: the word never goes down
    x = np.array([0.25, -0.75, 0.5], np.float32)
    assert R.peak_word(x, 0) == 0x3F400000 and R.peak_word(x, 0x3F800000) == 0x3F800000
    # PCM16 encoding: ties to even at +-16383.5, +-peak, the all-zero stream, and the two mistakes
    wav, n, out_ld = R.encode_case()
    out, peak = R.encode_pcm16(wav, np.full(3 * out_ld, 0x5A5A, np.int16), 3, n, out_ld)
    out = out.reshape(3, out_ld)
    assert out[0, 30] == 16384 and out[0, 40] == -16384 and out[0, 10] == 32439 and out[0, 20] == -32439
    assert (out[1, :n] == 0).all() and (out[:, n:] == 0x5A5A).all() and peak[1] == 0 and peak[0] == 0x3F800000
    for mut in ("trunc", "no_1e-7"):
        other, _ = R.encode_pcm16(wav, np.full(3 * out_ld, 0x5A5A, np.int16), 3, n, out_ld, mut=mut)
        assert np.any(other.reshape(3, out_ld)[[0, 2]] != out[[0, 2]]), mut
    assert R.encode_pcm16(wav, np.zeros(3 * out_ld, np.int16), 3, n, out_ld, mut="trunc")[0][30] == 16383
