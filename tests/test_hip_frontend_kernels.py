"""Every launch form the paths make from csrc/stft.hip and csrc/frontend.hip, through the host entries of
include/css_mi355_frontend.h, against the float64 references, derived bounds and exact float32 models of
tests/frontend_reference.py.  Three kinds of assertion per launch:

  ownership  outputs and the slack behind them start as the canary 0x7FC0BEEF (a quiet NaN with a payload); every float the
             launch does not own keeps its bits: plane columns outside [t_lo, t_hi), the padding columns of the feature rows,
             samples outside a range, whatever lies behind out_ld / n_out / n
  value      elementwise inside the bound (analysis, phase planes, features; split-f16 rows decoded first), bit for bit for the
             kernels that round nowhere or in a stated order; the worst ratio of each test is printed
  bits       where two launches must agree: a sub-range of frames against the whole range, float4 against scalar stores, with
             against without phase planes, a segment alone against the same segment among three, split rows against
             split_encode of the float32 rows.  The tuned feature kernels against the any-length one are held to the sum of
             their bounds (the kernel's comment states one ulp on the magnitude rows); the count of differing floats is printed.

Coverage (every launch function of stft.hip and frontend.hip that a path calls):
  launch_stft_fft                  test_analysis: C 1, 3, 7; eight ranges off the 16-frame tile; float4 and scalar stores (row_ld
                                   52 / 53 / 54, offset 1); both windows; with and without phase planes
  launch_features
    features_kernel<192>           test_features[T = 2 .. 192], test_features_phase_planes[24]
    features_kernel<256>           test_features[T = 193, 255, 256], test_features_phase_planes[200]
    features_kernel<512>           test_features[T = 257 .. 512], test_features_phase_planes[300]
    features_long_kernel           test_features[T = 513, 600], test_features_phase_planes[520], and at T = 2, 65, 186, 257 in a
                                   child process started with CSS_FORCE_LONG_PATH=1 (test_features_any_length_at_tuned_lengths)
  launch_wave_ola                  test_wave_ola
  launch_join_shards               test_join_shards
  launch_planes_to_rows            test_planes_to_rows
  launch_deinterleave              test_pcm_layout (split_out 0 and 1)
  launch_pcm16_to_float            test_pcm_layout
  launch_pcm16_to_channel_major    test_pcm_layout
  launch_pcm_peak_f32 / _i16       test_pcm_peaks
  launch_encode_pcm16              test_encode_pcm16 (peak_kernel and encode_pcm16_kernel)
Needs an MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

import frontend_reference as R
from conftest import pkg

pytestmark = pytest.mark.gpu

SLACK = 256                  # floats of slack behind every output


def _open():
    L = pkg("_lib")
    if L.load().css_device_count() < 1:
        pytest.fail("no HIP device visible")
    w = pkg("weights")
    desc = w.ModelDesc(num_blocks=1)
    return pkg("separator").HipSeparator(w.apply_golden_recipe(w.portable_state_dict(desc, 5)), None, device=0)


@pytest.fixture(scope="module")
def handle():
    sep = _open()
    yield sep.handle
    sep.close()


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    diff = np.argwhere(a.view(np.uint8).reshape(a.shape + (-1,)) != b.view(np.uint8).reshape(b.shape + (-1,)))
    assert diff.size == 0, (what, f"{len(np.unique(diff[:, :-1], axis=0))} values differ, the first at {diff[0][:-1]}")


def _all_canary(a, what):
    stray = np.flatnonzero(R.bits(a).reshape(-1) != R.CANARY)
    assert stray.size == 0, (what, f"{stray.size} floats the launch does not own were written, the first at {stray[0]}")


def _ratio(err, bound, what):
    """the worst err / bound; a zero bound asks for a zero error"""
    r = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
    worst = np.unravel_index(int(r.argmax()), r.shape)
    assert r[worst] <= 1.0, (what, f"ratio {r[worst]:.3f} at {worst}: error {err[worst]!r}, bound {np.broadcast_to(bound, err.shape)[worst]!r}")
    return float(r[worst])


# ---- analysis -----------------------------------------------------------------------------------------------------------------

def _analysis(handle, x, C_, t_lo, t_hi, row_ld, offset, window, want_phase, what):
    """one launch; returns the owned columns of the planes [C][514][t_hi - t_lo] and of the phase planes (or None) after the
    ownership checks"""
    n_out, n_ph = offset + C_ * 514 * row_ld + SLACK, offset + C_ * 257 * row_ld + SLACK
    out, ph = handle.analysis(R.analysis_input(x, t_lo, t_hi), C_, x.shape[1], t_lo, t_hi, row_ld, R.canary(n_out), offset=offset,
                              window=window, phase=R.canary(n_ph) if want_phase else None)
    got = []
    for a, rows in ((out, 514), (ph, 257)):
        if a is None:
            got.append(None)
            continue
        planes = a[offset:offset + C_ * rows * row_ld].reshape(C_, rows, row_ld)
        _all_canary(a[:offset], what + ": in front of the planes")
        _all_canary(a[offset + C_ * rows * row_ld:], what + ": behind the planes")
        _all_canary(planes[:, :, :t_lo], what + ": columns before t_lo")
        _all_canary(planes[:, :, t_hi:], what + ": columns from t_hi on")
        got.append(planes[:, :, t_lo:t_hi])
    return got


@pytest.mark.parametrize("window", (0, 1))
@pytest.mark.parametrize("C_", (1, 3, 7))
def test_analysis(handle, C_, window):
    x = R.analysis_samples(C_)
    T = R.ANALYSIS_FRAMES
    ref, bound = R.analysis(x, 0, T, window), R.analysis_bound(x, 0, T, window)
    base, base_ph = _analysis(handle, x, C_, 0, T, 52, 0, window, True, "the whole range")
    worst = {"planes": 0.0, "phase": 0.0}
    for row_ld, offset in R.ANALYSIS_LAYOUTS:
        for t_lo, t_hi in R.ANALYSIS_RANGES + ((0, T),):
            for want_phase in (True, False):
                what = f"C {C_} window {window} frames [{t_lo}, {t_hi}) row_ld {row_ld} offset {offset} phase {want_phase}"
                X, PH = _analysis(handle, x, C_, t_lo, t_hi, row_ld, offset, window, want_phase, what)
                assert np.isfinite(X).all(), (what, "a non-finite output: a sample outside the range was read")
                _same_bits(X, base[:, :, t_lo:t_hi], what + ": against the same frames of the whole range in float4 stores")
                assert not R.bits(X[:, [257, 513]]).any(), (what, "Im of DC / Nyquist is not the word 0")
                worst["planes"] = max(worst["planes"], _ratio(np.abs(X - ref[:, :, t_lo:t_hi]), bound[:, :, t_lo:t_hi], what))
                if not want_phase:
                    continue
                _same_bits(PH, base_ph[:, :, t_lo:t_hi], what + ": phase planes against the whole range")
                re, im = X[:, :257].astype(np.float64), X[:, 257:].astype(np.float64)
                neg, zero = (im == 0) & (re < 0), (im == 0) & (re == 0)
                assert (R.bits(PH)[neg] == R.bits(R.PHASE_NEG_REAL)).all(), (what, "a real negative bin is not CSS_PHASE_NEG_REAL")
                assert (PH[zero] == 0).all(), (what, "phase of (0, 0) is not 0")
                p64 = np.arctan2(im, re)
                judged = ~(neg | zero)
                worst["phase"] = max(worst["phase"], _ratio(np.abs(PH - p64)[judged], (R.C_ATAN2 * R.U * np.abs(p64))[judged], what + " phase"))
    families = R.ANALYSIS_FAMILIES[C_]
    if "negative" in families:
        c = families.index("negative")
        assert (base[c, 0] < 0).all() and (R.bits(base_ph[c, 0]) == R.bits(R.PHASE_NEG_REAL)).all()
    if "zero" in families:
        c = families.index("zero")
        assert not R.bits(base[c]).any() and not R.bits(base_ph[c]).any()
    for k, r in sorted(worst.items()):
        print(f"analysis C {C_} window {window} {k}: worst error / bound {r:.3f}")


# ---- features -----------------------------------------------------------------------------------------------------------------

def _cfg(opts):
    L = pkg("_lib")
    c = L.CssFeatureCfg(int(opts["log"]), int(opts["mvn"]), int(opts["norm"]), int(opts["version"]), int(opts["cos"]), len(opts["pairs"]))
    for i, (l, r) in enumerate(opts["pairs"]):
        c.pair_l[i], c.pair_r[i] = l, r
    return c


def _features(handle, c, split, what, seg_lo=None, nseg=None, PH=None, X=None):
    """one launch; returns the raw rows [nseg T][Kp] after asserting that the slack behind them kept the canary"""
    seg_lo, nseg = c["seg_lo"] if seg_lo is None else seg_lo, c["nseg"] if nseg is None else nseg
    rows = nseg * c["T"]
    feat = handle.features_host(c["X"] if X is None else X, c["C"], R.F, c["T_ld"], c["stft_frames"], seg_lo, nseg, c["T"], c["hop"],
                                c["Kp"], _cfg(c["opts"]), c["bias"], c["scale"], R.canary(rows * c["Kp"] + SLACK), split_out=split, PH=PH)
    _all_canary(feat[rows * c["Kp"]:], what + ": behind the last row")
    return feat[:rows * c["Kp"]].reshape(rows, c["Kp"])


def _feature_reference(c):
    """(y64, bound, judged) over all segments of the case: [nseg T][cols]"""
    parts = [R.features(c["X"], c["stft_frames"], s, c["T"], c["hop"], c["opts"], c["bias"], c["scale"], bound=True)
             for s in range(c["seg_lo"], c["seg_lo"] + c["nseg"])]
    y, b, d = (np.concatenate([p[i] for p in parts], axis=0) for i in range(3))
    return y, b, d <= R.UNCOND


def _check_features(handle, c, worst, PH=None, X=None):
    """the float32 and the split launch of one case against the reference; returns (float32 rows [nseg T][cols], y64, bound,
    judged)"""
    what, cols, Kp, T = c["name"], c["cols"], c["Kp"], c["T"]
    y64, bound, judged = _feature_reference(c)
    if c["family"] not in ("constant_difference", "analysis"):   # (the analysis inputs have a silent and a constant channel)
        assert (~judged).sum() <= 0.01 * judged.size, (what, "unconditioned elements", int((~judged).sum()))
    rows = _features(handle, c, 0, what, PH=PH, X=X)
    _all_canary(rows[:, cols:], what + ": padding columns of the float32 rows")
    y = rows[:, :cols]
    assert np.isfinite(y).all(), (what, "a non-finite output", np.argwhere(~np.isfinite(y))[:4])
    e = R.feature_error(y, y64, c["scale"], c["opts"])
    key = c["flags"]
    worst[key] = max(worst.get(key, 0.0), _ratio(np.where(judged, e, 0.0), bound, what))
    # split rows: the encoded float32 rows, the padding columns' halves untouched
    srows = _features(handle, c, 1, what + " split", PH=PH, X=X)
    padded = np.zeros((rows.shape[0], Kp), np.float32)
    padded[:, :cols] = y
    want = R.canary(rows.size).reshape(rows.shape).view(np.float16).reshape(-1, Kp // 32, 2, 32).copy()
    enc = R.split_encode(padded).view(np.float16).reshape(-1, Kp // 32, 2, 32)
    k = np.arange(cols)
    want[:, k // 32, :, k % 32] = enc[:, k // 32, :, k % 32]
    _same_bits(srows.view(np.float16).reshape(want.shape), want, what + ": split rows against split_encode of the float32 rows")
    dec = R.split_decode(split_zero_padding(srows, cols, Kp))[:, :cols]
    es = R.feature_error(dec, y64, c["scale"], c["opts"])
    worst[key + " split"] = max(worst.get(key + " split", 0.0),
                                _ratio(np.where(judged, es, 0.0), bound + R.SPLIT_ST * np.abs(y64) + R.SPLIT_FLOOR, what + " split"))
    # one segment alone against the same segment among three
    if c["nseg"] == 3:
        alone = _features(handle, c, 0, what + " alone", seg_lo=c["seg_lo"] + 1, nseg=1, PH=PH, X=X)
        _same_bits(alone[:, :cols], y[T:2 * T], what + ": the middle segment alone")
    return y, y64, bound, judged


def split_zero_padding(srows, cols, Kp):
    """the split rows with the halves of the padding columns (canary) set to zero, so that they decode"""
    h = srows.view(np.float16).reshape(-1, Kp // 32, 2, 32).copy()
    k = np.arange(cols, Kp)
    h[:, k // 32, :, k % 32] = 0
    return h.reshape(srows.shape[0], 2 * Kp).view(np.float32)


@pytest.mark.parametrize("T", R.FEATURE_T_TUNED + R.FEATURE_T_LONG)
def test_features(handle, T):
    worst = {}
    for k in range(len(R.FEATURE_FAMILIES)):
        _check_features(handle, R.feature_case(T, k), worst)
    for key, r in sorted(worst.items()):
        print(f"features T {T} {key}: worst error / bound {r:.3f}")


def _forced_dir(tmp):
    return os.path.join(str(tmp), "forced_long")


def _forced_child(out_dir):
    """in a process started with CSS_FORCE_LONG_PATH=1: every case of FEATURE_T_FORCED through features_long_kernel, held to the
    reference like the tuned kernels; the float32 rows are left in out_dir for the parent"""
    assert os.environ.get("CSS_FORCE_LONG_PATH") == "1"
    sep = _open()
    try:
        worst = {}
        for T in R.FEATURE_T_FORCED:
            for k in range(len(R.FEATURE_FAMILIES)):
                y = _check_features(sep.handle, R.feature_case(T, k), worst)[0]
                np.save(os.path.join(out_dir, f"rows_{T}_{k}.npy"), y)
        for key, r in sorted(worst.items()):
            print(f"features (any-length kernel at T {R.FEATURE_T_FORCED}) {key}: worst error / bound {r:.3f}")
    finally:
        sep.close()


def test_features_any_length_at_tuned_lengths(handle, tmp_path):
    out_dir = str(tmp_path)
    env = dict(os.environ, CSS_FORCE_LONG_PATH="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out_dir], env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    differ = {"spectral": [0, 0], "ipd": [0, 0]}
    worst = 0.0
    for T in R.FEATURE_T_FORCED:
        for k in range(len(R.FEATURE_FAMILIES)):
            c = R.feature_case(T, k)
            y_long = np.load(os.path.join(out_dir, f"rows_{T}_{k}.npy"))
            y = _features(handle, c, 0, c["name"])[:, :c["cols"]]
            _, bound, judged = _feature_reference(c)
            e = R.feature_error(y, y_long.astype(np.float64), c["scale"], c["opts"])
            worst = max(worst, _ratio(np.where(judged, e, 0.0), 2.0 * bound, c["name"] + ": tuned against any-length, sum of bounds"))
            d = R.bits(y) != R.bits(y_long)
            for key, sl in (("spectral", slice(0, R.F)), ("ipd", slice(R.F, None))):
                differ[key][0] += int(d[:, sl].sum())
                differ[key][1] += d[:, sl].size
    print(f"tuned against any-length kernel: worst difference / sum of bounds {worst:.3f}; differing floats: "
          + ", ".join(f"{k} {a} of {b}" for k, (a, b) in differ.items()))


@pytest.mark.parametrize("T", (24, 200, 300, 520))
def test_features_phase_planes(handle, T):
    """the same bits with or without the phase planes, the planes being the bits css_analysis_host wrote"""
    C_, frames, window = 7, 560, 0
    x = R.analysis_samples(C_, 256 * (frames - 1) + 512)
    out, ph = handle.analysis(x, C_, x.shape[1], 0, frames, frames, R.canary(C_ * 514 * frames), phase=R.canary(C_ * 257 * frames))
    X, PH = out.reshape(C_, 514, frames), ph.reshape(C_, 257, frames)
    assert np.isfinite(X).all() and np.isfinite(PH).all()
    hop = T // 2 - 1
    nseg = 3 if T < 200 else 1
    worst = {}
    for n, flags in enumerate(sorted(R.FLAG_SETS)):
        for pairs in (R.SHIPPED_PAIRS, R.THREE_PAIRS):
            cols = R.F * (1 + len(pairs))
            valid = (T, T - 3)[n % 2]
            stft_frames = (nseg - 1) * hop + valid
            Xc = X.copy()
            Xc[:, :, stft_frames:] = np.nan                       # (the phase planes behind stft_frames are not read either)
            PHc = PH.copy()
            PHc[:, :, stft_frames:] = np.nan
            bias, scale = R.feature_affine(cols, 500 + n)
            c = dict(family="analysis", flags=flags, C=C_, opts=dict(R.FLAG_SETS[flags], pairs=tuple(pairs)), nseg=nseg, seg_lo=0,
                     hop=hop, T=T, T_ld=frames, Kp=(cols + 31) // 32 * 32, cols=cols, stft_frames=stft_frames, X=Xc, bias=bias,
                     scale=scale, name=f"phase planes T {T} {flags} pairs {len(pairs)} valid {valid}")
            _check_features(handle, c, worst, PH=PHc)
            for split in (0, 1):
                a = _features(handle, c, split, c["name"], PH=PHc)
                b = _features(handle, c, split, c["name"])
                _same_bits(a, b, c["name"] + f": with against without phase planes, split_out {split}")
    for key, r in sorted(worst.items()):
        print(f"features with phase planes T {T} {key}: worst error / bound {r:.3f}")


# ---- synthesis tail -----------------------------------------------------------------------------------------------------------

def test_wave_ola(handle):
    n = 0
    for c in R.ola_cases():
        G = R.ola_input(c)
        full = c["B"] == 3 and c["T_frames"] == 5 and (c["f_lo"], c["f_hi"]) == (0, 5)
        for level in (R.LEVELS if full else (c["level"],)):
            size = c["B"] * c["out_ld"] + SLACK
            args = (c["B"], c["T_frames"], c["hop"], c["L"], c["q_lo"], c["q_hi"], c["f_lo"], c["f_hi"], c["out_ld"], c["out_q0"])
            want = R.wave_ola(G, R.canary(size), *args, level)
            got = handle.synthesis_tail(0, G if G.size else np.zeros(1, np.float32), R.canary(size), level=level,
                                        **{k: c[k] for k in ("B", "T_frames", "hop", "L", "q_lo", "q_hi", "f_lo", "f_hi", "out_ld", "out_q0")})
            _same_bits(got, want, f"wave_ola {c} level {level}")
            n += 1
    print(f"wave_ola: {n} launches bit for bit")


def test_join_shards(handle):
    for c in R.join_cases():
        g = np.random.RandomState(c["seed"]).standard_normal(c["world"] * c["S"] * c["ld"]).astype(np.float32)
        size = c["S"] * c["out_ld"] + SLACK
        want = R.join_shards(g, R.canary(size), c["ld"], c["t_lo"], c["t_hi"], c["S"], c["hop"], c["n_out"], c["out_ld"])
        got = handle.synthesis_tail(1, g, R.canary(size), t_lo=c["t_lo"], t_hi=c["t_hi"],
                                    **{k: c[k] for k in ("world", "S", "hop", "ld", "n_out", "out_ld")})
        _same_bits(got, want, f"join_shards {c}")


def test_planes_to_rows(handle):
    rs = np.random.RandomState(5)
    for T in (1, 31, 32, 33, 70):
        for KIp in (514, 544):
            for B in (1, 3):
                planes = rs.standard_normal(B * 514 * T).astype(np.float32)
                size = B * T * KIp + SLACK
                want = R.planes_to_rows(planes, R.canary(size), B, 514, T, KIp)
                got = handle.synthesis_tail(2, planes, R.canary(size), B=B, F2=514, T_frames=T, KIp=KIp)
                _same_bits(got, want, f"planes_to_rows B {B} T {T} KIp {KIp}")
                assert not R.bits(got[:B * T * KIp].reshape(B * T, KIp)[:, 514:]).any()


# ---- PCM edges ----------------------------------------------------------------------------------------------------------------

def test_pcm_layout(handle):
    rs = np.random.RandomState(6)
    for n in (1, 255, 256, 257, 1000):
        for C_ in (1, 7):
            n_pad = (n + 40) // 32 * 32 + 32
            pcm = rs.standard_normal((n, C_)).astype(np.float32)
            planes = rs.randint(-32768, 32768, (C_, n)).astype(np.int16)
            planes[:, 0] = -32768
            planes[:, -1] = 32767
            scaled = R.pcm16_scale(planes).T                        # [n][C]
            got = handle.pcm_edges(1, planes, R.canary(n * C_ + SLACK), C=C_, n=n)[0]
            _same_bits(got[:n * C_], scaled.reshape(-1), f"pcm16_to_float n {n} C {C_}")
            _all_canary(got[n * C_:], f"pcm16_to_float n {n} C {C_}: behind the samples")
            for i_lo, i_hi in R.pcm_ranges(n, n_pad):
                what = f"n {n} C {C_} n_pad {n_pad} samples [{i_lo}, {i_hi})"
                size = C_ * n_pad + SLACK
                kw = dict(C=C_, n=n, n_pad=n_pad, i_lo=i_lo, i_hi=i_hi)
                for split in (0, 1):
                    want = R.channel_major(pcm, R.canary(size), n, C_, n_pad, i_lo, i_hi, split)
                    got = handle.pcm_edges(0, pcm, R.canary(size), split_out=split, **kw)[0]
                    _same_bits(got, want, f"deinterleave split_out {split} " + what)
                want = R.channel_major(scaled, R.canary(size), n, C_, n_pad, i_lo, i_hi)
                got = handle.pcm_edges(2, planes, R.canary(size), **kw)[0]
                _same_bits(got, want, "pcm16_to_channel_major " + what)


def test_pcm_peaks(handle):
    rs = np.random.RandomState(8)
    word = lambda v: int(R.bits(np.array([v], np.float32))[0])
    for off, count, pos, above in R.peak_cases():
        # float32: everything in front of and behind the source is far above the maximum
        src = np.full(off + count + 8, 1e9, np.float32)
        body = rs.uniform(-0.5, 0.5, count).astype(np.float32)
        body[pos] = -0.9 if (off + pos) % 2 else 0.9
        src[off:off + count] = body
        before = word(2.0) if above else word(0.25)
        got = handle.pcm_edges(3, src, src_offset=off, count=count, peak_before=before)[1]
        assert int(got[0]) == R.peak_word(body, before), ("pcm_peak_f32", off, count, pos, above, hex(int(got[0])))
        src16 = np.full(off + count + 8, 32767, np.int16)
        body16 = rs.randint(-10000, 10001, count).astype(np.int16)
        body16[pos] = -32768 if (off + pos) % 2 else 30000
        src16[off:off + count] = body16
        got = handle.pcm_edges(4, src16, src_offset=off, count=count, peak_before=before)[1]
        assert int(got[0]) == R.peak_word(R.pcm16_scale(body16), before), ("pcm_peak_i16", off, count, pos, above, hex(int(got[0])))


def test_encode_pcm16(handle):
    wav, n, out_ld = R.encode_case()
    fill = np.full(3 * out_ld + 16, 0x5A5A, np.int16)
    want, peaks = R.encode_pcm16(wav, fill, 3, n, out_ld)
    got, got_peaks = handle.pcm_edges(5, wav, fill, S=3, n=n, out_ld=out_ld)
    _same_bits(got, want, "encode_pcm16")
    assert got_peaks.tolist() == peaks.tolist()
    assert got[30] == 16384 and got[40] == -16384                   # ties to even at +-16383.5


# ---- refusals -------------------------------------------------------------------------------------------------------------------

def test_refusals(handle):
    L = pkg("_lib")
    x = R.analysis_samples(1)
    out = R.canary(514 * 52)

    def refused(fn, *a, **kw):
        with pytest.raises(L.CssError) as e:
            fn(*a, **kw)
        assert e.value.code == L.CSS_ERR_INVALID_ARG, e.value

    refused(handle.analysis, x[:, :-1], 1, x.shape[1] - 1, 0, 4, 52, out)                  # odd x_stride
    refused(handle.analysis, x, 1, x.shape[1], -1, 4, 52, out)                             # t_lo < 0
    refused(handle.analysis, x, 1, x.shape[1], 0, 60, 64, R.canary(514 * 64))              # samples end before the last frame
    refused(handle.analysis, x, 1, x.shape[1], 0, 4, 52, out[:-1])                         # out too short
    c = R.feature_case(64, 0)
    feat = R.canary(c["nseg"] * c["T"] * c["Kp"])
    args = lambda **kw: {**dict(X=c["X"], C_=c["C"], F=R.F, T_ld=c["T_ld"], stft_frames=c["stft_frames"], seg_lo=c["seg_lo"],
                                nseg=c["nseg"], T=c["T"], hop=c["hop"], Kp=c["Kp"], cfg=_cfg(c["opts"]), in_bias=c["bias"],
                                in_scale=c["scale"], feat=feat), **kw}
    refused(lambda: handle.features_host(**args(T=1)))
    refused(lambda: handle.features_host(**args(Kp=c["cols"] - 1)))
    refused(lambda: handle.features_host(**args(Kp=c["cols"] + 1, split_out=1, feat=R.canary(c["nseg"] * c["T"] * (c["cols"] + 1)))))
    bad = _cfg(c["opts"])
    if bad.num_pairs:
        bad.pair_l[0] = c["C"]
        refused(lambda: handle.features_host(**args(cfg=bad)))
    refused(lambda: handle.features_host(**args(feat=feat[:-1])))
    g = np.zeros(3 * 512, np.float32)
    ola = dict(B=1, T_frames=3, hop=256, L=512, q_lo=0, q_hi=4, f_lo=0, f_hi=3, out_ld=1024, out_q0=0)
    refused(handle.synthesis_tail, 0, g, R.canary(1024), **{**ola, "q_lo": 0, "out_q0": 1})
    join = dict(world=1, S=1, hop=16, ld=64, n_out=40, out_ld=40)
    refused(handle.synthesis_tail, 1, np.zeros(64, np.float32), R.canary(40), t_lo=[0], t_hi=[2], **{**join, "hop": 18})
    refused(handle.synthesis_tail, 1, np.zeros(66, np.float32), R.canary(40), t_lo=[0], t_hi=[2], **{**join, "ld": 66})
    refused(handle.pcm_edges, 0, np.zeros(10, np.float32), R.canary(64), C=1, n=10, n_pad=64, i_lo=0, i_hi=65)
    refused(handle.pcm_edges, 0, np.zeros(10, np.float32), R.canary(40), C=1, n=10, n_pad=40, i_lo=0, i_hi=40, split_out=1)
    refused(handle.pcm_edges, 3, np.zeros(10, np.float32), src_offset=8, count=1)


if __name__ == "__main__":
    _forced_child(sys.argv[1])
