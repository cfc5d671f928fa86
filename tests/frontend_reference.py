"""Float64 references of the front-end kernels (csrc/stft.hip, csrc/frontend.hip), written from the definitions in feature.py
as oracle/css_oracle.py states them, the error bounds the kernels are held to, bit-exact float32 models of the kernels that
round nowhere or in a stated order, and the seeded case tables.  No GPU, no library: tests/test_frontend_reference.py checks
this file on the CPU (oracle ties, float32 evaluations inside every bound, every mutation caught),
tests/test_hip_frontend_kernels.py holds the kernels to it.  DESIGN.md 3.2e has the derivations.

References take `dtype` (float64: the reference; float32: the same formulas in numpy's float32 arithmetic, used to show that a
bound is reachable) and `mut`, the name of one deliberate defect (None: the definition).

Constants of the bounds (nothing here is fitted to what a kernel returns):
  U           2^-24, the unit roundoff of float32
  K_ANALYSIS  49: |X - X64| <= K_ANALYSIS U sum_n |w_n x_n| per bin and frame (analysis_bound; the count is in DESIGN.md 3.2e)
  C_ATAN2, C_SINCOS, C_COS, C_LOG   6, 4, 4, 3: the OpenCL single-precision limits (OpenCL C specification, "Relative error as
              ULPs": atan2 <= 6 ulp, sincos / sin / cos <= 4 ulp, log <= 3 ulp) the device library is built to, taken as
              c_f U |value|
  MAG_OPS     2: sqrtf(r r + i i) -- the sum of squares carries (1 + U)^2, its correctly rounded root (1 + U) on top of half that
  SLACK       1 + 2^-10: second-order terms of the first-order propagation
  UNCOND      1e-3 rad: an IPD element whose angle bound exceeds it is counted as unconditioned, not judged
"""
import numpy as np

from gemm_reference import split_decode, split_encode  # noqa: F401  (re-exported for the tests)

U = 2.0 ** -24
K_ANALYSIS = 49
C_ATAN2, C_SINCOS, C_COS, C_LOG = 6, 4, 4, 3
MAG_OPS = 2
SLACK = 1.0 + 2.0 ** -10
UNCOND = 1e-3
SPLIT_ST = 2.0 ** -21         # a value stored in the split format and decoded again (encoder_reference.SPLIT_ST)
SPLIT_FLOOR = 2.0 ** -26
EPS32 = np.float32(1.1920928955078125e-07)
PHASE_NEG_REAL = np.array([0xC0490FDA], np.uint32).view(np.float32)[0]    # kernels.hpp CSS_PHASE_NEG_REAL
CANARY = 0x7FC0BEEF
N_FFT, HOP, F = 512, 256, 257
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def canary(n):
    return np.full(int(n), CANARY, np.uint32).view(np.float32)


# ---- analysis -------------------------------------------------------------------------------------------------------------------

def window_table(window, mut=None):
    """the float32 window stft_build_tables(window) holds: torch.hann_window (periodic) in float64 rounded once; window 1 is its
    float32 square root over 16"""
    n = np.arange(N_FFT, dtype=np.float64)
    hann = (0.5 - 0.5 * np.cos(2.0 * np.pi * n / (N_FFT - 1 if mut == "sym_hann" else N_FFT))).astype(np.float32)
    return np.sqrt(hann) / f32(16.0) if window == 1 else hann


def _exact_cs():
    """cos, sin of 2 pi k / 512 for k = 0 .. 511 with the multiples of pi / 2 exact"""
    k = np.arange(N_FFT)
    c, s = np.cos(2.0 * np.pi * k / N_FFT), np.sin(2.0 * np.pi * k / N_FFT)
    s[k % 256 == 0] = 0.0
    c[k % 256 == 128] = 0.0
    c[k % 128 == 0] = np.round(c[k % 128 == 0])
    s[k % 128 == 0] = np.round(s[k % 128 == 0])
    return c, s


def _frames(x, t_lo, t_hi, shift=0):
    """x [C][n] -> [C][t_hi - t_lo][512]: frame t = samples [256 t, 256 t + 512)"""
    x = np.asarray(x)
    idx = (np.arange(t_lo, t_hi)[:, None] + shift) * HOP + np.arange(N_FFT)[None, :]
    return x[:, idx]


def analysis(x, t_lo, t_hi, window=0, dtype=np.float64, mut=None, win=None):
    """The windowed DFT sum X[c][f][t] = sum_n w_n x[c][256 t + n] exp(-2 pi i f n / 512), f = 0 .. 256, as planes
    [C][514][t_hi - t_lo] (Re rows, then Im rows).  The angle f n is reduced mod 512 in integers, so the sine rows of DC and
    Nyquist are exact zeros.  win: another window than the table's (the oracle tie uses the float64 Hann window)."""
    w = np.asarray(window_table(window, mut) if win is None else win, dtype)
    fr = _frames(x, t_lo, t_hi, 1 if mut == "frame_t1" else 0).astype(dtype) * w
    c, s = _exact_cs()
    k = np.outer(np.arange(F), np.arange(N_FFT)) % N_FFT
    cm, sm = c[k].astype(dtype), s[k].astype(dtype)
    if mut == "nyq_im":
        sm[256] = np.sin(np.pi * np.arange(N_FFT)).astype(dtype)       # the sine of a rounded pi n: not zero
    re = fr @ cm.T
    im = dtype(0.0) - fr @ sm.T
    return np.concatenate([np.moveaxis(re, 1, 2), np.moveaxis(im, 1, 2)], axis=1)


def analysis_bound(x, t_lo, t_hi, window=0):
    """K_ANALYSIS U sum_n |w_n x_n| per (channel, frame), broadcast over the 514 rows: [C][1][t_hi - t_lo]"""
    w = window_table(window).astype(np.float64)
    return K_ANALYSIS * U * np.abs(_frames(x, t_lo, t_hi).astype(np.float64) * w).sum(-1)[:, None, :]


def _cmul32(ar, ai, br, bi):
    return ar * br - ai * bi, ar * bi + ai * br


def analysis_radix4_f32(x, t_lo, t_hi, window=0):
    """the transform the way stft.hip evaluates it, in numpy's float32 arithmetic: packed real frame, four radix-4 Stockham
    stages with float32 twiddles, the real-spectrum step"""
    w = window_table(window)
    z = _frames(x, t_lo, t_hi).astype(np.float32) * w
    br, bi = np.ascontiguousarray(z[..., 0::2]), np.ascontiguousarray(z[..., 1::2])
    m = np.arange(256)
    twr, twi = np.cos(2 * np.pi * m / 256).astype(np.float32), (-np.sin(2 * np.pi * m / 256)).astype(np.float32)
    j = np.arange(64)
    for p in range(4):
        ns = 4 ** p
        k = j & (ns - 1)
        u = [(br[..., j + 64 * q], bi[..., j + 64 * q]) for q in range(4)]
        if p:
            mm = k * (64 // ns)
            u = [u[0]] + [_cmul32(u[q][0], u[q][1], twr[q * mm], twi[q * mm]) for q in (1, 2, 3)]
        a0 = (u[0][0] + u[2][0], u[0][1] + u[2][1]); a1 = (u[0][0] - u[2][0], u[0][1] - u[2][1])
        a2 = (u[1][0] + u[3][0], u[1][1] + u[3][1]); a3 = (u[1][1] - u[3][1], u[3][0] - u[1][0])
        r = [(a0[0] + a2[0], a0[1] + a2[1]), (a1[0] + a3[0], a1[1] + a3[1]), (a0[0] - a2[0], a0[1] - a2[1]),
             (a1[0] - a3[0], a1[1] - a3[1])]
        j0 = ((j - k) << 2) + k
        nr, ni = np.empty_like(br), np.empty_like(bi)
        for q in range(4):
            nr[..., j0 + q * ns], ni[..., j0 + q * ns] = r[q]
        br, bi = nr, ni
    f = np.arange(F)
    w5r, w5i = np.cos(2 * np.pi * f / 512).astype(np.float32), (-np.sin(2 * np.pi * f / 512)).astype(np.float32)
    z0r, z0i, z1r, z1i = br[..., f & 255], bi[..., f & 255], br[..., (256 - f) & 255], bi[..., (256 - f) & 255]
    h = f32(0.5)
    er, ei, orr, oi = h * (z0r + z1r), h * (z0i - z1i), h * (z0i + z1i), h * (z1r - z0r)
    wr, wi = _cmul32(w5r, w5i, orr, oi)
    re, im = er + wr, ei + wi
    re[..., 0], im[..., 0] = (z0r + z0i)[..., 0], 0
    re[..., 256], im[..., 256] = (z0r - z0i)[..., 256], 0
    return np.concatenate([np.moveaxis(re, 1, 2), np.moveaxis(im, 1, 2)], axis=1)


ANALYSIS_RANGES = ((0, 1), (0, 16), (0, 17), (5, 6), (15, 17), (16, 32), (3, 35), (13, 50))
ANALYSIS_FRAMES = 50
ANALYSIS_STRIDE = HOP * (ANALYSIS_FRAMES - 1) + N_FFT + 2
ANALYSIS_LAYOUTS = ((52, 0), (53, 0), (54, 0), (52, 1))          # (row_ld, offset): float4 stores, then three scalar layouts
ANALYSIS_FAMILIES = {7: ("gaussian", "tone", "pcm_scale", "impulses", "quiet", "negative", "zero"),
                     3: ("pcm_scale", "negative", "zero"), 1: ("gaussian",)}


def analysis_samples(C, n_samples=ANALYSIS_STRIDE):
    """[C][n_samples] float32, one input family per channel"""
    rs = np.random.RandomState(100 + C)
    n = np.arange(n_samples)
    x = np.zeros((C, n_samples), np.float32)
    for c, fam in enumerate(ANALYSIS_FAMILIES[C]):
        if fam == "gaussian":
            x[c] = rs.standard_normal(n.size)
        elif fam == "tone":                                    # exactly on bin 37
            x[c] = np.cos(2 * np.pi * ((37 * n) % 512) / 512.0)
        elif fam == "pcm_scale":                               # integer samples up to +-32768
            x[c] = np.clip(np.round(rs.standard_normal(n.size) * 12000), -32768, 32767)
            x[c, 5::997] = -32768
            x[c, 11::991] = 32767
        elif fam == "impulses":                                # an impulse at each end of every frame
            x[c, 0::256] = 1.0
            x[c, 255::256] = -0.5
        elif fam == "quiet":                                   # 1e-6 beside channels of 1
            x[c] = 1e-6 * rs.standard_normal(n.size)
        elif fam == "negative":                                # DC real and negative in every frame
            x[c] = -0.75
    return x


def analysis_input(x, t_lo, t_hi):
    """the samples with everything outside [256 t_lo, 256 (t_hi - 1) + 512) replaced by NaN"""
    y = np.full_like(x, np.nan)
    y[:, HOP * t_lo:HOP * (t_hi - 1) + N_FFT] = x[:, HOP * t_lo:HOP * (t_hi - 1) + N_FFT]
    return y


# ---- features -------------------------------------------------------------------------------------------------------------------

SHIPPED_PAIRS = tuple((m, 0) for m in range(1, 7))
THREE_PAIRS = ((1, 4), (2, 5), (3, 6))
FLAG_SETS = {                                                   # tests/test_feature_options.py OPTION_SETS plus the shipped one
    "shipped": dict(log=0, mvn=1, norm=1, version=1, cos=0),
    "log_v2_cos": dict(log=1, mvn=1, norm=1, version=2, cos=1),
    "v3": dict(log=0, mvn=1, norm=1, version=3, cos=0),
    "nomvn_nonorm": dict(log=0, mvn=0, norm=0, version=1, cos=0),
    "log_v1_cos": dict(log=1, mvn=1, norm=1, version=1, cos=1),
}
PAIR_SETS = ((7, SHIPPED_PAIRS), (7, THREE_PAIRS), (1, ()))
FEATURE_T_TUNED = (2, 3, 63, 64, 65, 186, 191, 192, 193, 255, 256, 257, 371, 511, 512)
FEATURE_T_LONG = (513, 600)
FEATURE_T_FORCED = (2, 65, 186, 257)
FEATURE_FAMILIES = ("gaussian", "magnitudes", "silent_ref", "silent", "negative_real", "constant_difference")


def feature_planes(family, C, T_ld, seed):
    """X [C][514][T_ld] float32.  DC and Nyquist are real in every family, as the transform makes them."""
    rs = np.random.RandomState(seed)
    z = rs.standard_normal((C, F, T_ld)) + 1j * rs.standard_normal((C, F, T_ld))
    if family == "magnitudes":
        z = z / np.abs(z) * 10.0 ** rs.uniform(-6, 3, (C, F, T_ld))
    elif family == "silent_ref":
        z[0] = 0
    elif family == "silent":
        z[:] = 0
    elif family == "constant_difference" and C > 1:
        for c in range(1, C):
            z[c] = z[0] * np.exp(1j * 0.3 * c) * rs.uniform(0.5, 2.0, (F, T_ld))
    z[:, 0] = z[:, 0].real
    z[:, 256] = z[:, 256].real
    if family == "negative_real":                               # real negative bins in some frames, beyond DC and Nyquist too
        z[:, 0, ::3] = -np.abs(z[:, 0, ::3].real)
        z[:, 256, 1::4] = -np.abs(z[:, 256, 1::4].real)
        z[:, 17, ::5] = -np.abs(z[:, 17, ::5].real)
    return np.concatenate([z.real, z.imag], axis=1).astype(np.float32)


def feature_affine(cols, seed):
    rs = np.random.RandomState(seed)
    return rs.uniform(-0.5, 0.5, cols).astype(np.float32), rs.uniform(0.5, 4.0, cols).astype(np.float32)


def feature_case(T, k):
    """case k of segment length T: a rotation through flag sets, pair sets, segment ranges, valid frames and families that
    shows every instantiation every value of each (5 and 6 are coprime: 30 consecutive cases pair every flag set with every
    family)"""
    n = (FEATURE_T_TUNED + FEATURE_T_LONG).index(T) * len(FEATURE_FAMILIES) + k
    family = FEATURE_FAMILIES[n % 6]
    flags = sorted(FLAG_SETS)[n % 5]
    C, pairs = PAIR_SETS[(n + n // 6) % 3]
    nseg, seg_lo = ((1, 0), (3, 0), (1, 2), (3, 2))[(n + n // 5) % 4]
    hop = max(1, T // 2 - 1) if T > 3 else 1
    last = (seg_lo + nseg - 1) * hop
    valid = (T, T - 1, 1, 0)[(n + n // 4) % 4]
    # a segment of silence has the unit phasor 1 in every frame: the mean-removed phasor of versions 1 and 2 is 0 / 0 there and
    # every IPD element unconditioned.  Silence (the family, or a last segment of padding alone) therefore takes version 3 or
    # no normalisation, whose angles are conditioned on it; the magnitude rows (sd = 0) are the same under every flag set
    if pairs and (family == "silent" or valid <= 1) and FLAG_SETS[flags]["norm"] and FLAG_SETS[flags]["version"] != 3:
        flags = "v3" if FLAG_SETS[flags]["mvn"] else "nomvn_nonorm"
    T_ld = last + T + 5
    cols = F * (1 + len(pairs))
    Kp = (cols + 31) // 32 * 32
    bias, scale = feature_affine(cols, 1000 + n)
    X = feature_planes(family, C, T_ld, 2000 + n)
    stft_frames = last + valid
    X[:, :, stft_frames:] = np.nan
    opts = dict(FLAG_SETS[flags], pairs=tuple(pairs))
    return dict(family=family, flags=flags, C=C, opts=opts, nseg=nseg, seg_lo=seg_lo, hop=hop, T=T, T_ld=T_ld, Kp=Kp, cols=cols,
                stft_frames=stft_frames, X=X, bias=bias, scale=scale, name=f"T {T} case {k}: {family}, {flags}, C {C} pairs "
                f"{len(pairs)}, nseg {nseg} seg_lo {seg_lo} hop {hop}, {valid} valid frames in the last segment")


def _segment(X, stft_frames, seg, T, hop):
    """re, im [C][F][T] of segment seg with X = 0 at and past stft_frames; tv = the number of valid frames"""
    X = np.asarray(X)
    C = X.shape[0]
    st = seg * hop
    tv = int(min(max(stft_frames - st, 0), T))
    seg_x = np.zeros((C, 2 * F, T), X.dtype)
    seg_x[:, :, :tv] = X[:, :, st:st + tv]
    return seg_x[:, :F], seg_x[:, F:], tv


def features(X, stft_frames, seg, T, hop, opts, bias, scale, dtype=np.float64, mut=None, bound=False):
    """Feature rows [T][F (1 + pairs)] of segment seg (feature.py:478-508 compute_spectra, 198-249 IPDFeature, the affine of
    conformer.py:298-299).  Phase convention: a bin with Im == 0 and Re < 0 has the float32 value CSS_PHASE_NEG_REAL, a bin
    (0, 0) phase 0; frames at or past stft_frames are X = 0 and take part in the statistics.
    bound=True (float64 only): returns (y, bound, d_angle): the elementwise bound on a float32 kernel's error, and the bound on
    the angle in front of the optional cosine and the affine (0 on the spectral columns)."""
    dt = dtype
    tr = (lambda fn, *a: fn(*a)) if dt == np.float64 else (lambda fn, *a: fn(*[np.asarray(v, np.float64) for v in a]).astype(dt))
    re, im, tv = _segment(X, stft_frames, seg, T, hop)
    re, im = re.astype(dt), im.astype(dt)
    nstat = tv if mut == "valid_only" else T
    sl = slice(0, nstat)
    mean = lambda v: v[..., sl].sum(-1, keepdims=True, dtype=dt) / dt(nstat)
    nl = -(-T // 64) + 6                                         # roundings on an element's path through a T-term sum
    def mean_err(v, d_v):                                        # the sum, 1.0f / T and the product with it
        return ((nl + 2) * U * np.abs(v).sum(-1, keepdims=True) + d_v.sum(-1, keepdims=True)) / T
    eps = dt(EPS32)
    a = np.maximum(np.sqrt(re[0] * re[0] + im[0] * im[0]), eps)
    d_a = MAG_OPS * U * a
    if opts["log"]:
        d_a = C_LOG * U * np.abs(np.log(a)) + d_a / a
        a = tr(np.log, a)
    if opts["mvn"]:
        mu = mean(a)
        dev = a - mu
        q = (dev[..., sl] * dev[..., sl]).sum(-1, keepdims=True, dtype=dt)
        var = q / dt(nstat if mut == "var_T" else nstat - 1)
        sd = np.sqrt(var)
        den = sd + eps
        spec = dev / den
        if bound:
            d_dev = d_a + mean_err(a, d_a) + U * np.abs(dev)
            d_q = (2 * np.abs(dev) * d_dev + d_dev * d_dev).sum(-1, keepdims=True) + (nl + 1) * U * q
            d_var = d_q / (T - 1) + U * var
            d_sd = d_var / (sd + np.sqrt(np.maximum(var - d_var, 0.0)) + 1e-300) + U * sd
            d_sd = np.minimum(d_sd, np.sqrt(d_var) + U * sd)
            d_den = d_sd + U * den
            d_spec = (d_dev + np.abs(spec) * d_den) / np.maximum(den - d_den, 0.5 * eps) + U * np.abs(spec)
    else:
        spec, d_spec = a, d_a
    rows, d_rows, d_ang = [spec], [d_spec if bound else None], [np.zeros_like(spec)]
    pairs = opts["pairs"]
    if pairs:
        special = (im == 0) & (re < 0)
        neg = dt(np.pi) if mut == "pi_plus" else dt(PHASE_NEG_REAL)
        ph = np.where(special, neg, tr(np.arctan2, im, re))
        d_ph = np.where(special | ((im == 0) & (re == 0)), 0.0, C_ATAN2 * U * np.abs(ph))
    for l, r in pairs:
        if mut == "swap_lr":
            l, r = r, l
        d = ph[l] - ph[r]
        d_d = d_ph[l] + d_ph[r] + U * np.abs(d)
        c, s = tr(np.cos, d), tr(np.sin, d)
        d_c, d_s = C_SINCOS * U * np.abs(c) + np.abs(s) * d_d, C_SINCOS * U * np.abs(s) + np.abs(c) * d_d
        v, d_v = d, d_d
        version = opts["version"] + (1 if mut == "v2_as_v3" and opts["version"] == 2 else 0)
        if opts["norm"]:
            yrm, yim = mean(c), mean(s)
            d_yrm, d_yim = mean_err(c, d_c), mean_err(s, d_s)
            if version == 1:
                ca, sa = c - yrm, s - yim
                v = tr(np.arctan2, sa, ca)
                with np.errstate(divide="ignore", invalid="ignore"):
                    d_v = ((d_c + d_yrm + U * np.abs(ca)) + (d_s + d_yim + U * np.abs(sa))) / np.hypot(ca, sa) + C_ATAN2 * U * np.abs(v)
                d_v = np.where(np.isfinite(d_v), d_v, np.inf)
            else:
                if version == 2:
                    shift = tr(np.arctan2, yim, yrm)
                    with np.errstate(divide="ignore", invalid="ignore"):
                        d_shift = (d_yrm + d_yim) / np.hypot(yrm, yim) + C_ATAN2 * U * np.abs(shift)
                    d_shift = np.where(np.isfinite(d_shift), d_shift, np.inf)
                else:
                    shift = mean(d)
                    d_shift = mean_err(d, d_d)
                v = d - shift
                d_v = d_d + d_shift + U * np.abs(v)
        d_ang.append(np.broadcast_to(d_v, v.shape))
        if opts["cos"]:
            if mut == "cos_first":
                v = tr(np.cos, d) - mean(tr(np.cos, d))
            else:
                d_v = C_COS * U * np.abs(np.cos(v)) + np.abs(np.sin(v)) * np.minimum(d_v, 1e30)
                v = tr(np.cos, v)
        rows.append(v)
        d_rows.append(np.broadcast_to(d_v, v.shape))
    v = np.concatenate(rows, axis=0).T                            # [T][cols]
    b, sc = np.asarray(bias, dt), np.asarray(scale, dt)
    y = (v + b) * sc
    if not bound:
        return y
    assert dt == np.float64
    d_v = np.concatenate(d_rows, axis=0).T
    d_y = ((d_v + U * np.abs(v + b)) * np.abs(sc) + U * np.abs(y)) * SLACK
    return y, d_y, np.concatenate(d_ang, axis=0).T


def angle_columns(opts):
    """columns that hold a raw angle (compared modulo 2 pi scale)"""
    cols = np.zeros(F * (1 + len(opts["pairs"])), bool)
    cols[F:] = not opts["cos"]
    return cols


def feature_error(y, y64, scale, opts):
    """|y - y64|, the raw-angle columns modulo 2 pi scale"""
    e = np.asarray(y, np.float64) - y64
    period = 2.0 * np.pi * np.abs(np.asarray(scale, np.float64))
    ang = angle_columns(opts)
    e[:, ang] -= np.round(e[:, ang] / period[ang]) * period[ang]
    return np.abs(e)


def oracle_features(O, X, stft_frames, seg, T, hop, opts, bias, scale):
    """the same rows through css_oracle.features(dtype=float64)"""
    re, im, _ = _segment(X, stft_frames, seg, T, hop)
    z = np.moveaxis(re.astype(np.float64) + 1j * im.astype(np.float64), 0, 2)        # [F][T][C]
    f = O.features(z if z.shape[2] > 1 else z[:, :, 0], dtype=np.float64, log_spectrogram=bool(opts["log"]),
                   mvn_spectrogram=bool(opts["mvn"]), ipd_mean_normalize=bool(opts["norm"]),
                   ipd_mean_normalize_version=opts["version"], ipd_cos=bool(opts["cos"]), pairs=list(opts["pairs"]) or None)
    return (f.T + np.asarray(bias, np.float64)) * np.asarray(scale, np.float64)


# ---- exact kernels: float32 numpy in the kernel's stated order --------------------------------------------------------------

def level_gain(word):
    """split_f16.hpp level_gain: the power of two that brings the peak into [0.5, 1); 1 for an absent word, silence, and a peak
    that is not below 3e38"""
    if word is None:
        return f32(1.0)
    p = np.array([word], np.uint32).view(np.float32)[0]
    if not (p > 0) or not (p < f32(3.0e38)):
        return f32(1.0)
    e = int(np.frexp(p)[1])
    return np.ldexp(f32(1.0), -min(max(e, -100), 100)).astype(np.float32)


def wave_ola(G, out, B, T_frames, hop, L, q_lo, q_hi, f_lo, f_hi, out_ld, out_q0, level, mut=None):
    """launch_wave_ola on the allocation `out` (flat): sample hop q + r takes the frames q - j that cover it, the oldest assigned,
    later ones added, then the exact power of two 1 / level_gain"""
    G = np.asarray(G, np.float32).reshape(-1)[:B * T_frames * L].reshape(B, T_frames, L)
    out = np.array(out, np.float32).reshape(-1)
    inv = f32(1.0) / level_gain(level)
    r = np.arange(hop)
    jmax = (L - 1 - r) // hop
    js = list(range(int(jmax.max()), -1, -1))
    if mut == "newest_first":
        js = js[::-1]
    if mut == "ignore_f_hi":
        f_hi = T_frames
    with np.errstate(over="ignore", invalid="ignore"):
        for b in range(B):
            for q in range(q_lo, q_hi):
                n0 = (q - out_q0) * hop
                v = np.zeros(hop, np.float32)
                for j in js:
                    t = q - j
                    ok = j <= jmax
                    if t < f_lo or t >= f_hi or not ok.any():
                        continue
                    xv = np.zeros(hop, np.float32)
                    xv[ok] = G[b, t, (r + j * hop)[ok]]
                    first = (j == jmax) if mut != "newest_first" else (j == 0)
                    v = np.where(ok, np.where(first, xv, v + xv), v)
                if level is not None:
                    v = v * inv
                m = n0 + r < out_ld
                out[b * out_ld + n0 + r[m]] = v[m]
    return out


def join_shards(g, out, ld, t_lo, t_hi, S, hop, n_out, out_ld):
    """launch_join_shards on the allocation `out` (flat): the sum over the ranks that hold a block, in rank order from 0.f"""
    g = np.asarray(g, np.float32).reshape(-1)
    out = np.array(out, np.float32).reshape(-1)
    n = np.arange(n_out)
    q, r = n // hop, n % hop
    for sp in range(S):
        v = np.zeros(n_out, np.float32)
        for k in range(len(t_lo)):
            if t_hi[k] <= t_lo[k]:
                continue
            m = (q >= t_lo[k]) & (q <= t_hi[k])
            v[m] = v[m] + g[(k * S + sp) * ld + (q[m] - t_lo[k]) * hop + r[m]]
        out[sp * out_ld:sp * out_ld + n_out] = v
    return out


def planes_to_rows(planes, out, B, F2, T, KIp):
    out = np.array(out, np.float32).reshape(-1)
    rows = np.zeros((B, T, KIp), np.float32)
    rows[:, :, :F2] = np.moveaxis(np.asarray(planes, np.float32).reshape(-1)[:B * F2 * T].reshape(B, F2, T), 1, 2)
    out[:B * T * KIp] = rows.reshape(-1)
    return out


def channel_major(src, out, n, C, n_pad, i_lo, i_hi, split_out=0):
    """launch_deinterleave / launch_pcm16_to_channel_major on the allocation `out`: src float32 [n][C] (already scaled), samples
    [i_lo, i_hi) of every channel row, zeros past n; split rows are split_encode of the float32 row, element by element"""
    src = np.asarray(src, np.float32).reshape(n, C)
    out = np.array(out, np.float32).reshape(-1)
    if i_hi <= i_lo:
        return out
    vals = np.zeros((C, i_hi - i_lo), np.float32)
    k = max(0, min(n, i_hi) - i_lo)
    vals[:, :k] = src[i_lo:i_lo + k].T
    if not split_out:
        for c in range(C):
            out[c * n_pad + i_lo:c * n_pad + i_hi] = vals[c]
        return out
    halves = out.view(np.float16)
    full = np.zeros((C, n_pad), np.float32)
    full[:, i_lo:i_hi] = vals
    enc = split_encode(full).view(np.float16).reshape(C, n_pad // 32, 2, 32)
    dst = halves[:C * n_pad * 2].reshape(C, n_pad // 32, 2, 32)
    i = np.arange(i_lo, i_hi)
    dst[:, i // 32, :, i % 32] = enc[:, i // 32, :, i % 32]
    return out


def pcm16_scale(planes):
    """int16 -> float32: x * 2^-15 (exact)"""
    return np.asarray(planes, np.int16).astype(np.float32) * f32(1.0 / 32768.0)


def peak_word(x, before):
    """launch_pcm_peak_*: max(word, max |x| as float bits); x float32 (int16 samples scaled by 2^-15 first)"""
    return max(int(before), int(bits(np.abs(np.asarray(x, np.float32)).max().reshape(1))[0]))


def encode_pcm16(wav, out, S, n, out_ld, mut=None):
    """launch_encode_pcm16 on the int16 allocation `out`: wavio's operations value for value.  Returns (out, peak words)."""
    wav = np.asarray(wav, np.float32).reshape(-1)[:S * n].reshape(S, n)
    out = np.array(out, np.int16).reshape(-1)
    peak = np.abs(wav).max(axis=1).astype(np.float32)
    den = peak if mut == "no_1e-7" else peak + f32(1e-7)
    with np.errstate(divide="ignore", invalid="ignore"):
        y = (wav * f32(0.99)) / den[:, None]
    v = y.astype(np.float64) * 32767.0
    v = np.trunc(v) if mut == "trunc" else np.rint(v)
    v = np.minimum(np.maximum(v, -32768.0), 32767.0)
    for s in range(S):
        out[s * out_ld:s * out_ld + n] = np.where(np.isnan(v[s]), 0, v[s]).astype(np.int16)   # (0 / 0 without the 1e-7)
    return out, bits(peak)


# ---- case tables of the exact kernels ---------------------------------------------------------------------------------------

LEVELS = (None, 0x00000000, 0x00000123, 0x35800000, 0x3F333333, 0x47000000, 0x7F800000)   # absent, 0, a subnormal, 2^-20, 0.7, 32768, +inf


def ola_cases():
    """every (L, hop), B, T_frames and frame window; q ranges that start behind out_q0 and end past the last frame's end; an
    out_ld that cuts the last block short; the levels in rotation"""
    cases, n = [], 0
    for L, hop in ((512, 256), (400, 160), (512, 128)):
        for B in (1, 3):
            for Tf in (1, 2, 5, 19):
                windows = {(0, Tf), (0, 0), (min(1, Tf), Tf), (0, Tf - 1), (Tf // 2, Tf // 2 + 1)}
                for f_lo, f_hi in sorted(windows):
                    out_q0 = n % 3
                    q_lo = out_q0 + 1 + n % 2
                    q_hi = Tf + (L + hop - 1) // hop + 1          # one block past the last frame's end
                    if q_hi <= q_lo:
                        q_hi = q_lo + 1
                    out_ld = (q_hi - out_q0) * hop - (hop // 2 + 3)
                    cases.append(dict(L=L, hop=hop, B=B, T_frames=Tf, f_lo=f_lo, f_hi=f_hi, q_lo=q_lo, q_hi=q_hi, out_q0=out_q0,
                                      out_ld=out_ld, level=LEVELS[n % len(LEVELS)], seed=n))
                    n += 1
    return cases


def ola_input(c):
    rs = np.random.RandomState(300 + c["seed"])
    return rs.standard_normal(c["B"] * c["T_frames"] * c["L"]).astype(np.float32)


def join_cases():
    """world 1, 2, 3, 8 with empty ranks and seams shared by two ranks; n_out % 4 in {0, 1, 3}"""
    cases = []
    hop = 16
    for n, (world, cuts) in enumerate(((1, [0, 9]), (2, [0, 4, 9]), (3, [0, 3, 3, 9]), (8, [0, 2, 2, 5, 6, 6, 6, 8, 9]))):
        for rem in (0, 1, 3):
            t_lo, t_hi = cuts[:-1], cuts[1:]                     # rank k holds blocks t_lo .. t_hi: the seam block is in both
            n_out = 9 * hop + hop - 4 + rem
            cases.append(dict(world=world, S=2 + n % 2, hop=hop, ld=((max(h - l for l, h in zip(t_lo, t_hi)) + 1) * hop + 4),
                              t_lo=t_lo, t_hi=t_hi, n_out=n_out, out_ld=(n_out + 7) // 4 * 4, seed=10 * n + rem))
    return cases


def pcm_ranges(n, n_pad):
    """[i_lo, i_hi): inside n, across n, past n, everything, empty"""
    return ((0, max(1, n // 2)), (n // 3, min(n_pad, n + 7)), (min(n + 1, n_pad), n_pad), (0, n_pad), (n // 2, n // 2))


def peak_cases():
    """(source offset, count, position of the maximum, prior word below / above)"""
    cases = []
    for off in range(8):
        for count in (1, 3, 7, 8, 9, 4097):
            spots = sorted({0, min(count - 1, 2), count - 1, count // 2})     # first element, unaligned head, tail, body
            for i, pos in enumerate(spots):
                cases.append((off, count, pos, (off + count + i) % 2))
    return cases


def encode_case():
    """S = 3 with an all-zero stream; stream 0 has values that land exactly on 16383.5 and -16383.5 after scaling (ties to even:
    16384 and -16384; truncation gives 16383) and +-peak; n = 1000, out_ld = 1008"""
    rs = np.random.RandomState(77)
    n = 1000
    wav = (0.3 * rs.standard_normal((3, n))).astype(np.float32)
    wav[1] = 0
    wav[0] = np.clip(wav[0], -0.9, 0.9)
    wav[0, 10], wav[0, 20] = 1.0, -1.0                           # +-peak
    den = f32(1.0) + f32(1e-7)
    x = f32(0.5) * den / f32(0.99)
    cand = x + np.arange(-64, 65) * np.spacing(x)
    hit = cand[(cand.astype(np.float32) * f32(0.99)) / den == f32(0.5)]
    assert hit.size, "no float32 lands on 0.5"
    wav[0, 30], wav[0, 40] = hit[0], -hit[0]
    return wav, n, 1008
