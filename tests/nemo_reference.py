"""Float64 reference of the NeMo log-mel hand-off (csrc/nemo.hip, csrc/api_nemo_handoff.hip; include/css_mi355_nemo_handoff.h), the
error bound its device path is held to, a float32 restatement of that path, the named mistakes as switches of the reference,
and the run tables and signals of tests/test_hip_nemo_kernels.py.  No GPU, no library: tests/test_nemo_reference.py checks this
file on the CPU.

The definition (NeMo's AudioToMelSpectrogramPreprocessor as transformers' ParakeetFeatureExtractor states it), per stream with
x = the concatenation of its kept ranges: y[0] = x[0], y[c] = x[c] - p x[c - 1] with the product and the difference rounded to
float32 one after the other (torch's own arithmetic, so y is an INPUT of everything below, not a source of error; p == 0:
y = x); 256 zeros before and behind y; frame j = padded samples [160 j, 160 j + 512); the window is zero on [0, 56) and
[456, 512) and the symmetric Hann 0.5 - 0.5 cos(2 pi n / 399), rounded to float32 once, at 56 + n; the 512-point DFT, 257 bins;
n // 160 frames; re^2 + im^2; the slaney bank [n_mels][257]; ln(mel + 2^-24); per band (v - mean) / (std + 1e-5) with
mean = sum / L and std = sqrt(sum (v - mean)^2 / (L - 1)) over the L frames (std := 0 for L == 1).  Everything after y is
evaluated in float64.

The bound, counted along the device path (U = 2^-24; every count is a number of float32 roundings):
  tables      one rounding per entry of the analysis matrix and of the bank                                          1, 1
  product     launch_gemm: a k-ordered fmaf chain over K = 512                                                      512
              -> |dRe| <= (512 + 1) U sum_n |a_n y_n| with the reference's own sum, likewise Im
  power       re re + im im: a term passes at most two roundings                                                      2
  mel sum     a 257-term fmaf chain of non-negative terms: relative                                                 257
              -> dmel <= sum_f w_f dp_f + (257 + 1) U sum_f w_f (p_f + dp_f)
  guard       mel + 2^-24: one rounding                                                                                1
  logf        C_LOG = 2 ulp: no accuracy table of the device library is installed beside it, so this is the fall-back the
              Whisper reference (tests/handoff_reference.py) uses for log10f, the one number here that is not derived; taken
              as 2 C_LOG U |value|.  Before it the logarithm carries the sum's error: ln(v + dv) - ln v above,
              ln v - ln(max(v - dv, 2^-24)) below (the device's sum is not negative, so its v is at least the guard).
              There is no floor to be exactly on: NO element is left out of any comparison.
  statistics  float64 sums on the device (their own error is 2^-29 of a float32 rounding): the mean carries the mean of the
              raw bounds and one rounding; d_j = v_j - mean carries e_j + mean(e), so the root of the sum of squares moves by
              at most the root of the sum of those squared (the triangle inequality in l2), and std is rounded once
  normalise   v - mean: one rounding; std + 1e-5f: one rounding and the distance of the float32 1e-5 from 1e-5; the
              quotient: one rounding; propagated as (e_num + |out| e_den) / (den - e_den)
  SECOND      1 + 2^-10 on every first-order term; TINY: a power below the smallest normal float32 may flush to zero

`mut` names one deliberate mistake (MISTAKES); None is the definition."""
import numpy as np

from frontend_reference import CANARY, U, bits, canary  # noqa: F401  (shared with the other kernel tests)

f32 = np.float32
SECOND = 1.0 + 2.0 ** -10
C_LOG = 2
TINY = 2.0 ** -126
NFFT, HOPW, BINS, WIN, WIN_OFF, PADW = 512, 160, 257, 400, 56, 256
GUARD = 2.0 ** -24
EPS = 1e-5
TILE = 32

MISTAKES = ("periodic_hann", "window_at_0", "reflect_pad", "preemph_restart", "extra_frame", "log10", "floor", "biased_var",
            "eps_in_sqrt", "stats_over_cap", "bank_201", "magnitude")


# ---- run tables -------------------------------------------------------------------------------------------------------------------

def run_table(ranges, cap_ranges):
    """[n][2] sample ranges -> (regs [cap][2], offs [cap], A, n) as the keep-scan leaves them (unused rows zero)"""
    ranges = np.asarray(ranges, np.int64).reshape(-1, 2)
    regs, offs = np.zeros((cap_ranges, 2), np.int64), np.zeros(cap_ranges, np.int64)
    n = len(ranges)
    lens = ranges[:, 1] - ranges[:, 0]
    regs[:n] = ranges
    offs[:n] = np.concatenate([[0], np.cumsum(lens)])[:n]
    return regs, offs, int(lens.sum()), n


def concat(row, ranges):
    ranges = np.asarray(ranges, np.int64).reshape(-1, 2)
    if len(ranges) == 0:
        return np.zeros(0, np.float32)
    return np.concatenate([row[a:b] for a, b in ranges]).astype(np.float32)


def preemphasised(row, ranges, p, mut=None):
    """y over the concatenation, float32, each operation rounded once; the mistake restarts at every range seam"""
    ranges = np.asarray(ranges, np.int64).reshape(-1, 2)
    x = concat(row, ranges)
    if not p or len(x) == 0:
        return x
    y = x.copy()
    y[1:] = x[1:] - f32(p) * x[:-1]
    if mut == "preemph_restart":
        for o in np.cumsum(ranges[:, 1] - ranges[:, 0])[:-1]:
            y[o] = x[o]
    return y


# ---- tables -----------------------------------------------------------------------------------------------------------------------

def window(mut=None):
    w = np.zeros(NFFT)
    n = np.arange(WIN)
    h = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / (WIN if mut == "periodic_hann" else WIN - 1))
    off = 0 if mut == "window_at_0" else WIN_OFF
    w[off:off + WIN] = h.astype(np.float32)
    return w


def analysis_matrix(mut=None):
    """[514][512] float64: rows f: w_n cos(2 pi f n / 512), rows 257 + f: -w_n sin(2 pi f n / 512)"""
    f, n = np.arange(BINS)[:, None], np.arange(NFFT)[None, :]
    a = 2.0 * np.pi * ((f * n) % NFFT) / NFFT
    return np.concatenate([np.cos(a), -np.sin(a)]) * window(mut)[None, :]


def mel_bank(n_mels, bins=BINS):
    """librosa.filters.mel(sr=16000, n_fft=2 (bins - 1), n_mels, fmin=0, fmax=8000, norm="slaney"), from the formula, float64"""
    f_sp, min_log_hz, logstep = 200.0 / 3.0, 1000.0, np.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp
    hz2mel = lambda f: np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-30) / min_log_hz) / logstep, f / f_sp)
    mel2hz = lambda m: np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)
    mel_f = mel2hz(np.linspace(hz2mel(np.float64(0.0)), hz2mel(np.float64(8000.0)), n_mels + 2))
    fft_f = np.linspace(0.0, 8000.0, bins)
    w = np.zeros((n_mels, bins))
    for i in range(n_mels):
        lower = (fft_f - mel_f[i]) / (mel_f[i + 1] - mel_f[i])
        upper = (mel_f[i + 2] - fft_f) / (mel_f[i + 2] - mel_f[i + 1])
        w[i] = np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (mel_f[i + 2] - mel_f[i]))
    return w


_TABLES = {}


def tables(n_mels, mut=None):
    key = (n_mels, mut if mut in ("periodic_hann", "window_at_0", "bank_201") else None)
    if key not in _TABLES:
        W = mel_bank(n_mels)
        if mut == "bank_201":   # Whisper's bank laid over the first 201 of the 257 bins
            W = np.concatenate([mel_bank(n_mels, 201), np.zeros((n_mels, BINS - 201))], axis=1)
        _TABLES[key] = (analysis_matrix(key[1]), W)
    return _TABLES[key]


# ---- the reference ----------------------------------------------------------------------------------------------------------------

class Ref:
    """x, y, nfr, re, im, power [257][nfr], mel, raw [n_mels][nfr], mean, std [n_mels], out (the normalised rows, or raw); with
    want_bound: e_raw, e_mean, e_std, bound (on out)"""


def frames_of(n, mut=None):
    return n // HOPW + (1 if mut == "extra_frame" else 0)


def padded(y, mut=None):
    y = np.asarray(y, np.float64)
    if mut == "reflect_pad" and len(y) > PADW:
        return np.concatenate([y[PADW:0:-1], y, y[-2:-PADW - 2:-1]])
    return np.concatenate([np.zeros(PADW), y, np.zeros(PADW + NFFT)])   # (room for the mistaken extra frame)


def reference(row, ranges, n_mels, preemph=0.97, normalize=True, mut=None, want_bound=True, cap=None):
    """row: a stream's samples (float32); ranges [n][2]: its kept ranges -> Ref.  cap: the frames the mistake `stats_over_cap`
    takes its statistics over (the columns behind the valid ones hold zeros there)"""
    r = Ref()
    r.y = preemphasised(np.asarray(row, np.float32), ranges, preemph, mut)
    n = len(r.y)
    nfr = r.nfr = frames_of(n, mut)
    r.mean, r.std = np.zeros(n_mels), np.zeros(n_mels)
    if nfr == 0:
        r.raw = r.out = r.bound = r.e_raw = np.zeros((n_mels, 0))
        return r
    A, W = tables(n_mels, mut)
    op = padded(r.y, mut)
    if len(op) < HOPW * (nfr - 1) + NFFT:
        op = np.concatenate([op, np.zeros(HOPW * (nfr - 1) + NFFT - len(op))])
    fr = np.lib.stride_tricks.sliding_window_view(op, NFFT)[::HOPW][:nfr].T               # [512][nfr]
    spec = A @ fr
    r.re, r.im = spec[:BINS], spec[BINS:]
    r.power = r.re * r.re + r.im * r.im
    r.mel = W @ (np.sqrt(r.power) if mut == "magnitude" else r.power)
    if mut == "log10":
        r.raw = np.log10(r.mel + GUARD)
    elif mut == "floor":
        r.raw = np.log(np.maximum(r.mel, GUARD))
    else:
        r.raw = np.log(r.mel + GUARD)
    L = nfr
    v = r.raw
    if mut == "stats_over_cap":
        L = int(cap if cap is not None else nfr + TILE)
        v = np.concatenate([r.raw, np.zeros((n_mels, L - nfr))], axis=1)
    r.mean = v.sum(axis=1) / L
    ss = ((v - r.mean[:, None]) ** 2).sum(axis=1)
    if L == 1:
        r.std = np.zeros(n_mels)
    elif mut == "biased_var":
        r.std = np.sqrt(ss / L)
    elif mut == "eps_in_sqrt":
        r.std = np.sqrt(ss / (L - 1) + EPS) - EPS     # (so that std + eps below is sqrt(var + eps))
    else:
        r.std = np.sqrt(ss / (L - 1))
    r.out = (r.raw - r.mean[:, None]) / (r.std[:, None] + EPS) if normalize else r.raw
    if not want_bound:
        return r
    assert mut is None, "the bound belongs to the definition"
    s = np.abs(A) @ np.abs(fr)
    r.s_re, r.s_im, r.W = s[:BINS], s[BINS:], W
    r.bound = bound(r, normalize)
    return r


def bound(r, normalize=True, k_prod=NFFT + 1, k_pow=2, k_mel=BINS + 1, c_log=C_LOG, k_stat=0.0):
    """the bound on r.out for a float32 path that rounds k_prod times per term of the product (table included), k_pow times per
    term of the power, k_mel times per term of the mel sum (table included) and takes a logarithm of c_log ulp: the device path by
    default (the module's header has the counts).  k_stat: float32 roundings per term of the two statistics' sums (0 on the
    device, whose sums are float64).  Leaves e_raw, e_mean, e_std on r."""
    e_re, e_im = SECOND * k_prod * U * r.s_re, SECOND * k_prod * U * r.s_im
    dp = 2 * np.abs(r.re) * e_re + e_re ** 2 + 2 * np.abs(r.im) * e_im + e_im ** 2
    e_pow = dp + SECOND * k_pow * U * (r.power + dp) + TINY
    e_mel = r.W @ e_pow + SECOND * k_mel * U * (r.W @ (r.power + e_pow))
    v = r.mel + GUARD
    e_v = e_mel + SECOND * U * (v + e_mel)
    prop = np.maximum(np.log(v + e_v) - r.raw, r.raw - np.log(np.maximum(v - e_v, GUARD)))
    r.e_raw = prop + SECOND * 2 * c_log * U * (np.abs(r.raw) + prop)
    if not normalize:
        return r.e_raw
    L = r.raw.shape[1]
    absmean = np.abs(r.raw).mean(axis=1)
    r.e_mean = r.e_raw.mean(axis=1) + SECOND * U * np.abs(r.mean) + SECOND * k_stat * L * U * absmean
    e_d = r.e_raw + r.e_raw.mean(axis=1)[:, None] + (SECOND * k_stat * L * U * absmean)[:, None]
    if L > 1:
        r.e_std = np.sqrt((e_d ** 2).sum(axis=1) / (L - 1)) + SECOND * (1 + k_stat * L) * U * (r.std + 1e-30)
    else:
        r.e_std = np.zeros_like(r.std)
    num = r.raw - r.mean[:, None]
    e_num = r.e_raw + r.e_mean[:, None] + SECOND * U * (np.abs(num) + r.e_raw + r.e_mean[:, None])
    den = r.std + EPS
    e_den = r.e_std + SECOND * U * (den + r.e_std) + abs(float(f32(EPS)) - EPS)
    # Where the denominator's bound reaches the denominator (a band that is constant over the frames, as digital silence: std = 0
    # and den = 1e-5) the quotient cannot be propagated; there the device's denominator is still at least the float32 1e-5, so
    # its value is at most (|num| + e_num) / 1e-5 in magnitude, and the element is held to that plus the reference's own value.
    sure = den > 2 * e_den
    q = (e_num + np.abs(r.out) * e_den[:, None]) / np.where(sure, den - e_den, 1.0)[:, None]
    loose = np.abs(r.out) + (np.abs(num) + e_num) / (EPS * (1.0 - 4 * U))
    q = np.where(sure[:, None], q, loose)
    return q + SECOND * U * (np.abs(r.out) + q)


def deviation(mref, ref):
    """how far a mistaken reference lies from the definition, in units of the bound: the largest |out' - out| / bound, inf where
    the shapes differ; (ratio, position)"""
    if mref.out.shape != ref.out.shape:
        return np.inf, None
    if ref.out.size == 0:
        return 0.0, None
    d = np.abs(mref.out - ref.out)
    q = np.where(d == 0, 0.0, d / np.maximum(ref.bound, 1e-300))
    pos = np.unravel_index(int(q.argmax()), q.shape)
    return float(q[pos]), pos


# ---- the device path in float32 ---------------------------------------------------------------------------------------------------

def _fma32(a, b, c):
    """fmaf on float32 arrays: the product is exact in float64, the sum rounds there once before the rounding to float32 (a
    double rounding in about one case in 2^29: a model, not the bits)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def model32(row, ranges, n_mels, preemph=0.97, normalize=True):
    """nemo.hip's arithmetic restated in numpy float32: float32 tables, ascending fmaf chains, fmaf(re, re, im im), the float32
    guard, the logarithm in float64 rounded once, float64 statistics rounded once, the float32 normalisation
    -> (raw, mean, std, out), float32"""
    y = preemphasised(np.asarray(row, np.float32), ranges, preemph)
    nfr = frames_of(len(y))
    A, W = tables(n_mels)
    A32, W32 = A.astype(np.float32), W.astype(np.float32)
    op = np.concatenate([np.zeros(PADW, np.float32), y, np.zeros(PADW, np.float32)])
    fr = np.lib.stride_tricks.sliding_window_view(op, NFFT)[::HOPW][:nfr].T
    acc = np.zeros((2 * BINS, nfr), np.float32)
    for k in range(NFFT):
        acc = _fma32(A32[:, k:k + 1], fr[k:k + 1, :], acc)
    re, im = acc[:BINS], acc[BINS:]
    p = _fma32(re, re, im * im)
    mel = np.zeros((n_mels, nfr), np.float32)
    for f in range(BINS):
        mel = _fma32(W32[:, f:f + 1], p[f:f + 1, :], mel)
    raw = np.log((mel + f32(GUARD)).astype(np.float64)).astype(np.float32)
    if nfr == 0:
        z = np.zeros(n_mels, np.float32)
        return raw, z, z, raw
    mean64 = raw.astype(np.float64).sum(axis=1) / nfr
    ss = ((raw.astype(np.float64) - mean64[:, None]) ** 2).sum(axis=1)
    mean, std = mean64.astype(np.float32), (np.sqrt(ss / (nfr - 1)) if nfr > 1 else np.zeros(n_mels)).astype(np.float32)
    out = (raw - mean[:, None]) / (std[:, None] + f32(EPS)) if normalize else raw
    return raw, mean, std, out.astype(np.float32)


# ---- signals and cases ------------------------------------------------------------------------------------------------------------

def signal(kind, n, seed=0):
    """float32 [n]; the first sample is never zero except for `zeros`"""
    t = np.arange(n) / 16000.0
    if kind == "noise":
        x = np.random.default_rng(2000 + seed).uniform(-0.5, 0.5, n)
    elif kind == "tones":
        x = 0.5 * np.sin(2 * np.pi * 1000.0 * t + 0.3) + 0.5e-3 * np.sin(2 * np.pi * 6100.0 * t)
    elif kind == "speechlike":   # a harmonic stack under a slow envelope, with stretches of exact silence
        env = np.clip(np.sin(2 * np.pi * 1.3 * t + seed), 0.0, None) ** 2
        x = env * sum(np.sin(2 * np.pi * 140.0 * h * t + h) / h for h in range(1, 24)) * 0.2 + 1e-4
    elif kind == "quiet":        # mel powers around the guard 2^-24: the logarithm's argument is mostly the guard, std is small
        x = 3e-5 * np.random.default_rng(3000 + seed).uniform(-0.5, 0.5, n)
    elif kind == "constant":
        x = np.full(n, 0.25)
    elif kind == "zeros":
        x = np.zeros(n)
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


def blocks_of(n, block=256):
    """the whole of [0, n) as ranges of `block` samples: one frame of 512 spans three of them, every seam lies inside the
    pre-emphasis"""
    return np.array([[a, min(a + block, n)] for a in range(0, n, block)], np.int64).reshape(-1, 2)


# the lengths the kernel tests run, in samples of the concatenation -> frames = n // 160
EDGE_LENGTHS = (0, 159, 160, 319, 320)
TILE_FRAMES = (31, 32, 33)
REDUCE_FRAMES = (255, 256, 257, 1025)
