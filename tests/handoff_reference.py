"""Float64 reference of the Whisper log-mel hand-off (csrc/handoff.hip, css_handoff_logmel in csrc/api_stages.hip), the error
bound its device path is held to, a float32 restatement of that path, the named mistakes as switches of the reference, and the
signals, gates and cases of tests/test_hip_handoff_values.py ("The hand-off's values").  No GPU, no library:
tests/test_handoff_reference.py checks this file on the CPU.

The definition (whisper/audio.py log_mel_spectrogram, as handoff.hip's header and tests/golden/gen_golden_whisper.py state it):
the kept sample ranges concatenated; reflect padding by 200 without edge repeat; frames of 400 at hop 160, the last one dropped
(n // 160 frames); the periodic Hann window rounded to float32 once (torch.hann_window); the 400-point DFT; |X|^2;
librosa.filters.mel(16000, 400, n_mels) (slaney scale and normalisation); log10(max(., 1e-10f)); max(., global max - 8);
(. + 4) / 4.  Everything after the samples is evaluated in float64 (the DFT as a float64 matrix product: its own error is
2^-29 of the bound's product term).

The bound on the normalised output, counted along the device path (U = 2^-24; every count is a number of float32 roundings):
  tables      one rounding per entry of the analysis matrix (window, already float32, times cos / sin in double) and of the
              filterbank (double formula)                                                                           1, 1
  product     launch_gemm: a k-ordered fmaf chain (gemm.hip's header) over the 400 non-zero columns of K = 416     400
              -> |dRe| <= (400 + 1) U sum_n |a_n x_n| with the reference's own sum, likewise Im
  power       re re + im im: a product rounded and an fma, or two products and a sum: a term passes at most          2
  mel sum     a 201-term fmaf chain of non-negative terms: relative                                                201
              -> dmel <= sum_f w_f dp_f + (201 + 1) U sum_f w_f (p_f + dp_f)
  log10f      C_LOG10 = 2 ulp (no accuracy table of the device library is installed beside it: the issue's stated fall-back,
              the one number here that is not derived), taken as 2 C_LOG10 U |value|; before it the floor and log10 carry dmel:
              log10(v + dmel) - log10 v above, log10 v - log10(max(v - dmel, floor)) below
  maximum     exact in any order; its error is the largest bound among the elements that can be the maximum
  clamp       max - 8.0f: one rounding; max(., .) is 1-Lipschitz: an element carries its own bound, the threshold's, or the
              larger of the two where the bounds cannot tell on which side it lies                                   1
  normalise   (. + 4) and the product by 0.25 (exact for a power of two, counted as the issue counts it)            2
  SECOND      1 + 2^-10 on every first-order term; TINY: a power below the smallest normal float32 may flush to zero
Where the reference's mel sum does not exceed the floor even with its bound added, the device value is the floor's, which
handoff_mel_tile writes as -10.0f (the device library's log10f(1e-10f) lies one ulp below it; Whisper's features of silence are
-1.5), and where the clamp threshold surely lies below -10 the output is the float32 -1.5 bit for bit (`exact`; the all-zero
signal is exact everywhere).  Elements that are surely clamped all hold the same float32 (`clamped`).

`mut` names one deliberate mistake (MISTAKES); None is the definition."""
import numpy as np

from frontend_reference import CANARY, U, bits, canary  # noqa: F401  (shared with the other kernel tests)

f32 = np.float32
SECOND = 1.0 + 2.0 ** -10
C_LOG10 = 2
TINY = 2.0 ** -126
NFFT, HOPW, BINS, PADW = 400, 160, 201, 200
BLOCK, FRAME = 256, 512                      # the separator's hop and frame: the gate's frame t spans samples [256 t, 256 t + 512)
FLOOR = float(f32(1e-10))
LOG_FLOOR = f32(-10.0)                       # what the mel tile writes at the floor
TILE = 32                                    # frames of a mel tile (MEL_TILE_FRAMES)

MISTAKES = ("symmetric_hann", "band_shift", "htk", "bf16_operands", "f16_operands", "left_edge_repeat", "right_edge_repeat",
            "last_frame_kept", "offs_plus_one", "tile_max", "signed_bits_max", "floor_after_log")


# ---- gate -> kept ranges -> concatenation -------------------------------------------------------------------------------------

def kept_ranges(gate, pad, n_out, drop=True):
    """gate [TL] bytes -> [n][2] sample ranges: maximal runs of active frames widened by pad frames, frame t spanning
    [256 t, 256 t + 512), clipped to n_out, overlapping and touching runs merged (css.py:303-312; api_ctx.hpp)"""
    if not drop:
        return np.array([[0, n_out]], np.int64)
    out, t, TL = [], 0, len(gate)
    while t < TL:
        if not gate[t]:
            t += 1
            continue
        e = t
        while e < TL and gate[e]:
            e += 1
        a, b = max(t - pad, 0) * BLOCK, min((e - 1 + pad) * BLOCK + FRAME, n_out)
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
        t = e
    return np.array(out, np.int64).reshape(-1, 2)


def concat(row, ranges, mut=None):
    """the kept samples of row (float32) behind one another"""
    ranges = np.asarray(ranges, np.int64).reshape(-1, 2)
    if len(ranges) == 0:
        return np.zeros(0, np.float32)
    x = np.concatenate([row[a:b] for a, b in ranges]).astype(np.float32)
    if mut == "offs_plus_one" and len(ranges) > 1:
        # offs[1] one too large: concatenation sample offs[1] is still looked up in region 0 (the sample behind its end), and
        # every sample of region 1 and its successors' table entry is read one sample early
        o1 = int(ranges[0, 1] - ranges[0, 0])
        n1 = int(ranges[1, 1] - ranges[1, 0])
        x[o1] = row[ranges[0, 0] + o1]
        x[o1 + 1:o1 + n1] = row[ranges[1, 0]:ranges[1, 0] + n1 - 1]
    return x


def operand(x, mut=None):
    """the concatenation reflect-padded by 200 at both ends (no edge repeat), float64 [n + 400]"""
    x = np.asarray(x, np.float64)
    left, right = x[PADW:0:-1], x[-2:-PADW - 2:-1]
    if mut == "left_edge_repeat":
        left = x[PADW - 1::-1]
    if mut == "right_edge_repeat":
        right = x[-1:-PADW - 1:-1]
    return np.concatenate([left, x, right])


# ---- tables -------------------------------------------------------------------------------------------------------------------

def hann(mut=None):
    """torch.hann_window(400): periodic, rounded to float32 once"""
    n = np.arange(NFFT)
    w = np.hanning(NFFT) if mut == "symmetric_hann" else 0.5 - 0.5 * np.cos(2.0 * np.pi * n / NFFT)
    return w.astype(np.float32).astype(np.float64)


def analysis_matrix(mut=None):
    """[402][400] float64: rows f: w_n cos(2 pi f n / 400), rows 201 + f: -w_n sin(2 pi f n / 400)"""
    f, n = np.arange(BINS)[:, None], np.arange(NFFT)[None, :]
    a = 2.0 * np.pi * ((f * n) % NFFT) / NFFT
    return np.concatenate([np.cos(a), -np.sin(a)]) * hann(mut)[None, :]


def mel_bank(n_mels, mut=None):
    """librosa.filters.mel(sr=16000, n_fft=400, n_mels): slaney scale (linear below 1 kHz, log-step ln 6.4 / 27 above) and
    slaney (area) normalisation, from the formula, float64 [n_mels][201]"""
    f_sp, min_log_hz, logstep = 200.0 / 3.0, 1000.0, np.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp
    if mut == "htk":
        hz2mel = lambda f: 2595.0 * np.log10(1.0 + f / 700.0)
        mel2hz = lambda m: 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    else:
        hz2mel = lambda f: np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-30) / min_log_hz) / logstep, f / f_sp)
        mel2hz = lambda m: np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)
    mel_f = mel2hz(np.linspace(hz2mel(np.float64(0.0)), hz2mel(np.float64(8000.0)), n_mels + 2))
    fft_f = np.linspace(0.0, 8000.0, BINS)
    w = np.zeros((n_mels, BINS))
    for i in range(n_mels):
        lower = (fft_f - mel_f[i]) / (mel_f[i + 1] - mel_f[i])
        upper = (mel_f[i + 2] - fft_f) / (mel_f[i + 2] - mel_f[i + 1])
        w[i] = np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (mel_f[i + 2] - mel_f[i]))
    if mut == "band_shift":
        w[n_mels // 2] = np.roll(w[n_mels // 2], 1)
    return w


def _bf16(a):
    """round to nearest even to bfloat16, returned as float64"""
    b = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32).astype(np.float64)


_TABLES = {}


def tables(n_mels, mut=None):
    key = (n_mels, mut if mut in ("symmetric_hann", "band_shift", "htk") else None)
    if key not in _TABLES:
        _TABLES[key] = (analysis_matrix(key[1]), mel_bank(n_mels, key[1]))
    return _TABLES[key]


# ---- the reference --------------------------------------------------------------------------------------------------------------

class Ref:
    """the intermediates: x (concatenation), op (padded), re, im, power [201][nfr], mel, raw [n_mels][nfr], mx, out; and with
    want_bound: bound (on out), exact (bool: out is the float32 -1.5 bit for bit), clamped (bool: surely at the threshold),
    e_re, e_im, e_pow, e_mel, e_raw, e_mx"""


def frames_of(n, mut=None):
    return n // HOPW + (1 if mut == "last_frame_kept" else 0) if n >= HOPW else 0


def reference(x, n_mels, mut=None, want_bound=True):
    """x: the concatenation (float32) -> Ref"""
    r = Ref()
    r.x = np.asarray(x, np.float32)
    n = len(r.x)
    nfr = frames_of(n, mut)
    r.nfr = nfr
    if nfr == 0:
        r.out = np.zeros((n_mels, 0))
        r.bound, r.exact, r.clamped = np.zeros((n_mels, 0)), np.zeros((n_mels, 0), bool), np.zeros((n_mels, 0), bool)
        return r
    A, W = tables(n_mels, mut)
    r.op = operand(r.x, mut)
    fr = np.lib.stride_tricks.sliding_window_view(r.op, NFFT)[::HOPW][:nfr].T            # [400][nfr]
    if mut == "bf16_operands":
        A, fr = _bf16(A), _bf16(fr)
    elif mut == "f16_operands":
        with np.errstate(over="ignore"):
            A, fr = A.astype(np.float32).astype(np.float16).astype(np.float64), fr.astype(np.float16).astype(np.float64)
    spec = A @ fr
    r.re, r.im = spec[:BINS], spec[BINS:]
    r.power = r.re * r.re + r.im * r.im
    r.mel = W @ r.power
    if mut == "floor_after_log":
        with np.errstate(divide="ignore"):
            r.raw = np.maximum(np.log10(r.mel), 1e-10)
    else:
        r.raw = np.log10(np.maximum(r.mel, FLOOR))
    if mut == "tile_max":
        mx = np.concatenate([np.full(min(TILE, nfr - j), r.raw[:, j:j + TILE].max()) for j in range(0, nfr, TILE)])[None, :]
    elif mut == "signed_bits_max":
        b = r.raw.astype(np.float32).view(np.int32)
        mx = r.raw.reshape(-1)[int(b.argmax())]
    else:
        mx = r.raw.max()
    r.mx = mx
    r.out = (np.maximum(r.raw, mx - 8.0) + 4.0) / 4.0
    if not want_bound:
        return r
    assert mut is None, "the bound belongs to the definition"
    s = np.abs(A) @ np.abs(fr)
    r.s_re, r.s_im, r.W = s[:BINS], s[BINS:], W
    r.bound = bound(r)
    return r


def bound(r, k_prod=NFFT + 1, k_pow=2, k_mel=BINS + 1, c_log=C_LOG10, floor_log_exact=True):
    """the bound on r.out for a float32 path that rounds k_prod times per term of the product (table included), k_pow times per
    term of the power, k_mel times per term of the mel sum (table included) and takes a log10 of c_log ulp: the device path by
    default (the module's header has the counts).  Leaves the intermediates e_re, e_im, e_pow, e_mel, e_raw, e_mx, exact and
    clamped on r."""
    r.e_re, r.e_im = SECOND * k_prod * U * r.s_re, SECOND * k_prod * U * r.s_im
    dp = 2 * np.abs(r.re) * r.e_re + r.e_re ** 2 + 2 * np.abs(r.im) * r.e_im + r.e_im ** 2
    r.e_pow = dp + SECOND * k_pow * U * (r.power + dp) + TINY
    r.e_mel = r.W @ r.e_pow + SECOND * k_mel * U * (r.W @ (r.power + r.e_pow))
    floor_sure = r.mel + r.e_mel <= FLOOR
    v = np.maximum(r.mel, FLOOR)
    prop = np.maximum(np.log10(v + r.e_mel) - r.raw, r.raw - np.log10(np.maximum(v - r.e_mel, FLOOR)))
    at_floor = 10.0 + np.log10(FLOOR) + (0.0 if floor_log_exact else 2 * c_log * U * 10.0)     # (-10.0f where the path's log10 gives that)
    r.e_raw = np.where(floor_sure, at_floor, prop + SECOND * 2 * c_log * U * (np.abs(r.raw) + prop))
    can_be_max = r.raw + r.e_raw >= (r.raw - r.e_raw).max()
    r.e_mx = float(r.e_raw[can_be_max].max())
    thr = r.mx - 8.0
    e_thr = r.e_mx + SECOND * U * (abs(thr) + r.e_mx)
    above, below = r.raw - r.e_raw > thr + e_thr, r.raw + r.e_raw < thr - e_thr
    e_c = np.where(above, r.e_raw, np.where(below, e_thr, np.maximum(r.e_raw, e_thr)))
    r.exact = floor_sure & (thr + e_thr < -10.0)
    r.clamped = below
    return e_c / 4 + SECOND * 2 * U * (np.abs(r.out) + e_c / 4)


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


# ---- the device path in float32 -------------------------------------------------------------------------------------------------

def _fma32(a, b, c):
    """fmaf on float32 arrays: the product is exact in float64, the sum rounds there once before the rounding to float32 (a
    double rounding in about one case in 2^29: a model, not the bits)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def model32(x, n_mels):
    """handoff.hip's arithmetic restated in numpy float32: float32 tables, ascending fmaf chains, fmaf(re, re, im im),
    log10 in float64 rounded once, the float32 clamp and normalisation -> float32 [n_mels][nfr]"""
    x = np.asarray(x, np.float32)
    nfr = frames_of(len(x))
    A, W = tables(n_mels)
    A32, W32 = A.astype(np.float32), W.astype(np.float32)
    fr = np.lib.stride_tricks.sliding_window_view(operand(x).astype(np.float32), NFFT)[::HOPW][:nfr].T
    acc = np.zeros((2 * BINS, nfr), np.float32)
    for k in range(NFFT):
        acc = _fma32(A32[:, k:k + 1], fr[k:k + 1, :], acc)
    re, im = acc[:BINS], acc[BINS:]
    p = _fma32(re, re, im * im)
    mel = np.zeros((n_mels, nfr), np.float32)
    for f in range(BINS):
        mel = _fma32(W32[:, f:f + 1], p[f:f + 1, :], mel)
    raw = np.log10(np.maximum(mel, f32(1e-10)).astype(np.float64)).astype(np.float32)
    return (np.maximum(raw, raw.max() - f32(8.0)) + f32(4.0)) * f32(0.25)


# ---- signals --------------------------------------------------------------------------------------------------------------------

SIGNALS = ("noise", "tones", "chirp", "quiet_chirp", "quiet_chirp_3e-2", "square", "zeros", "impulses")


def _chirp(n):
    """50 Hz -> 7.9 kHz, linear in time; the amplitude ramps geometrically from 1e-4 to 1"""
    t = np.arange(n) / 16000.0
    T = n / 16000.0
    phase = 2.0 * np.pi * (50.0 * t + 0.5 * (7900.0 - 50.0) / T * t * t)
    return 10.0 ** (-4.0 + 4.0 * t / T) * np.sin(phase)


def _zero_stretches(x):
    """exact zeros over 0.25 s in every second: whole frames of silence between the sounding ones"""
    x = x.copy()
    for s in range(0, len(x), 16000):
        x[s + 6000:s + 10000] = 0
    return x


def impulse_positions(ranges):
    """waveform samples that are concatenation samples 0, 1, 199, 200, 201, n_act - 2, n_act - 1, and the last two and the first
    two of every region (just before and just after each seam)"""
    ranges = np.asarray(ranges, np.int64).reshape(-1, 2)
    lens = ranges[:, 1] - ranges[:, 0]
    offs = np.concatenate([[0], np.cumsum(lens)])
    n_act = int(offs[-1])
    cpos = {0, 1, 199, 200, 201, n_act - 2, n_act - 1}
    for o in offs[1:-1]:
        cpos |= {int(o) - 2, int(o) - 1, int(o), int(o) + 1}
    pos = []
    for c in sorted(p for p in cpos if 0 <= p < n_act):
        r = int(np.searchsorted(offs, c, side="right")) - 1
        pos.append(int(ranges[r, 0] + c - offs[r]))
    return pos


def signal(kind, n, ranges=None, seed=0):
    """float32 [n]; `impulses` is laid out for the kept ranges it will be read through"""
    t = np.arange(n) / 16000.0
    if kind == "noise":
        x = np.random.default_rng(1000 + seed).uniform(-0.5, 0.5, n)
    elif kind == "tones":
        x = 0.5 * np.sin(2 * np.pi * 1000.0 * t) + 0.5e-3 * np.sin(2 * np.pi * 6100.0 * t)
    elif kind == "chirp":
        x = _chirp(n)
    elif kind == "quiet_chirp":
        x = _zero_stretches(3e-3 * _chirp(n))
    elif kind == "quiet_chirp_3e-2":
        x = _zero_stretches(3e-2 * _chirp(n))
    elif kind == "square":
        x = np.where((np.arange(n) // 23) % 2 == 0, 1.0, -1.0)
    elif kind == "zeros":
        x = np.zeros(n)
    elif kind == "impulses":
        x = np.zeros(n)
        # (signs and sizes differ, so that no two impulses can stand in for one another)
        for i, p in enumerate(impulse_positions(ranges)):
            x[p] = (1.0 if i % 2 == 0 else -1.0) * (1.0 + 0.125 * (i % 5))
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


# ---- gates and cases --------------------------------------------------------------------------------------------------------------

def gate_of(TL, runs):
    """runs: (first frame, kept blocks) at pad 0: frames [a, a + blocks - 1) keep blocks a .. a + blocks - 1"""
    g = np.zeros(TL, np.uint8)
    for a, blocks in runs:
        assert blocks >= 2 and a + blocks - 1 <= TL
        g[a:a + blocks - 1] = 1
    return g


def _split(blocks, parts):
    base = [blocks // parts] * parts
    base[0] += blocks - sum(base)
    return base


def cases(TL):
    """the list of tests/test_hip_handoff_values.py for a pass of TL frames (TL >= 360): dicts with name, n_mels, pad, drop, ld_extra
    (wav_ld = n_out + ld_extra), kinds [3] and runs [3] (per stream row; None with drop False).  Every gate meets the impulses
    (row i mod 3) and two of the other signals, which rotate; the block counts are the issue's: 2 (3 frames), 19 / 20 / 21 (30,
    32, 33 frames), 22, 40 / 41 (two tiles and one frame more); 20, 22 and 40 kept blocks read the right-hand reflection."""
    assert TL >= 360
    others = [k for k in SIGNALS if k != "impulses"]
    out = []

    def add(name, runs3, pad=0, drop=True, n_mels=None, kinds=None):
        i = len(out)
        if kinds is None:
            kinds = [others[(2 * i) % len(others)], others[(2 * i + 1) % len(others)]]
            kinds.insert(i % 3, "impulses")
        out.append(dict(name=name, n_mels=n_mels or (80, 128)[i % 2], pad=pad, drop=drop, ld_extra=i % 2, kinds=kinds, runs=runs3, seed=i))

    for blocks in (2, 19, 20, 21, 22, 40, 41):
        add(f"{blocks}_blocks", [[(60 + 7 * row, blocks)] for row in range(3)])
    add("4_blocks_2_runs", [[(30 + row, 2), (250 + 5 * row, 2)] for row in range(3)])
    for blocks in (19, 20, 21, 22, 40, 41):
        b1, b2 = _split(blocks, 2)
        add(f"{blocks}_blocks_2_runs", [[(20 + row, b1), (300 - 4 * row, b2)] for row in range(3)])
    for blocks in (22, 41):
        b1, b2, b3 = _split(blocks, 3)
        add(f"{blocks}_blocks_3_runs", [[(10 + row, b1), (150 + 3 * row, b2), (320 - 2 * row, b3)] for row in range(3)])
    add("pad_8", [[(40 + row, 3), (70 + row, 2), (200 + 9 * row, 6)] for row in range(3)], pad=8)
    add("whole_80", None, pad=8, drop=False, n_mels=80, kinds=["impulses", "chirp", "tones"])
    add("whole_128", None, pad=8, drop=False, n_mels=128, kinds=["noise", "impulses", "quiet_chirp"])
    add("whole_80_b", None, pad=8, drop=False, n_mels=80, kinds=["quiet_chirp_3e-2", "square", "noise"])
    add("whole_128_b", None, pad=8, drop=False, n_mels=128, kinds=["zeros", "chirp", "quiet_chirp_3e-2"])
    return out


def case_row(c, row, TL, n_out):
    """(gate [TL], ranges, waveform row [n_out]) of one stream row of a case"""
    gate = np.ones(TL, np.uint8) if c["runs"] is None else gate_of(TL, c["runs"][row])
    ranges = kept_ranges(gate, c["pad"], n_out, c["drop"])
    return gate, ranges, signal(c["kinds"][row], n_out, ranges, seed=c["seed"] * 3 + row)


_CASE_REFS = {}


def case_reference(c, row, TL, n_out):
    """(gate, ranges, waveform row, concatenation, Ref) of one stream row of a case, computed once per process and left unchanged"""
    key = (c["name"], row, TL, n_out)
    if key not in _CASE_REFS:
        gate, ranges, w = case_row(c, row, TL, n_out)
        x = concat(w, ranges)
        _CASE_REFS[key] = (gate, ranges, w, x, reference(x, c["n_mels"]))
    return _CASE_REFS[key]


# The cases (name, stream row) that catch each mistake; tests/test_handoff_reference.py shows every deviation above the bound.
# The first entry is where the deviation is also large beside COND; the float16 operands' second entry is the two-tone signal,
# where rounding both operands to 11 bits over 400 random terms (2^-11 sqrt 2 / sqrt 400 of sum |a x|) is of the order of the
# worst-case chain bound 401 U itself: caught, by a factor of three, and no more than that.
COND = 2e-4          # an element is well conditioned where its bound is at most this (the old tests' rms bar; a tenth of their max bar)
CAUGHT_BY = {
    "symmetric_hann": [("whole_128", 0), ("whole_80", 2)],
    "band_shift": [("whole_128", 0)],
    "htk": [("whole_128", 0)],
    "bf16_operands": [("whole_80", 2)],
    "f16_operands": [("whole_80", 1), ("whole_80", 2)],
    "left_edge_repeat": [("19_blocks", 1), ("whole_80", 0)],
    "right_edge_repeat": [("20_blocks", 2), ("22_blocks", 1), ("40_blocks", 2)],
    "last_frame_kept": [("2_blocks", 0)],
    "offs_plus_one": [("20_blocks_2_runs", 0), ("41_blocks_3_runs", 0), ("22_blocks_2_runs", 1)],
    "tile_max": [("whole_80_b", 0), ("whole_128_b", 2)],
    "signed_bits_max": [("whole_80_b", 0), ("whole_128_b", 2)],
    "floor_after_log": [("whole_128", 2), ("whole_80_b", 0)],
}
# kept-sample counts with n mod 160 >= 40 never read the right-hand reflection: the mistake there must NOT show
RIGHT_REFLECTION_UNREAD = [("19_blocks", 1), ("21_blocks", 0), ("41_blocks", 0)]


def oracle_tolerance(ref):
    """what oracle/css_oracle.py::whisper_log_mel may lie from this reference: it rounds the windowed samples to float32 (1) before
    its float64 transform, the power to float32 (1), holds the filterbank in float32 (1) and sums 201 non-negative float32 terms
    in an order of numpy's choosing (201: relative), takes a float32 log10 (4 ulp at most, as numpy states for its float32 loops),
    the float32 maximum, and rounds the sum with 4 and the quotient by 4"""
    exact, clamped = ref.exact, ref.clamped
    tol = bound(ref, k_prod=1, k_pow=1, k_mel=BINS + 1, c_log=4, floor_log_exact=False)
    ref.bound = bound(ref)
    assert np.array_equal(exact, ref.exact) and np.array_equal(clamped, ref.clamped)
    return tol
