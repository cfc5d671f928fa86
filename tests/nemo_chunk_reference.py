"""The exact numpy model of NeMo chunks out of a stream's frame history (include/css_mi355_nemo_chunk.h; csrc/nemo_stream.hip
nemo_chunk_kernel and the ring write of nemo_mel_multi_kernel), its named mistakes as switches, the bound of its statistics against
numpy's float64 two-pass values, and the shapes and values of tests/test_hip_nemo_chunk_kernels.py.  No GPU, no library:
tests/test_nemo_chunk_reference.py checks this file on the CPU.

A chunk of the raw frames raw [n_mels][n] of a span, padded to `width` columns:
  RAW           column c < n is raw[m][c]
  PER_FEATURE   column c < n is (raw[m][c] - mean[m]) / (std[m] + 1e-5f) in float32, each step rounded once
  columns n ..  pad_value, never normalised;  float16: the float32 value rounded to nearest-even
The statistics are float64 sums in ONE order, so this model is exact, not a bound: lane l of 64 adds frames l, l + 64, ... in
increasing order, then x[l] += x[l + s] for s = 32, 16, .. 1; mean = x[0] / n; d = (double)raw - mean, d * d and the addition
rounded apart, in the same order; std = n > 1 ? sqrt(x[0] / (n - 1)) : 0; mean and std rounded to float32 once each.

The ring after a round that completes n_new frames for a speaker whose count was J0: frame J0 + j goes to slot (J0 + j) mod hist
iff j >= n_new - hist (frames j and j + hist share a slot: in one launch only the last `hist` may be written).

The derived bound of mean and std against numpy's float64 two-pass values `ref` (stats_bound): 2^-23 |ref| + n 2^-50 max|raw|.  The
first term is one float32 ulp: the half-ulp of the final rounding, doubled to cover the double rounding float64 -> float32.  The
second is float64 accumulation over n <= 3000 terms, whatever the order: a sum of n terms of magnitude at most a is off by at most
n 2^-53 n a, that is n 2^-53 a after the division by n; the deviations d = raw - mean are at most 2 max|raw| and carry both
means' errors, which the factor 8 between 2^-53 and 2^-50 leaves room for.

`mut` names one deliberate mistake (MISTAKES); None is the definition."""
import numpy as np

from frontend_reference import CANARY, bits, canary  # noqa: F401  (shared with the other kernel tests)

f32 = np.float32
EPS = f32(1e-5)
LANES = 64
MAX_WIDTH = 3000
TABLE = 32
SILENCE = f32(np.log(np.float64(f32(2.0 ** -24))))   # ln(0 + 2^-24) as a float32: every band of a frame of digital silence

MISTAKES = ("biased", "eps_inside", "stats_over_width", "pad_normalised", "n1_nan", "float32_stats", "slot_plus_one", "oldest_last")


# ---- the statistics ---------------------------------------------------------------------------------------------------------------

def ordered_sum(x):
    """x [rows][n] float64 -> [rows]: lane l adds elements l, l + 64, ... in increasing order, then the tree x[l] += x[l + s]"""
    x = np.asarray(x, np.float64)
    lanes = np.zeros((x.shape[0], LANES))
    for c in range(x.shape[1]):
        lanes[:, c % LANES] = lanes[:, c % LANES] + x[:, c]
    s = LANES // 2
    while s >= 1:
        for l in range(s):
            lanes[:, l] = lanes[:, l] + lanes[:, l + s]
        s //= 2
    return lanes[:, 0].copy()


def stats(raw, mut=None):
    """raw [n_mels][n] float32 -> (mean, std) float32 [n_mels]"""
    raw = np.asarray(raw, np.float32)
    n = raw.shape[1]
    if mut == "float32_stats":
        mean = (raw.sum(axis=1, dtype=np.float32) / f32(n)).astype(np.float32)
        d = raw - mean[:, None]
        std = np.sqrt((d * d).sum(axis=1, dtype=np.float32) / f32(max(n - 1, 1))).astype(np.float32)
        return mean, std if n > 1 else np.zeros_like(std)
    x = raw.astype(np.float64)
    mean = ordered_sum(x) / np.float64(n)
    d = x - mean[:, None]
    ss = ordered_sum(d * d)
    if n == 1:
        std = np.full(raw.shape[0], np.nan) if mut == "n1_nan" else np.zeros(raw.shape[0])
    elif mut == "biased":
        std = np.sqrt(ss / np.float64(n))
    elif mut == "eps_inside":
        std = np.sqrt(ss / np.float64(n - 1) + 1e-5) - 1e-5     # (so that std + eps below is sqrt(var + eps))
    else:
        std = np.sqrt(ss / np.float64(n - 1))
    return mean.astype(np.float32), std.astype(np.float32)


def reference_stats(raw):
    """numpy's float64 two-pass values: (mean, std) float64 [n_mels]"""
    x = np.asarray(raw, np.float32).astype(np.float64)
    n = x.shape[1]
    mean = x.mean(axis=1)
    std = np.sqrt(((x - mean[:, None]) ** 2).sum(axis=1) / (n - 1)) if n > 1 else np.zeros(x.shape[0])
    return mean, std


def stats_bound(ref, n, max_abs):
    return 2.0 ** -23 * np.abs(ref) + n * 2.0 ** -50 * max_abs


# ---- a chunk ----------------------------------------------------------------------------------------------------------------------

def chunk(raw, width=None, normalize=True, dtype=np.float32, pad_value=0.0, mut=None):
    """raw [n_mels][n] float32 -> (out [n_mels][width] of dtype, mean, std); mean and std are None for a RAW chunk"""
    raw = np.asarray(raw, np.float32)
    n = raw.shape[1]
    width = n if width is None else int(width)
    assert 1 <= n <= width <= MAX_WIDTH
    out = np.full((raw.shape[0], width), f32(pad_value), np.float32)
    if not normalize:
        out[:, :n] = raw
        return out.astype(dtype), None, None
    src = out.copy() if mut == "stats_over_width" else raw
    if mut == "stats_over_width":
        src[:, :n] = raw
    mean, std = stats(src, mut)
    with np.errstate(invalid="ignore"):
        if mut == "pad_normalised":
            out[:, :n] = raw
            out = (out - mean[:, None]) / (std + EPS)[:, None]
        else:
            out[:, :n] = (raw - mean[:, None]) / (std + EPS)[:, None]
    return out.astype(dtype), mean, std


# ---- the ring ---------------------------------------------------------------------------------------------------------------------

def ring_after_round(ring, J0, frames, mut=None):
    """ring [n_mels][hist] (a copy is written), J0 frames so far, frames [n_mels][n_new] of the round -> the ring after it"""
    ring = np.array(ring, np.float32)
    hist, n_new = ring.shape[1], frames.shape[1]
    if mut == "oldest_last":       # every frame of the round is written, the oldest ones last: they win their slots
        order = list(range(n_new))[::-1]
    else:
        order = [j for j in range(n_new) if j >= n_new - hist]
    for j in order:
        ring[:, (J0 + j + (1 if mut == "slot_plus_one" else 0)) % hist] = frames[:, j]
    return ring


def span(ring, first, n):
    """frames [first, first + n) out of a ring [n_mels][hist] that holds them"""
    return ring[:, (first + np.arange(n)) % ring.shape[1]]


def ring_holding(frames, hist, J, fill=None):
    """the ring [n_mels][hist] that holds frames [max(J - hist, 0), J) of frames [n_mels][>= J]; other slots: canaries (or fill)"""
    ring = np.tile(canary(hist) if fill is None else np.full(hist, fill, np.float32), (frames.shape[0], 1))
    for j in range(max(J - hist, 0), J):
        ring[:, j % hist] = frames[:, j]
    return ring


# ---- values and shapes ------------------------------------------------------------------------------------------------------------

def frames(n_mels, n, seed=0, kind="logmel"):
    """float32 [n_mels][n] of plausible raw NeMo frames: band-dependent level and spread between ln(2^-24) and about 3; `silence`:
    every value ln(2^-24); `mixed`: stretches of silence in every band, one band silent throughout"""
    r = np.random.default_rng(9100 + seed)
    if kind == "silence":
        return np.full((n_mels, n), SILENCE, np.float32)
    level = r.uniform(-12.0, -2.0, (n_mels, 1))
    x = level + r.uniform(0.2, 3.0, (n_mels, 1)) * r.standard_normal((n_mels, n))
    x = np.maximum(x, np.float64(SILENCE)).astype(np.float32)
    if kind == "mixed":
        x[:, n // 3:n // 2] = SILENCE
        x[n_mels // 2] = SILENCE
    return x


N_FRAMES = (1, 2, 63, 64, 65, 127, 129, 255, 256, 257, 3000)
HISTS = (32, 33, 3000)


def widths_of(n):
    return sorted({n, min(n + 1, MAX_WIDTH), MAX_WIDTH})


def cases():
    """(name, n_mels, n, kind, seed): the spans the CPU tests hold the model to"""
    out = []
    for i, n in enumerate(N_FRAMES):
        out.append((f"n{n}", 80 if i % 2 == 0 else 128, n, "logmel", i))
    out += [("silence-1", 80, 1, "silence", 0), ("silence-200", 80, 200, "silence", 0), ("mixed-300", 128, 300, "mixed", 3)]
    return out
