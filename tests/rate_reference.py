"""Float64 reference of the rate kernels (csrc/resample.hip), written from the definition in DESIGN.md 7b and held to
scipy.signal.resample_poly by tests/test_rate_reference.py; shared by that file (CPU) and tests/test_hip_rate_kernels.py (GPU).

    half = 10 max(up, down), L = 2 half + 1, h = up firwin(L, 1 / max(up, down), window=("kaiser", 5.0))
    y[m] = sum_i x[i] h[half + m down - i up]   over 0 <= half + m down - i up <= 2 half

A job, as the kernels see it: x is zero everywhere except [N0 - H, N0) = hist and [N0, N0 + n) = piece (int16 samples count as
q 2^-15), the outputs are [m0, m0 + n_m).  A whole recording is the job H = 0, N0 = 0, m0 = 0.  Arrays here are channel-major:
piece [C, n], hist [C, H], outputs [C, n_m].

The bound is elementwise: P 2^-24 sum_i |x[i]| |h[...]|, the rounding bound of a length-P float32 fmaf chain from +0 (every step
rounds a partial sum whose magnitude the sum of magnitudes bounds; the products are exact inside the fmaf).  It is 0 where the
span is silent: silence must come out as exactly +0.0f.

`chain` is the same sum the way the kernels index it (i_hi by floor, a phase row of P taps with a leading zero where a phase has
P - 1); MISTAKES are named wrong variants of it, PCM_MISTAKES of the PCM16 lines.  Nothing here needs a GPU."""
import collections

import numpy as np

CANARY = 0x7FC0BEEF          # a quiet NaN with a payload
CANARY16 = 0x5A5A            # 23130: no planted PCM16 position encodes to it (those give 0, +-16384, +-32767, -32768 and neighbours)
RS_TILE, SO_TILE = 256, 1024

IN_RATIOS = ((1, 3), (160, 441), (1, 2), (2, 3), (320, 441), (2, 1), (1, 6))
OUT_RATIOS = ((3, 1), (441, 160), (3, 2), (441, 320), (6, 1))
EDGE_RATIO = (819, 818)
RATIOS = IN_RATIOS + OUT_RATIOS + (EDGE_RATIO,)
STREAM_INGEST_RATIOS = ((1, 3), (160, 441), (320, 441), (2, 1), (1, 6))
PIECES = (1, 7, 8, 9, 63, 257)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def canary(shape):
    return np.full(shape, CANARY, np.uint32).view(np.float32)


def canary16(shape):
    return np.full(shape, CANARY16, np.int16)


def geometry(up, down):
    """(half, L, P): the filter's half length, its taps, and the taps per output sample ceil(L / up)"""
    half = 10 * max(up, down)
    L = 2 * half + 1
    return half, L, -(-L // up)


def history_len(up, down):
    """the carried inputs of a stream, as css_stream_set_rate sizes them: ceil(2 half / up) + 1"""
    half, _, _ = geometry(up, down)
    return (2 * half + up - 1) // up + 1


def count(up, down, n_in, finished=True):
    """outputs of a recording of n_in inputs (finished), or computable after n_in inputs of an open stream"""
    half, _, _ = geometry(up, down)
    num = n_in * up - (0 if finished else half)
    return 0 if num <= 0 else -(-num // down)


def n_in_for(up, down, n_out):
    """the smallest n_in whose recording has at least n_out outputs"""
    n = (n_out - 1) * down // up + 1
    assert count(up, down, n) >= n_out and count(up, down, n - 1) < n_out
    return n


def taps64(up, down):
    """scipy's default resample_poly filter in float64"""
    from scipy.signal import firwin
    mx = max(up, down)
    return up * firwin(20 * mx + 1, 1.0 / mx, window=("kaiser", 5.0))


_TAPS32 = {}


def taps32(up, down):
    """the library's float32 taps (css_resample_taps: host code, no GPU)"""
    if (up, down) not in _TAPS32:
        from conftest import pkg
        _TAPS32[(up, down)] = pkg("_lib").resample_taps(up, down).copy()
    return _TAPS32[(up, down)]


def values(a):
    """samples as the kernels read them, in float64: int16 q -> q 2^-15"""
    a = np.asarray(a)
    return a.astype(np.float64) / 32768.0 if a.dtype == np.int16 else a.astype(np.float64)


def _line(piece, hist, N0):
    """[hist | piece] as float64 [C, H + n] and the input index of its first element"""
    piece = np.atleast_2d(values(piece))
    if hist is None or np.size(hist) == 0:
        return piece, N0
    hist = np.atleast_2d(np.asarray(hist, np.float64))
    return np.concatenate([hist, piece], axis=1), N0 - hist.shape[1]


def _gather(line, first, i):
    """x[i] of the line whose element 0 is input `first`; zero outside"""
    if line.shape[1] == 0:
        return np.zeros((line.shape[0],) + i.shape)
    s = i - first
    ok = (s >= 0) & (s < line.shape[1])
    return np.where(ok[None], line[:, np.clip(s, 0, line.shape[1] - 1)], 0.0)


def reference(piece, hist, N0, m0, n_m, up, down, taps=None):
    """(y, bound), float64 [C, n_m]: the definition and its elementwise rounding bound.  The inputs of output m are found from the
    definition's own condition 0 <= k <= 2 half: i from ceil((m down - half) / up) on, at most P of them."""
    half, L, P = geometry(up, down)
    h = (taps32(up, down) if taps is None else np.asarray(taps)).astype(np.float64)
    assert h.size == L
    line, first = _line(piece, hist, N0)
    m = np.arange(m0, m0 + n_m, dtype=np.int64)[:, None]
    i = -((half - m * down) // up) + np.arange(P, dtype=np.int64)[None, :]      # ceil((m down - half) / up) + j
    k = half + m * down - i * up
    assert (k <= 2 * half).all()
    w = np.where(k >= 0, h[np.clip(k, 0, 2 * half)], 0.0)
    x = _gather(line, first, i)
    return np.einsum("mp,cmp->cm", w, x), P * 2.0 ** -24 * np.einsum("mp,cmp->cm", np.abs(w), np.abs(x))


def recording(x, up, down, taps=None):
    """(y, bound) of a whole recording x [C, n]"""
    x = np.atleast_2d(np.asarray(x))
    return reference(x, None, 0, 0, count(up, down, x.shape[1]), up, down, taps)


def next_history(hist, piece):
    """the last H elements of [hist | piece], float32 [C, H] (int16 pieces as q 2^-15, exact in float32)"""
    hist = np.atleast_2d(np.asarray(hist, np.float32))
    both = np.concatenate([hist, np.atleast_2d(values(piece)).astype(np.float32)], axis=1)
    return both[:, both.shape[1] - hist.shape[1]:]


def pcm16(y, gain=1.0):
    """The two PCM16 lines of css_mi355_stream_out.h: v = float32(y * gain), q = clamp(rint(double(v) * 32767)).  Returns (int16,
    the number of samples the clamp changed)."""
    v = np.asarray(y, np.float32) * np.float32(gain)
    r = np.rint(v.astype(np.float64) * 32767.0)
    return np.clip(r, -32768.0, 32767.0).astype(np.int16), int(np.count_nonzero((r < -32768.0) | (r > 32767.0)))


# ---- the sum as the kernels index it, and named mistakes --------------------------------------------------------------------------

def phase_table(up, down, taps=None):
    """[up, P | 1]: row ph holds, for j < P, the tap of input i_hi - P + 1 + j: h[ph + (P - 1 - j) up], 0 past the last tap"""
    half, L, P = geometry(up, down)
    h = (taps32(up, down) if taps is None else np.asarray(taps)).astype(np.float64)
    k = np.arange(up)[:, None] + (P - 1 - np.arange(P | 1))[None, :] * up
    return np.where((np.arange(P | 1)[None, :] < P) & (k < L) & (k >= 0), h[np.clip(k, 0, L - 1)], 0.0)


def chain(piece, hist, N0, m0, n_m, up, down, *, model32=False, mistake=None, tile=RS_TILE):
    """The sum over the P inputs i_hi - P + 1 .. i_hi, i_hi = floor((m down + half) / up), taps of phase (m down + half) mod up.
    model32: each step float32(float64(acc) + float64(x) float64(h)) in ascending i (the float32 fmaf chain); mistake: a name
    of MISTAKES."""
    half, L, P = geometry(up, down)
    tab = phase_table(up, down)
    P_ld = tab.shape[1]
    line, first = _line(piece, hist, N0)
    scale = 1.0
    if mistake == "int16_over_32767" and np.asarray(piece).dtype == np.int16:
        line, first = _line(np.atleast_2d(np.asarray(piece)).astype(np.float64) / 32767.0, hist, N0)
    if mistake == "taps_without_up":
        scale = 1.0 / up
    m = np.arange(m0, m0 + n_m, dtype=np.int64)
    num = m * down + half
    i_hi, ph = num // up, num % up
    if mistake == "i_hi_by_ceiling":
        i_hi = -((-num) // up)
    if mistake == "phase_shifted":
        ph = (ph + 1) % up
    j = np.arange(P, dtype=np.int64)[None, :]
    i = (i_hi[:, None] - (P - 1)) + j
    if mistake == "pitch_P_on_the_read_side":
        flat = ph[:, None] * P + j
        w = tab.reshape(-1)[flat]
    else:
        w = tab[ph[:, None], j]
    if mistake == "phase_reversed":
        w = w[:, ::-1]
    if mistake == "no_leading_zero":      # a phase of P - 1 taps keeps them at j = 0 .. P - 2: every tap meets the input before its own
        short = (ph + (P - 1) * up >= L)[:, None]
        w = np.where(short, np.concatenate([w[:, 1:], np.zeros((w.shape[0], 1))], axis=1), w)
    x = _gather(line, first, i)
    if mistake == "history_one_late" and hist is not None and np.size(hist):
        late = _gather(line, first - 1, i)              # element s + 1 of the line where s was meant
        x = np.where((i < N0)[None], late, x)
    if mistake in ("first_input_repeated", "last_input_repeated") and (hist is None or not np.size(hist)) and line.shape[1]:
        if mistake == "first_input_repeated":
            x = np.where((i < N0)[None], line[:, :1, None], x)
        else:
            x = np.where((i >= N0 + line.shape[1])[None], line[:, -1:, None], x)
    t = m - m0
    tile_first = (((m0 + t // tile * tile) * down + half) // up - (P - 1))[:, None]      # the first input of the output's tile
    if mistake == "tile_edge_short":      # the last output of a tile: the span is one input short
        last = ((t % tile == tile - 1) | (t == n_m - 1))[:, None]
        x = np.where((last & (j == P - 1))[None], 0.0, x)
    if mistake == "swizzle_one_sided":    # staged positions from 32 on: the reader finds the input before
        x = np.where((i - tile_first >= 32)[None], _gather(line, first, i - 1), x)
    w = w * scale
    if not model32:
        return np.einsum("mp,cmp->cm", w, x)
    acc = np.zeros(x.shape[:2], np.float32)
    w32, x32 = w.astype(np.float32), x.astype(np.float32)
    for jj in range(P):
        acc = (acc.astype(np.float64) + x32[:, :, jj].astype(np.float64) * w32[None, :, jj].astype(np.float64)).astype(np.float32)
    return acc


MISTAKES = ("phase_shifted", "no_leading_zero", "phase_reversed", "i_hi_by_ceiling", "history_one_late", "first_input_repeated",
            "last_input_repeated", "int16_over_32767", "taps_without_up", "tile_edge_short", "swizzle_one_sided",
            "pitch_P_on_the_read_side")


def _pcm_half_away(y, gain):
    v = (np.asarray(y, np.float32) * np.float32(gain)).astype(np.float64) * 32767.0
    r = np.sign(v) * np.floor(np.abs(v) + 0.5)
    return np.clip(r, -32768.0, 32767.0).astype(np.int16), int(np.count_nonzero((r < -32768.0) | (r > 32767.0)))


def _pcm_half_up(y, gain):
    r = np.floor((np.asarray(y, np.float32) * np.float32(gain)).astype(np.float64) * 32767.0 + 0.5)
    return np.clip(r, -32768.0, 32767.0).astype(np.int16), int(np.count_nonzero((r < -32768.0) | (r > 32767.0)))


def _pcm_truncate(y, gain):
    r = np.trunc((np.asarray(y, np.float32) * np.float32(gain)).astype(np.float64) * 32767.0)
    return np.clip(r, -32768.0, 32767.0).astype(np.int16), int(np.count_nonzero((r < -32768.0) | (r > 32767.0)))


def _pcm_32768(y, gain):
    r = np.rint((np.asarray(y, np.float32) * np.float32(gain)).astype(np.float64) * 32768.0)
    return np.clip(r, -32768.0, 32767.0).astype(np.int16), int(np.count_nonzero((r < -32768.0) | (r > 32767.0)))


def _pcm_gain64(y, gain):
    r = np.rint(np.asarray(y, np.float32).astype(np.float64) * float(np.float32(gain)) * 32767.0)
    return np.clip(r, -32768.0, 32767.0).astype(np.int16), int(np.count_nonzero((r < -32768.0) | (r > 32767.0)))


def _pcm_clip_counts_full_scale(y, gain):
    q, _ = pcm16(y, gain)
    return q, int(np.count_nonzero(np.abs(q.astype(np.int32)) >= 32767))


# Rounding half away from zero is NOT in the table of mistakes, because no float32 sample tells it from rint: float32 v times
# 32767 is exact in float64, and it is k + 1/2 only for v = odd / 2 (32767 is odd and v is dyadic), in range only for v = +-0.5,
# where both rules give +-16384 (16384 is even).  tests/test_rate_reference.py proves the equality on the planted ties and on the
# samples; rounding half UP (floor(v + 0.5)) is the neighbouring mistake a sample can show: -16383.5 -> -16383.
PCM_SAME_AS_RINT = {"round_half_away": _pcm_half_away}
PCM_MISTAKES = {"round_half_up": _pcm_half_up, "truncation": _pcm_truncate, "times_32768": _pcm_32768,
                "gain_in_float64": _pcm_gain64, "clip_counts_full_scale": _pcm_clip_counts_full_scale}


def pcm_planted():
    """float32 samples every PCM16 test plants: the in-range ties of y * 32767 (+-0.5 -> +-16383.5 -> +-16384 by ties-to-even),
    +-1.0, the float32 neighbours of 32767.5 / 32767 on both sides, and values beyond +-1.0001"""
    edge = np.float32(32767.5 / 32767.0)
    near = [np.nextafter(edge, np.float32(0)), edge, np.nextafter(edge, np.float32(2))]
    v = [0.5, -0.5, 1.0, -1.0] + near + [-a for a in near] + [1.0002, -1.0002, 1.5, -3.0, 0.0]
    return np.array(v, np.float32)


PCM_CASES = (("unity gain", 1.0), ("gain 0.7", 0.7), ("gain 1.9", 1.9))


def pcm_samples(gain, seed=0):
    """uniform samples in [-1.1, 1.1) with pcm_planted() in front: 8192 in all (one sample in about a thousand sits close enough
    to a rounding boundary to show a gain applied without the float32 rounding)"""
    rs = np.random.RandomState(1000 + seed)
    return np.concatenate([pcm_planted(), rs.uniform(-1.1, 1.1, 8192 - pcm_planted().size).astype(np.float32)])


# ---- cases ------------------------------------------------------------------------------------------------------------------------

Case = collections.namedtuple("Case", "name up down C dtype n_in H N0 m0 n_m seed")
# A case is a job on data made by case_data: H = 0, N0 = 0, m0 = 0, n_m = count(n_in) is a whole recording (css_resample_host);
# a job with history is cut out of the recording case_data makes: hist = its inputs [N0 - H, N0), piece = [N0, N0 + n_in).


def samples(C, n, dtype, seed):
    """[C, n]: float32 uniform in [-1, 1), or the full int16 range with -32768 and 32767 planted at both ends of every channel"""
    rs = np.random.RandomState(seed)
    if np.dtype(dtype) == np.int16:
        x = rs.randint(-32768, 32768, (C, n)).astype(np.int16)
        if n:
            x[0::2, 0], x[1::2, 0] = -32768, 32767
            x[0::2, -1], x[1::2, -1] = (32767, -32768) if n > 1 else (-32768, 32767)
        return x
    return rs.uniform(-1.0, 1.0, (C, n)).astype(np.float32)


def out_lengths(up, down):
    """output counts at which the kernels can go wrong: 1, 2, P - 1, P, P + 1, both tiles at -1, 0, +1, two tiles + 1"""
    _, _, P = geometry(up, down)
    want = [1, 2, P - 1, P, P + 1] + [t + d for t in (RS_TILE, SO_TILE) for d in (-1, 0, 1)] + [2 * RS_TILE + 1, 2 * SO_TILE + 1]
    return sorted(set(want))


def in_lengths(up, down):
    """the smallest n_in reaching each count of out_lengths (a ratio above 1 reaches some counts only from above), and an n_in
    shorter than P"""
    _, _, P = geometry(up, down)
    return sorted(set([n_in_for(up, down, m) for m in out_lengths(up, down)] + [max(1, P // 2)]))


def stream_jobs(up, down, n_in, pieces=PIECES, H=None):
    """A recording of n_in inputs as a stream takes it: pieces of the given sizes, then the rest, then the flush.  Each job is
    (N0, n, m0, n_m, H, flush): the piece is inputs [N0, N0 + n), the history the H inputs before N0 (zeros before the
    recording), the outputs those that become computable with the piece; the flush has no piece and completes the count."""
    H = history_len(up, down) if H is None else H
    jobs, N0, m0 = [], 0, 0
    for k in list(pieces) + [n_in]:
        k = min(k, n_in - N0)
        if k <= 0:
            break
        m1 = count(up, down, N0 + k, finished=False)
        jobs.append((N0, k, m0, m1 - m0, H, False))
        N0, m0 = N0 + k, m1
    jobs.append((n_in, 0, m0, count(up, down, n_in) - m0, H, True))
    return jobs


LARGE_LDS = (((160, 441), 16), ((1, 6), 16), ((1, 2), 64), ((819, 818), 1), ((819, 818), 7))


def lds_bytes(up, down, C):
    """dynamic LDS of resample_kernel and the two ingest kernels: the taps [up][P | 1] and C rows of the padded span, in floats"""
    _, _, P = geometry(up, down)
    span = (RS_TILE * down + up - 1) // up + P + 1
    return 4 * (up * (P | 1) + C * (span - 1 + ((span - 1) >> 5) + 1))


def job_recording_len(up, down):
    """inputs of the recording the job cases cut: its last piece alone spans more than two tiles of outputs"""
    return n_in_for(up, down, 2 * RS_TILE + 1) + sum(PIECES) + 55


def cases():
    """The cases tests/test_rate_reference.py proves the bound and the mistakes on, and tests/test_hip_rate_kernels.py runs through
    css_resample_host (the recordings) and the stream ingest kernel (the jobs)."""
    out = []
    for r, (up, down) in enumerate(RATIOS):       # recordings of 8 channels (a test of C channels takes the first C), both types
        for k, n in enumerate(in_lengths(up, down)):
            for dtype in (np.float32, np.int16):
                out.append(Case(f"{up}/{down} recording n_in {n} {np.dtype(dtype).name}", up, down, 8, dtype, n, 0, 0, 0, count(up, down, n),
                                100 * r + k))
    for r, ((up, down), C) in enumerate(LARGE_LDS):       # launches above 64 KiB of dynamic LDS
        for k, m in enumerate((RS_TILE - 1, RS_TILE, RS_TILE + 1, 2 * RS_TILE + 1)):
            n, dtype = n_in_for(up, down, m), (np.int16 if (k + r) % 2 else np.float32)
            out.append(Case(f"large {up}/{down} C {C} recording n_in {n} {np.dtype(dtype).name}", up, down, C, dtype, n, 0, 0, 0,
                            count(up, down, n), 3000 + 10 * r + k))
    for r, (up, down) in enumerate(RATIOS):
        n_in = job_recording_len(up, down)
        dtype = np.int16 if r % 2 else np.float32
        for k, (N0, n, m0, n_m, H, flush) in enumerate(stream_jobs(up, down, n_in)):
            out.append(Case(f"{up}/{down} job {k} N0 {N0} n {n} m0 {m0} n_m {n_m} H {H} {np.dtype(dtype).name}", up, down, 2, dtype, n, H, N0,
                            m0, n_m, 5000 + r))
    return out


def case_data(c):
    """(piece [C, n], hist float32 [C, H] or None) of a case"""
    if c.H == 0:
        return samples(c.C, c.n_in, c.dtype, c.seed), None
    whole = samples(c.C, job_recording_len(c.up, c.down), c.dtype, c.seed)       # (one recording for all jobs of a ratio)
    return whole[:, c.N0:c.N0 + c.n_in], history_of(whole, c.N0, c.H)


def history_of(whole, N0, H):
    """inputs [N0 - H, N0) of a recording [C, n] as float32 [C, H]; zeros before the recording"""
    v = values(whole).astype(np.float32)
    pad = np.concatenate([np.zeros((v.shape[0], H), np.float32), v], axis=1)
    return pad[:, N0:N0 + H]
