"""References, error bounds, exact models, input families and case lists for the kernels of csrc/mvdr.hip and csrc/stitch.hip
(DESIGN.md 3.3d).  No GPU, no library: tests/test_backend_reference.py checks this file on the CPU, tests/test_hip_backend_kernels.py
holds the kernels to it through the host entries of include/css_mi355_backend.h.

U = 2^-24 and u = 2^-53 are the unit roundoffs of float32 and float64.  The float64 kernels (covariances, solve) are judged
against numpy longdouble (64-bit significand on x86-64: u / 2048), with sums and the elimination written out here; the float32
kernels that round in a stated order are modelled bit for bit.  Every bound is counted along the kernel's path (the count tables
are in DESIGN.md 3.3d) and was fixed before the first GPU run.  `mut` arguments name the deliberate mistakes of
tests/test_backend_reference.py."""
import numpy as np

from frontend_reference import CANARY, U, bits, canary, level_gain        # noqa: F401  (shared with the front-end tests)
from gemm_reference import split_decode, split_encode                      # noqa: F401

u = 2.0 ** -53
LD, CLD = np.longdouble, np.clongdouble
assert np.finfo(LD).nmant >= 63, "numpy longdouble is no wider than float64 here: the float64 kernels have no reference above them"
SECOND = 1.0 + 2.0 ** -10      # second-order terms of every first-order count below
NC, NPACK = 7, 49
FLOOR_W, DIAG = 1e-10, 1e-15   # mvdr_util.py:55, :63-65 (the doubles the kernel holds)
f32 = np.float32
CANARY_F64 = np.array([0x7FF8BEEF7FC0BEEF], np.uint64).view(np.float64)[0]
CANARY_BYTE = 0xA5


def canary64(n):
    return np.full(int(n), CANARY_F64, np.float64)


def canary8(n):
    return np.full(int(n), CANARY_BYTE, np.uint8)


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def valid_frames(stft_frames, seg, hop, T):
    return int(min(max(stft_frames - seg * hop, 0), T))


# ---- packed Hermitian 7 x 7: 7 real diagonal entries, then (Re, Im) of (c, d), c < d, row by row ----------------------------

PAIRS = [(c, d) for c in range(NC) for d in range(c + 1, NC)]


def pack_index(c, d):
    """index of Re (c, d), c < d; Im follows"""
    return NC + 2 * PAIRS.index((c, d))


def unpack(p):
    """packed [..., 49] -> Hermitian [..., 7, 7] (complex of the packed dtype's width)"""
    p = np.asarray(p)
    out = np.zeros(p.shape[:-1] + (NC, NC), CLD if p.dtype == LD else np.complex128)
    for c in range(NC):
        out[..., c, c] = p[..., c]
    for i, (c, d) in enumerate(PAIRS):
        v = p[..., NC + 2 * i] + 1j * p[..., NC + 2 * i + 1]
        out[..., c, d] = v
        out[..., d, c] = np.conj(v)
    return out


# ---- launch_scm -------------------------------------------------------------------------------------------------------------

def scm_k(T, long_path):
    """roundings a term of a packed entry passes: scm_kernel: the sum of two exact products, m - 1e-10, the
    weight product (3), the lane's chain of ceil(T / 16) additions, four reduce-scatter levels, the two levels that combine the
    four plain sums, the floor product and the sum with it (2), the diagonal (1); scm_long_kernel: 3 + a chain of T + the floor
    product and sum (2) + the diagonal (1)."""
    return T + 6 if long_path else -(-T // 16) + 12


def winners(m, S, ov=None, mut=None):
    """m [S + 1][..., t] float32 -> bool [S + 1][..., t]: every tied mask wins (mask == mask_max); ov: the override bytes"""
    nm = S + 1
    if ov is not None:
        ov = np.asarray(ov).astype(np.int64)
        return np.stack([np.where(ov >= 16, (ov >> j) & 1, ov == j).astype(bool) for j in range(nm)])
    win = m == m.max(axis=0, keepdims=True)
    if mut == "first_tied_only":
        first = np.argmax(win, axis=0)
        win = np.arange(nm).reshape((nm,) + (1,) * (m.ndim - 1)) == first[None]
    return win


def _segment(X, F, stft_frames, seg, T, hop, tv=None, shift=0):
    """the segment's valid frames of the planes X [7][2 F][T_ld] -> (re, im) [7][F][tv] float32"""
    tv = valid_frames(stft_frames, seg, hop, T) if tv is None else tv
    st = seg * hop + shift
    return X[:, :F, st:st + tv], X[:, F:2 * F, st:st + tv], tv


def _products(re, im, dtype):
    """P[e][f][t]: the 49 packed entries of x x^H per frame, and their absolute-term sums |a_c a_d| + |b_c b_d|"""
    a, b = re.astype(dtype), im.astype(dtype)
    P = np.empty((NPACK,) + a.shape[1:], dtype)
    Q = np.empty((NPACK,) + a.shape[1:], np.float64)
    aa, ab = np.abs(re.astype(np.float64)), np.abs(im.astype(np.float64))
    for c in range(NC):
        P[c] = a[c] * a[c] + b[c] * b[c]
        Q[c] = aa[c] * aa[c] + ab[c] * ab[c]
    for i, (c, d) in enumerate(PAIRS):
        P[NC + 2 * i] = a[c] * a[d] + b[c] * b[d]
        P[NC + 2 * i + 1] = b[c] * a[d] - a[c] * b[d]
        Q[NC + 2 * i] = aa[c] * aa[d] + ab[c] * ab[d]
        Q[NC + 2 * i + 1] = ab[c] * aa[d] + aa[c] * ab[d]
    return P, Q


def scm(X, F, stft_frames, masks, S, T, hop, seg, ov=None, long_path=False, mut=None):
    """(Phi [S + 1][F][49] longdouble, bound [S + 1][F][49] float64) of one segment: mvdr_util.py:50-65 with w_k = m_k where mask
    k is a maximum of the frame, else 1e-10; masks [(S + 1) F][mask_ld]; ov [segments][F][T] bytes or None.
    bound = K u (A + 1e-15 on the diagonal) + 2 K u 1e-10 B: A over the winner frames with their weights, B over all valid
    frames (a winner frame's floor share 1e-10 P is carried by both accumulator sets: the factor 2)."""
    nm = S + 1
    tv = T if mut == "past_tv" else None
    re, im, tv = _segment(X, F, stft_frames, seg, T, hop, tv, shift=1 if mut == "start_plus_one" else 0)
    m = masks.reshape(-1, F, masks.shape[-1])[:nm, :, seg * T:seg * T + tv]
    win = winners(m, S, None if ov is None else ov.reshape(-1, F, T)[seg][:, :tv], mut)
    w = np.where(win, m.astype(LD), LD(0.0) if mut == "no_floor" else LD(FLOOR_W))
    P, Q = _products(re, im, LD)
    if mut == "im_negated":
        P[NC + 1::2] = -P[NC + 1::2]
    phi = np.einsum("kft,eft->kfe", w, P)
    if mut != "no_diag":
        phi[:, :, :NC] += LD(DIAG)
    if mut == "slot_neighbour":       # a total of the reduce-scatter stored one slot further
        phi[:, :, [24, 25]] = phi[:, :, [25, 24]]
    A = np.einsum("kft,eft->kfe", np.where(win, np.abs(m.astype(np.float64)), 0.0), Q)
    B = np.broadcast_to(Q.sum(axis=2).T[None], A.shape)
    K = scm_k(T, long_path)
    diag = np.where(np.arange(NPACK) < NC, DIAG, 0.0)
    return phi, SECOND * u * (K * (A + diag) + 2 * K * FLOOR_W * B)


def scm_restated(X, F, stft_frames, masks, S, T, hop, seg, ov=None, long_path=False):
    """the two kernels' algorithms in numpy float64: scm_kernel's frames by winner, 16 lanes per list, crosswise weighted and
    plain sums, a four-level tree, Phi = weighted + 1e-10 (sum of the four plain sums); scm_long_kernel's in-order chains"""
    nm = S + 1
    re, im, tv = _segment(X, F, stft_frames, seg, T, hop)
    m = masks.reshape(-1, F, masks.shape[-1])[:nm, :, seg * T:seg * T + tv]
    win = winners(m, S, None if ov is None else ov.reshape(-1, F, T)[seg][:, :tv])
    P, _ = _products(re, im, np.float64)                      # [49][F][tv]
    out = np.zeros((nm, F, NPACK))
    first = win & (np.cumsum(win, axis=0) == 1)
    for f in range(F):
        if long_path:
            for k in range(nm):
                acc, plain = np.zeros(NPACK), np.zeros(NPACK)
                for t in range(tv):
                    acc = acc + (float(m[k, f, t]) - FLOOR_W if win[k, f, t] else 0.0) * P[:, f, t]
                    plain = plain + P[:, f, t]
                out[k, f] = acc + FLOOR_W * plain
            continue
        tot_w, tot_p = np.zeros((4, NPACK)), np.zeros((4, NPACK))
        for k in range(nm):
            lst = np.flatnonzero(win[k, f])
            acc, pl = np.zeros((16, NPACK)), np.zeros((16, NPACK))
            for l in range(16):
                for t in lst[l::16]:
                    acc[l] = acc[l] + (float(m[k, f, t]) - FLOOR_W) * P[:, f, t]
                    pl[l] = pl[l] + (1.0 if first[k, f, t] else 0.0) * P[:, f, t]
            for v, dst in ((acc, tot_w), (pl, tot_p)):
                a = v[:8] + v[:7:-1]
                a = a[:4] + a[:3:-1]
                a = a[:2] + a[2:]
                dst[k] = a[0] + a[1]
        plain = (tot_p[0] + tot_p[1]) + (tot_p[2] + tot_p[3])
        out[:, f] = tot_w[:nm] + FLOOR_W * plain
    out[:, :, :NC] += DIAG
    return out


# ---- launch_mvdr_solve ------------------------------------------------------------------------------------------------------

SOLVE_C = 3      # a complex product (two products and a sum: 2 sqrt(2) u), a chain of n - 1 complex sums, a reciprocal followed by a
#                  product (3 u + 2 sqrt(2) u): n + 8 <= 3 n roundings where the real analysis counts n
SOLVE_G = (SOLVE_C * 3 * NC + 2) * u       # + the two sums that form Phi_n from up to three covariances
JUDGED = 1e-9    # a system is judged where its bound is at most 1e-9 max |W|


def _cinv(a):
    d = a.real * a.real + a.imag * a.imag
    return (a.real / d) + 1j * (-a.imag / d)


def lu_solve(A, Bm, pivot=True, swap_rhs=True):
    """Z = A^-1 Bm by the kernel's elimination (partial pivoting on |re| + |im|, first on ties; a reciprocal and a product in
    place of each division) in the dtype of A.  Returns (Z, L, U, perm) with A[perm] = L U."""
    A, Z = A.copy(), Bm.copy()
    n = A.shape[0]
    perm = np.arange(n)
    for p in range(n):
        if pivot:
            best = p + int(np.argmax(np.abs(A[p:, p].real) + np.abs(A[p:, p].imag)))
            if best != p:
                A[[p, best]] = A[[best, p]]
                if swap_rhs:
                    Z[[p, best]] = Z[[best, p]]
                perm[[p, best]] = perm[[best, p]]
        ip = _cinv(A[p, p])
        for r in range(p + 1, n):
            l = A[r, p] * ip
            A[r, p] = l
            A[r, p + 1:] = A[r, p + 1:] - l * A[p, p + 1:]
    for r in range(1, n):
        for c in range(r):
            Z[r] = Z[r] - A[r, c] * Z[c]
    for r in range(n - 1, -1, -1):
        for c in range(r + 1, n):
            Z[r] = Z[r] - A[r, c] * Z[c]
        Z[r] = Z[r] * _cinv(A[r, r])
    return Z, np.tril(A, -1) + np.eye(n, dtype=A.dtype), np.triu(A), perm


def solve(scm_seg, S, F, dtype=LD, mut=None, want_bound=True):
    """scm_seg [S + 1][F][49] float64 (as uploaded) -> (W [S][F][7] complex of dtype, bound [S][F][7] float64 or None) of one
    segment: Phi_n = sum_{j != spk} Phi_j, Z = Phi_n^-1 Phi_spk, W = Z[:, 0] / (trace Z [+ 1e-15 at bin 0]).
    bound: |dZ| <= g |Phi_n^-1| (|L| |U|) |Z| (Higham, Accuracy and Stability, Thm 9.4, with L, U of this elimination), carried
    through the trace: dW = (dZ[:, 0] + |W| dtr) / |tr| + 6 u |W|, dtr = sum_c dZ[c, c] + 8 u sum_c |Z[c, c]|."""
    cd = CLD if dtype == LD else np.complex128
    H = unpack(np.asarray(scm_seg).astype(dtype))            # [S + 1][F][7][7]
    W = np.zeros((S, F, NC), cd)
    bound = np.zeros((S, F, NC)) if want_bound else None
    for spk in range(S):
        for f in range(F):
            others = [j for j in range(S + 1) if j != spk or mut == "own_left_in"]
            if mut == "noise_left_out":
                others = [j for j in others if j != S]
            A = np.zeros((NC, NC), cd)
            for j in others:
                A = A + H[j, f]
            Z, Lm, Um, perm = lu_solve(A, H[spk, f].copy(), pivot=mut != "no_pivot", swap_rhs=mut != "rhs_not_exchanged")
            tr = np.trace(Z) + (dtype(DIAG) if f == 0 else dtype(0))
            col = Z[0, :] if mut == "row_zero" else Z[:, 0]
            W[spk, f] = col * _cinv(tr)
            if not want_bound:
                continue
            inv, _, _, _ = lu_solve(A, np.eye(NC, dtype=cd))
            LU = np.empty((NC, NC))
            LU[perm] = np.abs(Lm).astype(np.float64) @ np.abs(Um).astype(np.float64)
            Za = np.abs(Z).astype(np.float64)
            dZ = SOLVE_G * np.abs(inv).astype(np.float64) @ LU @ Za
            dtr = np.trace(dZ) + 8 * u * np.trace(Za)
            Wa = np.abs(W[spk, f]).astype(np.float64)
            bound[spk, f] = SECOND * ((dZ[:, 0] + Wa * dtr) / float(np.abs(tr)) + 6 * u * Wa)
    return W, bound


def judged(W, bound):
    """[S][F] bool: the systems whose bound is at most 1e-9 max_c |W_c|"""
    return bound.max(axis=-1) <= JUDGED * np.abs(W).astype(np.float64).max(axis=-1)


def bfw_complex(raw):
    """bfw [..., 7][2] doubles -> complex128 [..., 7]"""
    raw = np.asarray(raw, np.float64)
    return raw[..., 0] + 1j * raw[..., 1]


# ---- launch_beamform --------------------------------------------------------------------------------------------------------

def beamform_plain(X, F, stft_frames, masks, S, T, hop, seg, floor, mut=None):
    """use_mvdr = 0, bit for bit: sep [S][F][T][2] = x_0 * max(mask, floor) in float32; frames from tv on are the word 0"""
    re, im, tv = _segment(X, F, stft_frames, seg, T, hop)
    m = masks.reshape(-1, F, masks.shape[-1])[:S, :, seg * T:(seg + 1) * T]
    m = np.minimum(m, f32(floor)) if mut == "floor_as_minimum" else np.maximum(m, f32(floor))
    out = np.zeros((S, F, T, 2), np.float32)
    out[:, :, :tv, 0] = re[0][None] * m[:, :, :tv]
    out[:, :, :tv, 1] = im[0][None] * m[:, :, :tv]
    return out


def beamform(X, F, stft_frames, masks, S, T, hop, seg, floor, W, mut=None):
    """use_mvdr = 1: (sep64 [S][F][T][2], bound) with y = sum_c conj(W_c) x_c in float64 from the uploaded weights W [S][F][7]
    complex128, times max(mask, floor); bound = (14 u sum |W| |x| + U/2 |y|) m + U/2 |y m| per component: U |y m| in all, what ONE
    rounding to float32 of the float64 product y m leaves (a value rounded to float32 twice, y and then y m, can be 2 U from it)."""
    re, im, tv = _segment(X, F, stft_frames, seg, T, hop)
    x = re.astype(np.float64) + 1j * im.astype(np.float64)                    # [7][F][tv]
    m = masks.reshape(-1, F, masks.shape[-1])[:S, :, seg * T:(seg + 1) * T]
    m = (np.minimum(m, f32(floor)) if mut == "floor_as_minimum" else np.maximum(m, f32(floor))).astype(np.float64)
    Wc = W if mut == "no_conj" else np.conj(W)
    y = np.einsum("sfc,cft->sft", Wc, x)
    mag = np.einsum("sfc,cft->sft", np.abs(W), np.abs(x))
    out, bound = np.zeros((S, F, T, 2)), np.zeros((S, F, T, 2))
    for i, part in enumerate((y.real, y.imag)):
        out[:, :, :tv, i] = part * m[:, :, :tv]
        bound[:, :, :tv, i] = (14 * u * mag + U / 2 * np.abs(part)) * m[:, :, :tv] + U / 2 * np.abs(part * m[:, :, :tv])
    return out, bound


def beamform_restated(X, F, stft_frames, masks, S, T, hop, seg, floor, W):
    """the kernel's arithmetic in numpy: float64 chain over the microphones, the mask product in float64, one rounding to float32"""
    re, im, tv = _segment(X, F, stft_frames, seg, T, hop)
    m = np.maximum(masks.reshape(-1, F, masks.shape[-1])[:S, :, seg * T:(seg + 1) * T], f32(floor))
    sr, si = np.zeros((S, F, tv)), np.zeros((S, F, tv))
    for c in range(NC):
        wr, wi = W[:, :, c].real[:, :, None], W[:, :, c].imag[:, :, None]
        xr, xi = re[c].astype(np.float64)[None], im[c].astype(np.float64)[None]
        sr = sr + (wr * xr + wi * xi)
        si = si + (wr * xi - wi * xr)
    out = np.zeros((S, F, T, 2), np.float32)
    out[:, :, :tv, 0] = (sr * m[:, :, :tv].astype(np.float64)).astype(np.float32)
    out[:, :, :tv, 1] = (si * m[:, :, :tv].astype(np.float64)).astype(np.float32)
    return out


# ---- launch_segment_power_norm ------------------------------------------------------------------------------------------------

def power_norm(X, F, stft_frames, sep, S, T, hop, seg):
    """(sep64 [S][F][T][2], bound, g): sep g with g = sqrt(sum |x_0|^2) / sqrt(sum |sum_k sep_k|^2) over the valid frames, the stream
    sum in float32 in ascending order (modelled exactly), the energies in float64: chains of 2 ceil(F tv / 256) additions, six
    wave levels and two block levels (L), three roundings for the roots and the quotient, one for the float64 product; then ONE
    rounding to float32: (U + (L + 4) u) |sep g| -- U and terms of second order beside it."""
    re, im, tv = _segment(X, F, stft_frames, seg, T, hop)
    em = (re[0].astype(LD) ** 2 + im[0].astype(LD) ** 2).sum()
    acc = np.zeros((F, tv, 2), np.float32)
    for k in range(S):
        acc = acc + sep[k, :, :tv]
    es = (acc.astype(LD) ** 2).sum()
    with np.errstate(invalid="ignore", divide="ignore"):
        g = float(np.sqrt(em) / np.sqrt(es))                  # (NaN where the segment has no valid frame or is silent)
    L = 2 * -(-F * tv // 256) + 8
    out = sep.astype(np.float64) * g
    return out, SECOND * (U + (L + 4) * u) * np.abs(out), g


def power_norm_restated(X, F, stft_frames, sep, S, T, hop, seg, twice=False):
    """the kernel's arithmetic in numpy: float64 energies and gain, the float64 product, one rounding to float32.  twice: the gain
    rounded to float32 and a float32 product after it (two roundings: up to 2 U from sep g)"""
    re, im, tv = _segment(X, F, stft_frames, seg, T, hop)
    em = (re[0].astype(np.float64) ** 2 + im[0].astype(np.float64) ** 2).sum()
    acc = np.zeros((F, tv, 2), np.float32)
    for k in range(S):
        acc = acc + sep[k, :, :tv]
    es = (acc.astype(np.float64) ** 2).sum()
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.sqrt(em) / np.sqrt(es)
        return sep * f32(g) if twice else (sep.astype(np.float64) * g).astype(np.float32)


# ---- launch_pit_costs ---------------------------------------------------------------------------------------------------------

PIT_CH = 48


def pit_levels(F, ov):
    """additions a term passes: the thread's chain over its chunk, four DPP steps, two levels over the rows, two over the waves,
    the 48 chunks; + 1 for the division"""
    n = max((F * (ch + 1) // PIT_CH - F * ch // PIT_CH) * ov for ch in range(PIT_CH))
    return -(-n // 256) + 4 + 2 + 2 + 48 + 1


def pit_costs(masks, sep, S, F, T, hop, b, loss, inp, mut=None):
    """(cost [S][S] longdouble, bound [S][S]) of boundary b: cost[a][c] = mean over F and the overlap of loss(L_a - R_c), L the
    last T - hop frames of segment b, R the first of segment b + 1.  Input 0 (masks [S F][mask_ld] at least): the float32 terms
    fabsf(l - r) / fl(d d) exactly; input 1 (sep [segments][S][F][T][2]): sqrtf(re re + im im) carries 2 U |a| (contraction is
    the compiler's choice), hence d carries 2 U (l + r) + U |d|."""
    ov = T - hop
    if inp == 0:
        m = masks.reshape(-1, F, masks.shape[-1])[:S]
        l, r = m[:, :, b * T + hop:(b + 1) * T], m[:, :, (b + 1) * T:(b + 1) * T + ov]
        if mut == "regions_swapped":
            l, r = m[:, :, b * T:b * T + ov], m[:, :, (b + 1) * T + hop:(b + 2) * T]
        d = l[:, None] - r[None]                                               # float32 [S][S][F][ov]
        term = (np.abs(d) if loss == 0 else d * d).astype(LD)
        slack = np.zeros(term.shape)
    else:
        v = sep.astype(np.float64)
        mag = np.sqrt(v[..., 0] ** 2 + v[..., 1] ** 2)                          # [segments][S][F][T]
        l, r = mag[b, :, :, hop:], mag[b + 1, :, :, :ov]
        if mut == "regions_swapped":
            l, r = mag[b, :, :, :ov], mag[b + 1, :, :, hop:]
        d = l[:, None] - r[None]
        dd = 2 * U * (l[:, None] + r[None]) + U * np.abs(d)
        term = (np.abs(d) if loss == 0 else d * d).astype(LD)
        slack = dd if loss == 0 else 2 * np.abs(d) * dd + dd * dd + U * d * d
    cost = term.sum(axis=(2, 3)) / LD(F * ov)
    if mut == "transposed":
        cost = cost.T
    bound = SECOND * (pit_levels(F, ov) * u * cost.astype(np.float64) + slack.sum(axis=(2, 3)) / (F * ov))
    return cost, bound


def pit_costs_restated(masks, sep, S, F, T, hop, b, loss, inp):
    """the kernel's sums in numpy: float32 terms, float64 chunk sums in chunk order"""
    ov = T - hop
    if inp == 0:
        m = masks.reshape(-1, F, masks.shape[-1])[:S]
        l, r = m[:, :, b * T + hop:(b + 1) * T], m[:, :, (b + 1) * T:(b + 1) * T + ov]
    else:
        mag = np.sqrt(sep[..., 0] * sep[..., 0] + sep[..., 1] * sep[..., 1])      # float32
        l, r = mag[b, :, :, hop:], mag[b + 1, :, :, :ov]
    d = l[:, None] - r[None]
    term = (np.abs(d) if loss == 0 else d * d).astype(np.float64)
    v = np.zeros((S, S))
    for ch in range(PIT_CH):
        v = v + term[:, :, F * ch // PIT_CH:F * (ch + 1) // PIT_CH].sum(axis=(2, 3))
    return v / (float(F) * ov)


# ---- launch_pit_scan ----------------------------------------------------------------------------------------------------------

def pit_scan(costs, S, lsap, b_lo=0, start=None, mut=None):
    """perms [n + 1][S] from the raw costs [n][S S] of boundaries [b_lo, n), rows b_lo + 1 .. n; row b_lo is `start` (identity at
    0).  lsap: oracle.css_oracle.lsap; a matrix with a non-finite cost keeps the rows' own columns."""
    costs = np.asarray(costs, np.float64).reshape(-1, S, S)
    n = costs.shape[0]
    perms = np.zeros((n + 1, S), np.int32)
    perms[b_lo] = np.arange(S) if start is None else start
    for b in range(b_lo, n):
        rows = costs[b] if mut == "raw_rows" else costs[b][perms[b]]
        try:       # (the oracle asserts where scipy raises "infeasible": every remaining column at an infinite distance)
            perms[b + 1] = np.arange(S) if S == 1 else lsap(rows)
        except AssertionError:
            perms[b + 1] = np.arange(S)
    return perms


# ---- overlap-add: the exact float32 models ------------------------------------------------------------------------------------

def contributor_class(T, hop):
    nc = -(-T // hop)
    return 2 if nc <= 2 else (4 if nc <= 4 else 0)


def coverage(num_segments, T, hop):
    return (num_segments - 1) * hop + T


def _weights(windows, seg, num_segments, mut=None):
    w_first, w_mid, w_last = windows
    if seg == 0:
        return w_first
    return w_last if seg == num_segments - 1 and mut != "mid_for_last" else w_mid


def _covering(t, T, hop, num_segments):
    lo = t - T + 1
    s0 = 0 if lo <= 0 else -(-lo // hop)
    return range(s0, min(t // hop, num_segments - 1) + 1)


def _ola_frame(rows, windows, perms, s_count, t, T, hop, num_segments, mut):
    """the float32 overlap-add of frame t: rows(seg, k, tl) -> float32 array of the stream's values; returns [S][...] (divided)"""
    segs = list(_covering(t, T, hop, num_segments))
    if mut == "descending":
        segs = segs[::-1]
    ws = f32(0)
    for seg in segs:
        ws = f32(ws + _weights(windows, seg, num_segments, mut)[t - seg * hop])
    out = []
    for s in range(s_count):
        v = None
        for seg in segs:
            k = perms[seg][s] if mut != "inverse_perm" else int(np.argsort(perms[seg])[s])
            w = _weights(windows, seg, num_segments, mut)[t - seg * hop]
            x = rows(seg, k, t - seg * hop)
            if mut == "divide_first":
                x = x / ws
            term = w * x
            v = (np.zeros_like(term) + term) if v is None else v + term
        if v is not None and mut != "divide_first":
            v = v / ws
        out.append(v)
    return out, bool(segs)


def ola_masks(masks, windows, perms, S, F, T, hop, num_segments, T_long, th, t_lo, t_hi, out=None, mut=None):
    """launch_ola_masks on the allocations out = (mask_st [S][F][T_long], activity [S][T_long], act_b [S][T_long]) (copies are
    returned): products, sums from 0 in ascending segment order, one division, all float32; the frequency mean as float64 sums
    over f = g, g + 16, ... per group, the 16 groups in order, / F, one rounding; act_b = activity >= th."""
    m = masks.reshape(-1, F, masks.shape[-1])
    mask_st, activity, act_b = (a.copy() for a in out)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(t_lo, t_hi):
            vals, _ = _ola_frame(lambda seg, k, tl: m[k, :, seg * T + tl], windows, perms, S, t, T, hop, num_segments, mut)
            for s in range(S):
                v = vals[s].astype(np.float32)
                mask_st[s, :, t] = v
                if mut == "mean_in_float32":
                    act = f32(v.sum(dtype=np.float32) / f32(F))
                else:
                    tot = 0.0
                    for g in range(16):
                        part = 0.0
                        for x in v[g::16]:
                            part += float(x)
                        tot += part
                    act = f32(tot / float(F))
                activity[s, t] = act
                act_b[s, t] = (act > f32(th)) if mut == "greater" else (act >= f32(th))
    return mask_st, activity, act_b


def morphology(act_b, S, T_long, dilation, erosion, t_lo, t_hi, out, dilate, erode, mut=None):
    """launch_morphology on the allocations out = (act_tmp, act_final) [S][T_long]: act_tmp over the dilated range
    [t_lo - erosion, t_hi + erosion) clipped to the recording, act_final over [t_lo, t_hi); dilate / erode: the oracle's
    (zero padding / one padding)."""
    act_tmp, act_final = (a.copy() for a in out)
    if t_hi <= t_lo:
        return act_tmp, act_final
    d_lo, d_hi = max(t_lo - erosion, 0), min(t_hi + erosion, T_long)
    for s in range(S):
        full = dilate(act_b[s].astype(np.uint8), dilation + (1 if mut == "radius_plus_one" else 0))
        act_tmp[s, d_lo:d_hi] = full[d_lo:d_hi]
        if mut == "erode_zero_padded":
            e = np.lib.stride_tricks.sliding_window_view(np.pad(full, erosion), 2 * erosion + 1).min(1)
        else:
            e = erode(full, erosion)
        act_final[s, t_lo:t_hi] = e[t_lo:t_hi]
    return act_tmp, act_final


def ola_stft(sep, windows, perms, gate, S, F, T, hop, num_segments, T_long, KIp, y_split, level, t_lo, t_hi, out, mut=None):
    """launch_ola_stft on the allocation out = Y [S][T_long][KIp] (a copy is returned): as ola_masks on Re and Im, then the gate
    product; row [Re F | Im F | zeros]; split rows are split_encode(v * level_gain(level) + 0).  gate: act_final [S][T_long], or
    act_b with mut 'gate_from_act_b' given by the caller."""
    Y = out.copy()
    lvl = level_gain(level) if y_split else f32(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(t_lo, t_hi):
            vals, any_ = _ola_frame(lambda seg, k, tl: sep[seg, k, :, tl, :], windows, perms, S, t, T, hop, num_segments, mut)
            for s in range(S):
                row = np.zeros(KIp, np.float32)
                if any_:
                    g = f32(1) if gate[s, t] else f32(0)
                    v = vals[s].astype(np.float32) * g
                    row[:F], row[F:2 * F] = v[:, 0], v[:, 1]
                # (split rows: + 0 -- the -0 of a gated frame leaves as +0 halves, stitch.hip pins what the fused conversion writes)
                Y[s, t] = split_encode((row * lvl + f32(0))[None])[0] if y_split else row
    return Y


# ---- inputs -------------------------------------------------------------------------------------------------------------------

def planes(family, F, T_ld, stft_frames, seed):
    """X [7][2 F][T_ld] float32, NaN from stft_frames on (a read of them shows up)"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((NC, 2 * F, T_ld)).astype(np.float32)
    if family == "magnitudes":
        X *= (10.0 ** rng.uniform(-6, 3, (1, 1, T_ld))).astype(np.float32)
    elif family == "silent_ref":
        X[0] = 0
    elif family == "silent":
        X[:] = 0
    elif family == "pairs":       # frame t: one nonzero microphone pair (c, d): 49 distinguishable entries
        X[:] = 0
        for t in range(T_ld):
            c, d = divmod(t % 49, 7)
            for mic in {c, d}:
                X[mic, :, t] = f32(1 + (t % 49)) * (rng.standard_normal(2 * F) * 0.25 + 1).astype(np.float32)
    elif family != "gaussian":
        raise ValueError(family)
    X[:, :, stft_frames:] = np.nan
    return X


MASK_FAMILIES = ("random", "tied_fourth", "all_equal", "all_zero", "one_always", "one_never", "ulp_apart")


def mask_rows(family, S, F, mask_ld, seg_lo, nseg, T, seed):
    """masks [(S + 1) F][mask_ld] float32: the columns of segments [seg_lo, seg_lo + nseg) filled, every other column NaN"""
    rng = np.random.default_rng(seed)
    nm = S + 1
    m = np.full((nm, F, mask_ld), np.nan, np.float32)
    n = nseg * T
    v = rng.uniform(0.01, 1.0, (nm, F, n)).astype(np.float32)
    if family == "tied_fourth":
        top = v.max(axis=0)
        v[0, :, ::4] = top[:, ::4]
        v[nm - 1, :, ::4] = top[:, ::4]
    elif family == "all_equal":
        v[:] = v[0]
    elif family == "all_zero":
        v[:] = 0
    elif family == "one_always":
        v[S // 2] = 1.5
    elif family == "one_never":
        v[0] = 0.001
    elif family == "ulp_apart":     # the two largest masks of every frame are adjacent floats: mask 0 at the maximum, mask 1 above it
        v[0] = v.max(axis=0)
        v[1 % nm] = np.nextafter(v[0], f32(2))
    elif family != "random":
        raise ValueError(family)
    m[:, :, seg_lo * T:seg_lo * T + n] = v
    return m.reshape(nm * F, mask_ld)


def override_bytes(kind, S, F, segs, T, seed):
    rng = np.random.default_rng(seed)
    if kind == "index":
        return rng.integers(0, S + 1, (segs, F, T)).astype(np.uint8)
    return (16 | rng.integers(1, 1 << (S + 1), (segs, F, T))).astype(np.uint8)


def scm_cases():
    """every T of the covariance table once, with S, F, (nseg, seg_lo), hop, the valid frames of the last segment, mask_ld, the
    mask family, the plane family and the override form each walking its own list at its own stride (the strides are coprime
    to the lists' lengths, so no two of them move together); then explicit cases for what three, four or two lengths per kernel
    cannot meet by rotation: ties on audible planes and the index override on scm_kernel<4>, ties, three segments and no override
    on the any-length kernel, the bits override with every frame valid, a short last segment at (nseg, seg_lo) = (1, 0)"""
    Ts = (1, 15, 16, 17, 63, 64, 65, 128, 186, 191, 192, 193, 255, 256, 257, 320, 511, 512, 513, 600)
    planes_f = ("gaussian", "magnitudes", "silent_ref", "pairs", "gaussian", "silent")

    def case(name, T, S, F, nseg, seg_lo, hop, short, wide, masks, planes, override, seed):
        segs = seg_lo + nseg
        return dict(name=name, T=T, S=S, F=F, nseg=nseg, seg_lo=seg_lo, hop=hop, stft_frames=(segs - 1) * hop + T - min(short, T),
                    T_ld=(segs - 1) * hop + T + 3, mask_ld=segs * T + (5 if wide else 0), masks=masks, planes=planes, override=override,
                    seed=seed)

    cases = []
    for i, T in enumerate(Ts):
        nseg, seg_lo = ((1, 0), (3, 0), (1, 2), (3, 2))[i % 4]
        if T > 512 and nseg == 3:
            nseg = 1                                     # (three segments on the any-length kernel: an explicit case below)
        short = (0, 1, T - 1, T)[(3 * i + 1) % 4] if T > 1 else i % 2           # frames missing from the last segment
        cases.append(case(f"T{T}", T, (3, 2, 1)[i % 3], (5, 2, 1)[(2 * i) % 3], nseg, seg_lo, (T, -(-T // 2), 1)[(i + i // 3) % 3], short,
                          i % 2, MASK_FAMILIES[(3 * i) % len(MASK_FAMILIES)], planes_f[(5 * i + i // 6) % len(planes_f)],
                          (None, "index", "bits")[(i + i // 4) % 3], 100 + i))
    # the pairs family and the tied masks at the shipped length, every S
    for j, S in enumerate((1, 2, 3)):
        cases.append(case(f"pairs_S{S}", 186, S, 2, 1, 0, 93, 0, 0, ("tied_fourth", "all_equal", "ulp_apart")[j], "pairs", None, 200 + j))
    cases += [
        case("T193_tied", 193, 3, 2, 3, 0, 97, 1, 1, "tied_fourth", "gaussian", None, 210),
        case("T255_all_equal_index", 255, 2, 2, 1, 2, 128, 0, 0, "all_equal", "magnitudes", "index", 211),
        case("T256_tied_bits_full", 256, 3, 1, 1, 0, 256, 0, 0, "tied_fourth", "pairs", "bits", 212),
        case("T513_tied_3seg", 513, 3, 2, 3, 0, 257, 2, 1, "tied_fourth", "gaussian", None, 213),
        case("T600_all_equal", 600, 2, 1, 1, 0, 600, 599, 0, "all_equal", "magnitudes", None, 214),
        case("T320_ulp_short", 320, 2, 2, 1, 0, 160, 319, 1, "ulp_apart", "gaussian", None, 215),
    ]
    return cases


SCM_FORCED_T = (17, 186, 257)


def scm_case_arrays(c):
    segs = c["seg_lo"] + c["nseg"]
    X = planes(c["planes"], c["F"], c["T_ld"], c["stft_frames"], c["seed"])
    M = mask_rows(c["masks"], c["S"], c["F"], c["mask_ld"], c["seg_lo"], c["nseg"], c["T"], c["seed"] + 1)
    ov = None if c["override"] is None else override_bytes(c["override"], c["S"], c["F"], segs, c["T"], c["seed"] + 2)
    return X, M, ov


def covariances(family, S, F, seed, T=64, scale=1.0, winners_n=None):
    """uploaded covariances [S + 1][F][49] float64 of one segment for the solve: sum_t w x x^H + 1e-15 I from Gaussian planes in
    float64 numpy (the solve is tested on what the test uploads).  family: 'well' (random masks), 'pivot' (microphone 0 silent), 'quiet_ref'
    (microphone 0 at 1e-7 of the others), 'rank' (winners_n winner frames in all), 'silent' (Phi = 1e-15 I)."""
    rng = np.random.default_rng(seed)
    nm = S + 1
    if family == "silent":
        out = np.zeros((nm, F, NPACK))
        out[:, :, :NC] = DIAG
        return out
    Tn = winners_n if family == "rank" else T
    x = (rng.standard_normal((NC, F, Tn)) + 1j * rng.standard_normal((NC, F, Tn))) * scale
    if family == "pivot":
        x[0] = 0
    if family == "quiet_ref":      # the leading column is 1e-7 of the others: the elimination exchanges rows
        x[0] *= 1e-7
    m = rng.uniform(0.01, 1.0, (nm, F, Tn))
    w = np.where(m == m.max(axis=0, keepdims=True), m, FLOOR_W)
    out = np.zeros((nm, F, NPACK))
    for k in range(nm):
        R = np.einsum("ft,cft,dft->fcd", w[k], x, np.conj(x))
        for c in range(NC):
            out[k, :, c] = R[:, c, c].real + DIAG
        for i, (c, d) in enumerate(PAIRS):
            out[k, :, NC + 2 * i], out[k, :, NC + 2 * i + 1] = R[:, c, d].real, R[:, c, d].imag
    return out


def solve_cases():
    """(name, family, complete) -> S, F and the arguments of covariances(); complete: every system must be judged"""
    cases = []
    i = 0
    for T in (64, 186):
        for scale in (1e-3, 1.0, 1e3):
            cases.append(dict(name=f"well_T{T}_x{scale:g}", family="well", complete=True, S=(1, 2, 3)[i % 3], F=(5, 1)[i % 2], T=T,
                              scale=scale, winners_n=None, seed=300 + i))
            i += 1
    for S in (1, 2, 3):
        cases.append(dict(name=f"pivot_S{S}", family="pivot", complete=False, S=S, F=5, T=64, scale=1.0, winners_n=None, seed=320 + S))
        cases.append(dict(name=f"quiet_ref_S{S}", family="quiet_ref", complete=False, S=S, F=5, T=64, scale=1.0, winners_n=None, seed=325 + S))
        cases.append(dict(name=f"silent_S{S}", family="silent", complete=False, S=S, F=(1, 5, 5)[S - 1], T=64, scale=1.0, winners_n=None,
                          seed=330 + S))
    for j, n in enumerate((1, 3, 6)):
        cases.append(dict(name=f"rank{n}", family="rank", complete=False, S=(3, 2, 1)[j], F=5, T=64, scale=1.0, winners_n=n, seed=340 + j))
    return cases


def solve_case_scm(c, nseg=1):
    """[nseg][S + 1][F][49]"""
    return np.stack([covariances(c["family"], c["S"], c["F"], c["seed"] + 17 * s, c["T"], c["scale"], c["winners_n"]) for s in range(nseg)])


PIT_F = (1, 5, 47, 48, 49, 257)
PIT_TH = ((2, 1), (16, 8), (17, 5), (186, 93), (64, 63))
PIT_RANGES = ((0, 3), (1, 2), (2, 3))


def pit_cases():
    cases = []
    i = 0
    for F in PIT_F:
        for T, hop in PIT_TH:
            cases.append(dict(name=f"F{F}_T{T}_hop{hop}", S=(1, 2, 3, 4)[i % 4], F=F, T=T, hop=hop, loss=i % 2, input=(i // 2) % 2, seed=400 + i))
            i += 1
    for S in (1, 2, 3, 4):       # every S with both losses and both inputs at one small shape
        for loss in (0, 1):
            for inp in (0, 1):
                cases.append(dict(name=f"S{S}_loss{loss}_in{inp}", S=S, F=5, T=17, hop=5, loss=loss, input=inp, seed=460 + 4 * S + 2 * loss + inp))
    return cases


def pit_inputs(S, F, T, num_segments, seed, mask_ld=None):
    """(masks [S F][mask_ld], sep [segments][S][F][T][2]) of a session"""
    rng = np.random.default_rng(seed)
    mask_ld = num_segments * T if mask_ld is None else mask_ld
    m = np.full((S * F, mask_ld), np.nan, np.float32)
    m[:, :num_segments * T] = rng.uniform(0, 1, (S * F, num_segments * T)).astype(np.float32)
    sep = (rng.standard_normal((num_segments, S, F, T, 2)) * 10.0 ** rng.uniform(-3, 2, (num_segments, S, 1, 1, 1))).astype(np.float32)
    return m, sep


SCAN_N = (1, 2, 4095, 4096, 4097, 8193)


def scan_costs(kind, n, S, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        c = rng.uniform(0, 1, (n, S * S))
    elif kind == "ties":
        c = rng.integers(0, 3, (n, S * S)).astype(np.float64)
    elif kind == "zero":
        c = np.zeros((n, S * S))
    elif kind in ("inf", "nan"):
        c = rng.uniform(0, 1, (n, S * S))
        c[n // 2, (S * S) // 2] = np.inf if kind == "inf" else np.nan
    else:
        raise ValueError(kind)
    return c


OLA_TH = {2: ((16, 8), (17, 9), (186, 93), (8, 8)), 4: ((16, 5), (16, 4), (9, 3)), 0: ((16, 3), (16, 1), (7, 1))}
OLA_F = (1, 15, 16, 17, 257)
OLA_RANGES = ((0, None), (0, 1), (5, 6), (15, 17), (16, 32), (3, 35))
OLA_PERM3 = (1, 2, 0)           # not an involution: its inverse is (2, 0, 1)
LEVEL_WORDS = (0, int(np.array([0.37], np.float32).view(np.uint32)[0]), int(np.array([5e4], np.float32).view(np.uint32)[0]))


def ola_cases():
    cases = []
    i = 0
    for cls, ths in OLA_TH.items():
        for T, hop in ths:
            for nseg in (1, 2, 5):
                S, F = (1, 3, 4)[i % 3], OLA_F[i % 5] if not (T == 186 and OLA_F[i % 5] == 257 and nseg == 5) else 17
                cov = coverage(nseg, T, hop)
                cases.append(dict(name=f"class{cls}_T{T}_hop{hop}_n{nseg}", cls=cls, S=S, F=F, T=T, hop=hop, num_segments=nseg,
                                  T_long=cov - (3 if i % 2 and cov > 3 else 0), window="random" if hop == T or nseg == 1 else ("cfg", "random")[i % 2],
                                  perm=("identity", "fixed", "random")[i % 3], KIp_extra=(0, 32)[i % 2], seed=500 + i))
                i += 1
    return cases


def ola_windows(kind, T, seed, calc_segment_weight):
    """[3][T] float32: w_first | w_mid | w_last -- the oracle's trapezoids (zero margins: only where segments overlap), else
    positive random windows"""
    m0, m1 = T // 8, T // 4
    if kind == "cfg" and T > 2 * m1 and m1 > m0:
        return np.stack([calc_segment_weight(T, m0, m1, is_first_seg=True), calc_segment_weight(T, m0, m1),
                         calc_segment_weight(T, m0, m1, is_last_seg=True)]).astype(np.float32)
    return np.random.default_rng(seed).uniform(0.05, 1.0, (3, T)).astype(np.float32)


def ola_perms(kind, S, num_segments, seed):
    rng = np.random.default_rng(seed)
    if kind == "identity":
        return np.tile(np.arange(S, dtype=np.int32), (num_segments, 1))
    if kind == "fixed":
        p = np.roll(np.arange(S, dtype=np.int32), -1) if S != 3 else np.array(OLA_PERM3, np.int32)
        return np.tile(p, (num_segments, 1))
    return np.stack([rng.permutation(S).astype(np.int32) for _ in range(num_segments)])


def ola_inputs(c, calc_segment_weight):
    S, F, T, n = c["S"], c["F"], c["T"], c["num_segments"]
    rng = np.random.default_rng(c["seed"])
    masks = rng.uniform(0, 1, (S * F, n * T)).astype(np.float32)
    sep = rng.standard_normal((n, S, F, T, 2)).astype(np.float32)
    return masks, sep, ola_windows(c["window"], T, c["seed"] + 1, calc_segment_weight), ola_perms(c["perm"], S, n, c["seed"] + 2)


def gates(S, T_long, seed):
    """act_b [S][T_long] bytes: runs that touch both ends, isolated frames and gaps"""
    rng = np.random.default_rng(seed)
    g = (rng.uniform(0, 1, (S, T_long)) < 0.35).astype(np.uint8)
    g[:, :min(2, T_long)] = 1
    g[0, -min(3, T_long):] = 1
    if S > 1:
        g[1, -1] = 0
    return g
