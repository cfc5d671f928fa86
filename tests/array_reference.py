"""tests/backend_reference.py's covariance, solve and beamformer references for microphone arrays of any size C (csrc/mvdr.hip is a
template over the microphone count, 2 .. 8).  No GPU, no library.  What does not depend on the microphone count
is imported from backend_reference; `scm`, `solve`, `beamform`, the packed layout and the input families are restated with C where
that file has 7: the same longdouble values and the same derived bounds -- K of `scm_k` (the pass structure of the C = 8 kernel
changes no count: an entry still passes one lane chain and four exchange levels), g = (3 * 3 C + 2) u of the solve, 2 C u of the
beamformer's chain.  tests/test_mic_arrays_host.py checks on the CPU that C = 7 reproduces backend_reference exactly and that the
float64 evaluation lies inside the bound at every C; tests/test_hip_mic_array_kernels.py holds the kernels to it."""
import numpy as np

from backend_reference import (CLD, DIAG, FLOOR_W, JUDGED, LD, MASK_FAMILIES, SECOND, SOLVE_C, U, _cinv, _segment, bfw_complex,   # noqa: F401
                               bits, bits64, canary, canary64, f32, judged, lu_solve, mask_rows, override_bytes, scm_k, u,
                               valid_frames, winners)

CS = (2, 3, 4, 5, 6, 7, 8)


def npack(C):
    return C * C


def pairs(C):
    return [(c, d) for c in range(C) for d in range(c + 1, C)]


def solve_g(C):
    return (SOLVE_C * 3 * C + 2) * u


def unpack(p, C):
    """packed [..., C C] -> Hermitian [..., C, C]"""
    p = np.asarray(p)
    out = np.zeros(p.shape[:-1] + (C, C), CLD if p.dtype == LD else np.complex128)
    for c in range(C):
        out[..., c, c] = p[..., c]
    for i, (c, d) in enumerate(pairs(C)):
        v = p[..., C + 2 * i] + 1j * p[..., C + 2 * i + 1]
        out[..., c, d] = v
        out[..., d, c] = np.conj(v)
    return out


def _products(re, im, dtype):
    """P[e][f][t]: the C C packed entries of x x^H per frame, and their absolute-term sums |a_c a_d| + |b_c b_d|"""
    C = re.shape[0]
    a, b = re.astype(dtype), im.astype(dtype)
    P = np.empty((C * C,) + a.shape[1:], dtype)
    Q = np.empty((C * C,) + a.shape[1:], np.float64)
    aa, ab = np.abs(re.astype(np.float64)), np.abs(im.astype(np.float64))
    for c in range(C):
        P[c] = a[c] * a[c] + b[c] * b[c]
        Q[c] = aa[c] * aa[c] + ab[c] * ab[c]
    for i, (c, d) in enumerate(pairs(C)):
        P[C + 2 * i] = a[c] * a[d] + b[c] * b[d]
        P[C + 2 * i + 1] = b[c] * a[d] - a[c] * b[d]
        Q[C + 2 * i] = aa[c] * aa[d] + ab[c] * ab[d]
        Q[C + 2 * i + 1] = ab[c] * aa[d] + aa[c] * ab[d]
    return P, Q


def scm(X, F, stft_frames, masks, S, T, hop, seg, ov=None, long_path=False, dtype=LD):
    """backend_reference.scm for X [C][2 F][T_ld]: (Phi [S + 1][F][C C] of `dtype`, bound [S + 1][F][C C] float64)"""
    C, nm = X.shape[0], S + 1
    re, im, tv = _segment(X, F, stft_frames, seg, T, hop)
    m = masks.reshape(-1, F, masks.shape[-1])[:nm, :, seg * T:seg * T + tv]
    win = winners(m, S, None if ov is None else ov.reshape(-1, F, T)[seg][:, :tv])
    w = np.where(win, m.astype(dtype), dtype(FLOOR_W))
    P, Q = _products(re, im, dtype)
    phi = np.einsum("kft,eft->kfe", w, P)
    phi[:, :, :C] += dtype(DIAG)
    A = np.einsum("kft,eft->kfe", np.where(win, np.abs(m.astype(np.float64)), 0.0), Q)
    B = np.broadcast_to(Q.sum(axis=2).T[None], A.shape)
    K = scm_k(T, long_path)
    diag = np.where(np.arange(C * C) < C, DIAG, 0.0)
    return phi, SECOND * u * (K * (A + diag) + 2 * K * FLOOR_W * B)


def solve(scm_seg, S, F, C, dtype=LD, want_bound=True):
    """backend_reference.solve for scm_seg [S + 1][F][C C]: (W [S][F][C] complex of dtype, bound [S][F][C] or None)"""
    cd = CLD if dtype == LD else np.complex128
    H = unpack(np.asarray(scm_seg).astype(dtype), C)
    W = np.zeros((S, F, C), cd)
    bound = np.zeros((S, F, C)) if want_bound else None
    for spk in range(S):
        for f in range(F):
            A = np.zeros((C, C), cd)
            for j in range(S + 1):
                if j != spk:
                    A = A + H[j, f]
            Z, Lm, Um, perm = lu_solve(A, H[spk, f].copy())
            tr = np.trace(Z) + (dtype(DIAG) if f == 0 else dtype(0))
            W[spk, f] = Z[:, 0] * _cinv(tr)
            if not want_bound:
                continue
            inv, _, _, _ = lu_solve(A, np.eye(C, dtype=cd))
            LU = np.empty((C, C))
            LU[perm] = np.abs(Lm).astype(np.float64) @ np.abs(Um).astype(np.float64)
            Za = np.abs(Z).astype(np.float64)
            dZ = solve_g(C) * np.abs(inv).astype(np.float64) @ LU @ Za
            dtr = np.trace(dZ) + 8 * u * np.trace(Za)
            Wa = np.abs(W[spk, f]).astype(np.float64)
            bound[spk, f] = SECOND * ((dZ[:, 0] + Wa * dtr) / float(np.abs(tr)) + 6 * u * Wa)
    return W, bound


def beamform(X, F, stft_frames, masks, S, T, hop, seg, floor, W):
    """backend_reference.beamform for X [C][2 F][T_ld] and W [S][F][C]: (sep64 [S][F][T][2], bound), the chain's term 2 C u"""
    C = X.shape[0]
    re, im, tv = _segment(X, F, stft_frames, seg, T, hop)
    x = re.astype(np.float64) + 1j * im.astype(np.float64)
    m = np.maximum(masks.reshape(-1, F, masks.shape[-1])[:S, :, seg * T:(seg + 1) * T], f32(floor)).astype(np.float64)
    y = np.einsum("sfc,cft->sft", np.conj(W), x)
    mag = np.einsum("sfc,cft->sft", np.abs(W), np.abs(x))
    out, bound = np.zeros((S, F, T, 2)), np.zeros((S, F, T, 2))
    for i, part in enumerate((y.real, y.imag)):
        out[:, :, :tv, i] = part * m[:, :, :tv]
        bound[:, :, :tv, i] = (2 * C * u * mag + U / 2 * np.abs(part)) * m[:, :, :tv] + U / 2 * np.abs(part * m[:, :, :tv])
    return out, bound


def beamform_plain(X, F, stft_frames, masks, S, T, hop, seg, floor):
    """use_mvdr = 0, bit for bit: microphone 0 times max(mask, floor) in float32"""
    re, im, tv = _segment(X, F, stft_frames, seg, T, hop)
    m = np.maximum(masks.reshape(-1, F, masks.shape[-1])[:S, :, seg * T:(seg + 1) * T], f32(floor))
    out = np.zeros((S, F, T, 2), np.float32)
    out[:, :, :tv, 0] = re[0][None] * m[:, :, :tv]
    out[:, :, :tv, 1] = im[0][None] * m[:, :, :tv]
    return out


# ---- inputs (backend_reference's families with C microphones) -----------------------------------------------------------------------

def planes(family, C, F, T_ld, stft_frames, seed):
    """X [C][2 F][T_ld] float32, NaN from stft_frames on.  'pairs': frame t holds one nonzero microphone pair (c, d) = divmod(t mod
    C C, C), so that every packed entry is told apart"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((C, 2 * F, T_ld)).astype(np.float32)
    if family == "magnitudes":
        X *= (10.0 ** rng.uniform(-6, 3, (1, 1, T_ld))).astype(np.float32)
    elif family == "silent_ref":
        X[0] = 0
    elif family == "silent":
        X[:] = 0
    elif family == "pairs":
        X[:] = 0
        for t in range(T_ld):
            c, d = divmod(t % (C * C), C)
            for mic in {c, d}:
                X[mic, :, t] = f32(1 + (t % (C * C))) * (rng.standard_normal(2 * F) * 0.25 + 1).astype(np.float32)
    elif family != "gaussian":
        raise ValueError(family)
    X[:, :, stft_frames:] = np.nan
    return X


def scm_case(name, C, T, S, F, nseg, seg_lo, hop, short, wide, masks, planes_f, override, seed):
    """backend_reference.scm_cases' record, with C"""
    segs = seg_lo + nseg
    return dict(name=name, C=C, T=T, S=S, F=F, nseg=nseg, seg_lo=seg_lo, hop=hop, stft_frames=(segs - 1) * hop + T - min(short, T),
                T_ld=(segs - 1) * hop + T + 3, mask_ld=segs * T + (5 if wide else 0), masks=masks, planes=planes_f, override=override,
                seed=seed)


SWEEP_T = (1, 16, 63, 64, 65, 186, 192, 193, 256, 257, 511, 512, 513, 600)


def scm_cases():
    """the issue's list.  Sweep in C: every C of {2, 3, 4, 5, 6, 8} at T = 65 and 186.  Sweep in T: C = 2, 4, 8 at every T of
    SWEEP_T (each tile variant's edges and the any-length kernel), S, F, segments, hop, the last segment's missing frames, mask
    family, plane family and override walking their own lists.  Then the shape details by name."""
    cases = []
    for j, C in enumerate((2, 3, 4, 5, 6, 8)):
        for T in (65, 186):
            cases.append(scm_case(f"C{C}_T{T}", C, T, (3, 2, 1)[j % 3], (5, 2)[j % 2], (1, 3)[j % 2], (0, 1)[(j // 2) % 2], (T + 1) // 2,
                                  (0, 1, T - 1)[j % 3], j % 2, MASK_FAMILIES[j % len(MASK_FAMILIES)], ("gaussian", "pairs", "magnitudes")[j % 3],
                                  (None, "index", "bits")[(j + T) % 3], 1000 + 10 * C + (T == 186)))
    planes_f = ("gaussian", "magnitudes", "silent_ref", "pairs", "gaussian", "silent")
    for C in (2, 4, 8):
        for i, T in enumerate(SWEEP_T):
            nseg, seg_lo = ((1, 0), (3, 0), (1, 2), (2, 1))[(i + C) % 4]
            if T > 256:
                nseg = 1          # (the long tiles and the any-length kernel: one segment keeps the case quick)
            short = (0, 1, T - 1, T)[(3 * i + C) % 4] if T > 1 else i % 2
            cases.append(scm_case(f"C{C}_sweep_T{T}", C, T, (3, 2, 1)[(i + C) % 3], (5, 2, 1)[(2 * i) % 3], nseg, seg_lo,
                                  (T, -(-T // 2), 1)[(i + i // 3) % 3], short, i % 2, MASK_FAMILIES[(3 * i + C) % len(MASK_FAMILIES)],
                                  planes_f[(5 * i + i // 6 + C) % len(planes_f)], (None, "index", "bits")[(i + i // 4) % 3], 2000 + 100 * C + i))
    for C in (2, 4, 8):
        cases += [
            scm_case(f"C{C}_F5_S3", C, 186, 3, 5, 2, 0, 93, 0, 0, "random", "gaussian", None, 3000 + C),           # an odd F over two bins per block
            scm_case(f"C{C}_F1_S1", C, 186, 1, 1, 1, 0, 93, 0, 0, "random", "gaussian", None, 3010 + C),
            scm_case(f"C{C}_S2_seglo", C, 65, 2, 2, 2, 3, 33, 0, 1, "random", "magnitudes", None, 3020 + C),        # seg_lo > 0
            scm_case(f"C{C}_short_last", C, 186, 3, 2, 3, 0, 93, 100, 0, "random", "gaussian", None, 3030 + C),     # a short last segment
            scm_case(f"C{C}_empty_last", C, 65, 2, 2, 2, 0, 65, 65, 0, "random", "gaussian", None, 3040 + C),       # a segment with no valid frame
            scm_case(f"C{C}_tied", C, 193, 3, 2, 2, 0, 97, 1, 1, "tied_fourth", "gaussian", None, 3050 + C),        # ties on audible planes
            scm_case(f"C{C}_all_equal", C, 186, 2, 2, 1, 0, 93, 0, 0, "all_equal", "magnitudes", None, 3060 + C),
            scm_case(f"C{C}_index", C, 186, 3, 2, 1, 1, 93, 0, 0, "all_equal", "gaussian", "index", 3070 + C),
            scm_case(f"C{C}_bits", C, 256, 3, 1, 1, 0, 256, 0, 0, "tied_fourth", "pairs", "bits", 3080 + C),
            scm_case(f"C{C}_pairs_S1", C, 186, 1, 2, 1, 0, 93, 0, 0, "tied_fourth", "pairs", None, 3090 + C),
            scm_case(f"C{C}_pairs_S3", C, 186, 3, 2, 1, 0, 93, 0, 0, "ulp_apart", "pairs", None, 3100 + C),
        ]
    return cases


SCM_FORCED = tuple((C, T) for C in (2, 4, 8) for T in (16, 186, 257))      # tuned against any-length on the same input


def scm_case_arrays(c):
    segs = c["seg_lo"] + c["nseg"]
    X = planes(c["planes"], c["C"], c["F"], c["T_ld"], c["stft_frames"], c["seed"])
    M = mask_rows(c["masks"], c["S"], c["F"], c["mask_ld"], c["seg_lo"], c["nseg"], c["T"], c["seed"] + 1)
    ov = None if c["override"] is None else override_bytes(c["override"], c["S"], c["F"], segs, c["T"], c["seed"] + 2)
    return X, M, ov


def covariances(family, C, S, F, seed, T=64, scale=1.0, winners_n=None):
    """backend_reference.covariances with C microphones: [S + 1][F][C C] float64 of one segment"""
    rng = np.random.default_rng(seed)
    nm = S + 1
    if family == "silent":
        out = np.zeros((nm, F, C * C))
        out[:, :, :C] = DIAG
        return out
    Tn = winners_n if family == "rank" else T
    x = (rng.standard_normal((C, F, Tn)) + 1j * rng.standard_normal((C, F, Tn))) * scale
    if family == "pivot":
        x[0] = 0
    if family == "quiet_ref":
        x[0] *= 1e-7
    m = rng.uniform(0.01, 1.0, (nm, F, Tn))
    w = np.where(m == m.max(axis=0, keepdims=True), m, FLOOR_W)
    out = np.zeros((nm, F, C * C))
    for k in range(nm):
        R = np.einsum("ft,cft,dft->fcd", w[k], x, np.conj(x))
        for c in range(C):
            out[k, :, c] = R[:, c, c].real + DIAG
        for i, (c, d) in enumerate(pairs(C)):
            out[k, :, C + 2 * i], out[k, :, C + 2 * i + 1] = R[:, c, d].real, R[:, c, d].imag
    return out


def solve_cases():
    """the families of backend_reference.solve_cases at C = 2, 4, 8 with S = 1 .. 3 and F = 5 / 1; complete: every system must be
    judged (checked on the CPU for these seeds by tests/test_mic_arrays_host.py)"""
    cases = []
    for C in (2, 4, 8):
        for i, scale in enumerate((1e-3, 1.0, 1e3)):
            cases.append(dict(name=f"C{C}_well_x{scale:g}", C=C, family="well", complete=True, S=(1, 2, 3)[(i + C) % 3], F=(5, 1)[i % 2],
                              T=(64, 186)[i % 2], scale=scale, winners_n=None, seed=4000 + 10 * C + i))
        for S in (1, 2, 3):
            cases.append(dict(name=f"C{C}_quiet_ref_S{S}", C=C, family="quiet_ref", complete=False, S=S, F=5, T=64, scale=1.0,
                              winners_n=None, seed=4100 + 10 * C + S))
        cases.append(dict(name=f"C{C}_silent", C=C, family="silent", complete=False, S=(3, 1, 2)[C % 3], F=(1, 5)[C % 2], T=64, scale=1.0,
                          winners_n=None, seed=4200 + C))
        for j, n in enumerate((1, C - 1)):
            cases.append(dict(name=f"C{C}_rank{n}_{j}", C=C, family="rank", complete=False, S=(3, 2)[j], F=5, T=64, scale=1.0, winners_n=n,
                              seed=4300 + 10 * C + j))
    return cases


def solve_case_scm(c, nseg=1):
    """[nseg][S + 1][F][C C]"""
    return np.stack([covariances(c["family"], c["C"], c["S"], c["F"], c["seed"] + 17 * s, c["T"], c["scale"], c["winners_n"])
                     for s in range(nseg)])
