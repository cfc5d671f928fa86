"""Float64 references of the non-GEMM kernels of the mask estimator (csrc/encoder.hip), written from the definitions in
conformer.py as oracle/css_oracle.py states them, the error bounds the kernels are held to, and the seeded case tables.  No
GPU, no library: tests/test_encoder_reference.py checks this file on the CPU (oracle tie, float32 evaluation inside every
bound, every mutation caught), tests/test_hip_encoder_kernels.py holds the kernels to it.

Every reference takes `dtype` (float64: the reference; float32: the oracle's formulas in numpy's float32 arithmetic, used to
show that a bound is reachable) and `mut`, the name of one deliberate defect (None: the definition) -- the mutations show
that a bound is not vacuous.  Rows are [nseg * T][D], segments adjacent in memory.

Constants of the bounds (nothing here is fitted to what a kernel returns):
  U        2^-24, the unit roundoff of float32 (one correctly rounded operation: |fl(a op b) - (a op b)| <= U |a op b|)
  TINY     2^-126, the smallest normal float32: v_exp_f32 and the library expf flush results below it to zero
  SUM_OPS  14: roundings on the path of one element through a row sum of D <= 1024 values as encoder.hip forms it -- at most
           4 float4 per lane, each (x + y) + (z + w) then s += (2 + 4 roundings), four DPP steps and two levels over the
           four row totals in wave_sum (6), the product with 1.0f / D (1), and 1 / D itself, not a power of two at D = 768 (1)
  EXP_ARG  6e-8 |z|: what encoder.hip's comments state for the rounding of the exponent's argument in front of v_exp_f32 (the
           conv module's gate: "the argument's rounding adds |z| * 6e-8"; the softmax: "|arg| * 6e-8 relative")
  ENVELOPE 1.5e-6 (tests/test_hip_gemm.py, gemm_reference.ENVELOPE): error of a float32-accumulated dot product relative
           to the sum of its absolute terms
  SPLIT_OP 2^-22: one split-f16 operand (hi + lo 2^-11 carries 22 bits; split_f16.hpp), also the dropped lo * lo product
  SPLIT_ST 2^-21: a value stored in the split format and decoded again (gemm_reference.value_bound), relative, for
           |x| >= 2^-14; SPLIT_FLOOR 2^-26 absolute below that (split_f16.hpp: hi is zero there, lo alone carries 11 bits)
"""
import numpy as np

from gemm_reference import ENVELOPE, split_decode, split_encode  # noqa: F401  (re-exported for the tests)

U = 2.0 ** -24
TINY = 2.0 ** -126
SUM_OPS = 14
EXP_ARG = 6e-8
SPLIT_OP = 2.0 ** -22
SPLIT_ST = 2.0 ** -21
SPLIT_FLOOR = 2.0 ** -26      # below 2^-14 the hi half is zero and lo = f16(x 2^11) carries 11 bits: 2^-12 |x| < 2^-26, absolute
SIGMOID_LIB = 2.0 ** -21      # expf, one add, one divide at a few ulp (gemm_reference.value_bound's r for the sigmoid)
SIGMOID_HW = 5 * U            # v_exp_f32 and v_rcp_f32 "1 ulp each" (2 U each, encoder.hip) and the add between them
LN_EPS = 1e-5


# ---- references ---------------------------------------------------------------------------------------------------------------

def layer_norm(x, w, b, dtype=np.float64, mut=None):
    """nn.LayerNorm over the last axis: biased variance, eps 1e-5 (conformer.py:48,98,137,170,207)"""
    x, w, b = np.asarray(x, dtype), np.asarray(w, dtype), np.asarray(b, dtype)
    d = x.shape[-1]
    mu = x.mean(-1, keepdims=True, dtype=dtype)
    xc = x - mu
    var = (xc * xc).sum(-1, keepdims=True, dtype=dtype) / dtype(d - 1 if mut == "var_dm1" else d)
    eps = dtype(1e-6 if mut == "eps_1e-6" else LN_EPS)
    return xc / np.sqrt(var + eps) * w + b


def _sigmoid(g, dtype):
    with np.errstate(over="ignore"):
        return dtype(1.0) / (dtype(1.0) + np.exp(-g))


def glu(u, pw, dtype=np.float64, mut=None):
    """scalar Conv2d(1, 2, 1) + GLU (conformer.py:100,116-117): (pw0 u + pw1) sigmoid(pw2 u + pw3)"""
    u, pw = np.asarray(u, dtype), np.asarray(pw, dtype)
    a, g = u * pw[0] + pw[1], u * pw[2] + pw[3]
    if mut == "glu_swapped":
        a, g = g, a
    return a * _sigmoid(g, dtype)


def ln_glu(x, w, b, pw, dtype=np.float64, mut=None):
    return glu(layer_norm(x, w, b, dtype, mut), pw, dtype, mut)


def dwconv_tail(z, h, wt, dwb, alpha, beta, pw, nseg, T, dtype=np.float64, mut=None):
    """Depthwise conv over time inside each segment (zero padding at the segment edges), folded eval BatchNorm, ReLU, scalar
    Conv2d(1, 1, 1), residual (conformer.py:119-126):  h + pw4 relu((conv(z) + b) alpha + beta) + pw5.   wt [taps][D]."""
    z, h, wt = np.asarray(z, dtype), np.asarray(h, dtype), np.asarray(wt, dtype)
    dwb, alpha, beta, pw = np.asarray(dwb, dtype), np.asarray(alpha, dtype), np.asarray(beta, dtype), np.asarray(pw, dtype)
    taps, D = wt.shape
    pad = (taps - 1) // 2
    if mut == "taps_reversed":
        wt = wt[::-1]
    zs = z.reshape(nseg, T, D)
    if mut == "pad_neighbour":   # the padding frames taken from the neighbouring segments (zero only at the two outer ends)
        flat = np.concatenate([np.zeros((pad, D), dtype), z.reshape(nseg * T, D), np.zeros((pad, D), dtype)])
        zp = np.stack([flat[s * T:s * T + T + 2 * pad] for s in range(nseg)])
    else:
        zp = np.zeros((nseg, T + 2 * pad, D), dtype)
        zp[:, pad:pad + T] = zs
    conv = np.zeros((nseg, T, D), dtype)
    for k in range(taps):
        conv += zp[:, k:k + T] * wt[k]
    if mut == "relu_first":
        y = np.maximum(conv + dwb, 0) * alpha + beta
    else:
        y = np.maximum((conv + dwb) * alpha + beta, 0)
    add = y * pw[4] + (dtype(0) if mut == "no_pw5" else pw[5])
    res = h.reshape(nseg, T, D)
    if mut == "residual_next":   # frame t takes the residual of frame t + 1 (the last frame of a segment its own)
        res = np.concatenate([res[:, 1:], res[:, -1:]], axis=1)
    return (res + add).reshape(nseg * T, D)


def conv_module(x, ln_w, ln_b, pw, wt, dwb, alpha, beta, nseg, T, dtype=np.float64, mut=None):
    """conformer.py:113-127 from LayerNorm to the residual"""
    z = ln_glu(x, ln_w, ln_b, pw, dtype, mut)
    return dwconv_tail(z, x, wt, dwb, alpha, beta, pw, nseg, T, dtype, mut)


def rel_index(T, maxlen, mut=None):
    """[T][T] rows of the table pe [2 maxlen][dk] (one zero row appended at 2 maxlen): clip(i - j, -maxlen, maxlen - 1) + maxlen
    (conformer.py:24-29,229-233)"""
    ii = np.arange(T)
    off = ii[:, None] - ii[None, :]
    if mut == "offset_plus":
        off = off + 1
    if mut == "offset_minus":
        off = off - 1
    if mut == "clamp_symmetric":
        return np.clip(off, -maxlen, maxlen) + maxlen          # row 2 maxlen is past the table: the appended zeros
    if mut == "no_clamp":
        return (off + maxlen) % (2 * maxlen)
    return np.clip(off, -maxlen, maxlen - 1) + maxlen


def _heads(a, nseg, T, H):
    return a.reshape(nseg, T, H, 64).transpose(0, 2, 1, 3)     # [nseg][H][T][64]


def relpos_attention(q, k, v, pe, nseg, T, H, maxlen, dtype=np.float64, mut=None, parts=False):
    """ctx [nseg T][64 H]: softmax_j((q_i . k_j + q_i . pe[rel(i, j)]) / sqrt(64)) v_j per segment and head (conformer.py:65-92).
    parts: also the probabilities p and the exponent arguments s - max, [nseg][H][T][T]."""
    q, k, v = (_heads(np.asarray(a, dtype), nseg, T, H) for a in (q, k, v))
    pe = np.concatenate([np.asarray(pe, dtype).reshape(2 * maxlen, 64), np.zeros((1, 64), dtype)])
    rel = rel_index(T, maxlen, mut)
    a = q @ k.transpose(0, 1, 3, 2)
    b = np.take_along_axis(q @ pe.T, np.broadcast_to(rel, a.shape), axis=3)
    s = (a + b) / dtype(np.sqrt(63.0 if mut == "scale_63" else 64.0))
    with np.errstate(over="ignore", invalid="ignore"):
        if mut == "no_max":    # exp of the raw score, in float32's range
            arg = s
            e = np.exp(s.astype(np.float32)).astype(dtype)
        else:
            arg = s - s.max(-1, keepdims=True)
            e = np.exp(arg)
        den = e.sum(-1, keepdims=True, dtype=dtype)
        if mut == "unmasked_keys":   # the keys of the last 32-key tile past T: score 0, value 0
            den = den + dtype(-T % 32) * np.exp(-s.max(-1, keepdims=True))
        p = e / den
        ctx = (p @ v).transpose(0, 2, 1, 3).reshape(nseg * T, H * 64)
    return (ctx, p, arg) if parts else ctx


# ---- bounds -------------------------------------------------------------------------------------------------------------------

def layer_norm_bound(x, w, b):
    """(y64, bound) of y = LN(x; w, b) as layernorm_kernel forms it: mean = sum / D, v = x - mean, var = sum(v v) / D,
    rstd = 1 / sqrt(var + eps), y = v rstd w + b.  With xc = x - mu, sigma2 = var + eps in float64:
      d_mu  <= SUM_OPS U mean|x|                       the row sum's roundings: the row's condition mean|x| / sigma once
                                                       multiplied by rstd below
      d_v   <= U |xc| + d_mu                           (d_mu is the same for the whole row)
      d_var <= (SUM_OPS + 2) U var + d_mu^2            the squares' and the sum's roundings and 2 U var from U |xc|; the
                                                       uniform shift d_mu enters in second order only (sum xc = 0)
      rstd: relative d_var / (2 sigma2) + 3 U          the add of eps, sqrtf and the division, correctly rounded
      y: |w| rstd d_v + |xc| rstd |w| (rel rstd + 2 U) + U |y|     two products and the add of b (or one fma)"""
    x64, w64, b64 = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(b, np.float64)
    mu = x64.mean(-1, keepdims=True)
    xc = x64 - mu
    var = (xc * xc).mean(-1, keepdims=True)
    sigma2 = var + LN_EPS
    rstd = 1.0 / np.sqrt(sigma2)
    y = xc * rstd * w64 + b64
    d_mu = SUM_OPS * U * np.abs(x64).mean(-1, keepdims=True)
    rel_rstd = ((SUM_OPS + 2) * U * var + d_mu ** 2) / (2 * sigma2) + 3 * U
    bound = np.abs(w64) * rstd * (U * np.abs(xc) + d_mu) + np.abs(xc) * rstd * np.abs(w64) * (rel_rstd + 2 * U) + U * np.abs(y)
    return y, bound


def glu_bound(u, d_u, pw, hw):
    """(y64, bound) of y = a s, a = pw0 u + pw1, s = sigmoid(g), g = pw2 u + pw3, for an input known to d_u:
      d_a <= |pw0| d_u + U (|pw0 u| + |pw1|),  d_g likewise
      d_s <= d_g / 4 + s r + TINY      the sigmoid's Lipschitz constant 1/4; r = SIGMOID_LIB for expf and a division
                                       (layernorm_kernel), SIGMOID_HW + EXP_ARG |g| for v_exp_f32 / v_rcp_f32
                                       (conv_module_kernel); TINY: a gate below the smallest normal is flushed to zero
      d_y <= |a| d_s + s d_a + U |y|"""
    u64, pw64 = np.asarray(u, np.float64), np.asarray(pw, np.float64)
    a, g = pw64[0] * u64 + pw64[1], pw64[2] * u64 + pw64[3]
    s = _sigmoid(g, np.float64)
    y = a * s
    d_a = abs(pw64[0]) * d_u + U * (np.abs(pw64[0] * u64) + abs(pw64[1]))
    d_g = abs(pw64[2]) * d_u + U * (np.abs(pw64[2] * u64) + abs(pw64[3]))
    r = SIGMOID_HW + EXP_ARG * np.abs(g) if hw else SIGMOID_LIB
    d_s = d_g / 4 + s * r + TINY
    return y, np.abs(a) * d_s + s * d_a + U * np.abs(y)


def ln_glu_bound(x, w, b, pw, hw=False):
    u, d_u = layer_norm_bound(x, w, b)
    return glu_bound(u, d_u, pw, hw)


def dwconv_tail_bound(z, d_z, h, wt, dwb, alpha, beta, pw, nseg, T):
    """(y64, bound) of dwconv_tail for GLU rows z known to d_z:
      conv: taps fused multiply-adds in a chain: taps U sum_k |w_k| |z_k| + sum_k |w_k| d_z_k
      c = conv + b (U |c|), n = c alpha + beta (U |c alpha| + U |n|), ReLU (Lipschitz 1),
      add = pw4 relu + pw5 (U |pw4 relu| + U |add|), out = h + add (U |out|)"""
    z64, wt64 = np.asarray(z, np.float64), np.asarray(wt, np.float64)
    taps, D = wt64.shape
    pad = (taps - 1) // 2
    y = dwconv_tail(z64, h, wt, dwb, alpha, beta, pw, nseg, T)
    az = np.zeros((nseg, T + 2 * pad, D))
    dz = np.zeros((nseg, T + 2 * pad, D))
    az[:, pad:pad + T] = np.abs(z64).reshape(nseg, T, D)
    dz[:, pad:pad + T] = np.broadcast_to(d_z, z64.shape).reshape(nseg, T, D)
    zp = np.zeros((nseg, T + 2 * pad, D))
    zp[:, pad:pad + T] = z64.reshape(nseg, T, D)
    conv, mag, carried = np.zeros((nseg, T, D)), np.zeros((nseg, T, D)), np.zeros((nseg, T, D))
    for k in range(taps):
        conv += zp[:, k:k + T] * wt64[k]
        mag += az[:, k:k + T] * np.abs(wt64[k])
        carried += dz[:, k:k + T] * np.abs(wt64[k])
    al, be, pw64 = np.asarray(alpha, np.float64), np.asarray(beta, np.float64), np.asarray(pw, np.float64)
    c = conv + np.asarray(dwb, np.float64)
    n = c * al + be
    add = pw64[4] * np.maximum(n, 0) + pw64[5]
    d_c = taps * U * mag + carried + U * np.abs(c)
    d_n = np.abs(al) * d_c + U * np.abs(c * al) + U * np.abs(n)
    d_add = abs(pw64[4]) * d_n + U * np.abs(pw64[4] * np.maximum(n, 0)) + U * np.abs(add)
    bound = (d_add + U * np.abs(y.reshape(nseg, T, D))).reshape(nseg * T, D)
    return y, bound


def conv_module_bound(x, ln_w, ln_b, pw, wt, dwb, alpha, beta, nseg, T, hw):
    """hw: the fused kernel's gate (v_exp_f32 / v_rcp_f32), else the two-kernel form's (expf, division)"""
    z, d_z = ln_glu_bound(x, ln_w, ln_b, pw, hw)
    return dwconv_tail_bound(z, d_z, x, wt, dwb, alpha, beta, pw, nseg, T)


def attention_keys_ops(T):
    """c of the context bound: roundings on an element's path through the T-term sums -- the P.V accumulation (T / 2 two-product
    MFMA steps per lane half, or T fused multiply-adds in the any-length kernel: T), the row sum of the probabilities (16 per
    key tile and lane half, T / 64 per lane in the any-length kernel, plus the cross-lane steps: T / 2 + T / 64 + 8, enters
    through 1 / sum), the reciprocal and the final product (2)"""
    return T + T // 2 + T // 64 + 10


def attention_bound(q, k, v, pe, nseg, T, H, maxlen, split=False, split_out=False, d_q=None, d_k=None, lib_exp=False):
    """(ctx64, bound).  With p the float64 probabilities, arg = s - max the exponent's argument and
      e_ij  = ENVELOPE (|q_i|.|k_j| + |q_i|.|pe_rel(i,j)|) / 8       the score's error (the GEMM envelope of test_hip_gemm.py)
              + (d_q.|k_j| + |q_i|.d_k_j + d_q.|pe_rel|) / 8          q and k known to d_q, d_k only (a rounded QKV product)
              + 3 SPLIT_OP (|q|.|k| + |q|.|pe|) / 8                   split mode: both operands and the dropped lo * lo
      eps_ij = e_ij + EXP_ARG |arg_ij| + 4 U                          relative error of exp(.): the argument's rounding as
                                                                      the kernel's comment states it, v_exp_f32 / expf and
                                                                      the subtraction; an error of the maximum scales a whole
                                                                      row and cancels in the normalisation
    ctx_id = sum_j p_ij v_jd / sum_j p_ij moves by at most sum_j p_ij eps_ij (|v_jd| + |ctx_id|) -- at most
    2 max_j eps_ij sum_j p_ij |v_jd| -- plus (c U [+ 3 SPLIT_OP: p and v as split operands, lo * lo dropped])
    sum_j p_ij |v_jd| for the sums (attention_keys_ops), U |ctx| for the store [SPLIT_ST |ctx| for a split row], and TINY."""
    ctx, p, arg = relpos_attention(q, k, v, pe, nseg, T, H, maxlen, parts=True)
    aq, ak, av = (_heads(np.abs(np.asarray(a, np.float64)), nseg, T, H) for a in (q, k, v))
    ape = np.abs(np.asarray(pe, np.float64).reshape(2 * maxlen, 64))
    rel = np.broadcast_to(rel_index(T, maxlen), p.shape)
    terms = aq @ ak.transpose(0, 1, 3, 2) + np.take_along_axis(aq @ ape.T, rel, axis=3)
    e = (ENVELOPE + (3 * SPLIT_OP if split else 0.0)) * terms / 8
    if d_q is not None:
        dq, dk = _heads(np.asarray(d_q, np.float64), nseg, T, H), _heads(np.asarray(d_k, np.float64), nseg, T, H)
        e = e + (dq @ ak.transpose(0, 1, 3, 2) + aq @ dk.transpose(0, 1, 3, 2) + np.take_along_axis(dq @ ape.T, rel, axis=3)) / 8
    eps = e + EXP_ARG * np.abs(arg) + 4 * U
    pe_ = p * eps
    actx = np.abs(_heads(ctx, nseg, T, H))
    pv = p @ av
    bound = pe_ @ av + pe_.sum(-1, keepdims=True) * actx + (attention_keys_ops(T) * U + (3 * SPLIT_OP if split else 0.0)) * pv
    bound = bound + ((SPLIT_ST if split_out else 0.0) + U) * actx + TINY + (SPLIT_FLOOR if split_out else 0.0)
    return ctx, bound.transpose(0, 2, 1, 3).reshape(nseg * T, H * 64)


# ---- case tables (seeded; both test files read them, so the CPU checks run on exactly the GPU tests' inputs) ----------------------

LN_WIDTHS = (256, 512, 768, 1024)
LN_ROWS = (1, 3, 4, 5, 130)
LN_FAMILIES = ("gaussian", "constant", "offset", "wide", "outlier", "quiet")
PW_MILD = (0.8, 0.1, 1.1, -0.2, 1.3, -0.2)
PW_WIDE = (0.8, 0.1, 40.0, 0.5, 1.3, -0.2)      # gate arguments over +-100 and beyond: past float32 exp overflow on both sides


def ln_case(rows, D, seed=0):
    """x [rows][D], row r of family LN_FAMILIES[(r + seed) % 6], and two sets of LayerNorm weights"""
    rs = np.random.RandomState(1000 * seed + 7 * rows + D)
    x = rs.standard_normal((rows, D))
    for r in range(rows):
        fam = LN_FAMILIES[(r + seed) % 6]
        if fam == "constant":
            x[r] = rs.uniform(-2, 2)                    # variance 0: eps alone decides
        elif fam == "offset":
            x[r] = 1e3 + 1e-2 * x[r]                    # mean 1e3, sigma 1e-2
        elif fam == "wide":
            x[r] = rs.uniform(-1e3, 1e3, D)             # |x| up to 1e3 (the trained-like regime)
        elif fam == "outlier":
            x[r, rs.randint(D)] = 300.0
        elif fam == "quiet":
            x[r] = 1e-3 * x[r]                          # variance 1e-6, below eps: eps decides the scale (not in the issue's list;
                                                        # a constant row is b whatever eps is, so it cannot tell 1e-5 from 1e-6)
    w = [(1.0 + 0.3 * rs.standard_normal(D)).astype(np.float32) for _ in range(2)]
    b = [(0.3 * rs.standard_normal(D)).astype(np.float32) for _ in range(2)]
    return dict(rows=rows, D=D, x=x.astype(np.float32), w=w[0], b=b[0], w2=w[1], b2=b[1])


def ln_cases():
    return [ln_case(rows, D, seed=i) for i, (D, rows) in enumerate((D, r) for D in LN_WIDTHS for r in LN_ROWS)]


CONV_T = (1, 2, 15, 16, 17, 30, 31, 32, 33, 61, 62, 63, 186, 187)


def conv_case(D, taps, nseg, T, seed=0, impulse=None):
    """segments adjacent in memory with different content, random asymmetric taps; impulse = t: one non-zero frame, frame t of
    the middle segment"""
    rs = np.random.RandomState(100 * seed + D + 13 * taps + 7 * nseg + T)
    x = rs.standard_normal((nseg, T, D)) * (1.0 + np.arange(nseg))[:, None, None] + 0.5 * np.arange(nseg)[:, None, None]
    if impulse is not None:
        x[:] = 0.0
        x[nseg // 2, impulse] = 3.0 * rs.standard_normal(D)
    f = lambda a: a.astype(np.float32)
    return dict(D=D, taps=taps, nseg=nseg, T=T, x=f(x.reshape(nseg * T, D)),
                ln_w=f(1.0 + 0.3 * rs.standard_normal(D)), ln_b=f(0.3 * rs.standard_normal(D)), pw=np.array(PW_MILD, np.float32),
                wt=f(rs.standard_normal((taps, D)) * 0.3 + 0.02 * np.arange(taps)[:, None]), dwb=f(0.2 * rs.standard_normal(D)),
                alpha=f(1.0 + 0.3 * rs.standard_normal(D)), beta=f(0.3 * rs.standard_normal(D)),
                ln2_w=f(1.0 + 0.3 * rs.standard_normal(D)), ln2_b=f(0.3 * rs.standard_normal(D)))


def conv_cases(fused):
    """(D, taps, nseg, T, impulse) of every case of one form.  Fused: D in {256, 512}, 33 taps; two-kernel: D in {256, 768, 1024},
    taps in {17, 31, 33}.  Every T of CONV_T with nseg 1 and 3 alternating over (D, taps); nseg 9 once (a grid that is neither a
    multiple of 8 nor below it); one impulse at each end of the middle segment."""
    forms = [(256, 33), (512, 33)] if fused else [(256, 17), (768, 31), (1024, 33), (256, 33)]
    out = []
    for i, T in enumerate(CONV_T):
        D, taps = forms[i % len(forms)]
        out.append((D, taps, 3 if i % 2 == 0 else 1, T, None))
        D, taps = forms[(i + 1) % len(forms)]
        out.append((D, taps, 1 if i % 2 == 0 else 3, T, None))
    D, taps = forms[0]
    out.append((D, taps, 9, 33, None))
    out.append((D, taps, 3, 63, 0))
    out.append((forms[1][0], forms[1][1], 3, 63, 62))
    return out


ATT_FAMILIES = ("gaussian", "peaky", "mag30", "position")


def att_case(family, nseg, T, D, maxlen, seed=0, delta=0):
    """q, k, v [nseg T][D] and the table pe [2 maxlen][64], float32.
      gaussian  O(1) everywhere
      peaky     q, k ~ 4 N(0, 1): scores of +-40 and more after the division, one key carries a row
      mag30     |q|, |k| in [15, 30]: the split format's range
      position  k = 0, one q for every query, a table with one dominant row at offset delta (clamped as the definition clamps):
                ctx_i = v_{i - delta} wherever i - delta is a key, uniform elsewhere"""
    rs = np.random.RandomState(10007 * seed + 31 * T + nseg + D + maxlen + 3 * ATT_FAMILIES.index(family))
    H = D // 64
    q, k, v = (rs.standard_normal((nseg * T, D)) for _ in range(3))
    pe = 0.5 * rs.standard_normal((2 * maxlen, 64))
    if family == "peaky":
        q, k = 4 * q, 4 * k
    elif family == "mag30":
        q = np.sign(q) * rs.uniform(15, 30, q.shape)
        k = np.sign(k) * rs.uniform(15, 30, k.shape)
    elif family == "position":
        qh = rs.standard_normal((H, 64))
        qh /= np.linalg.norm(qh, axis=1, keepdims=True)
        q = np.broadcast_to(qh.reshape(1, D), (nseg * T, D)) * 8.0
        k = np.zeros_like(k)
        pe = np.zeros((2 * maxlen, 64))
        row = int(np.clip(delta, -maxlen, maxlen - 1)) + maxlen
        pe[row] = 40.0 * np.linalg.lstsq(qh, np.ones(H), rcond=None)[0]        # q_h . pe[row] / 8 = 40 for every head
    f = lambda a: np.ascontiguousarray(a, np.float32)
    return dict(family=family, nseg=nseg, T=T, D=D, H=H, maxlen=maxlen, delta=delta, q=f(q), k=f(k), v=f(v), pe=f(pe))


def att_identity_operands(case):
    """x = [q | k | v] (K = 3 D), w = the identity, bias = 0: the float32 product is exact, the split one exact to the format"""
    D = case["D"]
    return np.concatenate([case["q"], case["k"], case["v"]], axis=1), np.eye(3 * D, dtype=np.float32), np.zeros(3 * D, np.float32)


def att_short_cases():
    """(family, nseg, T, D, maxlen, delta) of modes 0 and 1: for every NJT = 1 .. 16 the lengths 32 (NJT - 1) + 1, 32 NJT - 5 and
    32 NJT, plus T = 2, 186, 249, 499 at (256, 4); (512, 8) and (768, 12) at T in {33, 186}; nseg in {1, 3, 5}; maxlen in
    {16, T - 1, T, T + 1, 1000}; the families in turn; the position family at every delta of POSITION_DELTAS."""
    out = []
    lengths = sorted({t for n in range(1, 17) for t in (32 * (n - 1) + 1, 32 * n - 5, 32 * n)} | {2, 186, 249, 499})
    lengths = [t for t in lengths if t >= 2]   # (T = 1: css_make_run_cfg refuses a one-frame segment, so do modes 0 and 1)
    for i, T in enumerate(lengths):
        maxlen = (16, max(T - 1, 1), T, T + 1, 1000)[i % 5]
        out.append((ATT_FAMILIES[i % 3], (1, 3, 5)[i % 3] if T <= 256 else (1, 3)[i % 2], T, 256, maxlen, 0))
    for D in (512, 768):
        out.append(("gaussian", 3, 33, D, 1000, 0))
        out.append(("peaky", 1, 186, D, 100, 0))
    out.append(("gaussian", 5, 186, 256, 1000, 0))
    for T, maxlen in ((186, 1000), (99, 98), (130, 16)):
        for d in position_deltas(T, maxlen):
            out.append(("position", 1, T, 256, maxlen, d))
    return out


def position_deltas(T, maxlen):
    ds = [0]
    for d in (1, 31, 32, 33, 95, 96, 97, T - 1):
        if d <= T - 1:
            ds += [d, -d]
    ds += [maxlen + 3, -(maxlen + 3)]   # beyond maxlen: the clamp decides
    return sorted(set(ds))


ATT_LONG_T = (1, 7, 33, 64, 65, 200, 513, 801, 1603)


def att_long_cases():
    """mode 2: 16, 8 and 4 queries per block with tails T mod nq != 0 and nv mod 4 != 0"""
    out = []
    for i, T in enumerate(ATT_LONG_T):
        maxlen = (16, max(T - 1, 1), T + 1, 1000)[i % 4]
        out.append((ATT_FAMILIES[i % 3], 3 if T <= 200 else 1, T, 256, maxlen, 0))
    for d in (0, 1, -1, 33, -33, 199, -199, 19, -19):
        out.append(("position", 1, 200, 256, 16, d))
    out.append(("gaussian", 2, 65, 512, 1000, 0))
    return out
