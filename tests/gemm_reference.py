"""Float64 reference of one GEMM launch with its epilogue (GemmArgs, csrc/kernels.hpp), the error bound the kernels are held
to, and the split-f16 row format of csrc/split_f16.hpp in numpy.  No GPU, no library: tests/test_gemm_reference.py checks this
file on the CPU, tests/test_hip_gemm_epilogue.py holds the kernels to it.

A launch is described by a dict `desc` with the keys Handle.gemm (_lib.py) takes; the reference reads
    act       0 none, 1 ReLU, 2 sigmoid
    bias      None, "n" (one value per output column) or "m" (one per output row)
    residual  None, "separate" or "inplace"
    alpha     float (only with a residual)
and operands a [batch or 1][M][K], b [batch or 1][N][K] (a 2-d operand is shared by the batch entries), bias [N] or [M],
res [M][N] (shared by the batch entries, as GemmArgs::residual is)."""
import numpy as np

ACT_NONE, ACT_RELU, ACT_SIGMOID = 0, 1, 2
ENVELOPE = 1.5e-6   # pre-activation error relative to the sum of the absolute terms (tests/test_hip_gemm.py)


def _parts(desc, a, b, bias, res):
    a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a64.ndim == 2:
        a64 = a64[None]
    if b64.ndim == 2:
        b64 = b64[None]
    acc = np.matmul(a64, np.swapaxes(b64, 1, 2))                              # [batch][M][N]
    scale = np.matmul(np.abs(a64), np.swapaxes(np.abs(b64), 1, 2))           # sum of |terms| per output
    kind = desc.get("bias")
    if kind is not None:
        b1 = np.asarray(bias, np.float64)
        b1 = b1[None, None, :] if kind == "n" else b1[None, :, None]
        acc = acc + b1
        scale = scale + np.abs(b1)
    act = desc.get("act", ACT_NONE)
    if act == ACT_RELU:
        v = np.maximum(acc, 0.0)
    elif act == ACT_SIGMOID:
        v = 1.0 / (1.0 + np.exp(-acc))
    else:
        v = acc
    if desc.get("residual") is not None:
        alpha = float(desc.get("alpha", 1.0))
        r64 = np.asarray(res, np.float64)[None]
        y = r64 + alpha * v
    else:
        alpha, r64, y = 1.0, np.zeros((1, 1, 1)), v
    return y, scale, v, alpha, r64


def reference(desc, a, b, bias=None, res=None):
    """(y64, scale): y64 = res + alpha * act(a @ b.T + bias) in float64, [batch][M][N]; scale = |a| @ |b|.T + |bias|, the sum of
    the absolute terms of every pre-activation value (_case in tests/test_hip_gemm.py)."""
    y, scale, _, _, _ = _parts(desc, a, b, bias, res)
    return y, scale


def value_bound(desc, a, b, bias=None, res=None, split=None):
    """|y - y64| <= |alpha| L 1.5e-6 scale + r |y64| + 2^-22 (|res| + |alpha v64|), every term derived:
      * 1.5e-6 scale: the pre-activation envelope of the float32 accumulation (test_hip_gemm.py), carried through the
        activation by its Lipschitz constant L (1 for none / ReLU, 1/4 for the sigmoid) and through the residual by |alpha|;
      * r |y64|: the activation's own rounding -- expf, one add and one divide at a few ulp for the sigmoid (r = 2^-21), one
        rounding otherwise (r = 2^-23);
      * 2^-22 (|res| + |alpha v64|): the product alpha * v and the sum with the residual, half an ulp each.
    split: a boolean mask over the N output columns that leave in the split-f16 format; they add 2^-21 |y64| (the format)."""
    return reference_and_bound(desc, a, b, bias, res, split)[2]


def reference_and_bound(desc, a, b, bias=None, res=None, split=None):
    """(y64, scale, bound) of reference() and value_bound() from one evaluation"""
    y, scale, v, alpha, r64 = _parts(desc, a, b, bias, res)
    sig = desc.get("act", ACT_NONE) == ACT_SIGMOID
    lip, r = (0.25, 2.0 ** -21) if sig else (1.0, 2.0 ** -23)
    bound = abs(alpha) * lip * ENVELOPE * scale + r * np.abs(y) + 2.0 ** -22 * (np.abs(r64) + np.abs(alpha * v))
    if split is not None:
        bound = bound + np.where(np.asarray(split, bool)[None, None, :], 2.0 ** -21, 0.0) * np.abs(y)
    return y, scale, bound


# ---- split-f16 rows (split_f16.hpp): a row of K values (K % 32 == 0) is K / 32 groups of 128 bytes, each the 32 hi halves then
# the 32 lo halves of the same 32 values; hi = f16(x) (0 below 2^-14), lo = f16((x - hi) * 2^11), x = hi + lo * 2^-11.

def split_encode(x):
    """float32 [rows][K] -> the same rows in the split format, as a float32-typed array [rows][K] of raw bits"""
    x = np.ascontiguousarray(x, np.float32)
    rows, k = x.shape
    assert k % 32 == 0
    with np.errstate(over="ignore", invalid="ignore"):
        hi = np.where(np.abs(x) < np.float32(2.0 ** -14), np.float16(0), x.astype(np.float16)).astype(np.float16)
        lo = ((x - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    out = np.empty((rows, k // 32, 2, 32), np.float16)
    out[:, :, 0, :] = hi.reshape(rows, k // 32, 32)
    out[:, :, 1, :] = lo.reshape(rows, k // 32, 32)
    return out.reshape(rows, 2 * k).view(np.float32)


def split_decode(raw):
    """raw bits of split rows, float32-typed [rows][n] (n % 32 == 0) -> float64 [rows][n]"""
    raw = np.ascontiguousarray(raw, np.float32)
    rows, n = raw.shape
    assert n % 32 == 0
    halves = raw.view(np.float16).reshape(rows, n // 32, 2, 32).astype(np.float64)
    return (halves[:, :, 0, :] + halves[:, :, 1, :] * 2.0 ** -11).reshape(rows, n)
