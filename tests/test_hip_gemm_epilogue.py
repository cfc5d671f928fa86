"""Every launch form of the four GEMM kernels (gemm.hip, gemm_f32.hip, gemm_split.hip, gemm_split_wd.hip) through
css_gemm_host, against the float64 reference of tests/gemm_reference.py: bias along either axis, ReLU / sigmoid, residual
(separate and in place) with alpha, batch strides, padded and misaligned C, split-f16 output columns, the transposed output,
fragment-ordered float32 weights with their row-major fallback, and the launch hints.  Two assertions per launch:

  ownership  C and all the slack around it start as a canary (a quiet NaN with a payload); afterwards every float outside
             {(bz, m, n): m < M, n < N} still holds the canary's bits -- the ldc - N gap of every row, the rows between batch
             entries, everything before C and the 128 rows behind it.  (The fast epilogue of gemm_f32.hip has no m < M guard:
             its row clipping is the buffer descriptor's bound.)
  value      |y - y64| <= |alpha| L 1.5e-6 scale + r |y64| + 2^-22 (|res| + |alpha v64|)   (gemm_reference.value_bound; split
             output columns are decoded first and add 2^-21 |y64|)

and bit equality wherever two launches must agree.  Each test prints its worst ratio of error to bound.
Needs an MI355X."""
import itertools

import numpy as np
import pytest

import gemm_reference as R
from conftest import pkg

pytestmark = pytest.mark.gpu

CANARY = 0x7FC0BEEF          # a quiet NaN with a payload
PREFIX = 64                  # floats in front of C (a multiple of 4: C stays on a 16-byte boundary unless a case moves it)
KERNEL_NAMES = {0: "split-f16, weights direct", 1: "split-f16, LDS staged", 2: "exact float32"}
ACT_NAMES = {R.ACT_NONE: "none", R.ACT_RELU: "relu", R.ACT_SIGMOID: "sigmoid"}


@pytest.fixture(scope="module")
def handle():
    L = pkg("_lib")
    if L.load().css_device_count() < 1:
        pytest.fail("no HIP device visible")
    w = pkg("weights")
    desc = w.ModelDesc(num_blocks=1)
    sep = pkg("separator").HipSeparator(w.apply_golden_recipe(w.portable_state_dict(desc, 5)), None, device=0)
    yield sep.handle
    sep.close()


def _canary(n):
    return np.full(int(n), CANARY, np.uint32).view(np.float32)


class Ops:
    """Seeded O(1) operands of one shape, and the float64 results of the epilogues asked for (computed once each)."""

    def __init__(self, m, n, k, batch=1, seed=0, shared_b=True):
        rs = np.random.RandomState(seed + 7919 * m + 31 * n + k)
        self.m, self.n, self.k, self.batch = m, n, k, batch
        self.a = rs.standard_normal((batch, m, k)).astype(np.float32)
        self.b = rs.standard_normal((1 if shared_b else batch, n, k)).astype(np.float32)
        self.bias_n = rs.standard_normal(n).astype(np.float32)
        self.bias_m = rs.standard_normal(m).astype(np.float32)
        self.res = rs.standard_normal((m, n)).astype(np.float32)
        self._ref = {}

    def bias(self, desc):
        return {None: None, "n": self.bias_n, "m": self.bias_m}[desc.get("bias")]

    def ref(self, desc, split_out=0):
        key = (desc.get("act", 0), desc.get("bias"), desc.get("residual") is not None, float(desc.get("alpha", 1.0)), split_out)
        if key not in self._ref:
            split = np.arange(self.n) < split_out if split_out else None
            y64, _, bound = R.reference_and_bound(desc, self.a, self.b, self.bias(desc), self.res, split=split)
            self._ref[key] = (y64, bound)
        return self._ref[key]


def launch(handle, ops, desc, *, kernel, ldc=None, ldr=None, c_shift=0, r_off=0, a_off=0, stride_rows=None, **kw):
    """One css_gemm_host launch of `desc` on `ops`.  Returns (y [batch][rows][cols] as it lies in C -- rows x cols is N x M for a
    transposed launch --, the whole downloaded allocation, the boolean mask of the floats the launch owns)."""
    m, n, k, batch = ops.m, ops.n, ops.k, ops.batch
    tr = bool(kw.get("c_transposed"))
    rows, cols = (n, m) if tr else (m, n)
    ldc = cols if ldc is None else ldc
    stride_c = (rows if stride_rows is None else stride_rows) * ldc
    c_off = PREFIX + c_shift
    total = c_off + (batch - 1) * stride_c + rows * ldc + 128 * ldc
    idx = (c_off + np.arange(batch)[:, None, None] * stride_c + np.arange(rows)[None, :, None] * ldc + np.arange(cols)[None, None, :])
    c = _canary(total)
    res_kind = desc.get("residual")
    residual = None
    if res_kind == "inplace":
        assert batch == 1 and not tr
        c[idx[0]] = ops.res
        residual = "inplace"
    elif res_kind == "separate":
        ldr = n if ldr is None else ldr
        r2 = _canary(m * max(ldr, n)).reshape(m, -1)   # (a kernel that reads the ldr - N gap returns a NaN)
        r2[:, :n] = ops.res
        residual = np.concatenate([_canary(r_off), r2.reshape(-1)])
    a = np.concatenate([np.zeros(a_off, np.float32), ops.a.reshape(-1)])
    shared_b = ops.b.shape[0] == 1
    out = handle.gemm(a, ops.b, c, m, n, k, kernel=kernel, batch=batch, ldc=ldc, ldr=ldr, c_off=c_off, r_off=r_off, a_off=a_off,
                      strideA=m * k if batch > 1 else 0, strideB=0 if shared_b or batch == 1 else n * k,
                      strideC=stride_c if batch > 1 else 0, act=desc.get("act", 0), bias=ops.bias(desc),
                      bias_along_m=desc.get("bias") == "m", residual=residual, alpha=desc.get("alpha", 1.0), **kw)
    owned = np.zeros(total, bool)
    owned[idx.reshape(-1)] = True
    return out[idx], out, owned


def assert_ownership(out, owned, what):
    stray = np.flatnonzero(out.view(np.uint32)[~owned] != CANARY)
    assert stray.size == 0, (what, f"{stray.size} floats outside C were written; the first at {np.flatnonzero(~owned)[stray[:8]]}")


def ratio_to_bound(y, ops, desc, split_out=0):
    """max |y - y64| / bound; y [batch][M][N] float32 with the first split_out columns still in the split format"""
    y64, bound = ops.ref(desc, split_out)
    got = y.astype(np.float64)
    if split_out:
        got[:, :, :split_out] = R.split_decode(y[:, :, :split_out].reshape(-1, split_out)).reshape(y.shape[0], y.shape[1], split_out)
    err = np.abs(got - y64)
    assert np.isfinite(got).all()
    return float((err / bound).max())


def check(handle, ops, desc, what, split_out=0, **kw):
    y, out, owned = launch(handle, ops, desc, split_out=split_out, **kw)
    assert_ownership(out, owned, what)
    ratio = ratio_to_bound(y, ops, desc, split_out)
    assert ratio <= 1.0, (what, ratio)
    return y, ratio


def epilogues():
    """act x (no residual | separate, ldr = N + 4 | in place) x alpha x bias direction"""
    for act, (res, alpha), bias in itertools.product((R.ACT_NONE, R.ACT_RELU, R.ACT_SIGMOID),
                                                     ((None, 1.0), ("separate", 1.0), ("separate", 0.5), ("inplace", 1.0), ("inplace", 0.5)),
                                                     (None, "n", "m")):
        yield dict(act=act, residual=res, alpha=alpha, bias=bias)


# ---- a. the epilogue matrix -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape, kernel", [((97, 256, 64), 0), ((97, 256, 64), 1), ((97, 256, 64), 2), ((33, 130, 32), 1), ((33, 130, 32), 2)])
def test_epilogue_matrix(handle, shape, kernel):
    """(97, 256, 64): whole 128-column panels, an edge in M; (33, 130, 32): an edge in both, N % 4 != 0 (the narrow stores) and the
    shortest K loop the kernels accept.  The weights-direct kernel takes whole 32-column weight tiles, so it runs the first shape
    only (N % 32 there is not a launch form: css_gemm_host refuses it, test_refusals below)."""
    m, n, k = shape
    ops = Ops(m, n, k)
    worst = {}
    for d in epilogues():
        _, ratio = check(handle, ops, d, (shape, kernel, d), kernel=kernel, ldr=n + 4 if d["residual"] == "separate" else None)
        key = (ACT_NAMES[d["act"]], "residual" if d["residual"] else "no residual")
        worst[key] = max(worst.get(key, 0.0), ratio)
    for (act, res), v in sorted(worst.items()):
        print(f"ratio to bound | {KERNEL_NAMES[kernel]} | {m} x {n} x {k} | {act}, {res} | {v:.3f}")


# ---- b. gemm_f32.hip: the fast and the general epilogue, gemm.hip, fragment weights and their fallback: same bits -------------

@pytest.mark.parametrize("shape", [(97, 256, 64), (257, 384, 96)])
@pytest.mark.parametrize("epilogue", ["relu", "residual", "inplace"])
def test_f32_epilogue_kernels_agree(handle, shape, epilogue):
    m, n, k = shape
    ops = Ops(m, n, k, seed=1)
    d = {"relu": dict(act=R.ACT_RELU, bias="n"), "residual": dict(act=R.ACT_NONE, bias="n", residual="separate", alpha=0.5),
         "inplace": dict(act=R.ACT_RELU, bias=None, residual="inplace", alpha=0.5)}[epilogue]
    base, ratio = check(handle, ops, d, (shape, epilogue, "ldc = N"), kernel=2)
    print(f"ratio to bound | {KERNEL_NAMES[2]} | {m} x {n} x {k} | fast epilogue, {epilogue} | {ratio:.3f}")
    variants = [("b_frag32", dict(b_frag32=True)),
                ("ldc = N + 4 (fast)", dict(ldc=n + 4)), ("ldc = N + 4, b_frag32", dict(ldc=n + 4, b_frag32=True)),
                ("ldc = N + 1 (general)", dict(ldc=n + 1)), ("ldc = N + 1, b_frag32", dict(ldc=n + 1, b_frag32=True)),
                ("C moved by one float (general)", dict(c_shift=1)), ("C moved by one float, b_frag32", dict(c_shift=1, b_frag32=True)),
                ("layout 2 (gemm.hip)", dict(layout=2)), ("layout 2, ldc = N + 1", dict(layout=2, ldc=n + 1)),
                ("b_frag32, A moved by one float (B_rows)", dict(b_frag32=True, a_off=1)),
                ("A moved by one float", dict(a_off=1))]
    if epilogue == "residual":
        variants += [("residual moved by one float (general)", dict(r_off=1)), ("residual moved, b_frag32", dict(r_off=1, b_frag32=True)),
                     ("ldr = N + 4 (fast)", dict(ldr=n + 4)), ("ldr = N + 1 (general)", dict(ldr=n + 1))]
    for name, kw in variants:
        y, out, owned = launch(handle, ops, d, kernel=2, **kw)
        assert_ownership(out, owned, (shape, epilogue, name))
        assert np.array_equal(y, base), (shape, epilogue, name, float(np.abs(y - base).max()))


# ---- c. tall tiles with a residual --------------------------------------------------------------------------------------------

def test_tall_tiles_with_residual(handle):
    """130 row units x 32 column panels = 4160 units over the 1024 persistent blocks: tiles of 2, 3 and 4 units walk the fast
    residual path (prefetch_fast, the two alternating rv slots) in one launch.  Forced tile heights 11 .. 14 and gemm.hip's kernel
    (layout 2) give the same bits; the layout 2 result is held to the bound."""
    m, n, k = 4129, 4096, 32
    ops = Ops(m, n, k, seed=2)
    d = dict(act=R.ACT_NONE, bias="n", residual="separate", alpha=0.5)
    base, ratio = check(handle, ops, d, "layout 2", kernel=2, layout=2)
    print(f"ratio to bound | {KERNEL_NAMES[2]} | {m} x {n} x {k} | none, residual (layout 2) | {ratio:.3f}")
    for lay in (0, 11, 12, 13, 14):
        y, out, owned = launch(handle, ops, d, kernel=2, layout=lay, b_frag32=True)
        assert_ownership(out, owned, ("tall", lay))
        assert np.array_equal(y, base), (lay, float(np.abs(y - base).max()))


# ---- d. batch -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("shared_b", [True, False])
def test_batch_strides(handle, kernel, shared_b):
    """The streams' synthesis form at the hand-off's K: three entries of 45 rows -- the last (partial) row tile of entry bz ends
    where entry bz + 1 begins (strideC = M ldc) or three canary rows before it."""
    m, n, k = 45, 512, 416
    ops = Ops(m, n, k, batch=3, seed=3, shared_b=shared_b)
    d = dict(act=R.ACT_NONE, bias=None)
    ys = []
    for stride_rows in (m, m + 3):
        y, ratio = check(handle, ops, d, (kernel, shared_b, stride_rows), kernel=kernel, stride_rows=stride_rows)
        print(f"ratio to bound | {KERNEL_NAMES[kernel]} | 3 x {m} x {n} x {k} | none, no residual, strideC = {stride_rows} rows | {ratio:.3f}")
        ys.append(y)
    assert np.array_equal(ys[0], ys[1])
    if kernel == 2:   # the fast epilogue clips by the descriptor of EACH entry; the general one (ldc % 4 != 0) and gemm.hip agree
        for kw in (dict(ldc=n + 1), dict(layout=2), dict(ldc=n + 4, stride_rows=m + 1)):
            y, out, owned = launch(handle, ops, d, kernel=2, **kw)
            assert_ownership(out, owned, (shared_b, kw))
            assert np.array_equal(y, ys[0]), kw


# ---- e. the split kernels -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("split_out", [0, 32, 256])
def test_split_output_columns(handle, split_out):
    m, n, k = 97, 256, 64
    ops = Ops(m, n, k, seed=4)
    for d in (dict(act=R.ACT_NONE, bias="n"), dict(act=R.ACT_RELU, bias="n"), dict(act=R.ACT_NONE, bias="m", residual="separate", alpha=0.5)):
        y0, r0 = check(handle, ops, d, (0, split_out, d), split_out=split_out, kernel=0)
        y1, r1 = check(handle, ops, d, (1, split_out, d), split_out=split_out, kernel=1)
        assert np.array_equal(y0.view(np.uint32), y1.view(np.uint32))   # the two split kernels accumulate in the same order
        print(f"ratio to bound | split-f16 (both) | {m} x {n} x {k} | {ACT_NAMES[d['act']]}, {'residual' if d.get('residual') else 'no residual'}, "
              f"split_out = {split_out} | {max(r0, r1):.3f}")
        if split_out:   # the remaining columns are the plain launch's float32 values
            plain, _, _ = launch(handle, ops, d, kernel=1)
            assert np.array_equal(y1[:, :, split_out:], plain[:, :, split_out:])
            assert np.array_equal(R.split_decode(y1[0, :, :split_out]),
                                  R.split_decode(R.split_encode(plain[0, :, :split_out])))   # ... and the split ones their encoding


def test_weights_direct_tile_rows_agree(handle):
    m, n, k = 97, 256, 64
    ops = Ops(m, n, k, seed=5)
    for d, so in ((dict(act=R.ACT_RELU, bias="n"), 32), (dict(act=R.ACT_NONE, bias="n", residual="separate", alpha=0.5), 0),
                  (dict(act=R.ACT_NONE, bias=None, residual="inplace", alpha=0.5), 0)):
        base, _ = check(handle, ops, d, ("tile_rows 0", d), split_out=so, kernel=0)
        for tile in (32, 64, 96, 4, 128, 65):
            y, out, owned = launch(handle, ops, d, kernel=0, tile_rows=tile, split_out=so)
            assert_ownership(out, owned, (tile, d))
            assert np.array_equal(y.view(np.uint32), base.view(np.uint32)), (tile, d)


@pytest.mark.parametrize("shape", [(70, 96, 64), (186, 1056, 64)])   # (1056: the mask head's 1028 outputs in whole 32-column weight tiles)
def test_transposed_output(handle, shape):
    """column bias + sigmoid, C^T[n][m] at n ldc + m with ldc = M + 6: the transpose of the untransposed launch bit for bit, the
    ldc - M gap of every row untouched"""
    m, n, k = shape
    ops = Ops(m, n, k, seed=6)
    d = dict(act=R.ACT_SIGMOID, bias="n")
    y, ratio = check(handle, ops, d, shape, kernel=0)
    print(f"ratio to bound | {KERNEL_NAMES[0]} | {m} x {n} x {k} | sigmoid, no residual | {ratio:.3f}")
    for tile in (0, 65):
        yt, out, owned = launch(handle, ops, d, kernel=0, c_transposed=True, ldc=m + 6, tile_rows=tile)
        assert yt.shape == (1, n, m)
        assert_ownership(out, owned, (shape, "transposed", tile))
        assert np.array_equal(yt[0].T, y[0]), tile


# ---- f. flags that must not change a bit ------------------------------------------------------------------------------------------

def test_launch_hints_change_no_bit(handle):
    m, n, k = 257, 384, 96
    ops = Ops(m, n, k, seed=7)
    d = dict(act=R.ACT_RELU, bias="n", residual="separate", alpha=0.5)
    for kernel, forms in ((0, [dict(nt_store=True), dict(concurrent=True), dict(nt_store=True, split_out=64)]),
                          (1, [dict(m_fastest=True), dict(m_fastest=True, layout=64), dict(concurrent=True)]),
                          (2, [dict(m_fastest=True, layout=2), dict(m_fastest=True, layout=64), dict(m_fastest=True), dict(concurrent=True),
                               dict(nt_store=True)])):
        for kw in forms:
            off = {f: v for f, v in kw.items() if f not in ("nt_store", "concurrent", "m_fastest")}
            base, ratio = check(handle, ops, d, (kernel, off), kernel=kernel, **off)
            y, out, owned = launch(handle, ops, d, kernel=kernel, **kw)
            assert_ownership(out, owned, (kernel, kw))
            assert np.array_equal(y.view(np.uint32), base.view(np.uint32)), (kernel, kw)
        print(f"ratio to bound | {KERNEL_NAMES[kernel]} | {m} x {n} x {k} | relu, residual | {ratio:.3f}")


# ---- what css_gemm_host refuses (nothing is launched) -------------------------------------------------------------------------------

def test_refusals(handle):
    L = pkg("_lib")
    ops = Ops(33, 130, 32)
    ops32 = Ops(64, 96, 64)
    plain = dict(act=R.ACT_NONE, bias="n")
    res = dict(act=R.ACT_NONE, bias="n", residual="separate", alpha=1.0)
    bad = [(ops, plain, dict(kernel=0)),                                   # N % 32 on the weights-direct kernel
           (ops32, plain, dict(kernel=0, ldc=97)), (ops32, plain, dict(kernel=0, c_shift=1)),   # 16-byte pieces
           (ops32, plain, dict(kernel=1, split_out=16)), (ops32, plain, dict(kernel=1, split_out=128)), (ops32, plain, dict(kernel=2, split_out=32)),
           (ops32, res, dict(kernel=0, c_transposed=True)), (ops32, plain, dict(kernel=0, c_transposed=True, split_out=32)),
           (ops32, dict(act=0, bias="m"), dict(kernel=0, c_transposed=True)), (ops32, plain, dict(kernel=1, c_transposed=True)),
           (ops32, plain, dict(kernel=1, b_frag32=True)), (ops, plain, dict(kernel=2, b_frag32=True)),
           (ops32, plain, dict(kernel=2, layout=3)), (ops32, plain, dict(kernel=1, layout=11)), (ops32, plain, dict(kernel=0, tile_rows=16)),
           (ops32, plain, dict(kernel=2, ldc=95)), (ops32, res, dict(kernel=2, ldr=95))]
    for o, d, kw in bad:
        with pytest.raises(L.CssError) as e:
            launch(handle, o, d, **kw)
        assert e.value.code == L.CSS_ERR_INVALID_ARG, kw
    b3 = Ops(45, 64, 32, batch=3)
    for kw in (dict(kernel=0), dict(kernel=2, b_frag32=True), dict(kernel=2, stride_rows=44)):
        with pytest.raises(L.CssError) as e:
            launch(handle, b3, plain, **kw)
        assert e.value.code == L.CSS_ERR_INVALID_ARG, kw
    for k_bad in (16, 48):   # K % 32
        with pytest.raises(L.CssError) as e:
            handle.gemm(np.zeros(64 * k_bad, np.float32), np.zeros(64 * k_bad, np.float32), _canary(64 * 64), 64, 64, k_bad)
        assert e.value.code == L.CSS_ERR_INVALID_ARG
    with pytest.raises(L.CssError):   # an array shorter than its description
        handle.gemm(np.zeros(64 * 32 - 1, np.float32), np.zeros(64 * 32, np.float32), _canary(64 * 64), 64, 64, 32)
    with pytest.raises(L.CssError):
        handle.gemm(np.zeros(64 * 32, np.float32), np.zeros(64 * 32, np.float32), _canary(64 * 64 - 1), 64, 64, 32)
    # and the handle still computes
    check(handle, ops, plain, "after the refusals", kernel=2)
