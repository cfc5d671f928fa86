"""The parts of the GEMM epilogue tests that need no GPU: css_gemm_host is declared, exported and bound with one structure
layout, and refuses a NULL handle; the float64 reference of tests/gemm_reference.py applies the epilogue in the kernels' order;
and the numpy form of the split-f16 row format round-trips as csrc/split_f16.hpp says it does."""
import ctypes as C
import os
import re

import numpy as np

import gemm_reference as R
from conftest import ROOT, pkg


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "css_mi355.h")).read(), flags=re.S)


def test_header_library_and_binding_agree():
    L = pkg("_lib")
    text = _header()
    lib = L.load()
    assert re.search(r"\bint\s+css_gemm_host\s*\(", text), "css_gemm_host is not declared in css_mi355.h"
    assert hasattr(lib, "css_gemm_host") and "css_gemm_host" in L.SIGNATURES
    params = re.search(r"\bcss_gemm_host\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
    restype, argtypes = L.SIGNATURES["css_gemm_host"]
    assert restype is C.c_int and len(argtypes) == len(params) == 7
    assert all("*" in p or p.split()[0] == "css_handle_t" for p in params)
    # the descriptor: the header's fields in the header's order, with the header's types
    body = re.search(r"typedef struct CssGemmDesc \{(.*?)\} CssGemmDesc;", text, flags=re.S).group(1)
    kinds = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            kind, names = decl.split(None, 1)
            fields += [(n.strip(), kinds[kind]) for n in names.split(",")]
    assert fields == list(L.CssGemmDesc._fields_)
    assert C.sizeof(L.CssGemmDesc) == 8 * 4 + 14 * 8 + 9 * 4 + 4   # (four bytes of tail padding: the 64-bit fields' alignment)
    assert L.CssGemmDesc.lda.offset == 32 and L.CssGemmDesc.bias.offset == 144 and L.CssGemmDesc.concurrent.offset == 176
    assert len(L.SIGNATURES) == 85   # (84 before css_gemm_host)


def test_null_handle_and_null_descriptor_are_refused():
    L = pkg("_lib")
    lib = L.load()
    d = L.CssGemmDesc(kernel=2, M=32, N=32, K=32, batch=1, lda=32, ldb=32, ldc=32, a_floats=1024, b_floats=1024, c_floats=1024,
                      alpha=1.0)
    a = np.zeros(1024, np.float32)
    c = np.full(1024, 7.0, np.float32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    assert lib.css_gemm_host(None, C.byref(d), p(a), p(a), None, None, p(c)) == L.CSS_ERR_INVALID_ARG
    assert lib.css_gemm_host(None, None, p(a), p(a), None, None, p(c)) == L.CSS_ERR_INVALID_ARG
    assert (c == 7.0).all()


def test_split_f16_round_trip():
    """encode (the header's rule, written out in numpy) then decode: within 2^-21 relative for 2^-14 <= |x| <= 65504 (hi is x to
    11 bits, x - hi is exact in float32, lo carries it to 11 more: 2^-22 and the subnormal lo of the smallest values), exact for
    every value float16 represents; and the 128-byte groups are 32 hi halves followed by 32 lo halves."""
    rs = np.random.RandomState(0)
    mag = np.exp2(rs.uniform(-14.0, np.log2(65504.0), (64, 256)))
    x = (mag * rs.choice([-1.0, 1.0], mag.shape)).astype(np.float32)
    x[0, :4] = [2.0 ** -14, -2.0 ** -14, 65504.0, -65504.0]
    x = np.clip(x, -65504.0, 65504.0)
    x[np.abs(x) < 2.0 ** -14] = 2.0 ** -14
    raw = R.split_encode(x)
    assert raw.shape == x.shape and raw.dtype == np.float32
    back = R.split_decode(raw)
    rel = np.abs(back - x.astype(np.float64)) / np.abs(x)
    print(f"split-f16 round trip: max relative error {rel.max():.3e} (2^-21 = {2.0 ** -21:.3e})")
    assert rel.max() <= 2.0 ** -21
    # every finite float16 value, subnormals and zeros included, comes back exactly
    h = np.arange(65536, dtype=np.uint16).view(np.float16)
    h = h[np.isfinite(h)]
    h = np.concatenate([h, np.zeros(-h.size % 32, np.float16)]).astype(np.float32).reshape(-1, 32)
    assert np.array_equal(R.split_decode(R.split_encode(h)), h.astype(np.float64))
    # layout: element k of a row lives at half ((k >> 5) << 6) | (k & 31), its lo part 32 halves further (split_index)
    row = np.zeros((1, 64), np.float32)
    row[0, 33] = 1.0 + 2.0 ** -12       # hi = 1, lo = 2^-12 * 2^11 = 0.5
    halves = R.split_encode(row).view(np.float16)[0]
    assert halves[64 + 1] == 1.0 and halves[64 + 32 + 1] == 0.5 and np.count_nonzero(halves) == 2


def test_reference_applies_the_epilogue_in_the_kernels_order():
    """res + alpha * act(acc + bias) on a 2 x 2 case computed by hand (K = 2 here: the reference has no K rule of its own)"""
    a = np.array([[1.0, 2.0], [-3.0, 0.5]])
    b = np.array([[2.0, -1.0], [0.5, 4.0]])          # acc = a @ b.T = [[0, 8.5], [-6.5, 0.5]]
    bias_n = np.array([1.0, -9.0])                   # + bias along n: [[1, -0.5], [-5.5, -8.5]]
    bias_m = np.array([1.0, -9.0])                   # + bias along m: [[1, 9.5], [-15.5, -8.5]]
    res = np.array([[10.0, 20.0], [30.0, 40.0]])
    d = dict(act=R.ACT_RELU, bias="n", residual="separate", alpha=0.5)
    y, scale = R.reference(d, a, b, bias_n, res)
    assert y.shape == (1, 2, 2) and np.array_equal(y[0], [[10.5, 20.0], [30.0, 40.0]])
    assert np.array_equal(scale[0], [[5.0, 17.5], [7.5, 12.5]])          # |a| @ |b|.T + |bias|: [[4, 8.5], [6.5, 3.5]] + [1, 9]
    y, _ = R.reference(dict(act=R.ACT_RELU, bias="m", residual="inplace", alpha=0.5), a, b, bias_m, res)
    assert np.array_equal(y[0], [[10.5, 24.75], [30.0, 40.0]])
    y, _ = R.reference(dict(act=R.ACT_NONE, bias="n"), a, b, bias_n)     # no residual: alpha is not applied
    assert np.array_equal(y[0], [[1.0, -0.5], [-5.5, -8.5]])
    y, _ = R.reference(dict(act=R.ACT_SIGMOID, bias=None, residual="separate", alpha=2.0), a, b, None, res)
    want = res + 2.0 / (1.0 + np.exp(-np.array([[0.0, 8.5], [-6.5, 0.5]])))
    assert np.allclose(y[0], want, rtol=1e-15, atol=0) and y[0, 0, 0] == 11.0
    # the activation comes before the residual, alpha scales the activation's value only
    y, _ = R.reference(dict(act=R.ACT_RELU, bias=None, residual="separate", alpha=-1.0), a, b, None, res)
    assert np.array_equal(y[0], [[10.0, 11.5], [30.0, 39.5]])
    # a batched operand against a shared one
    y, scale = R.reference(dict(act=R.ACT_NONE, bias=None), np.stack([a, 2 * a]), b)
    assert y.shape == (2, 2, 2) and np.array_equal(y[1], 2 * y[0]) and np.array_equal(scale[1], 2 * scale[0])
    # the bound: its three terms on the first case, and the split columns' extra term
    bound = R.value_bound(d, a, b, bias_n, res)
    v = np.array([[1.0, 0.0], [0.0, 0.0]])
    want = 0.5 * 1.5e-6 * np.array([[5.0, 17.5], [7.5, 12.5]]) + 2.0 ** -23 * np.array([[10.5, 20.0], [30.0, 40.0]]) \
        + 2.0 ** -22 * (res + 0.5 * v)
    assert np.allclose(bound[0], want, rtol=1e-15, atol=0)
    more = R.value_bound(d, a, b, bias_n, res, split=[True, False])
    assert np.allclose(more[0] - bound[0], 2.0 ** -21 * np.array([[10.5, 0.0], [30.0, 0.0]]), rtol=1e-9, atol=0)
