"""Every launch form masknet_lane (csrc/api_stages.hip) makes from csrc/encoder.hip, through the host entries of
include/css_mi355_encoder.h, against the float64 references and derived bounds of tests/encoder_reference.py.  Three kinds of
assertion per launch:

  ownership  outputs and 128 rows of slack behind them start as the canary 0x7FC0BEEF (a quiet NaN with a payload); every float
             outside the rows the launch owns keeps its bits, and the input of the fused conv module is bit-identical afterwards
  value      |y - y64| <= bound elementwise (split-f16 rows decoded first); the worst ratio of each test is printed
             
  bits       where two launches must agree: float32 and split output of one LayerNorm (split_encode of the former),
             launch_layernorm2 against two launch_layernorm, the conv module's trailing z against launch_layernorm of its
             x_out, one segment alone against the same segment among others, the any-length attention's split rows against
             its float32 rows.  The fused conv module against the two-kernel form is held to the sum of their bounds (their
             sigmoids differ).

Coverage (every form masknet_lane launches from encoder.hip):
  layernorm_kernel<NV, 0>      test_layernorm: y, ys, both, in place with ys (the last block's closing LayerNorm)
  layernorm_kernel<NV, 1>      test_layernorm: ReLU (the embedding)
  layernorm_kernel<NV, 2>      test_layernorm (launch_ln_glu), test_conv_two_kernel
  layernorm2_kernel<NV>        test_layernorm: in place, z / zs / both
  conv_module_kernel           test_conv_fused: D 256 and 512, z and zs both, each alone, neither; uncovered (D, taps) reported
  dwconv_kernel<17 | 31 | 33>  test_conv_two_kernel
  relpos_attn_kernel<NJT, false, false>  test_attention_short[0]: NJT 1 .. 16, with pe_fragments_kernel(split = 0)
  relpos_attn_kernel<NJT, true, true>    test_attention_short[1]: the weights-direct GEMM's frag_out epilogue, launch_split_convert of
                                         the table, pe_fragments_kernel(split = 1), split P.V, split context rows
  relpos_attn_long_kernel      test_attention_long: 16, 8 and 4 queries per block, split_out 0 and 1
The any-length launch that needs more than 64 KB of LDS (segments beyond 16 000 frames) is out of reach of a test that takes
seconds: the float64 reference alone is 2 GB per head.  (relpos_attn_kernel<NJT, true, false> is instantiated but no path
launches it: launch_relpos_attention is always given the fragments in split mode.)
Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest

import encoder_reference as E
from conftest import pkg

pytestmark = pytest.mark.gpu

CANARY = 0x7FC0BEEF
SLACK = 128                  # rows of slack behind every output


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


def _canary(rows, D):
    return np.full((rows + SLACK) * D, CANARY, np.uint32).view(np.float32)


def _with_slack(x):
    """x [rows][D] followed by 128 rows of canary"""
    return np.concatenate([np.ascontiguousarray(x, np.float32).reshape(-1), _canary(0, x.shape[1])])


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _owned(out, rows, D, what):
    """the rows a launch owns, after asserting that the slack behind them kept the canary"""
    out = out.reshape(-1, D)
    stray = np.flatnonzero(_bits(out[rows:]) != CANARY)
    assert stray.size == 0, (what, f"{stray.size} floats behind the last row were written, the first at row {rows + stray[0] // D}")
    return out[:rows]


def _ratio(y, y64, bound, what, split=False):
    got = E.split_decode(y) if split else y.astype(np.float64)
    assert np.isfinite(got).all(), (what, "a non-finite output", np.argwhere(~np.isfinite(got))[:4])
    r = np.abs(got - y64) / (bound + (E.SPLIT_ST * np.abs(y64) + E.SPLIT_FLOOR if split else 0.0))
    worst = np.unravel_index(int(r.argmax()), r.shape)
    assert r[worst] <= 1.0, (what, f"ratio {r[worst]:.3f} at (row, column) {worst}: got {got[worst]!r}, float64 {y64[worst]!r}")
    return float(r[worst])


def _same_bits(a, b, what):
    diff = np.argwhere(_bits(a) != _bits(b))
    assert diff.size == 0, (what, f"{len(diff)} floats differ, the first at {diff[0]}")


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", E.LN_WIDTHS)
def test_layernorm(handle, D):
    worst = {}
    note = lambda k, r: worst.__setitem__(k, max(worst.get(k, 0.0), r))
    for i, rows in enumerate(E.LN_ROWS):
        c = E.ln_case(rows, D, seed=E.LN_WIDTHS.index(D) * len(E.LN_ROWS) + i)
        x, w, b, w2, b2 = c["x"], c["w"], c["b"], c["w2"], c["b2"]
        what = f"D {D} rows {rows}"
        y64, bound = E.layer_norm_bound(x, w, b)
        can = lambda: _canary(rows, D)
        # form 0: both outputs, each alone, in place with the split rows
        xo, y, _, ys = handle.layernorm(0, x, rows, D, w, b, y=can(), ys=can())
        _same_bits(xo, x.reshape(-1), what + ": the input changed")
        y, ys = _owned(y, rows, D, what + " y"), _owned(ys, rows, D, what + " ys")
        note("layernorm", _ratio(y, y64, bound, what + " y"))
        note("layernorm split", _ratio(ys, y64, bound, what + " ys", split=True))
        _same_bits(E.split_encode(y), ys, what + ": split rows against the encoded float32 rows")
        _same_bits(_owned(handle.layernorm(0, x, rows, D, w, b, y=can())[1], rows, D, what), y, what + ": y alone")
        _same_bits(_owned(handle.layernorm(0, x, rows, D, w, b, ys=can())[3], rows, D, what), ys, what + ": ys alone")
        xo, _, _, ys1 = handle.layernorm(0, _with_slack(x), rows, D, w, b, inplace=True, ys=can())
        _same_bits(_owned(xo, rows, D, what + " in place"), y, what + ": in place")
        _same_bits(_owned(ys1, rows, D, what), ys, what + ": ys of the in-place launch")
        # form 1: ReLU
        y1 = _owned(handle.layernorm(1, x, rows, D, w, b, y=can())[1], rows, D, what + " relu")
        note("layernorm relu", _ratio(y1, np.maximum(y64, 0), bound, what + " relu"))
        # (held to the bound, not to the bits of max(y, 0): the ReLU instantiation is another kernel, and at D = 768 the compiler
        #  contracts its affine step differently -- one ulp on the MI355X)
        # form 2: LayerNorm + GLU, gate arguments of O(1) and over +-100
        for pw in (E.PW_MILD, E.PW_WIDE):
            g64, gb = E.ln_glu_bound(x, w, b, pw, hw=False)
            pw6 = np.array(pw, np.float32)
            yg = _owned(handle.layernorm(2, x, rows, D, w, b, w2=pw6, y=can())[1], rows, D, what + " glu")
            note(f"ln_glu pw2 {pw[2]}", _ratio(yg, g64, gb, what + f" glu pw2 {pw[2]}"))
        # form 3: the pair, in place, against two single launches
        z_ref = _owned(handle.layernorm(0, y, rows, D, w2, b2, y=can())[1], rows, D, what)
        z64, zb = E.layer_norm_bound(y, w2, b2)
        for want_z, want_zs in ((True, False), (False, True), (True, True)):
            xo, _, z, zs = handle.layernorm(3, _with_slack(x), rows, D, w, b, w2=w2, b2=b2, inplace=True,
                                            z=can() if want_z else None, ys=can() if want_zs else None)
            _same_bits(_owned(xo, rows, D, what + " pair y"), y, what + ": pair, y against launch_layernorm")
            if want_z:
                z = _owned(z, rows, D, what + " pair z")
                _same_bits(z, z_ref, what + ": pair, z against launch_layernorm of y")
                note("layernorm2 z", _ratio(z, z64, zb, what + " pair z"))
            if want_zs:
                _same_bits(_owned(zs, rows, D, what + " pair zs"), E.split_encode(z_ref), what + ": pair, zs")
        _, y3, z3, _ = handle.layernorm(3, x, rows, D, w, b, w2=w2, b2=b2, y=can(), z=can())   # y apart from x
        _same_bits(_owned(y3, rows, D, what), y, what + ": pair with y apart")
        _same_bits(_owned(z3, rows, D, what), z_ref, what + ": pair with y apart, z")
    for k, r in sorted(worst.items()):
        print(f"D {D} {k}: worst error / bound {r:.3f}")


# ---- conv module ----------------------------------------------------------------------------------------------------------------

def _conv_ops(c):
    return (c["ln_w"], c["ln_b"], c["pw"], c["wt"], c["dwb"], c["alpha"], c["beta"])


def _conv_pair(handle, c, what):
    """the two-kernel form in place; returns the rows"""
    D, M = c["D"], c["nseg"] * c["T"]
    launched, xo, _, _, _ = handle.conv_module(1, _with_slack(c["x"]), c["nseg"], c["T"], D, c["taps"], *_conv_ops(c))
    assert launched
    return _owned(xo, M, D, what + " two-kernel")


def test_conv_fused(handle):
    worst = {"fused": 0.0, "fused vs two-kernel / sum of bounds": 0.0, "trailing z": 0.0}
    for n, (D, taps, nseg, T, imp) in enumerate(E.conv_cases(True)):
        c = E.conv_case(D, taps, nseg, T, impulse=imp)
        M, what = nseg * T, f"fused D {D} nseg {nseg} T {T} impulse {imp}"
        can = lambda: _canary(M, D)
        args = (c["x"], c["ln_w"], c["ln_b"], c["pw"], c["wt"], c["dwb"], c["alpha"], c["beta"], nseg, T)
        y64, bound = E.conv_module_bound(*args, hw=True)
        launched, xo, x_out, z, zs = handle.conv_module(0, c["x"], nseg, T, D, taps, *_conv_ops(c), c["ln2_w"], c["ln2_b"],
                                                        x_out=can(), z=can(), zs=can())
        assert launched, what
        _same_bits(xo, c["x"].reshape(-1), what + ": x_in changed")
        x_out, z, zs = (_owned(a, M, D, what + k) for a, k in ((x_out, " x_out"), (z, " z"), (zs, " zs")))
        worst["fused"] = max(worst["fused"], _ratio(x_out, y64, bound, what))
        z_ref = _owned(handle.layernorm(0, x_out, M, D, c["ln2_w"], c["ln2_b"], y=can())[1], M, D, what)
        _same_bits(z, z_ref, what + ": trailing z against launch_layernorm of x_out")
        _same_bits(zs, E.split_encode(z_ref), what + ": trailing zs")
        z64, zb = E.layer_norm_bound(x_out, c["ln2_w"], c["ln2_b"])
        worst["trailing z"] = max(worst["trailing z"], _ratio(z, z64, zb, what + " z"))
        # against the two-kernel form: the sum of the two bounds
        pair = _conv_pair(handle, c, what)
        _, bound_lib = E.conv_module_bound(*args, hw=False)
        r = float((np.abs(x_out.astype(np.float64) - pair) / (bound + bound_lib)).max())
        assert r <= 1.0, (what, "fused against two-kernel", r)
        worst["fused vs two-kernel / sum of bounds"] = max(worst["fused vs two-kernel / sum of bounds"], r)
        if n < 4 or imp is not None:   # the trailing LayerNorm's outputs each alone, and neither
            for want_z, want_zs in ((True, False), (False, True), (False, False)):
                _, _, xo2, z2, zs2 = handle.conv_module(0, c["x"], nseg, T, D, taps, *_conv_ops(c), c["ln2_w"], c["ln2_b"], x_out=can(),
                                                        z=can() if want_z else None, zs=can() if want_zs else None)
                _same_bits(_owned(xo2, M, D, what), x_out, what + f": x_out with z {want_z} zs {want_zs}")
                if want_z:
                    _same_bits(_owned(z2, M, D, what), z, what + ": z alone")
                if want_zs:
                    _same_bits(_owned(zs2, M, D, what), zs, what + ": zs alone")
        if imp is not None or (nseg == 3 and T in (33, 62)):   # the middle segment alone: the same bits
            mid = slice(T * (nseg // 2), T * (nseg // 2 + 1))
            _, _, xo1, z1, _ = handle.conv_module(0, c["x"][mid], 1, T, D, taps, *_conv_ops(c), c["ln2_w"], c["ln2_b"],
                                                  x_out=_canary(T, D), z=_canary(T, D))
            _same_bits(_owned(xo1, T, D, what), x_out[mid], what + ": the middle segment alone")
            _same_bits(_owned(z1, T, D, what), z[mid], what + ": the middle segment alone, z")
    for k, r in worst.items():
        print(f"conv module {k}: worst error / bound {r:.3f}")


def test_conv_fused_reports_what_it_does_not_cover(handle):
    for D, taps in ((768, 33), (1024, 33), (256, 17), (512, 31)):
        c = E.conv_case(D, taps, 2, 40)
        launched, xo, x_out, z, _ = handle.conv_module(0, c["x"], 2, 40, D, taps, *_conv_ops(c), c["ln2_w"], c["ln2_b"],
                                                       x_out=_canary(80, D), z=_canary(80, D))
        assert not launched, (D, taps)
        _same_bits(xo, c["x"].reshape(-1), "x_in")
        assert (_bits(x_out) == CANARY).all() and (_bits(z) == CANARY).all(), (D, taps)


def test_conv_two_kernel(handle):
    worst = 0.0
    for D, taps, nseg, T, imp in E.conv_cases(False):
        c = E.conv_case(D, taps, nseg, T, impulse=imp)
        what = f"two-kernel D {D} taps {taps} nseg {nseg} T {T} impulse {imp}"
        y64, bound = E.conv_module_bound(c["x"], c["ln_w"], c["ln_b"], c["pw"], c["wt"], c["dwb"], c["alpha"], c["beta"], nseg, T, hw=False)
        y = _conv_pair(handle, c, what)
        worst = max(worst, _ratio(y, y64, bound, what))
        if imp is not None or (nseg == 3 and T in (33, 62)):
            mid = slice(T * (nseg // 2), T * (nseg // 2 + 1))
            c1 = dict(c, nseg=1, x=c["x"][mid])
            _same_bits(_conv_pair(handle, c1, what), y[mid], what + ": the middle segment alone")
    print(f"conv module two-kernel: worst error / bound {worst:.3f}")


# ---- attention ------------------------------------------------------------------------------------------------------------------

def _attention(handle, mode, c, x, w, bias, split_out=0):
    """One css_attention_host call; returns (qkv rows [M][3 D], ctx rows [M][D]) after the ownership assertions"""
    nseg, T, D, H = c["nseg"], c["T"], c["D"], c["H"]
    M, what = nseg * T, f"mode {mode} {c['family']} nseg {nseg} T {T} D {D} maxlen {c['maxlen']} delta {c['delta']}"
    qkv, ctx = handle.attention(mode, x, w, bias, c["pe"], nseg, T, D, H, c["maxlen"], split_out=split_out, canary=CANARY,
                                slack_rows=SLACK)
    qkv, ctx = _owned(qkv, M, 3 * D, what + " qkv"), _owned(ctx, M, D, what + " ctx")
    if mode == 1:   # q and k left in operand order: their columns of qkv belong to nobody
        assert (_bits(qkv[:, :2 * D]) == CANARY).all(), what + ": the q / k columns of qkv were written"
    return qkv, ctx, what


def _identity_case(handle, mode, c, split_out=0):
    """w = identity: q, k, v are the caller's.  Returns (ratio, ctx rows as stored)"""
    D, H = c["D"], c["H"]
    x, w, bias = E.att_identity_operands(c)
    qkv, ctx, what = _attention(handle, mode, c, x, w, bias, split_out)
    split = mode == 1
    if split:
        v = E.split_decode(qkv[:, 2 * D:])
        assert (np.abs(v - c["v"]) <= E.SPLIT_ST * np.abs(c["v"]) + E.SPLIT_FLOOR).all(), what + ": v rows of the product"
        d_q, d_k = E.SPLIT_ST * np.abs(c["q"]) + E.SPLIT_FLOOR, E.SPLIT_ST * np.abs(c["k"]) + E.SPLIT_FLOOR
    else:
        _same_bits(qkv, x, what + ": the float32 product with the identity is exact")
        v, d_q, d_k = c["v"], None, None
    # (split_out = False: _ratio adds the term of split-stored rows itself)
    y64, bound = E.attention_bound(c["q"], c["k"], v, c["pe"], c["nseg"], c["T"], H, c["maxlen"], split=split, split_out=False,
                                   d_q=d_q, d_k=d_k)
    return _ratio(ctx, y64, bound, what, split=split or bool(split_out)), ctx


def _random_w_case(handle, mode, T, nseg, split_out=0):
    """a realistic product: x [M][256] Gaussian, w [768][256] / 16, a bias"""
    D, K = 256, 256
    c = E.att_case("gaussian", nseg, T, D, 1000, seed=9)
    rs = np.random.RandomState(5)
    x = rs.standard_normal((nseg * T, K)).astype(np.float32)
    w = (rs.standard_normal((3 * D, K)) / 16).astype(np.float32)
    bias = (0.3 * rs.standard_normal(3 * D)).astype(np.float32)
    qkv, ctx, what = _attention(handle, mode, c, x, w, bias, split_out)
    what += " random w"
    y = x.astype(np.float64) @ w.astype(np.float64).T + bias
    terms = np.abs(x).astype(np.float64) @ np.abs(w).astype(np.float64).T + np.abs(bias)
    split = mode == 1
    # the product itself: the GEMM envelope, one rounding of the result; split: two operands at 2^-22 and the stored format
    gb = (E.ENVELOPE + (2 * E.SPLIT_OP if split else 0.0)) * terms + E.U * np.abs(y)
    if split:
        v = E.split_decode(qkv[:, 2 * D:])
        _ratio(qkv[:, 2 * D:], y[:, 2 * D:], gb[:, 2 * D:], what + " v columns", split=True)
        q, k = y[:, :D], y[:, D:2 * D]
        d_q, d_k = gb[:, :D] + E.SPLIT_ST * np.abs(q) + E.SPLIT_FLOOR, gb[:, D:2 * D] + E.SPLIT_ST * np.abs(k) + E.SPLIT_FLOOR
    else:
        _ratio(qkv, y, gb, what + " qkv")
        q, k, v, d_q, d_k = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], None, None
    y64, bound = E.attention_bound(q, k, v, c["pe"], nseg, T, c["H"], 1000, split=split, split_out=False, d_q=d_q, d_k=d_k)
    return _ratio(ctx, y64, bound, what, split=split or bool(split_out))


@pytest.mark.parametrize("mode", [0, 1])
def test_attention_short(handle, mode):
    worst = {}
    for fam, nseg, T, D, maxlen, delta in E.att_short_cases():
        c = E.att_case(fam, nseg, T, D, maxlen, delta=delta)
        r, _ = _identity_case(handle, mode, c)
        worst[fam] = max(worst.get(fam, 0.0), r)
    worst["random w"] = max(_random_w_case(handle, mode, 186, 3), _random_w_case(handle, mode, 61, 1))
    for k, r in sorted(worst.items()):
        print(f"attention mode {mode} {k}: worst error / bound {r:.3f}")


@pytest.mark.parametrize("mode", [0, 1])
def test_attention_segment_alone(handle, mode):
    """segment 2 of five against the same segment alone: the same bits"""
    for T in (33, 186):
        c = E.att_case("gaussian", 5, T, 256, 1000, seed=3)
        _, ctx5 = _identity_case(handle, mode, c)
        rows = slice(2 * T, 3 * T)
        c1 = dict(c, nseg=1, q=c["q"][rows], k=c["k"][rows], v=c["v"][rows])
        _, ctx1 = _identity_case(handle, mode, c1)
        _same_bits(ctx1, ctx5[rows], f"mode {mode} T {T}: a segment alone")


def test_attention_long(handle):
    worst = {}
    for fam, nseg, T, D, maxlen, delta in E.att_long_cases():
        c = E.att_case(fam, nseg, T, D, maxlen, delta=delta)
        r, ctx = _identity_case(handle, 2, c)
        worst[fam] = max(worst.get(fam, 0.0), r)
        if T <= 801:
            _, ctx_s = _identity_case(handle, 2, c, split_out=1)
            _same_bits(ctx_s, E.split_encode(ctx), f"mode 2 T {T}: split rows against the encoded float32 rows")
    worst["random w"] = max(_random_w_case(handle, 2, 65, 2), _random_w_case(handle, 2, 65, 2, split_out=1))
    for k, r in sorted(worst.items()):
        print(f"attention mode 2 {k}: worst error / bound {r:.3f}")


# ---- refusals (nothing is launched, nothing is written) ---------------------------------------------------------------------------

def test_refusals(handle):
    L = pkg("_lib")
    lib, h = handle.lib, handle.h
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    big = np.full(1 << 16, 3.0, np.float32)         # every input
    outs = [np.full(1 << 16, 7.0, np.float32) for _ in range(3)]

    def refused(rc, what):
        assert rc == L.CSS_ERR_INVALID_ARG, (what, rc)
        assert lib.css_last_error(h), what
        assert (big == 3.0).all() and all((o == 7.0).all() for o in outs), (what, "an array was written")

    def ln(**kw):
        f = dict(form=0, rows=4, D=256, inplace=0, x_floats=1024, out_floats=1024)
        f.update(kw)
        return lib.css_layernorm_host(h, C.byref(L.CssLayerNormDesc(**f)), p(big), p(big), p(big), None, None, p(outs[0]), None, p(outs[1]))

    def conv(**kw):
        f = dict(form=0, nseg=1, T=4, D=256, taps=33, x_floats=1024, out_floats=1024)
        f.update(kw)
        launched = C.c_int32(-5)
        rc = lib.css_conv_module_host(h, C.byref(L.CssConvModuleDesc(**f)), p(big), *([p(big)] * 9), p(outs[0]), p(outs[1]), p(outs[2]),
                                      C.byref(launched))
        assert launched.value == (-5 if rc else 1)
        return rc

    def att(**kw):
        f = dict(mode=0, nseg=1, T=4, D=256, H=4, maxlen=8, K=32, split_out=0, canary=CANARY, x_floats=128, w_floats=768 * 32,
                 pe_floats=1024, qkv_floats=4 * 768, ctx_floats=1024)
        f.update(kw)
        return lib.css_attention_host(h, C.byref(L.CssAttentionDesc(**f)), p(big), p(big), p(big), p(big), p(outs[0]), p(outs[1]))

    for D in (128, 384, 1280):
        refused(ln(D=D, x_floats=4 * D, out_floats=4 * D), f"layernorm D {D}")
        refused(conv(D=D, x_floats=4 * D, out_floats=4 * D), f"conv D {D}")
        refused(att(D=D, H=D // 64, w_floats=3 * D * 32, qkv_floats=12 * D, ctx_floats=4 * D), f"attention D {D}")
    refused(att(H=3), "D != 64 H")
    refused(att(D=512, H=4, w_floats=1536 * 32, qkv_floats=4 * 1536, ctx_floats=2048), "D != 64 H")
    for taps in (15, 16, 32, 35):
        refused(conv(taps=taps), f"taps {taps}")
        refused(conv(form=1, taps=taps), f"taps {taps}, two-kernel")
    for mode in (0, 1):
        refused(att(mode=mode, T=513, x_floats=513 * 32, qkv_floats=513 * 768, ctx_floats=513 * 256), "T > 512")
        refused(att(mode=mode, T=1, x_floats=32, qkv_floats=768, ctx_floats=256), "a one-frame segment (css_make_run_cfg refuses it too)")
    for K in (16, 48, 100):
        refused(att(K=K, x_floats=4 * K, w_floats=768 * K), f"K {K}")
    refused(ln(rows=0), "rows 0")
    refused(ln(form=4), "form")
    refused(ln(x_floats=1023), "x shorter than rows * D")
    refused(ln(out_floats=1023), "outputs shorter than rows * D")
    refused(conv(x_floats=1023), "conv x short")
    refused(conv(out_floats=1023), "conv outputs short")
    refused(conv(form=1), "the two-kernel form with x_out")
    refused(att(x_floats=127), "attention x short")
    refused(att(w_floats=768 * 32 - 1), "attention w short")
    refused(att(pe_floats=1023), "attention pe short")
    refused(att(qkv_floats=4 * 768 - 1), "attention qkv short")
    refused(att(ctx_floats=1023), "attention ctx short")
    refused(att(mode=3), "mode")
    refused(att(mode=0, split_out=1), "split_out outside mode 2")
    # and the accepted neighbours of these descriptors do run
    assert ln() == L.CSS_OK and conv() == L.CSS_OK and att() == L.CSS_OK
