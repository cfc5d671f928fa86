"""The parts of the encoder kernel tests that need no GPU (include/css_mi355_encoder.h, tests/encoder_reference.py):
  1. the header, the library's exports and SIGNATURES_ENCODER agree, the descriptors match field for field, and a NULL handle
     or descriptor is refused with the outputs untouched;
  2. the references, chained into whole Conformer blocks, reproduce the oracle (css_oracle.conformer_forward in float64) to
     1e-11 on block0 and block1 of a 2-block golden-recipe model at T = 97, with maxlen 100 and the default;
  3. every bound is reachable: on every case of the tables the oracle's formulas in float32 numpy lie inside the bound of
     the float64 result (the worst ratio per family is printed: DESIGN.md 3.2d lists them beside the kernels');
  4. no bound is vacuous: each of fourteen mutations of a reference moves at least one output element of the tables' cases by
     10 x its bound or more."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import css_oracle as O
import encoder_reference as E
from conftest import ROOT, pkg

CSRC = os.path.join(ROOT, "notsofar1-challenge_amd", "csrc")
NAMES = ("css_layernorm_host", "css_conv_module_host", "css_attention_host")
DESCS = ("CssLayerNormDesc", "CssConvModuleDesc", "CssAttentionDesc")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "css_mi355_encoder.h")).read(), flags=re.S)


# ---- 1. the binding -------------------------------------------------------------------------------------------------------------

def test_header_library_and_binding_agree():
    L = pkg("_lib")
    lib = L.load()
    text = _header()
    assert '#include "css_mi355.h"' in text
    declared = re.findall(r"\bint\s+(css_\w+)\s*\(", text)
    assert sorted(declared) == sorted(NAMES) == sorted(L.SIGNATURES_ENCODER)
    assert not set(L.SIGNATURES_ENCODER) & (set(L.SIGNATURES) | set(L.SIGNATURES_RATE) | set(L.SIGNATURES_PREVIEW) |
                                            set(L.SIGNATURES_PREVIEW_HANDOFF) | set(L.SIGNATURES_FRONTEND))
    main = open(os.path.join(ROOT, "include", "css_mi355.h")).read()
    assert len(L.SIGNATURES) == 85
    kinds = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "float": C.c_float}
    for name in NAMES:
        assert not re.search(rf"\b{name}\b", main), f"{name} belongs to css_mi355_encoder.h alone"
        params = re.search(rf"\b{name}\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
        restype, argtypes = L.SIGNATURES_ENCODER[name]
        fn = getattr(lib, name)
        assert restype is C.c_int and len(argtypes) == len(params), name
        assert fn.restype is C.c_int and list(fn.argtypes) == list(argtypes)       # load() applied the fifth table
        assert all("*" in p or p.split()[0] == "css_handle_t" for p in params), name
    for desc in DESCS:   # the header's fields in the header's order, with the header's types
        body = re.search(rf"typedef struct {desc} \{{(.*?)\}} {desc};", text, flags=re.S).group(1)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                kind, names = decl.split(None, 1)
                fields += [(n.strip(), kinds[kind]) for n in names.split(",")]
        assert fields == list(getattr(L, desc)._fields_), desc
    assert C.sizeof(L.CssLayerNormDesc) == 32 and L.CssLayerNormDesc.x_floats.offset == 16
    assert C.sizeof(L.CssConvModuleDesc) == 40 and L.CssConvModuleDesc.x_floats.offset == 24
    assert C.sizeof(L.CssAttentionDesc) == 80 and L.CssAttentionDesc.canary.offset == 32 and L.CssAttentionDesc.x_floats.offset == 40
    deps = re.findall(r"^build(?:_asan)?/%\.o:.*$", open(os.path.join(CSRC, "Makefile")).read(), flags=re.M)
    assert len(deps) == 2 and all("../../include/css_mi355_encoder.h" in d and "../../include/css_mi355_frontend.h" in d for d in deps)
    front = open(os.path.join(ROOT, "include", "css_mi355_frontend.h")).read()
    for name in NAMES + tuple(DESCS):
        assert not re.search(rf"\b{name}\b", front), f"{name} belongs to css_mi355_encoder.h alone"


def test_null_handle_and_null_descriptor_are_refused():
    L = pkg("_lib")
    lib = L.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    x = np.full(1024, 3.0, np.float32)
    w = np.ones(1024, np.float32)
    outs = [np.full(1024, 7.0, np.float32) for _ in range(3)]
    launched = C.c_int32(-5)
    dl = L.CssLayerNormDesc(form=0, rows=4, D=256, x_floats=1024, out_floats=1024)
    dc = L.CssConvModuleDesc(form=0, nseg=1, T=4, D=256, taps=33, x_floats=1024, out_floats=1024)
    da = L.CssAttentionDesc(mode=0, nseg=1, T=2, D=256, H=4, maxlen=2, K=32, canary=1, x_floats=1024, w_floats=1024, pe_floats=1024,
                            qkv_floats=1024, ctx_floats=1024)
    for d_l, d_c, d_a in ((C.byref(dl), C.byref(dc), C.byref(da)), (None, None, None)):
        assert lib.css_layernorm_host(None, d_l, p(x), p(w), p(w), None, None, p(outs[0]), None, p(outs[1])) == L.CSS_ERR_INVALID_ARG
        assert lib.css_conv_module_host(None, d_c, p(x), p(w), p(w), p(w), p(w), p(w), p(w), p(w), p(w), p(w), p(outs[0]), p(outs[1]),
                                        p(outs[2]), C.byref(launched)) == L.CSS_ERR_INVALID_ARG
        assert lib.css_attention_host(None, d_a, p(x), p(w), p(w), p(w), p(outs[0]), p(outs[1])) == L.CSS_ERR_INVALID_ARG
    assert launched.value == -5 and (x == 3.0).all() and all((o == 7.0).all() for o in outs)


# ---- 2. the references against the oracle ---------------------------------------------------------------------------------------

def _block(st, l, x, T, H, maxlen):
    """One Conformer block (conformer.py:176-185) from the references of encoder_reference.py and plain float64 products"""
    g = lambda k: np.asarray(st["executor.nnet.conformer." + k], np.float64)
    pre = f"encoders.{l}."

    def ff(name, x_):
        u = E.layer_norm(x_, g(pre + name + ".layer_norm.weight"), g(pre + name + ".layer_norm.bias"))
        u = np.maximum(u @ g(pre + name + ".net.0.weight").T + g(pre + name + ".net.0.bias"), 0)
        return u @ g(pre + name + ".net.3.weight").T + g(pre + name + ".net.3.bias")

    x = x + 0.5 * ff("feed_forward_in", x)
    u = E.layer_norm(x, g(pre + "self_attn.layer_norm.weight"), g(pre + "self_attn.layer_norm.bias"))
    q, k, v = (u @ g(pre + f"self_attn.linear_{n}.weight").T + g(pre + f"self_attn.linear_{n}.bias") for n in "qkv")
    ctx = E.relpos_attention(q, k, v, g("pos_emb.pe_k.weight"), 1, T, H, maxlen)
    x = x + ctx @ g(pre + "self_attn.linear_out.weight").T + g(pre + "self_attn.linear_out.bias")
    # the conv module's operands as weights.pack_blob hands them to the kernels, folded in float64
    pw = np.concatenate([np.stack([g(pre + "conv.pw_conv_1.weight").reshape(2), g(pre + "conv.pw_conv_1.bias").reshape(2)], 1).reshape(4),
                         g(pre + "conv.pw_conv_2.weight").reshape(1), g(pre + "conv.pw_conv_2.bias").reshape(1)])
    alpha = g(pre + "conv.BN.weight") / np.sqrt(g(pre + "conv.BN.running_var") + 1e-5)
    beta = g(pre + "conv.BN.bias") - g(pre + "conv.BN.running_mean") * alpha
    x = E.conv_module(x, g(pre + "conv.layer_norm.weight"), g(pre + "conv.layer_norm.bias"), pw, g(pre + "conv.dw_conv_1d.weight")[:, 0, :].T,
                      g(pre + "conv.dw_conv_1d.bias"), alpha, beta, 1, T)
    x = x + 0.5 * ff("feed_forward_out", x)
    return E.layer_norm(x, g(pre + "layer_norm.weight"), g(pre + "layer_norm.bias"))


@pytest.mark.parametrize("maxlen", [100, 1000])
def test_references_chain_to_the_oracle(maxlen):
    W = pkg("weights")
    T = 97
    desc = W.ModelDesc(num_blocks=2, maxlen=maxlen)
    st = W.apply_golden_recipe(W.portable_state_dict(desc, 3))
    params = O.ConformerParams(st, np.float64)
    feat = np.random.RandomState(11).standard_normal((desc.in_features, T))
    taps = {}
    O.conformer_forward(params, feat, taps=taps)
    assert params.dims().maxlen == maxlen
    x = taps["embed"]
    for l in range(2):
        x = _block(params.st, l, x, T, desc.attention_heads, maxlen)
        err = float(np.abs(x - taps[f"block{l}"]).max())
        print(f"maxlen {maxlen} block{l}: max |references - oracle| = {err:.2e}")
        assert err <= 1e-11, (l, err)


# ---- 3. and 4.: the case tables ---------------------------------------------------------------------------------------------------

def _moved(y_mut, y64, bound):
    """whether some element moved by 10 x its bound or more (a NaN counts as moved)"""
    with np.errstate(invalid="ignore"):
        return bool((~(np.abs(np.asarray(y_mut, np.float64) - y64) < 10 * bound)).any())


def _ratio(y32, y64, bound):
    assert y32.dtype == np.float32 and np.isfinite(y32).all()
    return float((np.abs(y32.astype(np.float64) - y64) / bound).max())


def _ln_evals():
    """(name, float64 result, bound, evaluate(dtype, mut)) of every LayerNorm case: plain, and with the two GLU parameter sets"""
    for c in E.ln_cases():
        tag = f"D {c['D']} rows {c['rows']}"
        y, bd = E.layer_norm_bound(c["x"], c["w"], c["b"])
        yield "layernorm " + tag, y, bd, (lambda dt, mut, c=c: E.layer_norm(c["x"], c["w"], c["b"], dt, mut))
        for pw in (E.PW_MILD, E.PW_WIDE):
            y, bd = E.ln_glu_bound(c["x"], c["w"], c["b"], pw, hw=False)
            yield f"ln_glu pw2 {pw[2]} " + tag, y, bd, (lambda dt, mut, c=c, pw=pw: E.ln_glu(c["x"], c["w"], c["b"], pw, dt, mut))


def _conv_evals():
    for fused in (True, False):
        for D, taps, nseg, T, imp in E.conv_cases(fused):
            c = E.conv_case(D, taps, nseg, T, impulse=imp)
            args = (c["x"], c["ln_w"], c["ln_b"], c["pw"], c["wt"], c["dwb"], c["alpha"], c["beta"], nseg, T)
            y, bd = E.conv_module_bound(*args, hw=False)
            yield f"conv D {D} taps {taps} nseg {nseg} T {T} impulse {imp}", y, bd, (lambda dt, mut, a=args: E.conv_module(*a, dt, mut))


def _att_evals(long):
    for fam, nseg, T, D, maxlen, delta in (E.att_long_cases() if long else E.att_short_cases()):
        c = E.att_case(fam, nseg, T, D, maxlen, delta=delta)
        args = (c["q"], c["k"], c["v"], c["pe"], nseg, T, c["H"], maxlen)
        y, bd = E.attention_bound(*args)
        yield f"attention {fam} nseg {nseg} T {T} D {D} maxlen {maxlen} delta {delta}", y, bd, \
            (lambda dt, mut, a=args: E.relpos_attention(*a, dt, mut))


FAMILIES = {"layernorm": _ln_evals, "conv": _conv_evals, "attention": lambda: _att_evals(False), "attention_long": lambda: _att_evals(True)}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_float32_numpy_lies_inside_every_bound(family):
    worst = {}
    for name, y64, bound, ev in FAMILIES[family]():
        r = _ratio(ev(np.float32, None), y64, bound)
        key = " ".join(name.split()[:2])
        worst[key] = max(worst.get(key, 0.0), r)
        assert r <= 1.0, (name, r)
    for key, r in sorted(worst.items()):
        print(f"float32 numpy / bound, {key}: {r:.3f}")


MUTATIONS = [("layernorm", "var_dm1"), ("layernorm", "eps_1e-6"), ("layernorm", "glu_swapped"),
             ("conv", "taps_reversed"), ("conv", "pad_neighbour"), ("conv", "relu_first"), ("conv", "no_pw5"), ("conv", "residual_next"),
             ("attention", "offset_plus"), ("attention", "offset_minus"), ("attention", "clamp_symmetric"), ("attention", "no_clamp"),
             ("attention", "scale_63"), ("attention", "unmasked_keys"), ("attention", "no_max")]


@pytest.mark.parametrize("family, mut", MUTATIONS)
def test_mutation_is_caught(family, mut):
    """(offset i - j +- 1 is two mutations; the first case that catches one ends the search)"""
    for name, y64, bound, ev in FAMILIES[family]():
        if _moved(ev(np.float64, mut), y64, bound):
            print(f"{mut}: caught on {name}")
            return
    pytest.fail(f"no case of the {family} tables moves by 10 x its bound under {mut}")
