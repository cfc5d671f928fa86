"""Whole sessions at the capture rate (include/css_mi355_session_rate.h), the part that needs no GPU: the header against the
library's exports and the binding table, css_session_rate_samples against the closed forms and against css_stream_rate_samples
composed with css_plan, the refusals on a null handle or a bad argument, and the two new kernels compiled for gfx950 with the
shipped flags without scratch or spills (the manner of test_stream_rate_host.py / test_stream_output_host.py).

The binding table is ``_lib.SESSION_RATE_SIGNATURES`` (not SIGNATURES_...: tests/test_backend_reference.py counts the module's
SIGNATURES... tables, the reason ARRAY_SIGNATURES carries its name)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT, pkg
from test_stream_output_host import _makefile_flags, _points

CSRC = os.path.join(ROOT, "notsofar1-challenge_amd", "csrc")
NAMES = ("css_session_rate_samples", "css_run_rate", "css_run_pcm16_rate", "css_run_enqueue_rate", "css_run_enqueue_pcm16_rate",
         "css_session_rate_stats")
RATIOS = ((1, 3), (160, 441), (2, 1), (3, 1), (441, 160), (1, 2), (1, 1))
BAD_RATIOS = ((2, 2), (2, 4), (6, 2), (1, 7), (0, 1), (1, 0), (0, 0), (-3, 1), (3, -1), (820, 1), (1, 820))


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "css_mi355_session_rate.h")).read(), flags=re.S)


def _desc_cfg():
    L, CSS, W = pkg("_lib"), pkg("css"), pkg("weights")
    desc = W.ModelDesc(num_blocks=2)
    return desc, CSS.make_run_cfg(CSS.CssCfg(segment_size_sec=2.0, hop_size_sec=0.5), 16000, 7)


def test_header_library_and_binding_agree():
    L = pkg("_lib")
    text = _header()
    lib = L.load()
    assert '#include "css_mi355_rate.h"' in text
    declared = re.findall(r"\bint\s+(css_\w+)\s*\(", text)
    assert sorted(declared) == sorted(NAMES) == sorted(L.SESSION_RATE_SIGNATURES)
    others = [getattr(L, n) for n in dir(L) if (n.startswith("SIGNATURES") or n.endswith("_SIGNATURES")) and n != "SESSION_RATE_SIGNATURES"]
    assert len(others) == 12 and not any(set(L.SESSION_RATE_SIGNATURES) & set(t) for t in others)
    kinds = {"css_handle_t": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64}
    for name in NAMES:
        for other in os.listdir(os.path.join(ROOT, "include")):
            if other != "css_mi355_session_rate.h":
                assert not re.search(rf"\b{name}\b", open(os.path.join(ROOT, "include", other)).read()), (name, other)
        fn = getattr(lib, name)   # (AttributeError: the library does not export it)
        params = re.search(rf"\b{name}\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
        restype, argtypes = L.SESSION_RATE_SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == len(params), (name, params)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(argtypes)   # load() applied the table
        for p, a in zip(params, argtypes):
            p = p.strip()
            if "*" in p:
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p, a)
            else:
                assert a is kinds[p.split()[0]], (name, p, a)
    body = re.search(r"typedef struct CssSessionRate \{(.*?)\}", text, flags=re.S).group(1)
    assert " ".join(body.split()) == "int32_t in_up, in_down; int32_t out_up, out_down;"
    assert [f[0] for f in L.CssSessionRate._fields_] == ["in_up", "in_down", "out_up", "out_down"] and C.sizeof(L.CssSessionRate) == 16
    mk = open(os.path.join(CSRC, "Makefile")).read()
    deps = re.findall(r"^build(?:_asan)?/%\.o:.*$", mk, flags=re.M)
    assert len(deps) == 2 and all("css_mi355_session_rate.h" in d for d in deps)
    assert "api_session_rate.hip" in re.search(r"^SRCS\s*:=\s*(.*)$", mk, flags=re.M).group(1).split()


def test_session_rate_helper():
    L = pkg("_lib")
    f = lambda r: (r.in_up, r.in_down, r.out_up, r.out_down)
    assert f(L.session_rate()) == (1, 1, 1, 1)
    assert f(L.session_rate(48000)) == (1, 3, 1, 1)
    assert f(L.session_rate(48000, 48000)) == (1, 3, 3, 1)
    assert f(L.session_rate(44100, 44100)) == (160, 441, 441, 160)
    assert f(L.session_rate(8000, 16000)) == (2, 1, 1, 1)
    assert f(L.session_rate(None, 8000)) == (1, 1, 1, 2)
    assert f(L.session_rate(16000, 48000)) == (1, 1, 3, 1)
    CSS = pkg("css")
    assert CSS.session_rates(16000) == (16000, 16000, None) and CSS.session_rates(48000) == (48000, 48000, None)
    assert CSS.session_rates(16000, 16000, "input") == (16000, 16000, None)
    fs, out_sr, r = CSS.session_rates(48000, 16000)
    assert (fs, out_sr, f(r)) == (16000, 16000, (1, 3, 1, 1))
    fs, out_sr, r = CSS.session_rates(48000, 16000, "input")
    assert (fs, out_sr, f(r)) == (16000, 48000, (1, 3, 3, 1))
    fs, out_sr, r = CSS.session_rates(16000, None, 8000)
    assert (fs, out_sr, f(r)) == (16000, 8000, (1, 1, 1, 2))


@pytest.mark.parametrize("ratio", RATIOS, ids=lambda r: f"{r[0]}_{r[1]}")
def test_counts_are_the_rate_rule_composed_with_the_plan(ratio):
    """the ratio on the input side (1 / 1 on the output side), then on the output side (1 / 1 on the input side)"""
    L = pkg("_lib")
    desc, cfg = _desc_cfg()
    up, down = ratio
    ceil_rate = lambda n: n if (up, down) == (1, 1) else L.stream_rate_samples(up, down, n, True)
    for n in (p for p in _points(up, down) if 1 <= p <= 2 ** 40):
        n_model, n_out_model, n_out = L.session_rate_samples(desc, cfg, L.CssSessionRate(up, down, 1, 1), n)
        assert n_model == -(-n * up // down) == ceil_rate(n), (ratio, n)
        assert n_out_model == n_out == L.plan(desc, cfg, n_model).n_out, (ratio, n)
        n_model, n_out_model, n_out = L.session_rate_samples(desc, cfg, L.CssSessionRate(1, 1, up, down), n)
        assert n_model == n and n_out_model == L.plan(desc, cfg, n).n_out
        assert n_out == -(-n_out_model * up // down) == ceil_rate(n_out_model), (ratio, n)
    # both sides at once
    n_model, n_out_model, n_out = L.session_rate_samples(desc, cfg, L.CssSessionRate(up, down, down, up), 100001)
    assert (n_model, n_out_model, n_out) == (-(-100001 * up // down), L.plan(desc, cfg, n_model).n_out, -(-n_out_model * down // up))


def test_refusals_leave_the_out_words():
    L = pkg("_lib")
    lib = L.load()
    mdesc, cfg = _desc_cfg()
    desc = L.make_desc(mdesc)
    ok = L.CssSessionRate(1, 3, 3, 1)
    a, b, c = C.c_int64(-7), C.c_int64(-8), C.c_int64(-9)
    out = (C.byref(a), C.byref(b), C.byref(c))
    E = L.CSS_ERR_INVALID_ARG
    call = lib.css_session_rate_samples
    assert call(None, C.byref(cfg.c), C.byref(ok), 48000, *out) == E
    assert call(C.byref(desc), None, C.byref(ok), 48000, *out) == E
    assert call(C.byref(desc), C.byref(cfg.c), None, 48000, *out) == E
    for k in range(3):
        args = list(out)
        args[k] = None
        assert call(C.byref(desc), C.byref(cfg.c), C.byref(ok), 48000, *args) == E
    for n in (0, -1, 2 ** 40 + 1):
        assert call(C.byref(desc), C.byref(cfg.c), C.byref(ok), n, *out) == E, n
    for up, down in BAD_RATIOS:
        for bad in (L.CssSessionRate(up, down, 1, 1), L.CssSessionRate(1, 1, up, down), L.CssSessionRate(up, down, down, up)):
            assert call(C.byref(desc), C.byref(cfg.c), C.byref(bad), 48000, *out) == E, (up, down)
        with pytest.raises(L.CssError):
            L.session_rate_samples(mdesc, cfg, L.CssSessionRate(up, down, 1, 1), 48000)
    assert (a.value, b.value, c.value) == (-7, -8, -9)
    assert call(C.byref(desc), C.byref(cfg.c), C.byref(ok), 2 ** 40, *out) == L.CSS_OK and a.value == -(-2 ** 40 // 3)
    # a null handle: every call that takes one, and nothing is written
    a, b, c = C.c_int64(-7), C.c_int64(-8), C.c_int64(-9)
    x = np.zeros((4800, 7), np.float32)
    wav = np.full((3, 64), 5.0, np.float32)
    w16 = np.full((3, 64), 5, np.int16)
    peaks = np.full(3, 5.0, np.float32)
    planes = [np.zeros(4800, np.int16) for _ in range(7)]
    ptrs = (C.c_void_p * 7)(*[p.ctypes.data for p in planes])
    P = lambda arr: arr.ctypes.data_as(C.c_void_p)
    for fn in (lib.css_run_rate, lib.css_run_enqueue_rate):
        assert fn(None, P(x), 4800, 7, C.byref(cfg.c), C.byref(ok), P(wav), 64) == E
    for fn in (lib.css_run_pcm16_rate, lib.css_run_enqueue_pcm16_rate):
        assert fn(None, ptrs, 4800, 7, C.byref(cfg.c), C.byref(ok), P(w16), 64, P(peaks)) == E
    assert lib.css_session_rate_stats(None, C.byref(a), C.byref(b), C.byref(c)) == E
    assert (a.value, b.value, c.value) == (-7, -8, -9)
    assert np.all(wav == 5.0) and np.all(w16 == 5) and np.all(peaks == 5.0)


def test_session_kernels_compile_without_scratch_or_spills():
    """resample.hip for gfx950 with the Makefile's own flags; the compiler's resource report for the two session kernels"""
    flags, arch = _makefile_flags()
    assert arch == "gfx950" and "-O3" in flags
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
                                                                 "-I" + CSRC, os.path.join(CSRC, "resample.hip"), "-o", os.path.join(d, "resample.o")],
                             capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    usage, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"remark: +([^:]+): (\d+)", line)
        if m and name:
            usage[name][m.group(1).strip()] = int(m.group(2))
    for kernel in ("session_ingest_resample_kernel", "session_output_kernel"):
        mine = {k: v for k, v in usage.items() if kernel in k}
        assert len(mine) == 1, sorted(usage)
        (k, v), = mine.items()
        print(k, v)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
