"""Encoder windows of whole sessions (include/css_mi355_session_window.h; _lib.SessionWindows, Handle.run_enqueue_windows), the part
that needs no GPU: the header, the library and the binding table agree, the struct is laid out as the C compiler lays it out, a
NULL handle is refused, css_session_window_bounds is the stated arithmetic, stream.session_windows is the rule of the header, and
the window kernel compiles without scratch."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT, pkg

CSRC = os.path.join(ROOT, "notsofar1-challenge_amd", "csrc")
HEADER = "css_mi355_session_window.h"
NAMES = ("css_session_window_bounds", "css_handoff_windows_all", "css_run_enqueue_windows", "css_run_enqueue_pcm16_windows",
         "css_session_window_stats")
FIELDS = ["width", "stride", "dtype", "reserved", "windows_dev", "ld", "cap_windows", "mel_dev", "mel_ld", "n_windows", "window_max"]
HOP, FRAME = 256, 512


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)


def test_header_library_and_binding_agree():
    L = pkg("_lib")
    lib = L.load()
    text = _header()
    assert '#include "css_mi355_session_handoff.h"' in text
    declared = re.findall(r"\bint\s+(css_\w+)\s*\(", text)
    assert sorted(declared) == sorted(NAMES) == sorted(L.SESSION_WINDOW_BINDINGS)
    # the table is the module's own kind: neither a SIGNATURES... nor a ..._SIGNATURES one, and it shares no name with those
    tables = {n: getattr(L, n) for n in dir(L) if n.startswith("SIGNATURES") or n.endswith("_SIGNATURES")}
    assert "SESSION_WINDOW_BINDINGS" not in tables and len(tables) >= 13 and len(L.SIGNATURES) == 85
    for n, t in tables.items():
        assert not set(L.SESSION_WINDOW_BINDINGS) & set(t), n
    for f in os.listdir(os.path.join(ROOT, "include")):
        if f != HEADER:
            other = open(os.path.join(ROOT, "include", f)).read()
            for name in NAMES + ("CssSessionWindows",):
                assert not re.search(rf"\b{name}\b", other), f"{name} belongs to {HEADER} alone"
    kinds = {"css_handle_t": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64}
    for name in NAMES:
        fn = getattr(lib, name)   # (AttributeError: the library does not export it)
        params = re.search(rf"\b{name}\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
        restype, argtypes = L.SESSION_WINDOW_BINDINGS[name]
        assert restype is C.c_int and len(argtypes) == len(params), (name, params)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(argtypes)   # load() applied the table
        for p, a in zip(params, argtypes):
            p = p.strip()
            if "*" in p:
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p, a)
            else:
                assert a is kinds[p.split()[0]], (name, p, a)
    # the constants are css_mi355_window.h's
    assert L.WINDOW_DTYPES == {"float32": 0, "float16": 1} and L.WINDOW_MAX_WIDTH == 3000
    # the Makefile rebuilds on the header and lists the new unit
    mk = open(os.path.join(CSRC, "Makefile")).read()
    deps = re.findall(r"^build(?:_asan)?/%\.o:.*$", mk, flags=re.M)
    assert len(deps) == 2 and all(f"../../include/{HEADER}" in d and "../../include/css_mi355_session_handoff.h" in d for d in deps)
    assert "api_session_window.hip" in re.search(r"^SRCS\s*:=(.*)$", mk, flags=re.M).group(1).split()
    # the kernel's name does not contain the names the session hand-off's test looks for
    assert not any(k in "session_window_kernel" for k in ("session_keep_scan_kernel", "session_gather_kernel", "session_norm_kernel"))


def test_struct_layout_is_the_compilers():
    """sizeof / offsetof of CssSessionWindows from a compiled C99 probe against the ctypes mirror"""
    L = pkg("_lib")
    body = re.search(r"typedef struct CssSessionWindows \{(.*?)\} CssSessionWindows;", _header(), flags=re.S).group(1)
    members = [re.sub(r"\s+", " ", m).strip().split()[-1].lstrip("*") for m in body.split(";") if m.strip()]
    T = L.CssSessionWindows
    assert members == FIELDS == [n for n, _ in T._fields_]
    src = ('#include <stddef.h>\n#include <stdio.h>\n#include "' + HEADER + '"\nint main(void) {\n'
           '    printf("%zu", sizeof(CssSessionWindows));\n' +
           "".join(f'    printf(" %zu", offsetof(CssSessionWindows, {n}));\n' for n in FIELDS) + "    return 0;\n}\n")
    with tempfile.TemporaryDirectory() as d:
        c_file, exe = os.path.join(d, "probe.c"), os.path.join(d, "probe")
        open(c_file, "w").write(src)
        cc = "/opt/rocm/lib/llvm/bin/clang" if os.path.exists("/opt/rocm/lib/llvm/bin/clang") else "cc"
        subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), c_file, "-o", exe], check=True,
                       capture_output=True, timeout=120)
        got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.split()]
    assert got == [C.sizeof(T)] + [getattr(T, n).offset for n in FIELDS] == [72, 0, 4, 8, 12, 16, 24, 32, 40, 48, 56, 64]


def test_null_handle_is_refused_with_nothing_written():
    L = pkg("_lib")
    lib = L.load()
    ho = L.SessionHandoff(3, 80, 100, 4, pinned=False, fill=-7)
    hcfg = L.handoff_cfg()
    nw = np.full(3, -7, np.int32)
    wm = np.full(3, -7, np.float32)
    win = L.CssSessionWindows(96, 64, 1, 0, 4096, 96, 2, None, 0, nw.ctypes.data, wm.ctypes.data)
    x = np.zeros((4000, 7), np.float32)
    wav = np.full((3, 8192), 5.0, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.css_handoff_windows_all(None, p(wav), 8192, C.byref(hcfg), C.byref(ho.c), C.byref(win)) == L.CSS_ERR_INVALID_ARG
    assert lib.css_handoff_windows_all(None, None, 0, None, None, None) == L.CSS_ERR_INVALID_ARG
    assert lib.css_run_enqueue_windows(None, p(x), 4000, 7, None, p(wav), 8192, C.byref(hcfg), C.byref(ho.c), C.byref(win)) == L.CSS_ERR_INVALID_ARG
    assert lib.css_run_enqueue_pcm16_windows(None, None, 4000, 7, None, p(wav), 8192, None, C.byref(hcfg), C.byref(ho.c),
                                             C.byref(win)) == L.CSS_ERR_INVALID_ARG
    a, b = C.c_int64(-7), C.c_int64(-7)
    assert lib.css_session_window_stats(None, C.byref(a), C.byref(b)) == L.CSS_ERR_INVALID_ARG
    f, r, w = C.c_int64(-7), C.c_int32(-7), C.c_int64(-7)
    assert lib.css_session_window_bounds(None, None, None, 96, 64, 4000, C.byref(f), C.byref(r), C.byref(w)) == L.CSS_ERR_INVALID_ARG
    assert (a.value, b.value, f.value, r.value, w.value) == (-7,) * 5 and (wav == 5.0).all()
    assert (nw == -7).all() and (wm == -7).all()
    assert (ho.mel_all == -7).all() and (ho.ranges_all == -7).all() and (ho.n_frames == -7).all() and (ho.n_ranges == -7).all()


# ---- the bounds ---------------------------------------------------------------------------------------------------------------------

def _one_frame_cfg():
    """segments of one frame, so that every TL >= 1 is a plan's (tests/test_session_handoff_host.py _lib_bounds)"""
    L = pkg("_lib")
    w = np.ones(1, np.float32)
    return L.RunCfg(1, 1, 0, 0, True, 0, 0, False, 0.0, 0.3, w, w, w)


def test_bounds_are_the_closed_form():
    """frames = n_out // 160 with n_out = (TL + 1) 256, ranges as css_session_handoff_bounds, windows = ceil(frames / stride):
    stream lengths on both sides of every multiple of 160 samples, strides on both sides of the divisors of the frame count"""
    L, W = pkg("_lib"), pkg("weights")
    desc, rc = W.ModelDesc(num_blocks=2), _one_frame_cfg()
    seen = set()
    for TL in list(range(1, 41)) + [186, 187, 374, 375, 1874, 1875, 1876]:
        n = (TL - 1) * HOP + FRAME
        n_out = (TL + 1) * HOP
        frames = n_out // 160
        seen.add(n_out % 160)
        for pad, drop in ((8, True), (0, True), (8, False)):
            hcfg = L.handoff_cfg(80, pad, drop)
            f0, r0 = L.session_handoff_bounds(desc, rc, hcfg, n)
            assert f0 == frames
            strides = {1, 2, 7, 64, 100, 3000}
            for d in (frames, frames // 2, frames // 3):
                strides |= {s for s in (d - 1, d, d + 1) if 1 <= s <= 3000}
            for stride in sorted(strides):
                got = L.session_window_bounds(desc, rc, hcfg, 3000, stride, n)
                assert got == (frames, r0, -(-frames // stride)), (TL, stride, got)
                assert (got[2] - 1) * stride < frames <= got[2] * stride
    assert {0, 96, 32, 128, 64} <= seen   # every residue of a 256-sample block count modulo 160
    # the default segmentation, recordings around multiples of 160 samples
    rc = pkg("css").make_run_cfg(pkg("css").CssCfg(show_progressbar=False), 16000, 7)
    for n in (159, 160, 161, 47999, 48000, 48001, 96000 - 1, 96000, 96000 + 1, 16000 * 60):
        pl = L.plan(desc, rc, n)
        for width, stride in ((3000, 3000), (96, 64), (64, 7), (1, 1)):
            frames = int(pl.n_out) // 160
            assert L.session_window_bounds(desc, rc, L.handoff_cfg(), width, stride, n)[::2] == (frames, -(-frames // stride))
    for width, stride in ((0, 1), (3001, 3000), (96, 0), (96, 97), (-1, -1)):
        with pytest.raises(L.CssError):
            L.session_window_bounds(desc, rc, L.handoff_cfg(), width, stride, 48000)
    with pytest.raises(L.CssError):
        L.session_window_bounds(desc, rc, L.handoff_cfg(64, 8, True), 96, 64, 48000)


# ---- the numpy statement ------------------------------------------------------------------------------------------------------------

def _raw(n_mels, J, seed):
    rs = np.random.RandomState(seed)
    raw = (rs.randn(n_mels, J) * 2.0 - 3.0).astype(np.float32)
    raw[rs.rand(n_mels, J) < 0.1] = -10.0
    return raw


@pytest.mark.parametrize("dtype", ("float32", "float16"))
def test_one_window_over_all_frames_is_whisper_window(dtype):
    S = pkg("stream")
    for J, width in ((1, 1), (1, 96), (95, 96), (96, 96), (2999, 3000), (3000, 3000)):
        raw = _raw(80, J, J)
        got = S.session_windows(S.whisper_normalize(raw), raw.max(), width, width, dtype)
        want = S.whisper_window(raw, width, dtype)
        assert got.shape == (1, 80, width) and got.dtype == want.dtype and np.array_equal(got[0], want)


@pytest.mark.parametrize("width,stride", ((96, 64), (64, 7), (100, 100), (96, 96), (3000, 3000), (1, 1)))
def test_windows_tile_the_normalised_frames(width, stride):
    """stride < width, stride = width, J a multiple of the stride, J = 1, J = 0"""
    S = pkg("stream")
    for J in sorted({0, 1, stride - 1, stride, stride + 1, width, width + 1, 2 * stride, 3 * stride, 3 * stride + 5} - {-1}):
        raw = _raw(128, max(J, 1), 7 * J + width)[:, :J]
        M = np.float32(raw.max()) if J else np.float32(-3.0)
        mel = S.whisper_normalize(raw, M)
        fill = (max(np.float32(-10.0), M - np.float32(8.0)) + np.float32(4.0)) * np.float32(0.25)
        assert np.float32(fill) == S.session_window_fill(M)
        for dtype in ("float32", "float16"):
            got = S.session_windows(mel, M, width, stride, dtype)
            n = -(-J // stride)
            assert got.shape == (n, 128, width) and got.dtype == np.dtype(dtype)
            for w in range(n):
                k = min(width, J - w * stride)
                assert k >= 1
                assert np.array_equal(got[w, :, :k], mel[:, w * stride:w * stride + k].astype(dtype))
                assert (got[w, :, k:] == np.float32(fill).astype(dtype)).all()
            if n:
                assert (n - 1) * stride < J   # the last window holds a frame
    for bad in ((0, 1), (3001, 1), (96, 0), (96, 97)):
        with pytest.raises(ValueError):
            S.session_windows(np.zeros((80, 4), np.float32), 0.0, *bad)
    with pytest.raises(ValueError):
        S.session_windows(np.zeros((80, 4), np.float32), 0.0, 96, 64, "float64")


# ---- the kernel's resources ---------------------------------------------------------------------------------------------------------

def test_window_kernel_compiles_without_scratch_or_spills():
    """handoff.hip for gfx950 with the Makefile's own flags; the compiler's resource report for session_window_kernel"""
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, flags=re.M).group(1)
    flags = [f.replace("$(ARCH)", arch) for f in re.search(r"^CXXFLAGS\s*\?=\s*(.*)$", text, flags=re.M).group(1).split()]
    assert arch == "gfx950" and "-O3" in flags
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
                                                                 "-I" + CSRC, os.path.join(CSRC, "handoff.hip"), "-o", os.path.join(d, "handoff.o")],
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
    mine = {k: v for k, v in usage.items() if "session_window_kernel" in k}
    assert len(mine) == 1, sorted(usage)
    (k, v), = mine.items()
    print(k, v)
    assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
    assert v["LDS Size [bytes/block]"] == 0 and v["Occupancy [waves/SIMD]"] >= 4, (k, v)
