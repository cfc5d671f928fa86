"""The hand-off of whole sessions (include/css_mi355_session_handoff.h; _lib.SessionHandoff, Handle.run_enqueue_handoff), the part
that needs no GPU: the header, the library and the binding table agree, the struct is laid out as the C compiler lays it out, a
NULL handle is refused, css_session_handoff_bounds is attained by the densest gate and never exceeded, the block rule the
keep-scan kernel implements is the host's range rule, and the new kernels compile without scratch."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT, pkg

CSRC = os.path.join(ROOT, "notsofar1-challenge_amd", "csrc")
HEADER = "css_mi355_session_handoff.h"
OTHERS = ("css_mi355.h", "css_mi355_rate.h", "css_mi355_preview.h", "css_mi355_preview_handoff.h", "css_mi355_encoder.h",
          "css_mi355_window.h", "css_mi355_present_window.h", "css_mi355_frontend.h")
NAMES = ("css_session_handoff_bounds", "css_handoff_logmel_all", "css_run_enqueue_handoff", "css_run_enqueue_pcm16_handoff")
HOP, FRAME = 256, 512


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)


def test_header_library_and_binding_agree():
    L = pkg("_lib")
    lib = L.load()
    text = _header()
    assert '#include "css_mi355.h"' in text
    declared = re.findall(r"\bint\s+(css_\w+)\s*\(", text)
    assert sorted(declared) == sorted(NAMES) == sorted(L.SIGNATURES_SESSION_HANDOFF)
    assert not set(L.SIGNATURES_SESSION_HANDOFF) & (set(L.SIGNATURES) | set(L.SIGNATURES_RATE) | set(L.SIGNATURES_PREVIEW) |
                                                    set(L.SIGNATURES_PREVIEW_HANDOFF) | set(L.SIGNATURES_ENCODER) |
                                                    set(L.SIGNATURES_WINDOW) | set(L.SIGNATURES_PRESENT) | set(L.SIGNATURES_FRONTEND))
    assert len(L.SIGNATURES) == 85
    others = [open(os.path.join(ROOT, "include", f)).read() for f in OTHERS]
    for name in NAMES + ("CssSessionHandoffOut", "CSS_SESSION_SCAN_CHUNK"):
        for other in others:
            assert not re.search(rf"\b{name}\b", other), f"{name} belongs to {HEADER} alone"
    kinds = {"css_handle_t": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64}
    for name in NAMES:
        fn = getattr(lib, name)   # (AttributeError: the library does not export it)
        params = re.search(rf"\b{name}\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
        restype, argtypes = L.SIGNATURES_SESSION_HANDOFF[name]
        assert restype is C.c_int and len(argtypes) == len(params), (name, params)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(argtypes)   # load() applied the table
        for p, a in zip(params, argtypes):
            p = p.strip()
            if "*" in p:
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p, a)
            else:
                assert a is kinds[p.split()[0]], (name, p, a)
    # the scan step: the header's, the binding's and the kernel's are one number
    macro = int(re.search(r"#define\s+CSS_SESSION_SCAN_CHUNK\s+(\d+)", text).group(1))
    kern = open(os.path.join(CSRC, "kernels.hpp")).read()
    assert macro == L.SESSION_SCAN_CHUNK == int(re.search(r"constexpr int SESSION_SCAN_CHUNK = (\d+);", kern).group(1))
    # the Makefile rebuilds on the header and lists the new unit
    mk = open(os.path.join(CSRC, "Makefile")).read()
    deps = re.findall(r"^build(?:_asan)?/%\.o:.*$", mk, flags=re.M)
    assert len(deps) == 2 and all(f"../../include/{hd}" in d for d in deps for hd in OTHERS + (HEADER,))
    assert "api_session_handoff.hip" in re.search(r"^SRCS\s*:=(.*)$", mk, flags=re.M).group(1).split()


def test_struct_layout_is_the_compilers():
    """sizeof / offsetof of CssSessionHandoffOut from a compiled probe against the ctypes mirror"""
    L = pkg("_lib")
    body = re.search(r"typedef struct CssSessionHandoffOut \{(.*?)\} CssSessionHandoffOut;", _header(), flags=re.S).group(1)
    members = [re.sub(r"\s+", " ", m).strip() for m in body.split(";") if m.strip()]
    assert members == ["float* mel_host", "int64_t cap_frames", "int64_t* ranges_host", "int32_t cap_ranges", "int64_t* n_frames",
                       "int32_t* n_ranges"]
    T = L.CssSessionHandoffOut
    names = [n for n, _ in T._fields_]
    assert names == ["mel_host", "cap_frames", "ranges_host", "cap_ranges", "n_frames", "n_ranges"]
    src = ('#include <stddef.h>\n#include <stdio.h>\n#include "css_mi355_session_handoff.h"\nint main(void) {\n'
           '    printf("%zu", sizeof(CssSessionHandoffOut));\n' +
           "".join(f'    printf(" %zu", offsetof(CssSessionHandoffOut, {n}));\n' for n in names) + "    return 0;\n}\n")
    with tempfile.TemporaryDirectory() as d:
        c_file, exe = os.path.join(d, "probe.c"), os.path.join(d, "probe")
        open(c_file, "w").write(src)
        cc = "/opt/rocm/lib/llvm/bin/clang" if os.path.exists("/opt/rocm/lib/llvm/bin/clang") else "cc"
        subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), c_file, "-o", exe], check=True,
                       capture_output=True, timeout=120)
        got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.split()]
    assert got == [C.sizeof(T)] + [getattr(T, n).offset for n in names] == [48, 0, 8, 16, 24, 32, 40]


def test_null_handle_is_refused_with_nothing_written():
    L = pkg("_lib")
    lib = L.load()
    ho = L.SessionHandoff(3, 80, 100, 4, pinned=False, fill=-7)
    hcfg = L.handoff_cfg()
    x = np.zeros((4000, 7), np.float32)
    wav = np.full((3, 8192), 5.0, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.css_handoff_logmel_all(None, p(wav), 8192, C.byref(hcfg), C.byref(ho.c)) == L.CSS_ERR_INVALID_ARG
    assert lib.css_run_enqueue_handoff(None, p(x), 4000, 7, None, p(wav), 8192, C.byref(hcfg), C.byref(ho.c)) == L.CSS_ERR_INVALID_ARG
    assert lib.css_run_enqueue_pcm16_handoff(None, None, 4000, 7, None, p(wav), 8192, None, C.byref(hcfg), C.byref(ho.c)) == L.CSS_ERR_INVALID_ARG
    assert lib.css_handoff_logmel_all(None, None, 0, None, None) == L.CSS_ERR_INVALID_ARG
    f, r = C.c_int64(-7), C.c_int32(-7)
    assert lib.css_session_handoff_bounds(None, None, None, 4000, C.byref(f), C.byref(r)) == L.CSS_ERR_INVALID_ARG
    assert (f.value, r.value) == (-7, -7) and (wav == 5.0).all()
    assert (ho.mel_all == -7).all() and (ho.ranges_all == -7).all() and (ho.n_frames == -7).all() and (ho.n_ranges == -7).all()


# ---- the bounds and the range rule ------------------------------------------------------------------------------------------------

def _setup():
    W, css = pkg("weights"), pkg("css")
    desc = W.ModelDesc(num_blocks=2)
    return desc, css.make_run_cfg(css.CssCfg(show_progressbar=False), 16000, 7)


def _samples(TL):
    """a recording of exactly TL analysis frames"""
    return (TL - 1) * HOP + FRAME


def _block_rule(act, pad):
    """the rule of the header, in numpy: block q of 256 samples is kept iff a frame of [q - pad - 1, q + pad] is active; ranges are
    the maximal runs of kept blocks times 256"""
    TL = act.shape[0]
    keep = np.zeros(TL + 1, bool)
    for q in range(TL + 1):
        keep[q] = act[max(q - pad - 1, 0):min(q + pad, TL - 1) + 1].any()
    edge = np.diff(np.concatenate([[0], keep.astype(np.int8), [0]]))
    return np.stack([np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)], axis=1).astype(np.int64) * HOP, int(keep.sum()) * HOP


def _bound(TL, pad):
    return (TL - 1) // (2 * pad + 3) + 1


def _lib_bounds(TL, pad, drop=True):
    """css_session_handoff_bounds for a stream of TL frames: segments of one frame, so that every TL >= 1 is a plan's"""
    L = pkg("_lib")
    w = np.ones(1, np.float32)
    rc = L.RunCfg(1, 1, 0, 0, True, 0, 0, False, 0.0, 0.3, w, w, w)
    return L.session_handoff_bounds(pkg("weights").ModelDesc(num_blocks=2), rc, L.handoff_cfg(80, pad, drop), _samples(TL))


def test_bounds_are_the_stated_arithmetic():
    L = pkg("_lib")
    desc, rc = _setup()
    T = int(rc.c.segment_frames)
    for TL in (T, T + 1, 375, 1024):
        n = _samples(TL)
        pl = L.plan(desc, rc, n)
        assert int(pl.mix_frames) == TL and int(pl.n_out) == (TL + 1) * HOP
        for pad in (0, 1, 8, 40, 4096):
            assert L.session_handoff_bounds(desc, rc, L.handoff_cfg(80, pad, True), n) == (int(pl.n_out) // 160, _bound(TL, pad))
            assert L.session_handoff_bounds(desc, rc, L.handoff_cfg(128, pad, False), n) == (int(pl.n_out) // 160, 1)
    # a recording shorter than a segment is padded to one
    assert L.session_handoff_bounds(desc, rc, L.handoff_cfg(80, 0, True), 4000) == ((T + 1) * HOP // 160, _bound(T, 0))
    for bad in (L.handoff_cfg(64, 8, True), L.handoff_cfg(80, -1, True), L.handoff_cfg(80, 4097, True)):
        with pytest.raises(L.CssError):
            L.session_handoff_bounds(desc, rc, bad, 40000)
    with pytest.raises(L.CssError):
        L.session_handoff_bounds(pkg("weights").ModelDesc(num_blocks=2, frame_len=400, frame_hop=160, num_bins=201, in_features=1407), rc, L.handoff_cfg(), 40000)


@pytest.mark.parametrize("pad", (0, 1, 8))
def test_densest_gate_attains_the_range_bound(pad):
    """one active frame every 2 pad + 3 frames from frame 0: exactly css_session_handoff_bounds' ranges"""
    L = pkg("_lib")
    for TL in (1, 2, 186, 187):
        act = np.zeros(TL, np.uint8)
        act[::2 * pad + 3] = 1
        n_out = (TL + 1) * HOP
        reg = L.handoff_kept_ranges(act, 0, TL, pad, 0, n_out, n_out)
        frames, ranges = _lib_bounds(TL, pad)
        assert len(reg) == ranges == _bound(TL, pad), (TL, pad)
        assert frames == n_out // 160 and _lib_bounds(TL, pad, False) == (frames, 1)
        mine, n_act = _block_rule(act, pad)
        assert np.array_equal(mine, reg) and n_act == int((reg[:, 1] - reg[:, 0]).sum())
        assert n_act // 160 <= n_out // 160


def test_random_gates_stay_inside_the_bounds_and_follow_the_block_rule():
    L = pkg("_lib")
    rs = np.random.RandomState(19)
    for i in range(200):
        TL = int(rs.choice([1, 2, 3, 7, 79, 186, 187, 375, 1024])) if i % 2 else int(rs.randint(1, 80))
        pad = int(rs.choice([0, 1, 2, 8, 40]))
        if i % 3 == 0:
            act = (np.arange(TL) % int(rs.randint(1, 2 * pad + 6)) == int(rs.randint(0, 3))).astype(np.uint8)   # periodic
        else:
            act = (rs.rand(TL) < rs.choice([0.01, 0.05, 0.3, 0.9])).astype(np.uint8)
        n_out = (TL + 1) * HOP
        reg = L.handoff_kept_ranges(act, 0, TL, pad, 0, n_out, n_out)
        mine, n_act = _block_rule(act, pad)
        assert np.array_equal(mine, reg), (i, TL, pad)
        frames, ranges = _lib_bounds(TL, pad)
        assert len(reg) <= ranges == _bound(TL, pad) and n_act // 160 <= frames == n_out // 160
        assert (reg % HOP == 0).all() and n_act == int((reg[:, 1] - reg[:, 0]).sum())


# ---- the kernels' resources -------------------------------------------------------------------------------------------------------

def test_new_kernels_compile_without_scratch_or_spills():
    """handoff.hip for gfx950 with the Makefile's own flags; the compiler's resource report for the three session kernels"""
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
    for kernel in ("session_keep_scan_kernel", "session_gather_kernel", "session_norm_kernel"):
        mine = {k: v for k, v in usage.items() if kernel in k}
        assert len(mine) == 1, (kernel, sorted(usage))
        (k, v), = mine.items()
        print(k, v)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
