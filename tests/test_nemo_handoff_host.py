"""The hand-off to NeMo hosts (include/css_mi355_nemo_handoff.h; _lib.NemoHandoff, Handle.run_enqueue_nemo), the part that needs no
GPU: the header, the library and the binding table agree, the structs are laid out as the C compiler lays them out, a NULL handle
is refused, css_nemo_handoff_bounds is the session hand-off's arithmetic, attained by the densest gate and never exceeded, and
the new kernels compile without scratch or spills."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT, pkg

CSRC = os.path.join(ROOT, "notsofar1-challenge_amd", "csrc")
HEADER = "css_mi355_nemo_handoff.h"
NAMES = ("css_nemo_handoff_bounds", "css_handoff_nemo_all", "css_run_enqueue_nemo", "css_run_enqueue_pcm16_nemo", "css_nemo_kernels_host")
TYPES = ("CssNemoCfg", "CssNemoOut", "CssNemoArray", "CssNemoKernelsJob")
KERNELS = ("nemo_gather_kernel", "nemo_mel_kernel", "nemo_stats_kernel", "nemo_norm_kernel")
HOP, FRAME = 256, 512


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)


def test_header_library_and_binding_agree():
    L = pkg("_lib")
    lib = L.load()
    text = _header()
    assert '#include "css_mi355.h"' in text and "visibility push(default)" in text
    declared = re.findall(r"\bint\s+(css_\w+)\s*\(", text)
    assert sorted(declared) == sorted(NAMES) == sorted(L.NEMO_HANDOFF_ABI)
    # the table is its own kind: no earlier table counts it, and it shares no name with any of them
    tables = {n: getattr(L, n) for n in dir(L) if n.startswith("SIGNATURES") or n.endswith("_SIGNATURES") or n.endswith("_BINDINGS")}
    assert "NEMO_HANDOFF_ABI" not in tables and len(tables) == 17 and len(L.SIGNATURES) == 85
    for n, t in tables.items():
        assert not set(L.NEMO_HANDOFF_ABI) & set(t), n
    # the header's names are its own, and it takes no function or struct of another addition
    own = open(os.path.join(ROOT, "include", HEADER)).read()
    for f in os.listdir(os.path.join(ROOT, "include")):
        if f == HEADER:
            continue
        other = open(os.path.join(ROOT, "include", f)).read()
        for name in NAMES + TYPES:
            assert not re.search(rf"\b{name}\b", other), f"{name} belongs to {HEADER} alone"
        if f != "css_mi355.h":
            theirs = set(re.findall(r"\bint\s+(css_\w+)\s*\(", other)) | set(re.findall(r"\}\s*(Css\w+)\s*;", other))
            for name in theirs:
                assert not re.search(rf"\b{name}\b", own), f"{HEADER} names {name} of {f}"
    kinds = {"css_handle_t": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64}
    for name in NAMES:
        fn = getattr(lib, name)   # (AttributeError: the library does not export it)
        params = re.search(rf"\b{name}\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
        restype, argtypes = L.NEMO_HANDOFF_ABI[name]
        assert restype is C.c_int and len(argtypes) == len(params), (name, params)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(argtypes)   # load() applied the table
        for p, a in zip(params, argtypes):
            p = p.strip()
            if "*" in p:
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p, a)
            else:
                assert a is kinds[p.split()[0]], (name, p, a)
    # the Makefile rebuilds on the header, in its two pattern rules, and lists the new units
    mk = open(os.path.join(CSRC, "Makefile")).read()
    deps = re.findall(r"^build(?:_asan)?/%\.o:.*$", mk, flags=re.M)
    assert len(deps) == 2 and all(f"../../include/{HEADER}" in d for d in deps)
    srcs = re.search(r"^SRCS\s*:=(.*)$", mk, flags=re.M).group(1).split()
    assert "nemo.hip" in srcs and "api_nemo_handoff.hip" in srcs
    # the constants of the definition: the kernels', the reference's and the package's are one set of numbers
    kern = open(os.path.join(CSRC, "kernels.hpp")).read()
    m = re.search(r"constexpr int NEMO_NFFT = (\d+), NEMO_BINS = (\d+), NEMO_WIN = (\d+), NEMO_WIN_OFF = (\d+), NEMO_HOP = (\d+);", kern)
    import nemo_reference as N
    assert tuple(int(v) for v in m.groups()) == (N.NFFT, N.BINS, N.WIN, N.WIN_OFF, N.HOPW) == (512, 257, 400, 56, 160)
    assert float(re.search(r"NEMO_LOG_GUARD = ([0-9.e+-]+)f;", kern).group(1)) == 2.0 ** -24 == N.GUARD


def _layout_probe(struct, names):
    src = ('#include <stddef.h>\n#include <stdio.h>\n#include "%s"\nint main(void) {\n' % HEADER +
           f'    printf("%zu", sizeof({struct}));\n' + "".join(f'    printf(" %zu", offsetof({struct}, {n}));\n' for n in names) +
           "    return 0;\n}\n")
    with tempfile.TemporaryDirectory() as d:
        c_file, exe = os.path.join(d, "probe.c"), os.path.join(d, "probe")
        open(c_file, "w").write(src)
        cc = "/opt/rocm/lib/llvm/bin/clang" if os.path.exists("/opt/rocm/lib/llvm/bin/clang") else "cc"
        subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), c_file, "-o", exe], check=True,
                       capture_output=True, timeout=120)
        return [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.split()]


def test_struct_layouts_are_the_compilers():
    """sizeof / offsetof of the header's four structs from compiled probes against the ctypes mirrors"""
    L = pkg("_lib")
    text = _header()
    for struct in TYPES:
        T = getattr(L, struct)
        names = [n for n, _ in T._fields_]
        body = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", text, flags=re.S).group(1)
        members = [w.strip().lstrip("*") for m in body.split(";") if m.strip() for w in re.sub(r"^\s*(const\s+)?\w+\s*\*?", "", m.strip()).split(",")]
        assert members == names, (struct, members, names)
        got = _layout_probe(struct, names)
        assert got == [C.sizeof(T)] + [getattr(T, n).offset for n in names], struct
    assert C.sizeof(L.CssNemoCfg) == 20 and C.sizeof(L.CssNemoOut) == 64 and C.sizeof(L.CssNemoArray) == 16


def test_null_handle_is_refused_with_nothing_written():
    L = pkg("_lib")
    lib = L.load()
    ho = L.NemoHandoff(3, 80, 100, 4, pinned=False, fill=-7)
    ncfg = L.nemo_cfg()
    assert (ncfg.n_mels, ncfg.pad_frames, ncfg.drop_silence, ncfg.normalize) == (80, 8, 1, 1) and abs(ncfg.preemphasis - 0.97) < 1e-7
    x = np.zeros((4000, 7), np.float32)
    wav = np.full((3, 8192), 5.0, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.css_handoff_nemo_all(None, p(wav), 8192, C.byref(ncfg), C.byref(ho.c)) == L.CSS_ERR_INVALID_ARG
    assert lib.css_run_enqueue_nemo(None, p(x), 4000, 7, None, p(wav), 8192, C.byref(ncfg), C.byref(ho.c)) == L.CSS_ERR_INVALID_ARG
    assert lib.css_run_enqueue_pcm16_nemo(None, None, 4000, 7, None, p(wav), 8192, None, C.byref(ncfg), C.byref(ho.c)) == L.CSS_ERR_INVALID_ARG
    assert lib.css_handoff_nemo_all(None, None, 0, None, None) == L.CSS_ERR_INVALID_ARG
    assert lib.css_nemo_kernels_host(None, None) == L.CSS_ERR_INVALID_ARG
    f, r = C.c_int64(-7), C.c_int32(-7)
    assert lib.css_nemo_handoff_bounds(None, None, None, 4000, C.byref(f), C.byref(r)) == L.CSS_ERR_INVALID_ARG
    assert (f.value, r.value) == (-7, -7) and (wav == 5.0).all()
    assert (ho.mel_all == -7).all() and (ho.ranges_all == -7).all() and (ho.n_frames == -7).all() and (ho.n_ranges == -7).all()
    assert (ho.mean == -7).all() and (ho.std == -7).all()


# ---- the bounds ---------------------------------------------------------------------------------------------------------------------

def _setup():
    W, css = pkg("weights"), pkg("css")
    return W.ModelDesc(num_blocks=2), css.make_run_cfg(css.CssCfg(show_progressbar=False), 16000, 7)


def _lib_bounds(TL, pad, drop=True):
    """css_nemo_handoff_bounds for a stream of TL frames: segments of one frame, so that every TL >= 1 is a plan's"""
    L = pkg("_lib")
    w = np.ones(1, np.float32)
    rc = L.RunCfg(1, 1, 0, 0, True, 0, 0, False, 0.0, 0.3, w, w, w)
    return L.nemo_handoff_bounds(pkg("weights").ModelDesc(num_blocks=2), rc, L.nemo_cfg(80, pad, drop), (TL - 1) * HOP + FRAME)


def test_bounds_are_the_session_hand_offs():
    L = pkg("_lib")
    desc, rc = _setup()
    T = int(rc.c.segment_frames)
    for TL in (T, T + 1, 375, 1024):
        n = (TL - 1) * HOP + FRAME
        pl = L.plan(desc, rc, n)
        assert int(pl.mix_frames) == TL and int(pl.n_out) == (TL + 1) * HOP
        for pad in (0, 1, 8, 40, 4096):
            for drop in (True, False):
                want = (int(pl.n_out) // 160, (TL - 1) // (2 * pad + 3) + 1 if drop else 1)
                assert L.nemo_handoff_bounds(desc, rc, L.nemo_cfg(128, pad, drop, 0.0, False), n) == want
                assert L.session_handoff_bounds(desc, rc, L.handoff_cfg(128, pad, drop), n) == want
    for bad in (L.nemo_cfg(64), L.nemo_cfg(80, -1), L.nemo_cfg(80, 4097), L.nemo_cfg(80, 8, True, 1.0), L.nemo_cfg(80, 8, True, -0.01),
                L.nemo_cfg(80, 8, True, float("nan")), L.nemo_cfg(80, 8, True, float("inf"))):
        with pytest.raises(L.CssError):
            L.nemo_handoff_bounds(desc, rc, bad, 40000)
    with pytest.raises(L.CssError):
        L.nemo_handoff_bounds(pkg("weights").ModelDesc(num_blocks=2, frame_len=400, frame_hop=160, num_bins=201, in_features=1407), rc,
                              L.nemo_cfg(), 40000)


@pytest.mark.parametrize("pad", (0, 1, 8))
def test_densest_gate_attains_the_range_bound_and_random_gates_stay_inside(pad):
    """one active frame every 2 pad + 3 frames from frame 0: exactly the bound's ranges; random gates: never more, and the frames
    (kept samples // 160) never more than n_out // 160"""
    L = pkg("_lib")
    rs = np.random.RandomState(23 + pad)
    for TL in (1, 2, 186, 187):
        frames, ranges = _lib_bounds(TL, pad)
        n_out = (TL + 1) * HOP
        assert frames == n_out // 160 and _lib_bounds(TL, pad, False) == (frames, 1)
        act = np.zeros(TL, np.uint8)
        act[::2 * pad + 3] = 1
        assert len(L.handoff_kept_ranges(act, 0, TL, pad, 0, n_out, n_out)) == ranges
        for dens in (0.02, 0.3, 0.9):
            reg = L.handoff_kept_ranges((rs.rand(TL) < dens).astype(np.uint8), 0, TL, pad, 0, n_out, n_out)
            assert len(reg) <= ranges and int((reg[:, 1] - reg[:, 0]).sum()) // 160 <= frames


# ---- the kernels' resources ---------------------------------------------------------------------------------------------------------

def test_new_kernels_compile_without_scratch_or_spills():
    """nemo.hip for gfx950 with the Makefile's own flags; the compiler's resource report for the four new kernels"""
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, flags=re.M).group(1)
    flags = [f.replace("$(ARCH)", arch) for f in re.search(r"^CXXFLAGS\s*\?=\s*(.*)$", text, flags=re.M).group(1).split()]
    assert arch == "gfx950" and "-O3" in flags
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
                                                                 "-I" + CSRC, os.path.join(CSRC, "nemo.hip"), "-o", os.path.join(d, "nemo.o")],
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
    for kernel in KERNELS:
        mine = {k: v for k, v in usage.items() if kernel in k}
        assert len(mine) == 1, (kernel, sorted(usage))
        (k, v), = mine.items()
        print(k, v)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
        assert v["LDS Size [bytes/block]"] <= 65536
