"""The NeMo hand-off of a stream (include/css_mi355_stream_nemo.h; stream.py CssStream(nemo=...)), the part that needs no GPU: the
header, the library and the binding table agree, the structs are laid out as the C compiler lays them out, a NULL handle is
refused, css_stream_nemo_bounds is never exceeded by the round model of tests/stream_nemo_reference.py, final_frames is the model's
count without the gate, and the two new kernels compile without scratch or spills."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import stream_nemo_reference as M
from conftest import ROOT, pkg

CSRC = os.path.join(ROOT, "notsofar1-challenge_amd", "csrc")
HEADER = "css_mi355_stream_nemo.h"
NAMES = ("css_stream_nemo_open", "css_stream_nemo_bounds", "css_stream_nemo_final_frames", "css_stream_nemo_append_host",
         "css_stream_nemo_mel_host")
TYPES = ("CssStreamNemoCfg", "CssStreamNemoArray", "CssStreamNemoAppendJob", "CssStreamNemoMelJob")
KERNELS = ("nemo_append_kernel", "nemo_mel_multi_kernel")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)


def test_header_library_and_binding_agree():
    L = pkg("_lib")
    lib = L.load()
    text = _header()
    assert '#include "css_mi355.h"' in text and "visibility push(default)" in text
    declared = re.findall(r"\bint\s+(css_\w+)\s*\(", text)
    assert sorted(declared) == sorted(NAMES) == sorted(L.STREAM_NEMO_ABI)
    for n in dir(L):   # no other table of the binding holds one of the names
        if (n.startswith("SIGNATURES") or n.endswith("_SIGNATURES") or n.endswith("_BINDINGS") or n.endswith("_ABI")) and n != "STREAM_NEMO_ABI":
            assert not set(L.STREAM_NEMO_ABI) & set(getattr(L, n)), n
    for f in os.listdir(os.path.join(ROOT, "include")):   # the names are this header's alone
        if f != HEADER:
            other = open(os.path.join(ROOT, "include", f)).read()
            for name in NAMES + TYPES:
                assert not re.search(rf"\b{name}\b", other), f"{name} belongs to {HEADER} alone"
    kinds = {"css_handle_t": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64}
    for name in NAMES:
        fn = getattr(lib, name)   # (AttributeError: the library does not export it)
        params = re.search(rf"\b{name}\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
        restype, argtypes = L.STREAM_NEMO_ABI[name]
        assert restype is C.c_int and len(argtypes) == len(params), (name, params)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(argtypes)   # load() applied the table
        for p, a in zip(params, argtypes):
            p = p.strip()
            if "*" in p:
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p, a)
            else:
                assert a is kinds[p.split()[0]], (name, p, a)
    # the kernel entries' arrays: every array field of a job is named once, as an input or as an output
    for desc in ("CssStreamNemoAppendJob", "CssStreamNemoMelJob"):
        ins, outs = L.STREAM_NEMO_ARRAYS[desc]
        assert {n for n, _ in ins + outs} == {n for n, k in getattr(L, desc)._fields_ if k is L.CssStreamNemoArray}, desc
        assert len(ins + outs) == len({n for n, _ in ins + outs})
    # the Makefile rebuilds on the header, in its two pattern rules, and lists the new unit
    mk = open(os.path.join(CSRC, "Makefile")).read()
    deps = re.findall(r"^build(?:_asan)?/%\.o:.*$", mk, flags=re.M)
    assert len(deps) == 2 and all(f"../../include/{HEADER}" in d and "nemo_tile.hpp" in d for d in deps)
    assert "nemo_stream.hip" in re.search(r"^SRCS\s*:=(.*)$", mk, flags=re.M).group(1).split()
    # the constants: the kernels', the model's
    kern = open(os.path.join(CSRC, "kernels.hpp")).read()
    assert int(re.search(r"constexpr int NEMO_TAIL_LD = (\d+);", kern).group(1)) == M.TAIL_LD == 512
    # re * re + im * im of these features is written once, in the tile both paths share
    units = {f: open(os.path.join(CSRC, f)).read() for f in ("nemo.hip", "nemo_stream.hip", "nemo_tile.hpp")}
    assert [f for f, t in units.items() if re.search(r"re \* re \+ im \* im;", t)] == ["nemo_tile.hpp"]
    assert all('#include "nemo_tile.hpp"' in units[f] for f in ("nemo.hip", "nemo_stream.hip"))


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
    L = pkg("_lib")
    text = _header()
    for struct in TYPES:
        T = getattr(L, struct)
        names = [n for n, _ in T._fields_]
        body = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", text, flags=re.S).group(1)
        members = [w.strip().lstrip("*") for m in body.split(";") if m.strip() for w in re.sub(r"^\s*(const\s+)?\w+\s*\*?", "", m.strip()).split(",")]
        assert members == names, (struct, members, names)
        assert _layout_probe(struct, names) == [C.sizeof(T)] + [getattr(T, n).offset for n in names], struct
    assert C.sizeof(L.CssStreamNemoCfg) == 16 and C.sizeof(L.CssStreamNemoArray) == 16


def test_null_handle_is_refused_with_nothing_written():
    L = pkg("_lib")
    lib = L.load()
    ncfg = L.stream_nemo_cfg()
    assert (ncfg.n_mels, ncfg.pad_frames, ncfg.drop_silence) == (80, 8, 1) and abs(ncfg.preemphasis - 0.97) < 1e-7
    dst = np.full(64, 7.0, np.float32)
    assert lib.css_stream_nemo_open(None, 0, C.byref(ncfg)) == L.CSS_ERR_INVALID_ARG
    assert lib.css_stream_nemo_append_host(None, (L.CssStreamNemoAppendJob * 1)(), 1, dst.ctypes.data, 64) == L.CSS_ERR_INVALID_ARG
    assert lib.css_stream_nemo_mel_host(None, 3, dst.ctypes.data, 64, 1, (L.CssStreamNemoMelJob * 1)(), 1) == L.CSS_ERR_INVALID_ARG
    f, r, a = C.c_int64(-7), C.c_int32(-7), C.c_int64(-7)
    assert lib.css_stream_nemo_bounds(None, None, C.byref(ncfg), 4000, C.byref(f), C.byref(r), C.byref(a)) == L.CSS_ERR_INVALID_ARG
    assert lib.css_stream_nemo_final_frames(None, None, C.byref(ncfg), 4000, C.byref(f)) == L.CSS_ERR_INVALID_ARG
    assert (f.value, r.value, a.value) == (-7, -7, -7) and (dst == 7.0).all()


# ---- the bounds ---------------------------------------------------------------------------------------------------------------------

def _run_cfg(T, hop=1, halo=0):
    L = pkg("_lib")
    w = np.ones(T, np.float32)
    return L.RunCfg(T, hop, halo, 0, True, 0, 0, False, 0.0, 0.3, w, w, w)


def test_bounds_follow_the_whisper_streams_and_refuse_bad_values():
    L = pkg("_lib")
    desc = pkg("weights").ModelDesc(num_blocks=2)
    rc = pkg("css").make_run_cfg(pkg("css").CssCfg(show_progressbar=False), 16000, 7)
    for n in (-1, 0, 1, 255, 256, 24000, 10 ** 6):
        for pad, drop in ((0, True), (8, True), (4096, True), (8, False)):
            f, r, a = L.stream_nemo_bounds(desc, rc, L.stream_nemo_cfg(128, pad, drop, 0.0), n)
            fw, rw, aw = L.stream_handoff_bounds(desc, rc, L.handoff_cfg(128, pad, drop), n)
            # the same blocks, ranges and gate frames; a frame waits for 256 samples of the next hop instead of 200
            assert (r, a) == (rw, aw) and f == (a * 256 + 256) // 160 + 2 and fw <= f <= fw + 1
    for bad in (L.stream_nemo_cfg(64), L.stream_nemo_cfg(80, -1), L.stream_nemo_cfg(80, 4097), L.stream_nemo_cfg(80, 8, True, 1.0),
                L.stream_nemo_cfg(80, 8, True, -0.01), L.stream_nemo_cfg(80, 8, True, float("nan")), L.stream_nemo_cfg(80, 8, True, float("inf"))):
        with pytest.raises(L.CssError):
            L.stream_nemo_bounds(desc, rc, bad, 4000)
        with pytest.raises(L.CssError):
            L.stream_nemo_final_frames(desc, rc, bad, 4000)
    with pytest.raises(L.CssError):
        L.stream_nemo_bounds(desc, rc, L.stream_nemo_cfg(), -2)
    with pytest.raises(L.CssError):   # with the gate in play the count depends on the audio
        L.stream_nemo_final_frames(desc, rc, L.stream_nemo_cfg(80, 8, True), 40000)


@pytest.mark.parametrize("c", M.random_cases() + M.named_cases(), ids=lambda c: c["name"])
def test_bounds_are_never_exceeded_by_the_model(c):
    """Every round of the model against the bounds of a call that moves as many blocks: a push of n samples makes at most
    n / 256 + 1 + hop frames gated-final and decides at most as many blocks (segments of 2 frames at hop 1 here, so a push of
    (nb - 2) 256 samples is bounded for nb blocks), finish fewer than T + hop + halo + pad + 3 (T := the round's blocks)."""
    L = pkg("_lib")
    desc = pkg("weights").ModelDesc(num_blocks=2)
    ncfg = L.stream_nemo_cfg(80, c["pad"], bool(c["drop"]), c["preemphasis"])
    state = M.state0(c)
    for rnd in M.rounds_of(c):
        t_g0, t_g1, D0, D1, closing = rnd
        nb = max(t_g1 - t_g0, -(-(D1 - D0) // 256))
        if closing:
            frames, ranges, activity = L.stream_nemo_bounds(desc, _run_cfg(max(nb, 2)), ncfg, -1)
        else:
            frames, ranges, activity = L.stream_nemo_bounds(desc, _run_cfg(2), ncfg, max(nb - 2, 0) * 256)
        job = M.job_of(c, rnd, state)
        res = [M.append_round(job, k) for k in range(c["S"])]
        for r in res:
            assert r["n_new"] <= frames and len(r["ranges"]) <= ranges and len(r["act"]) <= activity, (c["name"], rnd)
            assert r["n_new"] <= r["rows"] - 4     # the frames and the rows their 512 columns reach into lie inside the speaker's rows
        state = M.next_state(job, res)


def test_final_frames_is_the_model_without_the_gate():
    """drop_silence = 0: every final sample is kept at once, so after n_pushed samples A = final_samples and J the open rule"""
    L = pkg("_lib")
    desc = pkg("weights").ModelDesc(num_blocks=2)
    rc = pkg("css").make_run_cfg(pkg("css").CssCfg(show_progressbar=False), 16000, 7)
    ncfg = L.stream_nemo_cfg(80, 8, False)
    seen = set()
    for n in list(range(0, 140000, 997)) + [57600 + d for d in (-1, 0, 1, 255, 256, 257)]:
        A = L.stream_final_samples(desc, rc, n)
        J = L.stream_nemo_final_frames(desc, rc, ncfg, n)
        assert J == M.open_frames(A)
        seen.add(J)
    assert len(seen) > 3 and 0 in seen
    # ... and a chain of the model over a recording without the gate ends, before its closing round, at that count
    c = next(c for c in M.named_cases() if c["name"] == "nodrop")
    state = M.state0(c)
    for rnd in M.rounds_of(c)[:-1]:
        job = M.job_of(c, rnd, state)
        state = M.next_state(job, [M.append_round(job, k) for k in range(c["S"])])
        assert all(int(s["A"]) == rnd[3] and int(s["J"]) == M.open_frames(rnd[3]) for s in state[2])


# ---- the kernels' resources ---------------------------------------------------------------------------------------------------------

def test_new_kernels_compile_without_scratch_or_spills():
    """nemo_stream.hip for gfx950 with the Makefile's own flags; the compiler's resource report for the two new kernels"""
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, flags=re.M).group(1)
    flags = [f.replace("$(ARCH)", arch) for f in re.search(r"^CXXFLAGS\s*\?=\s*(.*)$", text, flags=re.M).group(1).split()]
    assert arch == "gfx950" and "-O3" in flags
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
                                                                 "-I" + CSRC, os.path.join(CSRC, "nemo_stream.hip"), "-o", os.path.join(d, "nemo_stream.o")],
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
