"""NeMo chunks out of a stream's frame history (include/css_mi355_nemo_chunk.h; stream.py CssStream(nemo_history=...)), the part
that needs no GPU: the header, the library and the binding table agree, the structs are laid out as the C compiler lays them out, a
NULL handle is refused, the Python argument errors, and the kernels' resources: no scratch and no spills in nemo_chunk_kernel and
nemo_mel_multi_kernel, and the offline kernels of nemo.hip as they were before the history existed."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import nemo_chunk_reference as M
from conftest import ROOT, pkg

CSRC = os.path.join(ROOT, "notsofar1-challenge_amd", "csrc")
HEADER = "css_mi355_nemo_chunk.h"
NAMES = ("css_stream_nemo_history_open", "css_stream_nemo_history_range", "css_stream_nemo_chunks", "css_nemo_chunk_host",
         "css_stream_nemo_mel_history_host")
TYPES = ("CssStreamNemoChunk", "CssNemoChunkArray", "CssNemoChunkJob", "CssStreamNemoMelHistoryJob")
# nemo.hip's kernels before the frame history: (TotalSGPRs, VGPRs, LDS bytes per block, waves per SIMD)
OFFLINE = {"nemo_gather_kernel": (32, 12, 0, 8), "nemo_mel_kernel": (30, 24, 33924, 4)}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)


def test_header_library_and_binding_agree():
    L = pkg("_lib")
    lib = L.load()
    text = _header()
    assert '#include "css_mi355_stream_nemo.h"' in text and "visibility push(default)" in text
    declared = re.findall(r"\bint\s+(css_\w+)\s*\(", text)
    assert sorted(declared) == sorted(NAMES) == sorted(L.NEMO_CHUNK_ABI)
    for n in dir(L):   # no other table of the binding holds one of the names
        if (n.startswith("SIGNATURES") or n.endswith("_SIGNATURES") or n.endswith("_BINDINGS") or n.endswith("_ABI")) and n != "NEMO_CHUNK_ABI":
            assert not set(L.NEMO_CHUNK_ABI) & set(getattr(L, n)), n
    for f in os.listdir(os.path.join(ROOT, "include")):   # the names are this header's alone
        if f != HEADER:
            other = open(os.path.join(ROOT, "include", f)).read()
            for name in NAMES + TYPES:
                assert not re.search(rf"\b{name}\b", other), f"{name} belongs to {HEADER} alone"
    kinds = {"css_handle_t": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64}
    for name in NAMES:
        fn = getattr(lib, name)   # (AttributeError: the library does not export it)
        params = re.search(rf"\b{name}\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
        restype, argtypes = L.NEMO_CHUNK_ABI[name]
        assert restype is C.c_int and len(argtypes) == len(params), (name, params)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(argtypes)   # load() applied the table
        for p, a in zip(params, argtypes):
            p = p.strip()
            if "*" in p:
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p, a)
            else:
                assert a is kinds[p.split()[0]], (name, p, a)
    for desc in ("CssNemoChunkJob", "CssStreamNemoMelHistoryJob"):   # every array field of a job is named once, as an input or an output
        ins, outs = L.NEMO_CHUNK_ARRAYS[desc]
        assert {n for n, _ in ins + outs} == {n for n, k in getattr(L, desc)._fields_ if k is L.CssNemoChunkArray}, desc
        assert len(ins + outs) == len({n for n, _ in ins + outs})
    # the constants: the header's, the binding's, the kernel's, the model's
    consts = dict(re.findall(r"#define (CSS_NEMO_CHUNK_\w+) (\d+)", text))
    kern = open(os.path.join(CSRC, "kernels.hpp")).read()
    k = lambda name: int(re.search(rf"constexpr int {name} = (\d+);", kern).group(1))
    assert int(consts["CSS_NEMO_CHUNK_MAX_WIDTH"]) == L.NEMO_CHUNK_MAX_WIDTH == k("NEMO_CHUNK_MAX_WIDTH") == M.MAX_WIDTH == 3000
    assert int(consts["CSS_NEMO_CHUNK_TABLE"]) == L.NEMO_CHUNK_TABLE == k("NEMO_CHUNK_MULTI_MAX") == M.TABLE == 32
    assert re.search(r"enum \{ CSS_NEMO_CHUNK_RAW = 0, CSS_NEMO_CHUNK_PER_FEATURE = 1 \};", text)
    assert L.NEMO_CHUNK_NORMALIZE == {None: 0, "per_feature": 1} and L.WINDOW_DTYPES == {"float32": 0, "float16": 1}
    # the Makefile rebuilds on the header, in its two pattern rules, and lists the new unit
    mk = open(os.path.join(CSRC, "Makefile")).read()
    deps = re.findall(r"^build(?:_asan)?/%\.o:.*$", mk, flags=re.M)
    assert len(deps) == 2 and all(f"../../include/{HEADER}" in d and "window_vec.hpp" in d for d in deps)
    assert "api_nemo_chunk.hip" in re.search(r"^SRCS\s*:=(.*)$", mk, flags=re.M).group(1).split()


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
    assert C.sizeof(L.CssStreamNemoChunk) == 72 and C.sizeof(L.CssNemoChunkArray) == 16


def test_null_handle_is_refused_with_nothing_written():
    L = pkg("_lib")
    lib = L.load()
    dst = np.full(64, 7.0, np.float32)
    first, end = np.full(4, -7, np.int64), np.full(4, -7, np.int64)
    launches = C.c_int32(-7)
    assert lib.css_stream_nemo_history_open(None, 0, 1024) == L.CSS_ERR_INVALID_ARG
    assert lib.css_stream_nemo_history_range(None, 0, first.ctypes.data_as(C.POINTER(C.c_int64)), end.ctypes.data_as(C.POINTER(C.c_int64))) == L.CSS_ERR_INVALID_ARG
    item = (L.CssStreamNemoChunk * 1)()
    item[0].out_dev, item[0].n_frames, item[0].width, item[0].ld = dst.ctypes.data, 1, 1, 1
    assert lib.css_stream_nemo_chunks(None, item, 1, C.byref(launches)) == L.CSS_ERR_INVALID_ARG
    assert lib.css_nemo_chunk_host(None, (L.CssNemoChunkJob * 1)(), 1) == L.CSS_ERR_INVALID_ARG
    assert lib.css_stream_nemo_mel_history_host(None, 3, dst.ctypes.data, 64, 1, (L.CssStreamNemoMelHistoryJob * 1)(), 1) == L.CSS_ERR_INVALID_ARG
    assert (dst == 7.0).all() and (first == -7).all() and (end == -7).all() and launches.value == -7


def test_python_argument_errors():
    """what stream.py refuses before any library call (no separator is touched)"""
    S = pkg("stream")
    nemo = dict(n_mels=80, pad_frames=8, drop_silence=True, preemphasis=0.97)
    with pytest.raises(ValueError, match="nemo_history needs"):
        S.CssStream(None, nemo_history=1024)
    with pytest.raises(ValueError, match="nemo_history needs"):
        S.CssStream(None, handoff=dict(n_mels=80), nemo_history=1024)
    with pytest.raises(ValueError, match="not together"):
        S.CssStream(None, nemo=nemo, window_history=3000)
    with pytest.raises(ValueError, match="not together"):
        S.CssStream(None, nemo=nemo, window_history=3000, nemo_history=1024)

    class _Plain:      # a stream without a history, as far as the chunk calls look
        nemo_history = None
    with pytest.raises(ValueError, match="nemo_history="):
        S.CssStream.nemo_chunk(_Plain(), 0)
    for bad in (dict(normalize="per_utterance"), dict(dtype="float64"), dict(width=2), dict(pad_value=float("nan"))):
        with pytest.raises(ValueError):
            S.nemo_chunk_features(np.zeros((80, 4), np.float32), **bad)


def _usage(unit):
    """<unit> for gfx950 with the Makefile's own flags: the compiler's resource report per kernel"""
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, flags=re.M).group(1)
    flags = [f.replace("$(ARCH)", arch) for f in re.search(r"^CXXFLAGS\s*\?=\s*(.*)$", text, flags=re.M).group(1).split()]
    assert arch == "gfx950" and "-O3" in flags
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
                                                                 "-I" + CSRC, os.path.join(CSRC, unit), "-o", os.path.join(d, "unit.o")],
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
    return usage


def _one(usage, kernel):
    mine = {k: v for k, v in usage.items() if kernel in k}
    assert len(mine) == 1, (kernel, sorted(usage))
    (k, v), = mine.items()
    print(k, v)
    return v


def test_streamed_kernels_compile_without_scratch_or_spills():
    usage = _usage("nemo_stream.hip")
    for kernel in ("nemo_chunk_kernel", "nemo_mel_multi_kernel"):
        v = _one(usage, kernel)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (kernel, v)
        assert v["LDS Size [bytes/block]"] <= 65536
    # a wave's row of 3000 floats, four waves: the chunk kernel's LDS is exactly that
    assert _one(usage, "nemo_chunk_kernel")["LDS Size [bytes/block]"] == 4 * 4 * M.MAX_WIDTH


def test_offline_kernels_report_the_resources_they_had():
    usage = _usage("nemo.hip")
    for kernel, (sgprs, vgprs, lds, waves) in OFFLINE.items():
        v = _one(usage, kernel)
        assert (v["TotalSGPRs"], v["VGPRs"], v["LDS Size [bytes/block]"], v["Occupancy [waves/SIMD]"]) == (sgprs, vgprs, lds, waves), (kernel, v)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0
