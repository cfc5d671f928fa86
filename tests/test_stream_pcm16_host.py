"""PCM16 stream pushes (css_stream_push_pcm16, css_stream_push_many_pcm16; stream.py push_pcm16), the part that needs no GPU:
the header, the library and the binding agree on the two entry points, both refuse a NULL handle, stream.pcm16_layout maps
numpy layouts to the two stride forms the C ABI takes without copying what it can pass on, and the ingest kernel compiles
for gfx950 with the shipped flags without scratch or spills (the manner of test_gemm_f32_registers.py)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT, pkg

CSRC = os.path.join(ROOT, "notsofar1-challenge_amd", "csrc")
NEW = ("css_stream_push_pcm16", "css_stream_push_many_pcm16")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "css_mi355.h")).read(), flags=re.S)


def test_header_library_and_binding_agree():
    L = pkg("_lib")
    text = _header()
    lib = L.load()
    for name in NEW:
        assert re.search(rf"\bint\s+{name}\s*\(", text), f"{name} is not declared in css_mi355.h"
        assert hasattr(lib, name), f"libcss_mi355.so does not export {name}"
        assert name in L.SIGNATURES
    # the argument lists, parameter by parameter
    kinds = {"css_handle_t": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64}
    for name in NEW:
        params = re.search(rf"\b{name}\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
        restype, argtypes = L.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == len(params), (name, params)
        for p, a in zip(params, argtypes):
            p = p.strip()
            if "*" in p:
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p, a)
            else:
                assert a is kinds[p.split()[0]], (name, p, a)
    # the item structure: the header's fields in the header's order
    body = re.search(r"typedef struct CssStreamPushPcm16 \{(.*?)\} CssStreamPushPcm16;", text, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [n.strip().lstrip("*") for n in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl, count=1).split(",")]
    assert fields == [n for n, _ in L.CssStreamPushPcm16._fields_]
    assert fields == ["id", "pcm16_host", "n_samples", "sample_stride", "channel_stride", "out_host", "cap", "n_out"]
    assert C.sizeof(L.CssStreamPushPcm16) == 8 * 8   # (id is padded to the pointer's alignment)
    assert L.CssStreamPushPcm16.n_samples.offset == 16 and L.CssStreamPushPcm16.n_out.offset == 56


def test_null_handle_is_refused():
    L = pkg("_lib")
    lib = L.load()
    q = np.zeros((16, 7), np.int16)
    out = np.zeros((3, 64), np.float32)
    n_out = C.c_int64(-1)
    assert lib.css_stream_push_pcm16(None, 0, q.ctypes.data_as(C.c_void_p), 16, 7, 1, out.ctypes.data_as(C.c_void_p), 64, C.byref(n_out)) < 0
    assert n_out.value == -1
    items = (L.CssStreamPushPcm16 * 1)()
    assert lib.css_stream_push_many_pcm16(None, items, 1, None) < 0
    assert lib.css_stream_push_many_pcm16(None, None, 0, None) < 0


def test_pcm16_layout_strides_and_copies():
    S = pkg("stream")
    rs = np.random.RandomState(0)
    planes = rs.randint(-32768, 32768, (7, 5000)).astype(np.int16)
    inter = np.ascontiguousarray(planes.T)
    # interleaved: a C-contiguous [n, C] array, and a run of its rows
    for a in (inter, inter[100:900]):
        arr, ss, cs = S.pcm16_layout(a, 7)
        assert (ss, cs) == (7, 1) and np.shares_memory(arr, a) and arr.ctypes.data == a.ctypes.data
    # planar: the transposed view of [C, n], and a slice of it
    arr, ss, cs = S.pcm16_layout(planes.T, 7)
    assert (ss, cs) == (1, 5000) and np.shares_memory(arr, planes) and arr.ctypes.data == planes.ctypes.data
    view = planes[:, 1000:1800].T
    arr, ss, cs = S.pcm16_layout(view, 7)
    assert (ss, cs) == (1, 5000) and cs >= arr.shape[0] == 800 and np.shares_memory(arr, planes)
    assert arr.ctypes.data == planes.ctypes.data + 2 * 1000
    # what the C ABI reads through these strides is the array
    flat = planes.reshape(-1)
    assert all(flat[1000 + i * ss + c * cs] == view[i, c] for i in (0, 1, 799) for c in range(7))
    # anything else: one C-contiguous copy with the same values
    for odd in (inter[::2], planes.T[::3], inter[:, ::-1], planes[::-1].T):
        arr, ss, cs = S.pcm16_layout(odd, 7)
        assert (ss, cs) == (7, 1) and arr.flags.c_contiguous and not np.shares_memory(arr, odd) and np.array_equal(arr, odd)
    # one channel: [n] or [n, 1], both layouts coincide
    mono = planes[0]
    for a in (mono, mono[:, None], planes[:1].T):
        arr, ss, cs = S.pcm16_layout(a, 1)
        assert arr.shape == (5000, 1) and (ss, cs) == (1, 1) and np.shares_memory(arr, planes)
    arr, ss, cs = S.pcm16_layout(mono[::2], 1)
    assert (ss, cs) == (1, 1) and not np.shares_memory(arr, planes) and np.array_equal(arr[:, 0], mono[::2])
    # an empty chunk is passed on
    arr, ss, cs = S.pcm16_layout(inter[:0], 7)
    assert arr.shape == (0, 7) and (ss, cs) == (7, 1)
    # no silent conversion, no wrong channel count
    for bad in (inter.astype(np.float32), inter.astype(np.int32), inter.astype(np.uint16), inter.tolist()):
        with pytest.raises(TypeError):
            S.pcm16_layout(bad, 7)
    for a, ch in ((inter, 6), (mono, 7), (inter[None], 7)):
        with pytest.raises(ValueError):
            S.pcm16_layout(a, ch)


def _makefile_flags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*\?=\s*(.*)$", text, flags=re.M).group(1).split()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, flags=re.M).group(1)
    return [f.replace("$(ARCH)", arch) for f in flags], arch


def test_ingest_kernel_compiles_without_scratch_or_spills():
    """stream.hip for gfx950 with the Makefile's own flags; the compiler's resource report for stream_ingest_pcm16_kernel"""
    flags, arch = _makefile_flags()
    assert arch == "gfx950" and "-O3" in flags
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
                                                                 "-I" + CSRC, os.path.join(CSRC, "stream.hip"), "-o", os.path.join(d, "stream.o")],
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
    mine = {k: v for k, v in usage.items() if "stream_ingest_pcm16_kernel" in k}
    assert len(mine) == 1, sorted(usage)
    (k, v), = mine.items()
    print(k, v)
    assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
