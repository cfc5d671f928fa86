"""Pushes at the capture rate (include/css_mi355_rate.h; stream.py input_rate), the part that needs no GPU: the new header, the
library and the second binding table agree, every handle-taking entry point refuses NULL, the library's float32 taps are
scipy's firwin taps of resample_poly's default filter, the two count rules are resample_poly's length and the availability
formula, the ratios outside the rule are refused, and both resampling kernels compile for gfx950 with the shipped flags without
scratch or spills (the manner of test_stream_pcm16_host.py)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT, pkg

CSRC = os.path.join(ROOT, "notsofar1-challenge_amd", "csrc")
RATIOS = ((1, 3), (1, 2), (2, 1), (2, 3), (160, 441), (1, 6), (320, 441),      # the capture rates,
          (3, 1), (441, 160), (3, 2), (441, 320), (6, 1), (819, 818))           # the playback rates and the rule's edge
NAMES = ("css_stream_set_rate", "css_stream_rate_samples", "css_resample_taps", "css_resample_host")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "css_mi355_rate.h")).read(), flags=re.S)


def test_header_library_and_binding_agree():
    L = pkg("_lib")
    text = _header()
    lib = L.load()
    assert '#include "css_mi355.h"' in text
    declared = re.findall(r"\bint\s+(css_\w+)\s*\(", text)
    assert sorted(declared) == sorted(NAMES) == sorted(L.SIGNATURES_RATE)
    assert not set(L.SIGNATURES_RATE) & set(L.SIGNATURES)
    main = open(os.path.join(ROOT, "include", "css_mi355.h")).read()
    kinds = {"css_handle_t": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64}
    for name in NAMES:
        assert not re.search(rf"\b{name}\b", main), f"{name} belongs to css_mi355_rate.h alone"
        fn = getattr(lib, name)   # (AttributeError: the library does not export it)
        params = re.search(rf"\b{name}\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
        restype, argtypes = L.SIGNATURES_RATE[name]
        assert restype is C.c_int and len(argtypes) == len(params), (name, params)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(argtypes)   # load() applied the second table
        for p, a in zip(params, argtypes):
            p = p.strip()
            if "*" in p:
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p, a)
            else:
                assert a is kinds[p.split()[0]], (name, p, a)
    deps = re.findall(r"^build(?:_asan)?/%\.o:.*$", open(os.path.join(CSRC, "Makefile")).read(), flags=re.M)
    assert len(deps) == 2 and all("css_mi355_rate.h" in d for d in deps)
    assert "resample.hip" in re.search(r"^SRCS\s*:=\s*(.*)$", open(os.path.join(CSRC, "Makefile")).read(), flags=re.M).group(1).split()


def test_null_handle_is_refused():
    L = pkg("_lib")
    lib = L.load()
    assert lib.css_stream_set_rate(None, 0, 1, 3) == L.CSS_ERR_INVALID_ARG
    x = np.zeros((64, 7), np.float32)
    out = np.full((32, 7), 5.0, np.float32)
    n_out = C.c_int64(-1)
    assert lib.css_resample_host(None, x.ctypes.data_as(C.c_void_p), 0, 64, 7, 7, 1, 1, 3, out.ctypes.data_as(C.c_void_p), 32,
                                 C.byref(n_out)) == L.CSS_ERR_INVALID_ARG
    assert n_out.value == -1 and np.all(out == 5.0)


def _scipy_taps(up, down):
    from scipy.signal import firwin
    mx = max(up, down)
    return (up * firwin(20 * mx + 1, 1.0 / mx, window=("kaiser", 5.0))).astype(np.float32)


def test_taps_are_scipys_to_one_ulp():
    """Two float64 evaluations of one formula differ only across a rounding boundary of the float32 result: every tap within
    one float32 ulp of (up * firwin(L, 1 / max(up, down), window=('kaiser', 5.0))).astype(float32)."""
    L = pkg("_lib")
    differing = 0
    for up, down in RATIOS:
        t, ref = L.resample_taps(up, down), _scipy_taps(up, down)
        assert t.dtype == np.float32 and t.shape == ref.shape == (20 * max(up, down) + 1,)
        hi, lo = np.nextafter(ref, np.float32(np.inf)), np.nextafter(ref, np.float32(-np.inf))
        assert np.all((t >= lo) & (t <= hi)), (up, down, int(np.argmax((t < lo) | (t > hi))))
        assert np.array_equal(t, t[::-1])   # (linear phase: the filter adds no fractional delay of its own)
        n = int(np.count_nonzero(t != ref))
        print(f"{up}/{down}: {t.size} taps, {n} differ from scipy's")
        differing += n
    print("differing taps, all ratios:", differing)


def test_counts_are_resample_polys_and_the_availability_rule():
    from scipy.signal import resample_poly
    L = pkg("_lib")
    for up, down in RATIOS:
        half = 10 * max(up, down)
        fin = [L.stream_rate_samples(up, down, n, True) for n in range(2001)]
        av = [L.stream_rate_samples(up, down, n, False) for n in range(2001)]
        for n in range(2001):
            assert fin[n] == len(resample_poly(np.zeros(n), up, down)), (up, down, n)
        assert fin == [-(-n * up // down) for n in range(2001)]   # (resample_poly's length rule, every n)
        assert av == [max(0, -(-(n * up - half) // down)) for n in range(2001)]
        assert all(b >= a for a, b in zip(av, av[1:])) and all(a <= f for a, f in zip(av, fin))
        # output avail(n) is the first that needs an input that has not arrived: floor((m down + half) / up) >= n
        for n in (1, 30, 31, 500, 2000):
            m = av[n]
            assert (m * down + half) // up >= n and (m == 0 or ((m - 1) * down + half) // up < n)


def test_refused_ratios_and_capacities():
    L = pkg("_lib")
    lib = L.load()
    n, nt = C.c_int64(-7), C.c_int32(-7)
    taps = np.full(20000, 9.0, np.float32)
    tp = taps.ctypes.data_as(C.c_void_p)
    bad = ((1, 1), (3, 3), (2, 4), (4, 2), (1, 7), (0, 3), (1, 0), (0, 0), (-1, 3), (1, -3), (-1, -3), (1, 820), (820, 1), (819, 1639))
    for up, down in bad:
        assert lib.css_stream_rate_samples(up, down, 100, 0, C.byref(n)) == L.CSS_ERR_INVALID_ARG and n.value == -7, (up, down)
        assert lib.css_resample_taps(up, down, tp, taps.size, C.byref(nt)) == L.CSS_ERR_INVALID_ARG and nt.value == -7, (up, down)
        with pytest.raises(L.CssError):
            L.stream_rate_samples(up, down, 10)
    assert np.all(taps == 9.0)
    # 1 / 7 is the first ratio past the bound of 128 taps per output sample (141); 1 / 6 (121) and 819 / 818 are inside
    assert L.resample_taps(1, 6).size == 121 and L.resample_taps(819, 818).size == 16381
    assert lib.css_stream_rate_samples(1, 3, -1, 0, C.byref(n)) == L.CSS_ERR_INVALID_ARG
    assert lib.css_stream_rate_samples(1, 3, 10, 0, None) == L.CSS_ERR_INVALID_ARG
    # a capacity below L: the count is reported, no tap is written; L itself is enough
    assert lib.css_resample_taps(1, 3, tp, 60, C.byref(nt)) == L.CSS_ERR_INVALID_ARG and nt.value == 61 and np.all(taps == 9.0)
    assert lib.css_resample_taps(1, 3, None, 61, C.byref(nt)) == L.CSS_ERR_INVALID_ARG
    assert lib.css_resample_taps(1, 3, tp, 61, None) == L.CSS_ERR_INVALID_ARG
    assert lib.css_resample_taps(1, 3, tp, 61, C.byref(nt)) == L.CSS_OK and nt.value == 61 and np.all(taps[61:] == 9.0)
    assert L.rate_ratio(48000) == (1, 3) and L.rate_ratio(44100) == (160, 441) and L.rate_ratio(8000) == (2, 1)
    assert L.rate_ratio(32000) == (1, 2) and L.rate_ratio(24000) == (2, 3) and L.rate_ratio(96000) == (1, 6)
    assert L.rate_ratio(22050) == (320, 441)


def _makefile_flags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*\?=\s*(.*)$", text, flags=re.M).group(1).split()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, flags=re.M).group(1)
    return [f.replace("$(ARCH)", arch) for f in flags], arch


def test_resampling_kernels_compile_without_scratch_or_spills():
    """resample.hip for gfx950 with the Makefile's own flags; the compiler's resource report for both kernels"""
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
    for kernel in ("stream_ingest_resample_kernel", "15resample_kernel"):
        mine = {k: v for k, v in usage.items() if kernel in k}
        assert len(mine) == 1, sorted(usage)
        (k, v), = mine.items()
        print(k, v)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
