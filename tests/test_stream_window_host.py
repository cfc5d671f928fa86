"""Encoder windows out of a stream's frame history (include/css_mi355_window.h; stream.py window / windows), the part that needs
no GPU: the header, the library and the binding table agree, the item struct is laid out as the ctypes mirror lays it out, the
entry points refuse NULL, the Makefile rebuilds on the header, and whisper_window -- the numpy statement of the rule the GPU
tests compare with -- is what its text says."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, pkg

CSRC = os.path.join(ROOT, "notsofar1-challenge_amd", "csrc")
HEADER = "css_mi355_window.h"
OTHERS = ("css_mi355.h", "css_mi355_rate.h", "css_mi355_preview.h", "css_mi355_preview_handoff.h", "css_mi355_encoder.h",
          "css_mi355_frontend.h")
NAMES = ("css_stream_window_open", "css_stream_window_range", "css_stream_windows")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)


def test_header_library_and_binding_agree():
    L = pkg("_lib")
    text = _header()
    lib = L.load()
    assert '#include "css_mi355.h"' in text
    declared = re.findall(r"\bint\s+(css_\w+)\s*\(", text)
    assert sorted(declared) == sorted(NAMES) == sorted(L.SIGNATURES_WINDOW)
    assert not set(L.SIGNATURES_WINDOW) & (set(L.SIGNATURES) | set(L.SIGNATURES_RATE) | set(L.SIGNATURES_PREVIEW) |
                                           set(L.SIGNATURES_PREVIEW_HANDOFF) | set(L.SIGNATURES_ENCODER) | set(L.SIGNATURES_FRONTEND))
    others = [open(os.path.join(ROOT, "include", f)).read() for f in OTHERS]
    kinds = {"css_handle_t": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64}
    for name in NAMES + ("CssStreamWindow", "CSS_WINDOW_F32", "CSS_WINDOW_F16", "CSS_WINDOW_TABLE", "CSS_WINDOW_MAX_WIDTH"):
        for other in others:
            assert not re.search(rf"\b{name}\b", other), f"{name} belongs to {HEADER} alone"
    for name in NAMES:
        fn = getattr(lib, name)   # (AttributeError: the library does not export it)
        params = re.search(rf"\b{name}\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
        restype, argtypes = L.SIGNATURES_WINDOW[name]
        assert restype is C.c_int and len(argtypes) == len(params), (name, params)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(argtypes)   # load() applied the table
        for p, a in zip(params, argtypes):
            p = p.strip()
            if "*" in p:
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p, a)
            else:
                assert a is kinds[p.split()[0]], (name, p, a)
    # the constants
    enum = re.search(r"enum\s*\{(.*?)\}", text, flags=re.S).group(1)
    assert dict((k.strip(), int(v)) for k, v in (e.split("=") for e in enum.split(","))) == {"CSS_WINDOW_F32": 0, "CSS_WINDOW_F16": 1}
    assert L.WINDOW_DTYPES == {"float32": 0, "float16": 1}
    macro = lambda n: int(re.search(rf"#define\s+{n}\s+(\d+)", text).group(1))
    assert macro("CSS_WINDOW_TABLE") == L.WINDOW_TABLE >= 16 and macro("CSS_WINDOW_MAX_WIDTH") == L.WINDOW_MAX_WIDTH == 3000
    kern = open(os.path.join(CSRC, "kernels.hpp")).read()
    assert int(re.search(r"constexpr int WINDOW_MULTI_MAX = (\d+);", kern).group(1)) == L.WINDOW_TABLE


def test_item_struct_layout():
    L = pkg("_lib")
    body = re.search(r"typedef struct CssStreamWindow \{(.*?)\} CssStreamWindow;", _header(), flags=re.S).group(1)
    members = [re.sub(r"\s+", " ", m).strip() for m in body.split(";") if m.strip()]
    assert members == ["int32_t id, speaker", "int64_t first_frame", "int32_t n_frames", "int32_t width", "int32_t dtype",
                       "void* out_dev", "int64_t ld", "float window_max"]
    T = L.CssStreamWindow
    assert [n for n, _ in T._fields_] == ["id", "speaker", "first_frame", "n_frames", "width", "dtype", "out_dev", "ld", "window_max"]
    assert [getattr(T, n).offset for n, _ in T._fields_] == [0, 4, 8, 16, 20, 24, 32, 40, 48] and C.sizeof(T) == 56


def test_null_handle_is_refused():
    L = pkg("_lib")
    lib = L.load()
    first, end = (C.c_int64 * 3)(-7, -7, -7), (C.c_int64 * 3)(-7, -7, -7)
    items = (L.CssStreamWindow * 2)()
    for it in items:
        it.id, it.speaker, it.first_frame, it.n_frames, it.width, it.dtype, it.out_dev, it.ld, it.window_max = 0, 0, 0, 1, 1, 0, 64, 1, 5.0
    launches = C.c_int32(-7)
    assert lib.css_stream_window_open(None, 0, 3000) == L.CSS_ERR_INVALID_ARG
    assert lib.css_stream_window_range(None, 0, first, end) == L.CSS_ERR_INVALID_ARG
    assert lib.css_stream_windows(None, items, 2, C.byref(launches)) == L.CSS_ERR_INVALID_ARG
    assert lib.css_stream_windows(None, None, 0, None) == L.CSS_ERR_INVALID_ARG
    assert list(first) == list(end) == [-7] * 3 and launches.value == -7 and all(it.window_max == 5.0 for it in items)


def test_makefile_names_the_header():
    deps = re.findall(r"^build(?:_asan)?/%\.o:.*$", open(os.path.join(CSRC, "Makefile")).read(), flags=re.M)
    assert len(deps) == 2 and all(f"../../include/{hd}" in d for d in deps for hd in OTHERS + (HEADER,))


def _raws():
    rs = np.random.RandomState(7)
    out = []
    for n_mels, n in ((80, 1), (80, 37), (128, 300), (80, 3000)):
        out.append((rs.randn(n_mels, n) * 2.0 - 3.0).astype(np.float32))
    out.append(np.full((80, 17), -1.25, np.float32))                 # all equal
    out.append(np.full((80, 9), -10.0, np.float32))                  # digital silence: the fill equals the frames
    last = (rs.randn(80, 50) - 6.0).astype(np.float32)
    last[13, -1] = 1.75                                              # the maximum in the last column
    out.append(last)
    return out


@pytest.mark.parametrize("i", range(7))
def test_whisper_window_is_the_stated_rule(i):
    S = pkg("stream")
    raw = _raws()[i]
    n = raw.shape[1]
    if i == 6:
        assert np.unravel_index(raw.argmax(), raw.shape) == (13, n - 1)
    M = np.float32(raw.max())
    fill = (np.maximum(np.float32(-10.0), M - np.float32(8.0)) + np.float32(4.0)) / np.float32(4.0)
    assert fill.dtype == np.float32
    for width in sorted({n, min(n + 5, 3000), 3000}):
        w32 = S.whisper_window(raw, width, "float32")
        assert w32.dtype == np.float32 and w32.shape == (raw.shape[0], width)
        assert np.array_equal(w32[:, :n], S.whisper_normalize(raw))
        assert width == n or (np.all(w32[:, n:] == fill) and w32[:, n:].size > 0)
        w16 = S.whisper_window(raw, width, "float16")
        assert w16.dtype == np.float16 and np.array_equal(w16, w32.astype(np.float16))
    if i == 5:
        assert np.all(S.whisper_window(raw, n + 5, "float32") == np.float32(-1.5))
    # no fill at n == width; what does not fit, or another dtype, is an error
    assert S.whisper_window(raw, n, "float32").shape[1] == n
    with pytest.raises(ValueError):
        S.whisper_window(raw, n - 1, "float32")
    with pytest.raises(ValueError):
        S.whisper_window(raw, 3000, "float64")
