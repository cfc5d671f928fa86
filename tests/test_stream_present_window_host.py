"""Encoder windows that reach the present (include/css_mi355_present_window.h; stream.py present_window / present_windows), the
part that needs no GPU: the header, the library and the binding table agree, both structs are laid out as their ctypes mirrors
lay them out, the entry point refuses a NULL handle, NULL items and n_items < 1 with nothing written, and the Makefile rebuilds
on the header."""
import ctypes as C
import os
import re

from conftest import ROOT, pkg

CSRC = os.path.join(ROOT, "notsofar1-challenge_amd", "csrc")
HEADER = "css_mi355_present_window.h"
OTHERS = ("css_mi355.h", "css_mi355_rate.h", "css_mi355_preview.h", "css_mi355_preview_handoff.h", "css_mi355_encoder.h",
          "css_mi355_window.h", "css_mi355_frontend.h")
NAMES = ("css_stream_present_windows",)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)


def _members(struct):
    body = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", _header(), flags=re.S).group(1)
    return [re.sub(r"\s+", " ", m).strip() for m in body.split(";") if m.strip()]


def test_header_library_and_binding_agree():
    L = pkg("_lib")
    text = _header()
    lib = L.load()
    assert '#include "css_mi355_preview_handoff.h"' in text and '#include "css_mi355_window.h"' in text
    declared = re.findall(r"\bint\s+(css_\w+)\s*\(", text)
    assert sorted(declared) == sorted(NAMES) == sorted(L.SIGNATURES_PRESENT)
    assert not set(L.SIGNATURES_PRESENT) & (set(L.SIGNATURES) | set(L.SIGNATURES_RATE) | set(L.SIGNATURES_PREVIEW) |
                                            set(L.SIGNATURES_PREVIEW_HANDOFF) | set(L.SIGNATURES_ENCODER) | set(L.SIGNATURES_WINDOW) |
                                            set(L.SIGNATURES_FRONTEND))
    others = [open(os.path.join(ROOT, "include", f)).read() for f in OTHERS]
    for name in NAMES + ("CssStreamPresentWindow", "CssStreamPresentItem"):
        for other in others:
            assert not re.search(rf"\b{name}\b", other), f"{name} belongs to {HEADER} alone"
    kinds = {"css_handle_t": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64}
    for name in NAMES:
        fn = getattr(lib, name)   # (AttributeError: the library does not export it)
        params = re.search(rf"\b{name}\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
        restype, argtypes = L.SIGNATURES_PRESENT[name]
        assert restype is C.c_int and len(argtypes) == len(params), (name, params)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(argtypes)   # load() applied the table
        for p, a in zip(params, argtypes):
            p = p.strip()
            if "*" in p:
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p, a)
            else:
                assert a is kinds[p.split()[0]], (name, p, a)
    restype, argtypes = L.SIGNATURES_PRESENT["css_stream_present_windows"]
    assert argtypes[1]._type_ is L.CssStreamPresentItem and argtypes[3]._type_ is L.CssStreamGroupStats and argtypes[4]._type_ is C.c_int32
    # the table's size is the one css_mi355_window.h states: no constant of its own
    assert not re.search(r"#define|enum", text.split("#define CSS_MI355_PRESENT_WINDOW_H")[1])


def test_window_struct_layout():
    L = pkg("_lib")
    assert _members("CssStreamPresentWindow") == ["int32_t speaker", "int32_t n_frames", "int32_t width, dtype", "void* out_dev", "int64_t ld",
                                                  "int64_t first_frame", "int32_t n_used", "int32_t n_provisional", "float window_max"]
    T = L.CssStreamPresentWindow
    assert [n for n, _ in T._fields_] == ["speaker", "n_frames", "width", "dtype", "out_dev", "ld", "first_frame", "n_used", "n_provisional",
                                          "window_max"]
    assert [getattr(T, n).offset for n, _ in T._fields_] == [0, 4, 8, 12, 16, 24, 32, 40, 44, 48] and C.sizeof(T) == 56
    assert [t for _, t in T._fields_] == [C.c_int32] * 4 + [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_float]


def test_item_struct_layout():
    L = pkg("_lib")
    assert _members("CssStreamPresentItem") == ["CssStreamPreviewHandoff ph", "CssStreamPresentWindow* windows", "int32_t n_windows"]
    T = L.CssStreamPresentItem
    assert [n for n, _ in T._fields_] == ["ph", "windows", "n_windows"]
    # CssStreamPreviewHandoff: CssStreamPreview (id, out_host, cap, n_out, first_sample, status: 48 bytes), ho, first_frame
    assert C.sizeof(L.CssStreamPreview) == 48 and C.sizeof(L.CssStreamPreviewHandoff) == 64
    assert dict(T._fields_)["ph"] is L.CssStreamPreviewHandoff and dict(T._fields_)["windows"]._type_ is L.CssStreamPresentWindow
    assert [getattr(T, n).offset for n, _ in T._fields_] == [0, 64, 72] and C.sizeof(T) == 80


def test_null_arguments_are_refused_with_nothing_written():
    L = pkg("_lib")
    lib = L.load()
    wins = (L.CssStreamPresentWindow * 2)()
    for w in wins:
        w.speaker, w.n_frames, w.width, w.dtype, w.out_dev, w.ld = 0, 1, 1, 0, 64, 1
        w.first_frame, w.n_used, w.n_provisional, w.window_max = -7, -7, -7, 5.0
    items = (L.CssStreamPresentItem * 1)()
    items[0].ph.p.status, items[0].ph.p.n_out, items[0].windows, items[0].n_windows = -7, -7, wins, 2
    stats = L.CssStreamGroupStats(-7, -7)
    launches = C.c_int32(-7)
    call = lambda h, it, n: lib.css_stream_present_windows(h, it, n, C.byref(stats), C.byref(launches))
    assert call(None, items, 1) == L.CSS_ERR_INVALID_ARG
    assert call(None, None, 1) == call(None, items, 0) == call(None, items, -1) == L.CSS_ERR_INVALID_ARG
    assert lib.css_stream_present_windows(None, None, 0, None, None) == L.CSS_ERR_INVALID_ARG
    assert (stats.estimator_batches, stats.estimator_segments, launches.value) == (-7, -7, -7)
    assert (items[0].ph.p.status, items[0].ph.p.n_out) == (-7, -7)
    assert all((w.first_frame, w.n_used, w.n_provisional, w.window_max) == (-7, -7, -7, 5.0) for w in wins)


def test_makefile_names_the_header():
    deps = re.findall(r"^build(?:_asan)?/%\.o:.*$", open(os.path.join(CSRC, "Makefile")).read(), flags=re.M)
    assert len(deps) == 2 and all(f"../../include/{hd}" in d for d in deps for hd in OTHERS + (HEADER,))


def test_window_header_points_here():
    """css_mi355_window.h no longer says that windows over a preview's provisional frames do not exist"""
    text = open(os.path.join(ROOT, "include", "css_mi355_window.h")).read()
    assert HEADER in text and "Not covered: windows over a preview" not in text
