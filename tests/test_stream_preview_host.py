"""Previews of streamed sessions (include/css_mi355_preview.h; stream.py preview), the part that needs no GPU: the new header,
the library and the third binding table agree, the handle-taking entry points refuse NULL, and css_stream_preview_samples is
css_stream_final_samples and css_plan put together -- over which the one-pending-segment argument (a preview estimates exactly
one segment per stream, whatever the prefix) is restated."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, pkg

CSRC = os.path.join(ROOT, "notsofar1-challenge_amd", "csrc")
NAMES = ("css_stream_preview_samples", "css_stream_preview", "css_stream_preview_many")
SEGMENTATIONS = ((3.0, 1.5), (2.0, 0.5), (10.0, 5.0))


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "css_mi355_preview.h")).read(), flags=re.S)


def test_header_library_and_binding_agree():
    L = pkg("_lib")
    text = _header()
    lib = L.load()
    assert '#include "css_mi355.h"' in text
    declared = re.findall(r"\bint\s+(css_\w+)\s*\(", text)
    assert sorted(declared) == sorted(NAMES) == sorted(L.SIGNATURES_PREVIEW)
    assert not set(L.SIGNATURES_PREVIEW) & (set(L.SIGNATURES) | set(L.SIGNATURES_RATE))
    others = [open(os.path.join(ROOT, "include", f)).read() for f in ("css_mi355.h", "css_mi355_rate.h")]
    kinds = {"css_handle_t": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64}
    for name in NAMES:
        for other in others:
            assert not re.search(rf"\b{name}\b", other), f"{name} belongs to css_mi355_preview.h alone"
        fn = getattr(lib, name)   # (AttributeError: the library does not export it)
        params = re.search(rf"\b{name}\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
        restype, argtypes = L.SIGNATURES_PREVIEW[name]
        assert restype is C.c_int and len(argtypes) == len(params), (name, params)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(argtypes)   # load() applied the third table
        for p, a in zip(params, argtypes):
            p = p.strip()
            if "*" in p:
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p, a)
            else:
                assert a is kinds[p.split()[0]], (name, p, a)
    # the item struct as the header lays it out: int32 id, pointer, three int64, int32 status (natural alignment)
    assert [n for n, _ in L.CssStreamPreview._fields_] == ["id", "out_host", "cap", "n_out", "first_sample", "status"]
    assert C.sizeof(L.CssStreamPreview) == 48 and L.CssStreamPreview.out_host.offset == 8 and L.CssStreamPreview.status.offset == 40
    deps = re.findall(r"^build(?:_asan)?/%\.o:.*$", open(os.path.join(CSRC, "Makefile")).read(), flags=re.M)
    assert len(deps) == 2 and all("css_mi355_preview.h" in d and "css_mi355_rate.h" in d for d in deps)


def test_null_handle_is_refused():
    L = pkg("_lib")
    lib = L.load()
    out = np.full((3, 64), 5.0, np.float32)
    n_out, first = C.c_int64(-7), C.c_int64(-7)
    assert lib.css_stream_preview(None, 0, out.ctypes.data_as(C.c_void_p), 64, C.byref(n_out), C.byref(first)) == L.CSS_ERR_INVALID_ARG
    assert (n_out.value, first.value) == (-7, -7) and np.all(out == 5.0)
    items = (L.CssStreamPreview * 2)()
    for it in items:
        it.id, it.out_host, it.cap, it.n_out, it.first_sample, it.status = 0, out.ctypes.data, 64, -7, -7, 77
    stats = L.CssStreamGroupStats(-7, -7)
    assert lib.css_stream_preview_many(None, items, 2, C.byref(stats)) == L.CSS_ERR_INVALID_ARG
    assert all((it.n_out, it.first_sample, it.status) == (-7, -7, 77) for it in items) and np.all(out == 5.0)
    assert (stats.estimator_batches, stats.estimator_segments) == (-7, -7)


def _cfg(seg, hop):
    CSS = pkg("css")
    return CSS.make_run_cfg(CSS.CssCfg(segment_size_sec=seg, hop_size_sec=hop), 16000, 7)


def _prefixes(T, hop):
    edges = [T * 256 + 511, T * 256 + 512, (T + hop) * 256 + 511, (T + hop) * 256 + 512]
    return sorted(set(list(range(0, 6 * T * 256, 97)) + edges))


@pytest.mark.parametrize("seg,hop_s", SEGMENTATIONS)
def test_preview_samples_are_final_samples_and_the_plan(seg, hop_s):
    L = pkg("_lib")
    desc = pkg("weights").ModelDesc.mc_v1()
    rc = _cfg(seg, hop_s)
    T, hop, halo = rc.c.segment_frames, rc.c.hop_frames, rc.c.dilation_frames + rc.c.erosion_frames
    lib, d = L.load(), L.make_desc(desc)
    ok = refused = 0
    for n in _prefixes(T, hop):
        first, count = C.c_int64(-1), C.c_int64(-1)
        status = lib.css_stream_preview_samples(C.byref(d), C.byref(rc.c), n, C.byref(first), C.byref(count))
        p = L.plan(desc, rc, n)
        assert first.value == L.stream_final_samples(desc, rc, n), n
        assert first.value + count.value == p.n_out, n
        assert status == (L.CSS_ERR_ZERO_WEIGHT if p.zero_weight else L.CSS_OK), n
        assert 0 < count.value <= (T + halo - 1) * 256 + 512, (n, count.value)
        assert (first.value, count.value, status) == L.stream_preview_samples(desc, rc, n)
        ok += status == L.CSS_OK
        refused += status != L.CSS_OK
    # with the default windows a prefix of at most one segment has no preview, every longer one has
    assert refused == sum(1 for n in _prefixes(T, hop) if n < T * 256 + 512) and ok > 0
    # arguments: nothing is written on a refusal
    first, count = C.c_int64(-1), C.c_int64(-1)
    for args in ((None, C.byref(rc.c), 10, C.byref(first), C.byref(count)), (C.byref(d), None, 10, C.byref(first), C.byref(count)),
                 (C.byref(d), C.byref(rc.c), -1, C.byref(first), C.byref(count)), (C.byref(d), C.byref(rc.c), 10, None, C.byref(count)),
                 (C.byref(d), C.byref(rc.c), 10, C.byref(first), None)):
        assert lib.css_stream_preview_samples(*args) == L.CSS_ERR_INVALID_ARG
    assert (first.value, count.value) == (-1, -1)


@pytest.mark.parametrize("seg,hop_s", SEGMENTATIONS)
def test_exactly_one_segment_is_pending_for_every_prefix(seg, hop_s):
    """css_stream_final_samples(n) = max(segments_done hop - halo, 0) * 256, so with halo = 0 it counts the segments that are
    done; css_plan(n).num_segments is the recording's count.  Their difference -- what a preview has to estimate -- is 1."""
    L, CSS = pkg("_lib"), pkg("css")
    desc = pkg("weights").ModelDesc.mc_v1()
    rc = CSS.make_run_cfg(CSS.CssCfg(segment_size_sec=seg, hop_size_sec=hop_s, activity_dilation_sec=0.0, activity_erosion_sec=0.0), 16000, 7)
    T, hop = rc.c.segment_frames, rc.c.hop_frames
    assert rc.c.dilation_frames == 0 and rc.c.erosion_frames == 0
    for n in _prefixes(T, hop):
        fin = L.stream_final_samples(desc, rc, n)
        assert fin % (hop * 256) == 0
        assert L.plan(desc, rc, n).num_segments - fin // (hop * 256) == 1, n
