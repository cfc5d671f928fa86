"""Previews with hand-off (include/css_mi355_preview_handoff.h; stream.py preview(handoff=True)), the part that needs no GPU:
the fourth header, the library and the fourth binding table agree, the item struct is laid out as the ctypes mirror lays it out,
the entry points refuse NULL, and the capacities css_stream_handoff_bounds(..., -1, ...) gives for finish hold for a preview
with hand-off after every prefix -- which is why the header declares no bounds function of its own."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, pkg

CSRC = os.path.join(ROOT, "notsofar1-challenge_amd", "csrc")
HEADERS = ("css_mi355.h", "css_mi355_rate.h", "css_mi355_preview.h", "css_mi355_preview_handoff.h")
NAMES = ("css_stream_preview_handoff", "css_stream_preview_handoff_many")
SEGMENTATIONS = ((3.0, 1.5), (2.0, 0.5), (10.0, 5.0))     # test_stream_preview_host.py's


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADERS[3])).read(), flags=re.S)


def test_header_library_and_binding_agree():
    L = pkg("_lib")
    text = _header()
    lib = L.load()
    assert '#include "css_mi355_preview.h"' in text
    declared = re.findall(r"\bint\s+(css_\w+)\s*\(", text)
    assert sorted(declared) == sorted(NAMES) == sorted(L.SIGNATURES_PREVIEW_HANDOFF)
    assert not set(L.SIGNATURES_PREVIEW_HANDOFF) & (set(L.SIGNATURES) | set(L.SIGNATURES_RATE) | set(L.SIGNATURES_PREVIEW))
    others = [open(os.path.join(ROOT, "include", f)).read() for f in HEADERS[:3]]
    kinds = {"css_handle_t": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64}
    for name in NAMES:
        for other in others:
            assert not re.search(rf"\b{name}\b", other), f"{name} belongs to {HEADERS[3]} alone"
        fn = getattr(lib, name)   # (AttributeError: the library does not export it)
        params = re.search(rf"\b{name}\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
        restype, argtypes = L.SIGNATURES_PREVIEW_HANDOFF[name]
        assert restype is C.c_int and len(argtypes) == len(params), (name, params)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(argtypes)   # load() applied the fourth table
        for p, a in zip(params, argtypes):
            p = p.strip()
            if "*" in p:
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p, a)
            else:
                assert a is kinds[p.split()[0]], (name, p, a)
    # no bounds function of its own: css_stream_handoff_bounds(..., -1, ...) is the rule, and the header says so
    assert not any("bounds" in n for n in declared)
    assert "css_stream_handoff_bounds" in open(os.path.join(ROOT, "include", HEADERS[3])).read()


def test_item_struct_layout():
    """CssStreamPreviewHandoff as the header lays it out: the 48-byte CssStreamPreview first, then two pointers"""
    L = pkg("_lib")
    body = re.search(r"typedef struct CssStreamPreviewHandoff \{(.*?)\} CssStreamPreviewHandoff;", _header(), flags=re.S).group(1)
    members = [re.sub(r"\s+", " ", m).strip() for m in body.split(";") if m.strip()]
    assert members == ["CssStreamPreview p", "CssStreamHandoffOut* ho", "int64_t* first_frame"]
    T = L.CssStreamPreviewHandoff
    assert [n for n, _ in T._fields_] == ["p", "ho", "first_frame"]
    assert T._fields_[0][1] is L.CssStreamPreview and C.sizeof(L.CssStreamPreview) == 48
    assert (T.p.offset, T.ho.offset, T.first_frame.offset, C.sizeof(T)) == (0, 48, 56, 64)
    assert T.ho.size == T.first_frame.size == C.sizeof(C.c_void_p) == 8
    # the outputs struct it points to is css_mi355.h's, unchanged
    assert C.sizeof(L.CssStreamHandoffOut) == 88 and L.CssStreamHandoffOut.first_activity_frame.offset == 80


def test_makefile_names_all_four_headers():
    deps = re.findall(r"^build(?:_asan)?/%\.o:.*$", open(os.path.join(CSRC, "Makefile")).read(), flags=re.M)
    assert len(deps) == 2 and all(all(f"../../include/{hd}" in d for hd in HEADERS) for d in deps)


def _out(S, n_mels, caps, fill=5.0):
    L = pkg("_lib")
    keep = dict(mel=np.full((S, n_mels, caps[0]), fill, np.float32), ranges=np.full((S, caps[1], 2), -7, np.int64),
                act=np.full((S, caps[2]), 9, np.uint8), nf=np.full(S, -7, np.int64), nr=np.full(S, -7, np.int32), mx=np.full(S, fill, np.float32))
    o = L.CssStreamHandoffOut()
    o.mel_host, o.cap_frames = keep["mel"].ctypes.data, caps[0]
    o.ranges_host, o.cap_ranges = keep["ranges"].ctypes.data, caps[1]
    o.activity_host, o.cap_activity = keep["act"].ctypes.data, caps[2]
    o.n_frames, o.n_ranges, o.raw_max = keep["nf"].ctypes.data, keep["nr"].ctypes.data, keep["mx"].ctypes.data
    o.n_activity, o.first_activity_frame = -7, -7
    return o, keep


def _untouched(o, keep, fill=5.0):
    return (np.all(keep["mel"] == fill) and np.all(keep["ranges"] == -7) and np.all(keep["act"] == 9) and np.all(keep["nf"] == -7) and
            np.all(keep["nr"] == -7) and np.all(keep["mx"] == fill) and (o.n_activity, o.first_activity_frame) == (-7, -7))


def test_null_handle_and_null_pointers_are_refused():
    L = pkg("_lib")
    lib = L.load()
    out = np.full((3, 64), 5.0, np.float32)
    ho, keep = _out(3, 80, (400, 120, 300))
    first_frame = np.full(3, -7, np.int64)
    n_out, first = C.c_int64(-7), C.c_int64(-7)
    ptr, ff = out.ctypes.data_as(C.c_void_p), first_frame.ctypes.data_as(C.c_void_p)
    assert lib.css_stream_preview_handoff(None, 0, ptr, 64, C.byref(n_out), C.byref(first), C.byref(ho), ff) == L.CSS_ERR_INVALID_ARG
    assert lib.css_stream_preview_handoff(None, 0, ptr, 64, C.byref(n_out), C.byref(first), None, None) == L.CSS_ERR_INVALID_ARG
    items = (L.CssStreamPreviewHandoff * 2)()
    for it in items:
        it.p.id, it.p.out_host, it.p.cap, it.p.n_out, it.p.first_sample, it.p.status = 0, out.ctypes.data, 64, -7, -7, 77
        it.ho, it.first_frame = C.pointer(ho), first_frame.ctypes.data
    stats = L.CssStreamGroupStats(-7, -7)
    assert lib.css_stream_preview_handoff_many(None, items, 2, C.byref(stats)) == L.CSS_ERR_INVALID_ARG
    assert lib.css_stream_preview_handoff_many(None, None, 2, None) == L.CSS_ERR_INVALID_ARG
    assert all((it.p.n_out, it.p.first_sample, it.p.status) == (-7, -7, 77) for it in items)
    assert (n_out.value, first.value) == (-7, -7) and np.all(out == 5.0) and np.all(first_frame == -7) and _untouched(ho, keep)
    assert (stats.estimator_batches, stats.estimator_segments) == (-7, -7)


def _cfg(seg, hop):
    CSS = pkg("css")
    return CSS.make_run_cfg(CSS.CssCfg(segment_size_sec=seg, hop_size_sec=hop), 16000, 7)


def _frames_emitted(A):
    """frames a stream has emitted for a concatenation of A samples while it is open (handoff.hip: J frames need 160 J + 40)"""
    return (A - 200) // 160 + 1 if A >= 201 else 0


@pytest.mark.parametrize("drop", [True, False])
@pytest.mark.parametrize("pad", [0, 8, 64])
@pytest.mark.parametrize("seg,hop_s", SEGMENTATIONS)
def test_finish_bounds_hold_for_every_preview(seg, hop_s, pad, drop):
    """Pure arithmetic.  After n samples a preview with hand-off returns the gate bits of frames [t_g, mix_frames), the kept
    ranges of [D, n_out) (D = max(t_g - pad, 0) * 256, t_g = css_stream_final_samples(n) / 256) and the frames J .. A' / 160 - 1,
    where A' are the kept samples of [0, n_out), A those of [0, D) and J the frames A samples complete.  For random gates and
    every n in steps of 97 samples up to 20 s, none exceeds css_stream_handoff_bounds(..., -1, ...)."""
    L = pkg("_lib")
    desc = pkg("weights").ModelDesc.mc_v1()
    rc = _cfg(seg, hop_s)
    hcfg = L.handoff_cfg(80, pad, drop)
    cap_frames, cap_ranges, cap_act = L.stream_handoff_bounds(desc, rc, hcfg, -1)
    pad_eff = pad if drop else 0
    rs = np.random.RandomState(1000 * pad + int(drop) + int(10 * seg))
    total = 20 * 16000
    frames_all = int(L.plan(desc, rc, total).mix_frames) + 8
    # random gates with runs of random lengths: short and long pauses, so that blocks really drop at every pad
    gate = np.zeros(frames_all, np.uint8)
    t, on = 0, True
    while t < frames_all:
        run = int(rs.randint(1, 2 * pad + 40 if not on else 30))
        gate[t:t + run] = on
        t, on = t + run, not on
    most = [0, 0, 0]
    seen = 0
    for n in range(0, total + 1, 97):
        p = L.plan(desc, rc, n)
        if p.zero_weight:
            continue
        seen += 1
        TL, n_out = int(p.mix_frames), int(p.n_out)
        t_g = L.stream_final_samples(desc, rc, n) // 256
        D = max(t_g - pad_eff, 0) * 256
        assert 0 <= t_g <= TL and D <= n_out
        if drop:
            whole = L.handoff_kept_ranges(gate[:TL], 0, TL, pad, 0, n_out, n_out)
            first = max(D // 256 - pad - 2, 0)
            prov = L.handoff_kept_ranges(gate[first:TL], first, TL, pad, D, n_out, n_out)
            # the same rule on the whole prefix, cut at D: what is decided, and the rest
            clipped = [(max(int(a), D), int(b)) for a, b in whole if b > D]
            assert [tuple(map(int, r)) for r in prov] == clipped, n
            A1 = int((whole[:, 1] - whole[:, 0]).sum())
            A0 = A1 - sum(b - a for a, b in clipped)
        else:
            prov = np.array([[D, n_out]], np.int64) if n_out > D else np.zeros((0, 2), np.int64)
            A0, A1 = D, n_out
        n_frames = A1 // 160 - _frames_emitted(A0)
        assert 0 <= n_frames <= cap_frames, (n, n_frames, cap_frames)
        assert len(prov) <= cap_ranges, (n, len(prov), cap_ranges)
        assert TL - t_g <= cap_act, (n, TL - t_g, cap_act)
        most = [max(most[0], n_frames), max(most[1], len(prov)), max(most[2], TL - t_g)]
    print("seg", seg, "pad", pad, "drop", drop, "most (frames, ranges, gate frames)", most, "bounds", (cap_frames, cap_ranges, cap_act))
    assert seen > 0 and most[0] > 0 and most[2] > 0
    if drop:
        assert most[1] >= 2          # the gates really cut the undecided span into several ranges
