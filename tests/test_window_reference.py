"""tests/window_reference.py on the CPU, on the cases tests/test_hip_window_kernels.py gives the kernels (DESIGN.md 7b "The window
and session hand-off kernels, launch form by launch form"):
  (a) header, library, binding and Makefile line of include/css_mi355_handoff_kernels.h agree; a null handle and a null table are
      refused;
  (b) composition: the scan model's runs are handoff_reference.kept_ranges on every case and on random gates; the gather model is
      handoff_reference.operand(concat(...)) rounded to float32; norm and session windows are the package's whisper_normalize,
      session_windows and session_window_fill; the stream-window model is the package's whisper_window on a simulated ring; the
      restated walks (scan_walk, row_walk) are the definitions on every case;
  (c) every named mistake changes at least one asserted element on at least one case of the GPU module's own case list (the
      catching case is printed).
No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import handoff_reference as H
import window_reference as W
from conftest import ROOT, pkg

CSRC = os.path.join(ROOT, "notsofar1-challenge_amd", "csrc")
HEADER = "css_mi355_handoff_kernels.h"
NAMES = ("css_session_scan_host", "css_session_gather_host", "css_session_norm_host", "css_session_windows_host", "css_stream_windows_host")
DESCS = ("CssSessionScanJob", "CssSessionGatherJob", "CssSessionNormJob", "CssSessionWindowsJob", "CssStreamWindowJob")


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------

def test_header_library_and_binding_agree():
    L = pkg("_lib")
    lib = L.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)
    assert '#include "css_mi355_stream_kernels.h"' in text and "typedef struct CssKArray" not in text
    assert sorted(re.findall(r"\bint\s+(css_\w+)\s*\(", text)) == sorted(NAMES) == sorted(L.HANDOFF_KERNEL_BINDINGS)
    tables = [n for n in dir(L) if n.startswith("SIGNATURES") or n.endswith("_SIGNATURES") or n.endswith("_BINDINGS")]
    assert len(tables) == 17
    for n in tables:
        assert n == "HANDOFF_KERNEL_BINDINGS" or not set(L.HANDOFF_KERNEL_BINDINGS) & set(getattr(L, n)), n
    for f in os.listdir(os.path.join(ROOT, "include")):
        if f != HEADER:
            other = open(os.path.join(ROOT, "include", f)).read()
            for name in NAMES + DESCS:
                assert not re.search(rf"\b{name}\b", other), f"{name} belongs to {HEADER} alone"
    for name in NAMES:
        params = re.search(rf"\b{name}\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
        restype, argtypes = L.HANDOFF_KERNEL_BINDINGS[name]
        fn = getattr(lib, name)   # (AttributeError: the library does not export it)
        assert restype is C.c_int and len(argtypes) == len(params), name
        assert fn.restype is C.c_int and list(fn.argtypes) == list(argtypes)
    kinds = {"int32_t": C.c_int32, "int64_t": C.c_int64, "CssKArray": L.CssKArray}
    for desc in DESCS:   # the header's fields in the header's order, with the header's types
        body = re.search(rf"typedef struct {desc} \{{(.*?)\}} {desc};", text, flags=re.S).group(1)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                kind, names = decl.split(None, 1)
                fields += [(n.strip(), kinds[kind]) for n in names.split(",")]
        assert fields == list(getattr(L, desc)._fields_), desc
        ins, outs = L.HANDOFF_KERNEL_ARRAYS[desc]
        assert {n for n, _ in ins + outs} == {n for n, k in fields if k is L.CssKArray}, desc
    assert L.HANDOFF_STATE == W.STATE and L.WINDOW_OUT == W.RES and L.WINDOW_OUT.itemsize == 24
    assert int(re.search(r"#define CSS_WINDOW_KERNEL_ITEMS (\d+)", text).group(1)) == L.WINDOW_KERNEL_ITEMS == 2 * W.TABLE
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "api_handoff_kernels.hip" in re.search(r"^SRCS\s*:=(.*)$", mk, flags=re.M).group(1).split()
    assert re.search(rf"^build/api_handoff_kernels\.o build_asan/api_handoff_kernels\.o:.*include/{HEADER}", mk, flags=re.M)
    for rule in re.findall(r"^build(?:_asan)?/%\.o:(.*)$", mk, flags=re.M):   # (the staging both kernel-entry units share)
        assert "api_kernel_stage.hpp" in rule.split()


def test_null_handle_and_null_table_are_refused():
    L = pkg("_lib")
    lib = L.load()
    res = np.full(24, 7, np.uint8)
    assert lib.css_session_scan_host(None, (L.CssSessionScanJob * 1)()) == L.CSS_ERR_INVALID_ARG
    assert lib.css_session_scan_host(None, None) == L.CSS_ERR_INVALID_ARG
    assert lib.css_session_gather_host(None, (L.CssSessionGatherJob * 1)()) == L.CSS_ERR_INVALID_ARG
    assert lib.css_session_gather_host(None, None) == L.CSS_ERR_INVALID_ARG
    assert lib.css_session_norm_host(None, (L.CssSessionNormJob * 1)()) == L.CSS_ERR_INVALID_ARG
    assert lib.css_session_norm_host(None, None) == L.CSS_ERR_INVALID_ARG
    assert lib.css_session_windows_host(None, (L.CssSessionWindowsJob * 1)()) == L.CSS_ERR_INVALID_ARG
    assert lib.css_session_windows_host(None, None) == L.CSS_ERR_INVALID_ARG
    assert lib.css_stream_windows_host(None, (L.CssStreamWindowJob * 1)(), 1, res.ctypes.data, 1) == L.CSS_ERR_INVALID_ARG
    assert lib.css_stream_windows_host(None, None, 0, None, 0) == L.CSS_ERR_INVALID_ARG
    assert (res == 7).all()


# ---- (b) composition ----------------------------------------------------------------------------------------------------------------

def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


def _rows_of(c):
    return [c["gate"][c["gate_off"] + k * c["TL"]:c["gate_off"] + (k + 1) * c["TL"]] for k in range(c["S"])]


def test_scan_runs_are_kept_ranges():
    rng = np.random.default_rng(5)
    extra = [W._scan_case(f"random_{i}", 1, int(rng.integers(1, 2600)), int(rng.choice([0, 1, 2, 7, 40])), 1, int(rng.integers(4)),
                          (("sparse", "dense", "bytes")[i % 3],), 10_000 + i) for i in range(60)]
    for c in W.scan_cases() + extra:
        big = dict(c, cap_ranges=max(max(c["counts"]), 1))
        o = W.scan(big)
        S, TL, cap = c["S"], c["TL"], big["cap_ranges"]
        for k, row in enumerate(_rows_of(c)):
            want = H.kept_ranges(row, c["pad"], 256 * (TL + 1), bool(c["drop"]))
            n = int(o["n_ranges"][k])
            assert n == len(want) == c["counts"][k], (c["name"], k)
            _same(o["regs"][k * cap * 2:(k * cap + n) * 2].reshape(-1, 2), want, (c["name"], k, "regs"))
            _same(o["ranges_out"][:S * cap * 2], o["regs"][:S * cap * 2], c["name"])
            lens = want[:, 1] - want[:, 0]
            _same(o["offs"][k * cap:k * cap + n], np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)[:n], (c["name"], k, "offs"))
            assert o["st"]["A"][k] == lens.sum() and o["st"]["J"][k] == lens.sum() // 160 == o["n_new"][k] == o["n_frames_out"][k]
            if c["drop"]:
                assert o["psum"][k * (TL + 1) + TL] == np.count_nonzero(row) and o["psum"][k * (TL + 1)] == 0
        # the first cap runs of the case's own capacity are the first cap rows of the full table; nothing else is written
        small, cs = W.scan(c), c["cap_ranges"]
        for k in range(S):
            n = min(c["counts"][k], cs)
            _same(small["regs"][k * cs * 2:(k * cs + n) * 2], o["regs"][k * cap * 2:(k * cap + n) * 2], (c["name"], k, "cap"))
            assert (small["regs"][(k * cs + n) * 2:(k + 1) * cs * 2] == W.CANARY64).all() and (small["offs"][k * cs + n:(k + 1) * cs] == W.CANARY64).all()
            assert small["n_ranges"][k] == c["counts"][k]
        assert (small["st"]["pad"] == W.CANARY32).all() and (small["regs"][S * cs * 2:] == W.CANARY64).all()
        if not c["drop"]:
            assert (small["psum"] == W.CANARY32).all()


def test_scan_walk_is_the_definition():
    for c in W.scan_cases():
        a, b = W.scan(c), W.scan_walk(c)
        for k in a:
            _same(a[k], b[k], (c["name"], k))


def test_scan_cases_cover_the_issue():
    cs = W.scan_cases()
    assert {c["TL"] for c in cs} >= set(W.SCAN_TLS) and {c["pad"] for c in cs} >= set(W.PADS)
    for TL in W.SCAN_TLS:
        assert {c["gate_off"] for c in cs if c["TL"] == TL} >= {0, 1, 2, 3}, TL
    assert {c["S"] for c in cs} == {1, 2, 3, 4} and {k for c in cs for k in c["kinds"]} == set(W.GATE_KINDS)
    assert any(not c["drop"] for c in cs)
    for pad in W.PADS[:4]:   # (2 pad + 2 frames apart: one block between the runs; 2 pad + 1: the runs are one)
        split = [c for c in cs if c["name"] == f"scan_gap_split_TL1027_pad{pad}"][0]
        merge = [c for c in cs if c["name"] == f"scan_gap_merge_TL1027_pad{pad}"][0]
        r = H.kept_ranges(_rows_of(split)[0], pad, 256 * 1028)
        assert len(r) > 1 and r[1, 0] - r[0, 1] == 256, pad
        t2 = np.flatnonzero(_rows_of(merge)[0])[1]
        assert H.kept_ranges(_rows_of(merge)[0], pad, 256 * 1028)[0, 1] > 256 * t2 >= r[0, 1]
    # a run ends and a run starts at each of the frames 1023, 1024, 1025 under each row alignment
    seen = set()
    for c in cs:
        for k, row in enumerate(_rows_of(c)):
            a = (c["gate_off"] + k * c["TL"]) & 3
            act = np.concatenate([[0], row != 0, [0]]).astype(np.int8)
            d = np.diff(act)
            for t in (1023, 1024, 1025):
                if t < c["TL"] and d[t] == 1:
                    seen.add((a, t, "start"))
                if t < c["TL"] and d[t + 1] == -1:
                    seen.add((a, t, "end"))
    assert len(seen) == 4 * 3 * 2, sorted({(a, t, w) for a in range(4) for t in (1023, 1024, 1025) for w in ("start", "end")} - seen)
    over = [c for c in cs if max(c["counts"]) > c["cap_ranges"]]
    assert {c["cap_ranges"] == 1 for c in over} == {True, False} and any(max(c["counts"]) == c["cap_ranges"] > 1 for c in cs)
    assert any(c["cap_ranges"] == W.path_cap(c["TL"], c["pad"]) for c in cs)
    assert any((r == v).any() for c in cs for r in _rows_of(c) for v in (0x80, 0xFF))


def test_gather_is_the_padded_concatenation():
    seen_over = 0
    for c in W.gather_cases():
        S, cap, per = c["S"], c["cap_ranges"], c["rows"] * 160
        got = W.gather(c, W.canary(S * per + 416))
        regs = c["regs"].reshape(S, cap, 2)
        assert not np.isnan(got).any(), c["name"]
        last = int(c["st"]["A"][S - 1]) + 400 if c["n_ranges"][S - 1] > 0 and c["st"]["A"][S - 1] > 0 else 0
        assert (got[max(S * per, (S - 1) * per + last):] == 0).all()      # (the last speaker's padded samples may reach into the 416)
        for k in range(S):
            A, n = int(c["st"]["A"][k]), int(c["n_ranges"][k])
            row = c["wav"][c["wav_off"] + k * c["wav_ld"]:c["wav_off"] + (k + 1) * c["wav_ld"]]
            if n > cap:
                seen_over += 1      # (the runs the table lacks are the last tabulated run's continuation: stated, not a concatenation)
                continue
            if A < 201 or n == 0:
                assert A in (0, 1) or n == 0
                continue
            want = H.operand(H.concat(row, regs[k, :n])).astype(np.float32)
            assert len(want) == A + 400
            m = min(len(want), per + (416 if k == S - 1 else 0))
            _same(got[k * per:k * per + m], want[:m], (c["name"], k))
            assert (got[k * per + m:(k + 1) * per] == 0).all()
    assert seen_over >= 4
    names = " ".join(c["name"] for c in W.gather_cases())
    assert "gather_A256" in names and "gather_A512" in names and "nodrop" in names
    assert {c["rows"] - W.path_rows((c["wav_ld"] - 3) // 256 - 1) for c in W.gather_cases() if c["name"].startswith("gather_scan")} == {0, 1}


def test_norm_and_session_windows_are_the_packages_rule():
    S_ = pkg("stream")
    for c in W.norm_cases():
        S, nm = c["S"], c["n_mels"]
        out = W.session_norm(c, W.canary(S * nm * c["out_ld"] + W.SLACK))
        body = out[:S * nm * c["out_ld"]].reshape(S, nm, c["out_ld"])
        mel = c["mel"][:S * nm * c["mel_ld"]].reshape(S, nm, c["mel_ld"])
        for k in range(S):
            n = min(int(c["st"]["J"][k]), c["out_ld"]) if c["rows"] > 0 else 0
            _same(body[k, :, :n], S_.whisper_normalize(mel[k, :, :n], W.decode_max(c["st"]["gmax"][k])), (c["name"], k))
            assert (W.bits(body[k, :, n:]) == W.CANARY).all()
    for c in W.session_window_cases():
        if "ties" in c["name"]:      # (a NaN frame: whisper_normalize has np.maximum's rule, the kernel fmaxf's; test_ties states the values)
            continue
        o = W.session_windows(c)
        S, nm, mel_ld = c["S"], c["n_mels"], c["mel_ld"]
        mel = c["mel"][c["mel_off"]:c["mel_off"] + S * nm * mel_ld].reshape(S, nm, mel_ld)
        dt = np.float16 if c["f16"] else np.float32
        for k in range(S):
            J = min(int(c["st"]["J"][k]), c["max_frames"])
            M = W.decode_max(c["st"]["gmax"][k])
            assert o["n_windows_out"][k] == -(-J // c["stride"]) and o["window_max_out"][k] == M
            normed = S_.whisper_normalize(mel[k, :, :J], M)
            if "win" in o:
                win = o["win"][c["win_off"]:c["win_off"] + S * c["cap_windows"] * nm * c["ld"]].reshape(S, c["cap_windows"], nm, c["ld"])
                want = S_.session_windows(normed, M, c["width"], c["stride"], dt) if J else np.zeros((0, nm, c["width"]), dt)
                _same(win[k, :len(want), :, :c["width"]].view(dt), want, (c["name"], k, "win"))
                rest = np.concatenate([win[k, len(want):].reshape(-1), win[k, :, :, c["width"]:].reshape(-1)])
                assert (rest == W.CANARY16).all() if c["f16"] else (W.bits(rest) == W.CANARY).all()
            if "whole" in o and J:
                whole = o["whole"][c["whole_off"]:c["whole_off"] + S * nm * c["whole_ld"]].reshape(S, nm, c["whole_ld"]).view(dt)
                n = min(J, c["whole_ld"])
                _same(whole[k, :, :n], normed[:, :n].astype(dt), (c["name"], k, "whole"))
                assert (whole[k, :, n:] == dt(S_.session_window_fill(M))).all()


def test_row_walk_is_the_definition_and_a_head_in_bytes_shows_nowhere():
    n = 0
    for c in W.session_window_cases():
        if c["width"] > 100 or c["whole_ld"] > 100:     # (the walk is a Python loop per column)
            continue
        a = W.session_windows(c)
        for mut in ("walk",) + W.WINDOW_MISTAKES_UNREAD:
            b = W.session_windows(c, mut=mut)
            for k in a:
                _same(a[k], b[k], (c["name"], k, mut))
        n += 1
    assert n >= 64 + 12


def _history(it, seed):
    """a history of J + P frames of which the ring holds the last `hist` final ones, as the stream would have left it"""
    rng = np.random.default_rng(seed)
    nm, hist, J = it["n_mels"], it["hist"], it["J"]
    P = W.span(it)[4]
    lo = max(J - hist, 0)
    frames = (rng.random((nm, J - lo + P)) * 12 - 10).astype(np.float32)     # frames lo .. J + P - 1
    ring, fmax = np.full((nm, hist), np.inf, np.float32), np.full(hist, np.inf, np.float32)
    slots = np.arange(lo, J) % hist
    ring[:, slots], fmax[slots] = frames[:, :J - lo], frames[:, :J - lo].max(axis=0)
    it = dict(it, ring=np.concatenate([np.zeros(it["ring_off"], np.float32), ring.reshape(-1)]), fmax=fmax)
    if it.get("pv") is not None:
        pv, pvmax = np.full((nm, it["pv_ld"]), np.inf, np.float32), np.full(it["pv_ld"], np.inf, np.float32)
        pv[:, :P], pvmax[:P] = frames[:, J - lo:], frames[:, J - lo:].max(axis=0)
        it.update(pv=np.concatenate([np.zeros(it["pv_off"], np.float32), pv.reshape(-1)]), pvmax=pvmax)
    return it, frames, lo


def test_stream_windows_are_whisper_window_on_a_simulated_ring():
    S_ = pkg("stream")
    n = 0
    for name, items in W.stream_tables():
        for i, it in enumerate(items):
            if "ties" in it["name"] or "nan" in it["name"]:
                continue
            sim, frames, lo = _history(it, 31 * n + i)
            out, res = W.stream_window(sim, W.stream_out_blank(sim), W.canary_res(1)[0])
            a, used, n_prov, p0, P = W.span(sim)
            E = it["J"] + P
            assert a == max(E - it["n_frames"], lo) and used == E - a and n_prov == min(used, P)
            assert (res["first_frame"], res["n_used"], res["n_provisional"]) == (a, used, n_prov) and res["pad"] == W.CANARY32
            dt = np.float16 if it["f16"] else np.float32
            body = out[it["out_off"]:it["out_off"] + it["n_mels"] * it["ld"]].reshape(it["n_mels"], it["ld"])
            canary = W.CANARY16 if it["f16"] else W.CANARY
            raw_canary = (lambda v: v) if it["f16"] else W.bits
            assert (raw_canary(body[:, it["width"]:]) == canary).all() and (raw_canary(out[:it["out_off"]]) == canary).all()
            if used == 0:
                assert (raw_canary(body) == canary).all() and W.bits(res["window_max"]) == np.uint32(W.CANARY32)
                continue
            span = frames[:, a - lo:a - lo + used]
            _same(body[:, :it["width"]].view(dt), S_.whisper_window(span, it["width"], dt), (name, it["name"]))
            assert res["window_max"] == span.max()
        n += 1


def test_ties_nan_and_negative_maxima():
    half = lambda w: np.array([w], np.uint16).view(np.float16)[0]
    for c in W.tie_cases_session():
        o = W.session_windows(c)
        if "ties" not in c["name"]:
            assert all(W.decode_max(g) < 0 for g in c["st"]["gmax"]) and o["window_max_out"][0] == np.float32(-3.96875)
            continue
        at = c["win_off"]
        row = o["win"][at:at + 4]
        if c["f16"]:
            assert [float(half(w)) for w in row] == [1.0, 1 + 2.0 ** -9, 3.0, 1.0]      # tie to even down, tie to even up, the maximum, the floor
        else:
            assert [float(v) for v in row] == [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 3.0, 1.0]
    for it in W.tie_items():
        out, res = W.stream_window(it, W.stream_out_blank(it), W.canary_res(1)[0])
        if "ties" in it["name"]:
            row = out[it["out_off"]:it["out_off"] + 4]
            want = [1.0, 1 + 2.0 ** -9, 1 + 2.0 ** -9, 1.0] if it["f16"] else [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 5 * 2.0 ** -11, 1.0]
            assert [float(half(w)) if it["f16"] else float(w) for w in row] == want and res["window_max"] == 8.0
        else:
            assert np.isnan(it["ring"]).sum() + np.isnan(it["pv"]).sum() == 1
            body = out[it["out_off"]:it["out_off"] + it["n_mels"] * it["ld"]]
            vals = body.view(np.float16) if it["f16"] else body.view(np.float32)
            assert not np.isnan(vals.reshape(it["n_mels"], it["ld"])[:, :it["width"]].astype(np.float32)).any()
            floor = (np.float32(res["window_max"]) - np.float32(8) + np.float32(4)) * np.float32(0.25)
            assert (vals.astype(np.float32) == floor).any()


def test_stream_tables_cover_the_issue():
    tabs = W.stream_tables()
    items = [it for _, t in tabs for it in t]
    assert {it["hist"] for it in items} >= set(W.HISTS) and max(it["J"] for it in items) == 2 ** 32 + 5
    assert sorted(len(t) for _, t in tabs)[-2:] == [64, 64] and 33 in [len(t) for _, t in tabs] and all(len(t) <= 64 for _, t in tabs)
    assert {(it["ring_off"], it["pv_off"], it["out_off"], it["f16"]) for it in items if it["name"].startswith("align")} == \
        {(r, p, o, f) for r in range(4) for p in range(4) for o in range(8) for f in (0, 1)}
    assert {it["width"] for it in items} >= set(range(1, 18)) | {3000} and {it["n_mels"] for it in items} >= {5, 8, 9, 80, 128}
    wraps, seams, above, whole_pv = set(), set(), 0, 0
    for it in items:
        assert 1 <= it["n_frames"] <= it["width"] <= min(it["ld"], 3000) and it["hist"] >= 1 and it["J"] >= 0, it["name"]      # (the entry's preconditions)
        assert it.get("pv") is not None or it["n_frames"] <= min(it["J"], it["hist"]), it["name"]
        a, used, n_prov, p0, P = W.span(it)
        V = 8 if it["f16"] else 4
        head = (-(it["out_off"] * (2 if it["f16"] else 4)) % 16) // (2 if it["f16"] else 4)
        n_ring = used - n_prov
        first = a % it["hist"]
        if n_ring and first + n_ring > it["hist"] and it["hist"] - first >= head:
            wraps.add((it["f16"], (it["hist"] - first - head) % V))
        if n_prov and n_ring >= head:
            seams.add((it["f16"], (n_ring - head) % V))
        above += it.get("pv") is not None and int(it["n_new"][0]) > it["pv_ld"]
        whole_pv += used > 0 and n_prov == used and it["J"] == 0
    for f16, V in ((0, 4), (1, 8)):
        assert {p for f, p in wraps if f == f16} == set(range(V)) and {p for f, p in seams if f == f16} == set(range(V)), (wraps, seams)
    assert above >= 9 and whole_pv >= 2
    big = [t for n_, t in tabs if n_ == "table_64"][0]
    assert len({id(it) for it in big}) < 64 and len({it["n_mels"] for it in big}) >= 4


# ---- (c) every named mistake is caught ------------------------------------------------------------------------------------------------

def _differs(a, b):
    if isinstance(a, dict):
        return any(a[k].tobytes() != b[k].tobytes() for k in a)
    if isinstance(a, tuple):
        return any(x.tobytes() != y.tobytes() for x, y in zip(a, b))
    return a.tobytes() != b.tobytes()


def _catch(mistakes, cases, run):
    caught = {}
    for m in mistakes:
        for c in cases:
            if _differs(run(c, None), run(c, m)):
                caught[m] = c["name"]
                break
    return caught


def test_every_scan_and_gather_mistake_is_caught():
    caught = _catch(W.SCAN_MISTAKES, W.scan_cases(), lambda c, m: W.scan(c, mut=m))
    print("\n".join(f"  scan    {m:22s} {caught.get(m)}" for m in W.SCAN_MISTAKES))
    assert set(caught) == set(W.SCAN_MISTAKES)
    assert "cap" in caught["no_cap_guard"]
    g = _catch(W.GATHER_MISTAKES, W.gather_cases(), lambda c, m: W.gather(c, W.canary(c["S"] * c["rows"] * 160 + 416), m))
    print("\n".join(f"  gather  {m:22s} {g.get(m)}" for m in W.GATHER_MISTAKES))
    assert set(g) == set(W.GATHER_MISTAKES)


def test_every_norm_and_window_mistake_is_caught():
    n = _catch(W.NORM_MISTAKES, W.norm_cases(), lambda c, m: W.session_norm(c, W.canary(c["S"] * c["n_mels"] * c["out_ld"] + W.SLACK), m))
    print("\n".join(f"  norm    {m:22s} {n.get(m)}" for m in W.NORM_MISTAKES))
    assert set(n) == set(W.NORM_MISTAKES)
    cases = sorted(W.session_window_cases(), key=lambda c: c["width"] * c["S"] + c["whole_ld"])      # (the walk is slow on the long rows)
    w = _catch(W.WINDOW_MISTAKES, cases, lambda c, m: W.session_windows(c, mut=m))
    print("\n".join(f"  windows {m:22s} {w.get(m)}" for m in W.WINDOW_MISTAKES))
    assert set(w) == set(W.WINDOW_MISTAKES)
    assert "whole" in w["chunk_start_dropped"]


def test_every_stream_window_mistake_is_caught():
    items = [it for _, t in W.stream_tables() for it in t]
    s = _catch(W.STREAM_MISTAKES, items, lambda it, m: W.stream_window(it, W.stream_out_blank(it), W.canary_res(1)[0], m))
    print("\n".join(f"  stream  {m:22s} {s.get(m)}" for m in W.STREAM_MISTAKES))
    assert set(s) == set(W.STREAM_MISTAKES)
