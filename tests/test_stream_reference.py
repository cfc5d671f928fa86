"""tests/stream_reference.py on the CPU, on the cases tests/test_hip_stream_kernels.py gives the kernels (DESIGN.md 7b "The stream
kernels, launch form by launch form"):
  (a) header, library and binding of include/css_mi355_stream_kernels.h agree, and a null handle is refused;
  (b) composition: the windowed models over the cases' windows and ranges, and over random ones, reproduce backend_reference's
      whole-recording results bit for bit; the append model over the cases' cuttings and random ones reproduces
      handoff_reference's whole-recording concatenation, frame count n // 160 and padded operand;
  (c) every named mistake changes at least one asserted element on at least one case of the GPU module's own case list (the
      catching case is printed).
No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import backend_reference as B
import css_oracle as O
import handoff_reference as H
import stream_reference as R
from conftest import ROOT, pkg

CSRC = os.path.join(ROOT, "notsofar1-challenge_amd", "csrc")
HEADER = "css_mi355_stream_kernels.h"
NAMES = ("css_stream_tail_host", "css_stream_scatter_host", "css_stream_ingest_host", "css_stream_append_host", "css_stream_mel_host")
DESCS = ("CssKArray", "CssStreamTailJob", "CssStreamScatterJob", "CssStreamIngestJob", "CssStreamAppendJob", "CssStreamMelJob")


def test_header_library_and_binding_agree():
    L = pkg("_lib")
    lib = L.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)
    assert '#include "css_mi355.h"' in text
    assert sorted(re.findall(r"\bint\s+(css_\w+)\s*\(", text)) == sorted(NAMES) == sorted(L.STREAM_KERNEL_BINDINGS)
    for n in dir(L):
        if (n.startswith("SIGNATURES") or n.endswith("_SIGNATURES") or n.endswith("_BINDINGS")) and n != "STREAM_KERNEL_BINDINGS":
            assert not set(L.STREAM_KERNEL_BINDINGS) & set(getattr(L, n)), n
    assert len([n for n in dir(L) if n.startswith("SIGNATURES") or n.endswith("_SIGNATURES") or n.endswith("_BINDINGS")]) == 17
    for f in os.listdir(os.path.join(ROOT, "include")):
        if f != HEADER:
            other = open(os.path.join(ROOT, "include", f)).read()
            for name in NAMES + DESCS:
                if name == "CssKArray" and f == "css_mi355_handoff_kernels.h":    # (its companion includes this header and uses the type)
                    assert f'#include "{HEADER}"' in other and "typedef struct CssKArray" not in other
                    continue
                assert not re.search(rf"\b{name}\b", other), f"{name} belongs to {HEADER} alone"
    for name in NAMES:
        params = re.search(rf"\b{name}\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
        restype, argtypes = L.STREAM_KERNEL_BINDINGS[name]
        fn = getattr(lib, name)   # (AttributeError: the library does not export it)
        assert restype is C.c_int and len(argtypes) == len(params), name
        assert fn.restype is C.c_int and list(fn.argtypes) == list(argtypes)
    kinds = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "CssKArray": L.CssKArray}
    for desc in DESCS:   # the header's fields in the header's order, with the header's types
        body = re.search(rf"typedef struct {desc} \{{(.*?)\}} {desc};", text, flags=re.S).group(1)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            if "*" in decl:
                fields.append((decl.split("*")[-1].strip(), C.c_void_p))
            else:
                kind, names = decl.split(None, 1)
                fields += [(n.strip(), kinds[kind]) for n in names.split(",")]
        assert fields == list(getattr(L, desc)._fields_), desc
        if desc != "CssKArray":
            ins, outs = L.STREAM_KERNEL_ARRAYS[desc]
            assert [n for n, _ in ins + outs if True] and {n for n, _ in ins + outs} == {n for n, k in fields if k is L.CssKArray}, desc
    assert L.HANDOFF_STATE == R.STATE and L.HANDOFF_STATE.itemsize == 24
    assert int(re.search(r"#define CSS_STREAM_KERNEL_JOBS (\d+)", text).group(1)) == L.STREAM_KERNEL_JOBS >= 33
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "api_stream_kernels.hip" in re.search(r"^SRCS\s*:=(.*)$", mk, flags=re.M).group(1).split()
    assert re.search(rf"^build/api_stream_kernels\.o build_asan/api_stream_kernels\.o:.*include/{HEADER}", mk, flags=re.M)


def test_null_handle_and_null_table_are_refused():
    L = pkg("_lib")
    lib = L.load()
    dst = np.full(64, 7.0, np.float32)
    assert lib.css_stream_tail_host(None, 0, (L.CssStreamTailJob * 1)(), 1) == L.CSS_ERR_INVALID_ARG
    assert lib.css_stream_tail_host(None, 1, None, 0) == L.CSS_ERR_INVALID_ARG
    sj = (L.CssStreamScatterJob * 1)()
    sj[0].dst.p, sj[0].dst.elems = dst.ctypes.data, 64
    assert lib.css_stream_scatter_host(None, dst.ctypes.data, 64, 8, 1, sj, 1) == L.CSS_ERR_INVALID_ARG
    ij = (L.CssStreamIngestJob * 1)()
    ij[0].dst.p, ij[0].dst.elems = dst.ctypes.data, 64
    assert lib.css_stream_ingest_host(None, ij, 1) == L.CSS_ERR_INVALID_ARG
    assert lib.css_stream_append_host(None, (L.CssStreamAppendJob * 1)(), 1, dst.ctypes.data, 64) == L.CSS_ERR_INVALID_ARG
    assert lib.css_stream_mel_host(None, 3, dst.ctypes.data, 64, 1, (L.CssStreamMelJob * 1)(), 1) == L.CSS_ERR_INVALID_ARG
    assert (dst == 7.0).all()


# ---- (b) composition: the stitching tail ---------------------------------------------------------------------------------------------

def _whole(c):
    """backend_reference on the whole recording of a case, closed (N segments, T_long TL) and open (one more segment to come):
    {closed: (act_b, Y of the gate gate_in)}"""
    if "_whole" in c:
        return c["_whole"]
    r = R.tail_recording(c)
    S, F, T, hop, N, TL = c["S"], c["F"], c["T"], c["hop"], c["N"], c["TL"]
    out = {}
    for closed in (True, False):
        nseg = N if closed else N + 1
        top = TL if closed else min(TL, N * hop)     # (an open window never asks for a frame its last slot does not cover alone)
        zero = (np.zeros((S, F, TL), np.float32), np.zeros((S, TL), np.float32), np.zeros((S, TL), np.uint8))
        act_b = B.ola_masks(r["masks"], r["windows"], r["perms"], S, F, T, hop, nseg, TL, c["th"], 0, top, zero)[2]
        blank = (np.zeros((S, TL), np.uint8), np.zeros((S, TL), np.uint8))
        fin = B.morphology(r["gate_in"], S, TL, c["dilation"], c["erosion"], 0, TL, blank, O.dilate, O.erode)[1]
        for s in range(S):
            assert (fin[s] == R.dilate_erode(r["gate_in"][s], TL, c["dilation"], c["erosion"])).all()
        Y = B.ola_stft(r["sep"], r["windows"], r["perms"], np.ones((S, TL), np.uint8), S, F, T, hop, nseg, TL, c["KIp"], 0, None, 0, top,
                       np.zeros((S, TL, c["KIp"]), np.float32))
        out[closed] = (act_b, fin, Y)
    c["_whole"] = out
    return out


def _check_window(c, wd):
    """every range of a window against the whole recording: activity bytes, gate bytes, Y rows, ring columns"""
    w, a = R.window_inputs(c, wd)
    act_w, fin_w, Y_w = _whole(c)[wd["closed"]]
    win = (a["w_first"], a["w_mid"], a["w_last"])
    fb, S, TL = w["frame_base"], c["S"], c["TL"]
    halo = c["dilation"] + c["erosion"]
    for lo, hi in wd["ranges"]:
        blank = R.canary8(S * w["ld_frames"]).reshape(S, -1)
        got = R.activity(w, a["masks"], win, a["perms"], lo, hi, blank)
        assert (got[:, lo:hi] == act_w[:, fb + lo:fb + hi]).all(), (c["name"], wd, lo, hi, "activity")
        assert (got[:, :lo] == R.CANARY_BYTE).all() and (got[:, hi:] == R.CANARY_BYTE).all()
        Y0 = R.canary(S * w["ld_frames"] * c["KIp"]).reshape(S, w["ld_frames"], c["KIp"])
        ring0 = R.canary8(S * c["gate_ld"]).reshape(S, -1)
        Y, ring = R.gate_ola(w, a["sep"], win, a["perms"], a["act_b"], lo, hi, Y0, ring0)
        keep = R.gate_bytes(w, a["act_b"], lo, hi)
        for t in range(lo, hi):
            # (an open window has no end: its gate is the recording's wherever the recording's end is out of the morphology's reach)
            if wd["closed"] or fb + t + halo < TL:
                assert (keep[:, t - lo] == fin_w[:, fb + t]).all(), (c["name"], wd, t, "gate")
            for s in range(S):
                want = Y_w[s, fb + t] * (R.f32(1) if keep[s, t - lo] else R.f32(0))
                assert np.array_equal(R.bits(Y[s, t]), R.bits(want)), (c["name"], wd, t, s, "Y")
                assert ring[s, (fb + t) & (c["gate_ld"] - 1)] == keep[s, t - lo]
        assert (R.bits(Y[:, :lo]) == R.CANARY).all() and (R.bits(Y[:, hi:]) == R.CANARY).all()
        assert (ring != R.CANARY_BYTE).sum() == S * (hi - lo)


SMALL = [c for c in R.tail_cases() if c["F"] <= 17 and c["erosion"] < 100]


@pytest.mark.parametrize("c", SMALL, ids=lambda c: c["name"])
def test_windows_compose_to_the_whole_recording(c):
    assert R.tail_cases()[0]["name"] == SMALL[0]["name"]
    for wd in c["windows"]:
        _check_window(c, wd)
    # ... and ANY window base, slot count and range that holds all covering segments of its frames
    rng = np.random.default_rng(c["seed"] + 50)
    T, hop, N, halo = c["T"], c["hop"], c["N"], c["dilation"] + c["erosion"]
    if c.get("threshold_rows"):
        return
    for _ in range(6):
        b = int(rng.integers(0, N))
        n = int(rng.integers(1, N - b + 1))
        closed = bool(rng.integers(0, 2)) and b + n == N
        wd = dict(seg_base=b, num_slots=n, closed=closed, ranges=[], mask_pad=int(rng.integers(0, 4)))
        flo, fhi = R.final_frames(c, wd)
        flo = max(flo, halo if b else 0)
        if fhi <= flo:
            continue
        cuts = sorted(int(x) for x in rng.integers(flo, fhi + 1, 4))
        # (a launch finalises at most gate_ld frames: more would write a ring column twice)
        wd["ranges"] = [(a, min(b, a + c["gate_ld"])) for a, b in ((cuts[0], cuts[1]), (cuts[1], cuts[2]), (cuts[2], cuts[3]))]
        wd["ld_frames"] = max(fhi, cuts[3]) + halo + 16
        _check_window(c, wd)


def test_tail_cases_cover_the_issue():
    cs = R.tail_cases()
    assert {(c["T"], c["hop"]) for c in cs} >= {(8, 8), (8, 4), (8, 3), (16, 1), (186, 179)}
    assert {c["F"] for c in cs} >= {5, 16, 17} and any(c["F"] == 257 and c["T"] == 186 for c in cs)
    assert {c["S"] for c in cs} >= {1, 3, 4}
    assert {c["KIp"] - 2 * c["F"] for c in cs} >= {0} and any(c["KIp"] % 32 == 0 and c["KIp"] - 2 * c["F"] >= 32 for c in cs)
    assert {(c["dilation"], c["erosion"]) for c in cs} >= {(0, 0), (3, 1), (5, 0), (0, 5), (2, 130)}
    assert {c["gate"] for c in cs} == set(R.GATE_KINDS)
    kinds = {(wd["seg_base"] > 0, wd["closed"]) for c in cs for wd in c["windows"]}
    assert kinds == {(False, False), (True, False), (True, True), (False, True)}
    lens = {hi - lo for c in cs for wd in c["windows"] for lo, hi in wd["ranges"]}
    assert lens >= {0, 1, 15, 16, 17, 33}
    assert any(lo % 16 for c in cs for wd in c["windows"] for lo, _ in wd["ranges"])
    assert any(wd["closed"] and (c["TL"] - wd["seg_base"] * c["hop"] - lo) % 16 and hi == c["TL"] - wd["seg_base"] * c["hop"]
               for c in cs for wd in c["windows"] for lo, hi in wd["ranges"])
    # the ring's wrap inside one launch's range; the last block reaching the row's permitted end
    assert any((wd["seg_base"] * c["hop"] + lo) // c["gate_ld"] != (wd["seg_base"] * c["hop"] + hi - 1) // c["gate_ld"]
               for c in cs for wd in c["windows"] for lo, hi in wd["ranges"] if hi > lo)
    for c in cs:
        for wd in c["windows"]:
            w = R.window_of(c, wd)
            assert max(R.morph_reads(w, lo, hi)[1] for lo, hi in wd["ranges"] if hi > lo) <= w["ld_frames"]
    # the last block looking past the row's end (what the path makes: see the last case), and ending exactly at it
    assert any(R.morph_reads(R.window_of(c, wd), lo, hi, blocks=True)[1] > wd["ld_frames"] for c in cs for wd in c["windows"]
               for lo, hi in wd["ranges"] if hi > lo)
    assert any(R.morph_reads(R.window_of(c, wd), lo, hi)[1] == wd["ld_frames"] for c in cs for wd in c["windows"]
               for lo, hi in wd["ranges"] if hi > lo)
    for n in (17, 33):
        jobs = R.tail_table_jobs(n)
        assert len(jobs) == n and {(j[0]["S"], j[0]["F"]) for j in jobs} == {(3, 5)}
        assert len({j[0]["erosion"] for j in jobs}) > 1 and len({j[0]["seg_base"] for j in jobs}) > 1
        assert any(j[3] == j[2] for j in jobs) and jobs[-1][3] - jobs[-1][2] == max(j[3] - j[2] for j in jobs) > jobs[0][3] - jobs[0][2]


def test_activity_at_the_threshold():
    """the planted rows: the mean equals th in float32 (on), its lower neighbour (off), its upper neighbour (on), in every frame"""
    for c in R.tail_cases():
        if not c.get("threshold_rows"):
            continue
        for w, a, lo, hi in R.tail_jobs(c):
            got = R.activity(w, a["masks"], (a["w_first"], a["w_mid"], a["w_last"]), a["perms"], lo, hi, R.canary8(3 * w["ld_frames"]).reshape(3, -1))
            assert (got[0, lo:hi] == 1).all() and (got[1, lo:hi] == 0).all() and (got[2, lo:hi] == 1).all(), c["name"]


# ---- (b) composition: the append -----------------------------------------------------------------------------------------------------

def _compose(c, rounds=None):
    defs = [R.append_definition(c, k) for k in range(c["S"])]
    frames = [0] * c["S"]
    got = [[] for _ in range(c["S"])]

    def on_round(job, res, _):
        for k, r in enumerate(res):
            A0, J0 = int(job["st"][k]["A"]), int(job["st"][k]["J"])
            x, nfr, P = defs[k]
            assert r["A1"] <= len(x) and np.array_equal(R.bits(r["xs"][A0 - r["base"]:]), R.bits(x[A0:r["A1"]])), (c["name"], k, "concatenation")
            want = np.zeros(r["defined"], np.float32)
            seg = P[160 * J0:160 * J0 + r["defined"]]
            want[:len(seg)] = seg
            assert np.array_equal(R.bits(want), R.bits(r["operand"][:r["defined"]])), (c["name"], k, job["t_g1"], "operand")
            assert np.isfinite(r["operand"]).all() and np.isfinite(r["carry"]).all() and np.isfinite(r["tail"]).all()
            frames[k] += r["n_new"]
            got[k].extend(r["act"])
    st = R.append_chain(c, rounds=rounds, on_round=on_round)[2]
    gate = R.append_recording(c)[1]
    for k in range(c["S"]):
        x, nfr, P = defs[k]
        assert st[k]["A"] == len(x) and st[k]["J"] == nfr == frames[k] == len(x) // 160, (c["name"], k)
        assert (np.array(got[k], np.uint8) == gate[k]).all()
        if len(x) >= 201:
            assert np.array_equal(P, H.operand(x).astype(np.float32))


@pytest.mark.parametrize("c", R.append_cases(), ids=lambda c: c["name"])
def test_rounds_compose_to_the_whole_recording(c):
    _compose(c)
    if c["TL"] > 200:
        return
    rng = np.random.default_rng(c["seed"] + 9)
    pad = c["pad"] if c["drop"] else 0
    for _ in range(3):   # ... and ANY cutting
        cuts = sorted(set(int(t) for t in rng.integers(1, c["TL"], int(rng.integers(1, 6)))))
        rounds, t_g, D = [], 0, 0
        for t1 in cuts:
            if t1 - max(min(t_g, D // 256 - pad - 1), 0) > c["gate_ld"]:
                continue
            rounds.append((t_g, t1, D, max(t1 - pad, 0) * 256, 0))
            t_g, D = t1, max(t1 - pad, 0) * 256
        if c["TL"] - max(min(t_g, D // 256 - pad - 1), 0) > c["gate_ld"]:
            continue
        rounds.append((t_g, c["TL"], D, c["n_out"], 1))
        _compose(c, rounds)


def test_append_cases_cover_the_issue():
    cs = R.append_cases()
    assert {c["pad"] for c in cs} == {0, 1, 3, 8, 300} and {c["drop"] for c in cs} == {0, 1}
    assert {c["cut"] for c in cs} >= {"every_frame", "7", "16", "100", "all_at_once"}
    closing_A1, blocks = set(), {0: 0, 1: 0}
    for c in cs:
        def on_round(job, res, _, c=c):
            blocks[job["closing"]] = max(blocks[job["closing"]], -(-job["D1"] // 256) - job["D0"] // 256)
            if job["closing"]:
                closing_A1.update(r["A1"] for r in res)
        R.append_chain(c, on_round=on_round)
    assert blocks[0] > 256 and blocks[1] > 256                      # one open and one closing round of more than 256 blocks
    assert 0 in closing_A1 and any(0 < a < 201 for a in closing_A1) and any(a % 256 for a in closing_A1)
    # ring wrap inside the keep rule's look-back
    assert any(t1 // c["gate_ld"] != max(D0 // 256 - c["pad"] - 1, 0) // c["gate_ld"] for c in cs if c["drop"] for _, t1, D0, _, _ in R.append_rounds(c))


# ---- (c) the named mistakes ----------------------------------------------------------------------------------------------------------

def _differs(a, b):
    return any(x.shape != y.shape or (x != y).any() for x, y in zip(a, b))


def _tail_outputs(w, a, lo, hi, mut, with_ring):
    """what the GPU test compares of a job: the ring only where its job runs with one"""
    win = (a["w_first"], a["w_mid"], a["w_last"])
    S = w["S"]
    act = R.activity(w, a["masks"], win, a["perms"], lo, hi, R.canary8(S * w["ld_frames"]).reshape(S, -1), mut)
    Y, ring = R.gate_ola(w, a["sep"], win, a["perms"], a["act_b"], lo, hi, R.canary(S * w["ld_frames"] * w["KIp"]).reshape(S, w["ld_frames"], -1),
                         R.canary8(S * w["gate_ld"]).reshape(S, -1) if with_ring else None, mut)
    return [act, R.bits(Y)] + ([ring] if with_ring else [])


def test_every_tail_mistake_is_caught():
    caught = {}
    cache = {}
    for mut in R.TAIL_MISTAKES:
        for c in R.tail_cases():
            if c["F"] > 17 or mut in caught:
                continue
            for i, (w, a, lo, hi) in enumerate(R.tail_jobs(c)):
                if (c["name"], i) not in cache:
                    cache[(c["name"], i)] = _tail_outputs(w, a, lo, hi, None, R.tail_with_ring(i))
                if _differs(cache[(c["name"], i)], _tail_outputs(w, a, lo, hi, mut, R.tail_with_ring(i))):
                    caught[mut] = f"{c['name']} window base {w['seg_base']} range [{lo}, {hi})"
                    break
    print("\n".join(f"  {m:22s} {caught.get(m)}" for m in R.TAIL_MISTAKES))
    assert set(caught) == set(R.TAIL_MISTAKES), sorted(set(R.TAIL_MISTAKES) - set(caught))


def test_every_append_mistake_is_caught():
    caught = {}
    big_c, big_state, big_rounds = R.append_big_state()
    for mut in R.APPEND_MISTAKES:
        for c in R.append_cases():
            if mut in caught:
                break

            def on_round(job, res, mres, c=c, mut=mut):
                if mut not in caught and any(_differs(R.append_asserted(r), R.append_asserted(m)) for r, m in zip(res, mres)):
                    caught[mut] = f"{c['name']} round to frame {job['t_g1']}" + (" (closing)" if job["closing"] else "")
            R.append_chain(c, mut=mut, on_round=on_round)
    print("\n".join(f"  {m:22s} {caught.get(m)}" for m in R.APPEND_MISTAKES))
    assert set(caught) == set(R.APPEND_MISTAKES), sorted(set(R.APPEND_MISTAKES) - set(caught))
    # the clamp of the reflection decides no defined column, whatever the total
    rng = np.random.default_rng(3)
    for n in range(1, 402):
        x = rng.uniform(-1, 1, n).astype(np.float32)
        defined = 160 * (n // 160 - 1) + 400 if n >= 160 else 0
        i = np.arange(defined)
        assert np.array_equal(R.padded_cols(x, 0, n, i, True), R.padded_cols(x, 0, n, i, True, "no_clamp")), n
        assert n >= 101 or not np.array_equal(R.padded_cols(x, 0, n, np.arange(n + 400), True), R.padded_cols(x, 0, n, np.arange(n + 400), True, "no_clamp"))
    assert R.APPEND_MISTAKES_UNREAD == ("no_clamp",)
    # the far-out state composes like any other: its two rounds add the definition's samples behind A0
    state, total = big_state, [0] * big_c["S"]
    for rnd in big_rounds:
        job = R.append_job(big_c, rnd, state)
        res = [R.append_round(job, k) for k in range(big_c["S"])]
        assert all(r["A1"] > R.BIG and r["J1"] == (r["A1"] // 160 if rnd[4] else R.open_frames(r["A1"])) for r in res)
        assert all(np.isfinite(r["operand"]).all() for r in res)
        total = [t + r["n_new"] for t, r in zip(total, res)]
        state = R.append_next(job, res)
    assert all(t > 0 for t in total), total


def test_every_mel_and_ingest_mistake_is_caught():
    caught = {}
    rng = np.random.default_rng(5)
    for mut in R.MEL_MISTAKES:
        for c in R.mel_cases():
            for k in range(3):
                # (the float32 of the reference's own values for the case's spectra stands in for what the launch writes)
                mel = rng.uniform(-9.5, 1.5, (c["n_mels"], c["rows"])).astype(np.float32)
                nfr = min(c["n_new"][k], c["rows"])
                if nfr:
                    mel[:, :nfr] = R.mel_reference(R.mel_spectra(c["kinds"][k], nfr, c["seed"] + k), nfr, 0, nfr, c["n_mels"])[0]
                preset = {"reset": R.GMAX_NONE, "below": R.order_int(R.f32(-20.0)), "above": R.order_int(R.f32(30.0))}[c["presets"][k]]
                a = R.mel_side(mel, c["n_new"][k], c["rows"], c["J"][k], preset, c["hist"])
                b = R.mel_side(mel, c["n_new"][k], c["rows"], c["J"][k], preset, c["hist"], mut)
                if mut not in caught and (a[0] != b[0] or a[2] != b[2]):
                    caught[mut] = f"{c['name']} speaker {k}"
    for mut in R.INGEST_MISTAKES:
        for c in R.ingest_cases():
            src, plane_ld, dst, dst_ld = R.ingest_inputs(c)
            a = R.ingest(src, c["C"], c["n"], plane_ld, dst, c["dst_col"], dst_ld)
            b = R.ingest(src, c["C"], c["n"], plane_ld, dst, c["dst_col"], dst_ld, mut)
            if mut not in caught and (R.bits(a) != R.bits(b)).any():
                caught[mut] = c["name"]
    print("\n".join(f"  {m:22s} {caught.get(m)}" for m in R.MEL_MISTAKES + R.INGEST_MISTAKES))
    assert set(caught) == set(R.MEL_MISTAKES + R.INGEST_MISTAKES)


def test_ingest_and_scatter_cases_cover_the_issue():
    cs = R.ingest_cases()
    assert {c["C"] for c in cs} == {1, 2, 7, 8, 64} and {c["layout"] for c in cs} == {"interleaved", "planar", "planar_ld"}
    assert {c["dst_col"] for c in cs} == {0, 1, 2, 3}
    for C_ in (1, 2, 7, 8, 64):
        t = R.ingest_tile(C_)
        assert t % 64 == 0 and t * C_ * 2 <= 32768
        assert {c["n"] for c in cs if c["C"] == C_} >= {0, 1, 7, 8, 9, 63, 64, 65, t - 1, t, t + 1, 2 * t + 3}
    for c in cs:
        src, plane_ld, dst, dst_ld = R.ingest_inputs(c)
        got = R.ingest(src, c["C"], c["n"], plane_ld, dst, c["dst_col"], dst_ld)
        own = np.zeros(dst.size, bool)
        for ch in range(c["C"]):
            own[c["dst_col"] + ch * dst_ld:c["dst_col"] + ch * dst_ld + c["n"]] = True
        assert (R.bits(got)[~own] == R.CANARY).all() and np.isfinite(got[own]).all() and (np.abs(got[own]) <= 1).all()
        if c["n"] > 2:
            assert {-1.0, 32767 / 32768} <= set(got[own].tolist())
    assert {r for r, _ in R.SCATTER_TABLES} == set(R.SCATTER_ROWS) and {n for _, n in R.SCATTER_TABLES} == set(R.SCATTER_ENTRIES)
    es = [e for rows, n in R.SCATTER_TABLES for e in R.scatter_entries(n, rows)]
    assert {e["n_cols"] for e in es} == set(R.SCATTER_COLS) and {e["src_col"] % 4 for e in es} == {e["dst_off"] % 4 for e in es} == {0, 1, 2, 3}


def test_mel_reference_is_handoff_reference_without_the_product():
    """on spectra that ARE the float64 product rounded once, the reference lies within handoff_reference's own raw values by the
    rounding of the spectra, and the all-zero and subnormal spectra sit at the floor"""
    for n_mels in (80, 128):
        x = H.signal("chirp", 160 * 20 + 400, seed=1)
        spec = R.mel_spectra("chirp", 20, 1)
        raw, e_raw, floor = R.mel_reference(spec, 20, 0, 20, n_mels)
        fr = np.lib.stride_tricks.sliding_window_view(x.astype(np.float64), H.NFFT)[::H.HOPW][:20].T
        s = H.tables(n_mels)[0] @ fr
        want = np.log10(np.maximum(H.tables(n_mels)[1] @ (s[:201] ** 2 + s[201:] ** 2), H.FLOOR))
        assert np.abs(raw - want).max() < 1e-5 and (e_raw > 0).all() and e_raw.max() < 1e-3
        for kind in ("zeros", "subnormal"):
            raw, e_raw, floor = R.mel_reference(R.mel_spectra(kind, 5, 0), 5, 0, 5, n_mels)
            assert floor.all()
