"""tests/rate_reference.py on the CPU, on the cases tests/test_hip_rate_kernels.py gives the kernels:
  (a) the reference IS scipy.signal.resample_poly: same length, values to 1e-13 of max |y|, every ratio, n = 1, 2, 31, 1000, 4099
      (the index algebra is pinned to scipy's code, not to a restatement of the kernel's);
  (b) a job with history is the matching slice of the whole recording, and the sum as the kernels index it (rate_reference.chain)
      is the same sum;
  (c) the bound is reachable: a float32 model of the fmaf chain stays inside it on every case (the worst ratio per ratio is printed);
  (d) the bound is not vacuous: every named mistake exceeds it (PCM16: changes an int16 or the clip count) on a named case.
The first two tests pin include/css_mi355_rate_kernels.h against the library and its binding.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rate_reference as R
from conftest import ROOT, pkg

CSRC = os.path.join(ROOT, "notsofar1-challenge_amd", "csrc")
HEADER = "css_mi355_rate_kernels.h"
NAMES = ("css_rate_ingest_host", "css_rate_output_host")
DESCS = ("CssRateIngestJob", "CssRateOutputJob")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)


def test_header_library_and_binding_agree():
    L = pkg("_lib")
    lib = L.load()
    text = _header()
    assert '#include "css_mi355.h"' in text
    declared = re.findall(r"\bint\s+(css_\w+)\s*\(", text)
    assert sorted(declared) == sorted(NAMES) == sorted(L.RATE_KERNEL_BINDINGS)
    tables = {n: getattr(L, n) for n in dir(L) if n.startswith("SIGNATURES") or n.endswith("_SIGNATURES") or n.endswith("_BINDINGS")}
    assert len(tables) == 17
    for n, t in tables.items():
        assert n == "RATE_KERNEL_BINDINGS" or not set(L.RATE_KERNEL_BINDINGS) & set(t), n
    for f in os.listdir(os.path.join(ROOT, "include")):
        if f != HEADER:
            other = open(os.path.join(ROOT, "include", f)).read()
            for name in NAMES + DESCS:
                assert not re.search(rf"\b{name}\b", other), f"{name} belongs to {HEADER} alone"
    for name in NAMES:
        params = re.search(rf"\b{name}\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")
        restype, argtypes = L.RATE_KERNEL_BINDINGS[name]
        fn = getattr(lib, name)   # (AttributeError: the library does not export it)
        assert restype is C.c_int and len(argtypes) == len(params), name
        assert fn.restype is C.c_int and list(fn.argtypes) == list(argtypes)       # load() applied the fifteenth of its sixteen tables
    kinds = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "float": C.c_float}
    for desc in DESCS:   # the header's fields in the header's order, with the header's types; every pointer is a void pointer
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
    assert C.sizeof(L.CssRateIngestJob) == 40 + 10 * 8 + 4 * 8 and L.CssRateIngestJob.plane_ld.offset == 40
    assert C.sizeof(L.CssRateOutputJob) == 32 + 9 * 8 + 6 * 8 and L.CssRateOutputJob.src_ld.offset == 32
    assert int(re.search(r"#define CSS_RATE_KERNEL_JOBS (\d+)", text).group(1)) == L.RATE_KERNEL_JOBS >= 17
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "api_rate_kernels.hip" in re.search(r"^SRCS\s*:=(.*)$", mk, flags=re.M).group(1).split()
    assert re.search(rf"^build/api_rate_kernels\.o build_asan/api_rate_kernels\.o:.*include/{HEADER}", mk, flags=re.M)


def test_null_handle_and_null_table_are_refused():
    L = pkg("_lib")
    lib = L.load()
    dst = np.full(64, 7.0, np.float32)
    ji, jo = (L.CssRateIngestJob * 1)(), (L.CssRateOutputJob * 1)()
    ji[0].dst = jo[0].dst = dst.ctypes.data
    ji[0].dst_floats = jo[0].dst_elems = 64
    for form in (0, 1):
        assert lib.css_rate_ingest_host(None, form, ji, 1) == L.CSS_ERR_INVALID_ARG
        assert lib.css_rate_output_host(None, form, 1, jo, 1) == L.CSS_ERR_INVALID_ARG
        assert lib.css_rate_ingest_host(None, form, None, 0) == L.CSS_ERR_INVALID_ARG
        assert lib.css_rate_output_host(None, form, 0, None, 0) == L.CSS_ERR_INVALID_ARG
    assert (dst == 7.0).all()


# ---- (a) scipy ----------------------------------------------------------------------------------------------------------------------

def test_taps64_are_the_float64_of_the_library_taps():
    for up, down in R.RATIOS:
        h64, h32 = R.taps64(up, down), R.taps32(up, down)
        assert h64.shape == h32.shape == (R.geometry(up, down)[1],)
        assert np.all(np.abs(h64 - h32.astype(np.float64)) <= np.spacing(np.abs(h32)).astype(np.float64)), (up, down)


@pytest.mark.parametrize("ratio", R.RATIOS, ids=lambda r: f"{r[0]}_{r[1]}")
def test_reference_is_resample_poly(ratio):
    from scipy.signal import resample_poly
    up, down = ratio
    h64 = R.taps64(up, down)
    worst = 0.0
    for n in (1, 2, 31, 1000, 4099):
        x = np.random.RandomState(n).uniform(-1.0, 1.0, (2, n))
        y, _ = R.recording(x, up, down, taps=h64)
        ref = resample_poly(x, up, down, axis=1, window=h64 / up)
        assert y.shape == ref.shape == (2, -(-n * up // down)), (ratio, n)
        err = float(np.max(np.abs(y - ref))) / float(np.max(np.abs(ref)))
        worst = max(worst, err)
        assert err <= 1e-13, (ratio, n, err)
    print(f"{up}/{down}: reference against resample_poly, worst {worst:.2g} of max |y|")


# ---- (b) one definition -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ratio", R.RATIOS, ids=lambda r: f"{r[0]}_{r[1]}")
def test_jobs_are_slices_of_the_recording(ratio):
    """hist and piece cut from a recording: the job's outputs and bounds are the recording's, exactly (same terms, same order);
    the carried history is next_history of the round before; the pieces' outputs tile [0, count) without gap or overlap"""
    up, down = ratio
    for dtype in (np.float32, np.int16):
        n_in = R.job_recording_len(up, down)
        whole = R.samples(2, n_in, dtype, 7)
        y, b = R.recording(whole, up, down)
        H = R.history_len(up, down)
        hist = np.zeros((2, H), np.float32)
        at = 0
        for N0, n, m0, n_m, H_, flush in R.stream_jobs(up, down, n_in):
            assert m0 == at and H_ == H
            piece = whole[:, N0:N0 + n]
            assert np.array_equal(hist, R.history_of(whole, N0, H))
            yj, bj = R.reference(piece, hist, N0, m0, n_m, up, down)
            assert np.array_equal(yj, y[:, m0:m0 + n_m]) and np.array_equal(bj, b[:, m0:m0 + n_m]), (ratio, N0)
            cj = R.chain(piece, hist, N0, m0, n_m, up, down)
            assert np.all(np.abs(cj - yj) <= 1e-15 * np.maximum(bj * 2.0 ** 24, 1e-300)), (ratio, N0)
            hist = R.next_history(hist, piece)
            at += n_m
        assert at == y.shape[1] == R.count(up, down, n_in)
        # a history shorter than the filter's reach is NOT the recording: the definition's zeros take the place of the lost inputs
        N0, n = R.PIECES[0] + R.PIECES[1] + 300, 40
        m0 = R.count(up, down, N0, finished=False)
        n_m = R.count(up, down, N0 + n, finished=False) - m0
        short, _ = R.reference(whole[:, N0:N0 + n], R.history_of(whole, N0, 2), N0, m0, n_m, up, down)
        assert n_m > 0 and not np.array_equal(short, y[:, m0:m0 + n_m])


# ---- (c) the bound is reachable -------------------------------------------------------------------------------------------------------

def test_float32_chain_is_inside_the_bound():
    worst = {}
    for c in R.cases():
        piece, hist = R.case_data(c)
        y, b = R.reference(piece, hist, c.N0, c.m0, c.n_m, c.up, c.down)
        m32 = R.chain(piece, hist, c.N0, c.m0, c.n_m, c.up, c.down, model32=True)
        assert m32.dtype == np.float32 and m32.shape == y.shape == (c.C, c.n_m)
        err = np.abs(m32.astype(np.float64) - y)
        assert np.all(err <= b), (c.name, float(np.max(err / np.maximum(b, 1e-300))))
        assert np.all(R.bits(m32)[b == 0] == 0), c.name       # silence is +0.0f
        r = float(np.max(np.where(err == 0, 0.0, err / np.maximum(b, 1e-300)))) if err.size else 0.0
        worst[(c.up, c.down)] = max(worst.get((c.up, c.down), 0.0), r)
    for (up, down), r in worst.items():
        print(f"{up}/{down}: float32 chain, worst error / bound {r:.3f}")
    assert set(worst) == set(R.RATIOS)


# ---- (d) the bound is not vacuous -----------------------------------------------------------------------------------------------------

def test_every_named_mistake_is_caught():
    caught = {}
    data = [(c, R.case_data(c)) for c in R.cases()]
    refs = [R.reference(p, h, c.N0, c.m0, c.n_m, c.up, c.down) for c, (p, h) in data]
    for name in R.MISTAKES:
        for (c, (piece, hist)), (y, b) in zip(data, refs):
            if c.n_m == 0:
                continue
            wrong = R.chain(piece, hist, c.N0, c.m0, c.n_m, c.up, c.down, mistake=name)
            over = np.abs(wrong - y) > b
            if over.any():
                caught[name] = (c.name, int(np.count_nonzero(over)), over.size)
                break
    for name, (case, k, n) in caught.items():
        print(f"{name}: caught by [{case}], {k} of {n} outputs outside the bound")
    assert sorted(caught) == sorted(R.MISTAKES), sorted(set(R.MISTAKES) - set(caught))


def test_every_pcm16_mistake_is_caught():
    planted = R.pcm_planted()
    q, clips = R.pcm16(planted, 1.0)
    assert list(q[:4]) == [16384, -16384, 32767, -32767] and not np.any(np.abs(q.astype(np.int32)) == R.CANARY16)
    # the clamp changes the four values beyond +-1.0001 and the first float32 past +32767.5 / 32767 (-> 32768); its mirror image
    # gives -32768, which is in range
    assert clips == 5 and list(q[4:10]) == [32767, 32767, 32767, -32767, -32767, -32768]
    L = pkg("_lib")
    caught = {}
    for what, gain in R.PCM_CASES:
        y = R.pcm_samples(gain)
        q, clips = R.pcm16(y, gain)
        assert np.array_equal(q, L.pcm16_encode(y, gain)[0]) and clips == L.pcm16_encode(y, gain)[1]
        for name, fn in R.PCM_SAME_AS_RINT.items():      # (rate_reference.py says why no sample can show this one)
            wq, wc = fn(y, gain)
            assert np.array_equal(wq, q) and wc == clips, name
        for name, fn in R.PCM_MISTAKES.items():
            wq, wc = fn(y, gain)
            if name not in caught and (not np.array_equal(wq, q) or wc != clips):
                caught[name] = (what, int(np.count_nonzero(wq != q)), wc - clips)
    for name, (what, k, dc) in caught.items():
        print(f"{name}: caught at {what}, {k} samples differ, clip count off by {dc}")
    assert sorted(caught) == sorted(R.PCM_MISTAKES)
