"""The MVDR kernels of csrc/mvdr.hip at every microphone count, through css_mvdr_array_host (include/css_mi355_array.h), against
the extended-precision references and derived bounds of tests/array_reference.py.  As in
tests/test_hip_backend_kernels.py: outputs and 256 elements of slack behind them start as a canary and everything a launch does not
own keeps its bits; values are judged by error / bound <= 1 (the worst ratio of each test is printed); launches that must agree are
compared bit for bit.

  launch_scm             test_scm[C*_T65, C*_T186]: every C of {2, 3, 4, 5, 6, 8}; [C*_sweep_T*]: C = 2, 4, 8 at every edge of the
                         three tile forms and on the any-length kernel; the named shape details (odd F over two bins per block and
                         F = 1, S = 1 .. 3, seg_lo > 0, a short and an empty last segment, ties on audible planes, both override
                         forms, the pairs planes); test_scm_tuned_against_any_length (a child process with CSS_FORCE_LONG_PATH=1)
  C = 7                  test_seven_is_css_mvdr_host: forms 0 .. 3 bit for bit the entry of css_mi355_backend.h
  launch_mvdr_solve      test_solve[every family at C = 2, 4, 8], single launch, a segment alone, the multi launch of one set
  launch_mvdr_solve_multi  test_solve_multi[C]: sets of unequal length against their single launches
  launch_beamform        test_beamform[C]: use_mvdr 1 and 0, floor 0.05, T = 17 and 186
  refusals               test_refusals: C = 1, 9, S = 4, form 4, short arrays; the outputs keep their bits
Needs an MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import pkg
import array_reference as A
import backend_reference as R

pytestmark = pytest.mark.gpu

SLACK = 256


def _open():
    L = pkg("_lib")
    if L.load().css_device_count() < 1:
        pytest.fail("no HIP device visible")
    w = pkg("weights")
    desc = w.ModelDesc(num_blocks=1)
    return pkg("separator").HipSeparator(w.apply_golden_recipe(w.portable_state_dict(desc, 5)), None, device=0)


@pytest.fixture(scope="module")
def handle():
    sep = _open()
    yield sep.handle
    sep.close()


def _raw(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,))


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    diff = np.argwhere(_raw(a) != _raw(b))
    assert diff.size == 0, (what, f"{len(np.unique(diff[:, :-1], axis=0))} values differ, the first at {diff[0][:-1]}: "
                                  f"{a[tuple(diff[0][:-1])]!r} against {b[tuple(diff[0][:-1])]!r}")


def _kept(a, what):
    a = np.ascontiguousarray(a)
    want = {np.dtype(np.float32): R.canary(1), np.dtype(np.float64): R.canary64(1)}[a.dtype]
    stray = np.flatnonzero((_raw(a.reshape(-1)) != _raw(want)).any(axis=1))
    assert stray.size == 0, (what, f"{stray.size} elements the launch does not own were written, the first at {stray[0]}")


def _ratio(err, bound, what):
    err, bound = np.asarray(err, np.float64), np.broadcast_to(np.asarray(bound, np.float64), np.shape(err))
    r = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
    if r.size == 0:
        return 0.0
    worst = np.unravel_index(int(r.argmax()), r.shape)
    assert r[worst] <= 1.0, (what, f"ratio {r[worst]:.3f} at {worst}: error {err[worst]!r}, bound {bound[worst]!r}")
    return float(r[worst])


# ---- covariances ----------------------------------------------------------------------------------------------------------------

def _scm_launch(handle, c, arrays, seg_lo, nseg, what, entry="mvdr_array_host"):
    X, M, ov = arrays
    C, S, F = c["C"], c["S"], c["F"]
    segs, per = c["seg_lo"] + c["nseg"], (S + 1) * F * C * C
    out = getattr(handle, entry)(0, X=X, masks=M, override=ov, scm=R.canary64(segs * per + SLACK), C=C, F=F, S=S, T=c["T"], hop=c["hop"],
                                 nseg=nseg, seg_lo=seg_lo, stft_frames=c["stft_frames"], T_ld=c["T_ld"], mask_ld=c["mask_ld"])
    _kept(out[segs * per:], what + ": the slack")
    out = out[:segs * per].reshape(segs, S + 1, F, C * C)
    _kept(out[:seg_lo], what + ": segments before seg_lo")
    _kept(out[seg_lo + nseg:], what + ": segments from seg_lo + nseg on")
    return out[seg_lo:seg_lo + nseg]


def _check_scm(handle, c, long_path):
    arrays = A.scm_case_arrays(c)
    X, M, ov = arrays
    C = c["C"]
    got = _scm_launch(handle, c, arrays, c["seg_lo"], c["nseg"], c["name"])
    assert np.isfinite(got).all(), (c["name"], "a non-finite covariance: a NaN plane or mask column was read")
    worst = 0.0
    for i in range(c["nseg"]):
        seg = c["seg_lo"] + i
        phi, bound = A.scm(X, c["F"], c["stft_frames"], M, c["S"], c["T"], c["hop"], seg, ov, long_path)
        worst = max(worst, _ratio(np.abs(got[i].astype(R.LD) - phi), bound, f"{c['name']} segment {seg}"))
        if c["planes"] == "silent" or R.valid_frames(c["stft_frames"], seg, c["hop"], c["T"]) == 0:
            want = np.broadcast_to(np.where(np.arange(C * C) < C, R.DIAG, 0.0), got[i].shape)
            _same_bits(got[i], want, c["name"] + ": no signal gives 1e-15 on the diagonal and the word 0 elsewhere")
    if c["nseg"] >= 2:
        alone = _scm_launch(handle, c, arrays, c["seg_lo"] + 1, 1, c["name"] + " alone")
        _same_bits(alone[0], got[1], c["name"] + ": the second segment alone")
    return got, worst


@pytest.mark.parametrize("c", A.scm_cases(), ids=lambda c: c["name"])
def test_scm(handle, c):
    _, worst = _check_scm(handle, c, c["T"] > 512)
    print(f"covariances {c['name']} (C {c['C']} T {c['T']} S {c['S']} F {c['F']} hop {c['hop']} masks {c['masks']} planes {c['planes']} "
          f"override {c['override']}): worst error / bound {worst:.3f}")


def _forced_cases():
    return [c for c in A.scm_cases() if "_sweep_" in c["name"] and (c["C"], c["T"]) in A.SCM_FORCED]


def _forced_child(out_dir):
    """in a process started with CSS_FORCE_LONG_PATH=1: the cases through scm_long_kernel, held to its bound"""
    assert os.environ.get("CSS_FORCE_LONG_PATH") == "1"
    sep = _open()
    try:
        worst = 0.0
        for c in _forced_cases():
            got, r = _check_scm(sep.handle, c, True)
            worst = max(worst, r)
            np.save(os.path.join(out_dir, f"scm_{c['name']}.npy"), got)
        print(f"covariances (any-length kernel at tuned lengths): worst error / bound {worst:.3f}")
    finally:
        sep.close()


def test_scm_tuned_against_any_length(handle, tmp_path):
    cases = _forced_cases()
    assert sorted((c["C"], c["T"]) for c in cases) == sorted(A.SCM_FORCED)
    out_dir = str(tmp_path)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out_dir], env=dict(os.environ, CSS_FORCE_LONG_PATH="1"),
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    differ, total, worst = 0, 0, 0.0
    for c in cases:
        arrays = A.scm_case_arrays(c)
        X, M, ov = arrays
        long_ = np.load(os.path.join(out_dir, f"scm_{c['name']}.npy"))
        tuned = _scm_launch(handle, c, arrays, c["seg_lo"], c["nseg"], c["name"])
        for i in range(c["nseg"]):
            args = (X, c["F"], c["stft_frames"], M, c["S"], c["T"], c["hop"], c["seg_lo"] + i, ov)
            both = A.scm(*args, False)[1] + A.scm(*args, True)[1]
            worst = max(worst, _ratio(np.abs(tuned[i] - long_[i]), both, c["name"] + ": tuned against any-length, sum of bounds"))
        differ += int((R.bits64(tuned) != R.bits64(long_)).sum())
        total += tuned.size
    print(f"tuned against any-length covariance kernel: worst difference / sum of bounds {worst:.3f}; differing doubles: {differ} of {total}")


# ---- C = 7 through the new entry ------------------------------------------------------------------------------------------------

def test_seven_is_css_mvdr_host(handle):
    """forms 0 .. 3 at C = 7: css_mvdr_array_host makes the launches of css_mvdr_host"""
    both = lambda form, **kw: (handle.mvdr_array_host(form, **kw), handle.mvdr_host(form, **kw))
    for c in [c for c in R.scm_cases() if c["name"] in ("T65", "T186", "T193", "T257", "T513", "pairs_S3")]:
        c = dict(c, C=7)
        arrays = R.scm_case_arrays(c)
        a = _scm_launch(handle, c, arrays, c["seg_lo"], c["nseg"], c["name"])
        b = _scm_launch(handle, c, arrays, c["seg_lo"], c["nseg"], c["name"], entry="mvdr_host")
        _same_bits(a, b, c["name"] + ": covariances at C = 7")
    S, F = 3, 5
    scm = np.stack([R.covariances(fam, S, F, 900 + i, winners_n=3) for i, fam in enumerate(("well", "quiet_ref", "rank"))])
    kw = dict(scm=scm, bfw=R.canary64(3 * S * F * 14 + SLACK), C=7, F=F, S=S, T=64, hop=32)
    a, b = both(1, nseg=3, seg_lo=0, **kw)
    _same_bits(a, b, "solve at C = 7")
    a, b = both(2, sets=[(0, 2, 0, 0), (0, 1, 2 * (S + 1) * F * 49, 2 * S * F * 14)], **kw)
    _same_bits(a, b, "multi solve at C = 7")
    c = dict({c["name"]: c for c in R.scm_cases()}["T65"], C=7)
    X, M, _ = R.scm_case_arrays(c)
    segs = c["seg_lo"] + c["nseg"]
    rng = np.random.default_rng(3)
    W = rng.standard_normal((segs, c["S"], c["F"], 7, 2)) / 7
    for use in (1, 0):
        a, b = both(3, X=X, masks=M, bfw=W, sep=R.canary(segs * c["S"] * c["F"] * c["T"] * 2 + SLACK), C=7, F=c["F"], S=c["S"], T=c["T"],
                    hop=c["hop"], nseg=c["nseg"], seg_lo=c["seg_lo"], stft_frames=c["stft_frames"], T_ld=c["T_ld"], mask_ld=c["mask_ld"],
                    use_mvdr=use, mask_floor=0.05)
        _same_bits(a, b, f"beamformer at C = 7, use_mvdr {use}")


# ---- solve ----------------------------------------------------------------------------------------------------------------------

def _solve_launch(handle, scm, C, S, F, seg_lo, nseg, what):
    segs, per = scm.shape[0], S * F * 2 * C
    out = handle.mvdr_array_host(1, scm=scm, bfw=R.canary64(segs * per + SLACK), C=C, F=F, S=S, T=64, hop=32, nseg=nseg, seg_lo=seg_lo)
    _kept(out[segs * per:], what + ": the slack")
    out = out[:segs * per].reshape(segs, S, F, C, 2)
    _kept(out[:seg_lo], what + ": segments before seg_lo")
    _kept(out[seg_lo + nseg:], what + ": segments from seg_lo + nseg on")
    return out[seg_lo:seg_lo + nseg]


@pytest.mark.parametrize("c", A.solve_cases(), ids=lambda c: c["name"])
def test_solve(handle, c):
    C, S, F = c["C"], c["S"], c["F"]
    scm = A.solve_case_scm(c, 3)
    raw = _solve_launch(handle, scm, C, S, F, 0, 3, c["name"])
    assert np.isfinite(raw).all(), (c["name"], "a non-finite weight")
    worst, n_judged, n = 0.0, 0, 0
    for seg in range(3):
        W, bound = A.solve(scm[seg], S, F, C)
        j = A.judged(W, bound)
        if c["complete"]:
            assert j.all(), (c["name"], "a well-conditioned system is not judged")
        err = np.abs(R.bfw_complex(raw[seg]).astype(R.CLD) - W).astype(np.float64)
        worst = max(worst, _ratio(np.where(j[..., None], err, 0.0), bound, f"{c['name']} segment {seg}"))
        n_judged, n = n_judged + int(j.sum()), n + j.size
    _same_bits(_solve_launch(handle, scm, C, S, F, 2, 1, c["name"] + " alone")[0], raw[2], c["name"] + ": segment 2 alone")
    one = handle.mvdr_array_host(2, scm=scm, bfw=R.canary64(raw.size + SLACK), sets=[(0, 3, 0, 0)], C=C, F=F, S=S, T=64, hop=32)
    _same_bits(one[:raw.size].reshape(raw.shape), raw, c["name"] + ": the multi launch of one set")
    _kept(one[raw.size:], c["name"] + ": the slack of the multi launch")
    print(f"solve {c['name']} (C {C} S {S} F {F}): judged {n_judged} of {n} systems, worst error / bound {worst:.4f}")


@pytest.mark.parametrize("C", (2, 4, 8))
def test_solve_multi(handle, C):
    """nine sets of unequal length (more than one table: the batching loop runs twice) against the single launches"""
    S, F = (3, 2, 1)[C % 3], (5, 1)[C // 8]
    nsegs = (3, 1, 2, 1, 1, 2, 3, 1, 2)
    fams = ("well", "quiet_ref", "rank", "quiet_ref", "silent", "well", "rank", "well", "quiet_ref")
    per_w = S * F * 2 * C
    sets, blocks, singles, s_off, w_off = [], [], [], 0, 0
    for i, n in enumerate(nsegs):
        seg_lo = i % 2
        scm = np.stack([A.covariances(fams[i], C, S, F, 5000 + 100 * C + 10 * i + s, winners_n=max(C - 1, 1)) for s in range(seg_lo + n)])
        blocks.append(scm.reshape(-1))
        sets.append((seg_lo, n, s_off, w_off))
        singles.append((_solve_launch(handle, scm, C, S, F, seg_lo, n, f"set {i}"), w_off + seg_lo * per_w))
        s_off, w_off = s_off + scm.size + 7 * 8, w_off + (seg_lo + n) * per_w + 14
        blocks.append(R.canary64(7 * 8))
    out = handle.mvdr_array_host(2, scm=np.concatenate(blocks), bfw=R.canary64(w_off + SLACK), sets=sets, C=C, F=F, S=S, T=64, hop=32)
    owned = np.zeros(out.size, bool)
    for (raw, at) in singles:
        _same_bits(out[at:at + raw.size].reshape(raw.shape), raw, "a set of the multi launch against its single launch")
        owned[at:at + raw.size] = True
    _kept(out[~owned], "the multi launch: between and behind the sets")


# ---- beamformer -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", (2, 4, 8))
def test_beamform(handle, C):
    worst = 0.0
    for T in (17, 186):
        c = A.scm_case(f"beam_C{C}_T{T}", C, T, (3, 2, 1)[(C + T) % 3], (5, 2)[T % 2], 2, 1, -(-T // 2), 3, 1, "random", "gaussian", None, 6000 + C + T)
        X, M, _ = A.scm_case_arrays(c)
        S, F = c["S"], c["F"]
        segs, per = c["seg_lo"] + c["nseg"], S * F * T * 2
        rng = np.random.default_rng(c["seed"])
        W = (rng.standard_normal((segs, S, F, C)) + 1j * rng.standard_normal((segs, S, F, C))) / C
        for use in (1, 0):
            out = handle.mvdr_array_host(3, X=X, masks=M, bfw=np.stack([W.real, W.imag], axis=-1) if use else None, sep=R.canary(segs * per + SLACK),
                                         C=C, F=F, S=S, T=T, hop=c["hop"], nseg=c["nseg"], seg_lo=c["seg_lo"], stft_frames=c["stft_frames"],
                                         T_ld=c["T_ld"], mask_ld=c["mask_ld"], use_mvdr=use, mask_floor=0.05)
            _kept(out[segs * per:], c["name"] + ": the slack")
            got = out[:segs * per].reshape(segs, S, F, T, 2)
            _kept(got[:c["seg_lo"]], c["name"] + ": segments before seg_lo")
            assert np.isfinite(got[c["seg_lo"]:]).all(), (c["name"], "a NaN plane was read")
            for seg in range(c["seg_lo"], segs):
                args = (X, F, c["stft_frames"], M, S, T, c["hop"], seg, 0.05)
                if use:
                    ref, bound = A.beamform(*args, W[seg])
                    worst = max(worst, _ratio(np.abs(got[seg] - ref), bound, f"{c['name']} segment {seg}"))
                else:
                    _same_bits(got[seg], A.beamform_plain(*args), f"{c['name']} segment {seg}: x_0 max(mask, floor) in float32")
                tv = R.valid_frames(c["stft_frames"], seg, c["hop"], T)
                assert not R.bits(got[seg][:, :, tv:]).any(), (c["name"], "frames from tv on are not the word 0")
    print(f"beamformer (MVDR) at C = {C}: worst error / bound {worst:.3f}")


# ---- refusals -------------------------------------------------------------------------------------------------------------------

def test_refusals(handle):
    L = pkg("_lib")
    c = A.scm_case("r", 4, 17, 2, 2, 1, 0, 9, 0, 0, "random", "gaussian", None, 7000)
    X, M, _ = A.scm_case_arrays(c)
    good = dict(C=4, F=2, S=2, T=17, hop=9, nseg=1, seg_lo=0, stft_frames=c["stft_frames"], T_ld=c["T_ld"], mask_ld=c["mask_ld"])
    n_scm, n_bfw, n_sep = 3 * 2 * 16, 2 * 2 * 8, 2 * 2 * 17 * 2

    def refused(form, what, **kw):
        args = dict(good, **kw)
        scm, bfw, sep = args.pop("scm", R.canary64(n_scm)), args.pop("bfw", R.canary64(n_bfw)), args.pop("sep", R.canary(n_sep))
        Xa, Ma = args.pop("X", X), args.pop("masks", M)
        d = L.CssMvdrArrayDesc(form=form, x_floats=Xa.size, mask_floats=Ma.size, scm_doubles=scm.size, bfw_doubles=bfw.size, sep_floats=sep.size,
                               **{k: (float(v) if k == "mask_floor" else int(v)) for k, v in args.items()})
        p = lambda a: a.ctypes.data_as(L.C.c_void_p)
        rc = handle.lib.css_mvdr_array_host(handle.h, L.C.byref(d), p(Xa), p(Ma), None, p(scm), p(bfw), p(sep))
        assert rc == L.CSS_ERR_INVALID_ARG, (what, rc)
        assert b"css_mvdr_array_host" in handle.lib.css_last_error(handle.h), what
        for a in (scm, bfw, sep):
            _kept(a, what + ": an output was written")

    for form in (0, 1, 3):
        refused(form, f"form {form}: C = 1", C=1, use_mvdr=1)
        refused(form, f"form {form}: C = 9", C=9, use_mvdr=1)
        refused(form, f"form {form}: S = 4", S=4, use_mvdr=1)
    refused(3, "C = 1 without MVDR", C=1, use_mvdr=0)
    refused(4, "form 4 (the power normalisation is css_mvdr_host's)")
    refused(-1, "form -1")
    refused(0, "short scm", scm=R.canary64(n_scm - 1))
    refused(0, "short X", X=X.reshape(-1)[:-1])
    refused(0, "short masks", masks=M.reshape(-1)[:-1])
    refused(1, "short bfw", bfw=R.canary64(n_bfw - 1))
    refused(1, "short scm for the solve", scm=R.canary64(n_scm - 1))
    refused(3, "short sep", sep=R.canary(n_sep - 1), use_mvdr=1)
    refused(3, "short bfw for the beamformer", bfw=R.canary64(n_bfw - 1), use_mvdr=1)
    # and the good descriptor is taken
    out = handle.mvdr_array_host(0, X=X, masks=M, scm=R.canary64(n_scm), **good)
    assert np.isfinite(out).all()


if __name__ == "__main__":      # the child of test_scm_tuned_against_any_length
    _forced_child(sys.argv[1])
