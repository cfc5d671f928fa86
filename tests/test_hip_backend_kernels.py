"""Every launch form the paths make from csrc/mvdr.hip and csrc/stitch.hip, through the host entries of
include/css_mi355_backend.h, against the extended-precision references, derived bounds and exact models of
tests/backend_reference.py.  Three kinds of assertion per launch:

  ownership  outputs and 256 elements of slack behind them start as a canary (0x7FC0BEEF for floats, a NaN pattern for doubles,
             0xA5 for bytes, a negative word for the permutations); everything the launch does not own keeps its bits: segments
             outside [seg_lo, seg_lo + nseg), boundaries outside the range, frames outside [t_lo, t_hi), act_tmp outside the
             dilated range, the slack.  Planes at and past stft_frames and the mask columns of other segments are NaN.
  value      elementwise inside the bound (covariances, solve, MVDR beamformer, power normalisation, costs), bit for bit for the
             kernels that round nowhere or in a stated order (plain beamformer, scan, both overlap-adds, activity, gate); the
             worst ratio of each test is printed
  bits       where two launches must agree: a sub-range against the whole range, a multi launch against the single launches, a
             segment alone against the same segment among three, a scan in two calls against one.  The tuned covariance kernels
             against the any-length one are held to the sum of their bounds; the count of differing doubles is printed.

Coverage (every launch function of mvdr.hip and stitch.hip, every template instantiation):
  launch_scm
    scm_kernel<4, 192>             test_scm[T1 .. T192, pairs_S1 .. S3]
    scm_kernel<4>                  test_scm[T193, T255, T256, T193_tied, T255_all_equal_index, T256_tied_bits_full]
    scm_kernel<8>                  test_scm[T257, T320, T511, T512, T320_ulp_short]
    scm_long_kernel                test_scm[T513, T600, T513_tied_3seg, T600_all_equal], and at T = 17, 186, 257 in a child process started with
                                   CSS_FORCE_LONG_PATH=1 (test_scm_any_length_at_tuned_lengths)
  launch_mvdr_solve                test_solve[every family]
  launch_mvdr_solve_multi          test_solve_multi (3 sets with nseg 3, 1, 2; 9 sets: two launches of mvdr_solve_multi_kernel)
  launch_beamform                  test_beamform_plain (use_mvdr 0), test_beamform_mvdr (use_mvdr 1)
  launch_segment_power_norm        test_power_norm (segment_energy_kernel, segment_scale_kernel)
  launch_pit_costs                 test_pit_costs[every case] (pit_cost_kernel, pit_cost_final_kernel)
  launch_pit_costs_multi           test_pit_costs_multi (num_segments 4, 1, 2; 9 sessions: two launches of each multi kernel)
  launch_pit_scan                  test_pit_scan[S], test_pit_scan_resume
  launch_ola_masks                 test_overlap_add[class2 ..] ola_masks_kernel<2>, [class4 ..] <4>, [class0 ..] <0>
  launch_ola_stft                  the same cases: ola_stft_kernel<2>, <4>, <0>, float32 and split rows
  launch_morphology                test_morphology (morph_kernel, dilation and erosion)
Needs an MI355X."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import pkg      # (first: it puts the oracle on the path, also for the child process below)
import backend_reference as R
import css_oracle as O

pytestmark = pytest.mark.gpu

SLACK = 256                  # elements of slack behind every output
PERM_CANARY = -0x41104111    # a word no permutation holds


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
    """every element still holds the canary of its type"""
    a = np.ascontiguousarray(a)
    want = {np.dtype(np.float32): R.canary(1), np.dtype(np.float64): R.canary64(1), np.dtype(np.uint8): R.canary8(1),
            np.dtype(np.int32): np.array([PERM_CANARY], np.int32)}[a.dtype]
    stray = np.flatnonzero((_raw(a.reshape(-1)) != _raw(want)).any(axis=1))
    assert stray.size == 0, (what, f"{stray.size} elements the launch does not own were written, the first at {stray[0]}")


def _ratio(err, bound, what):
    """the worst err / bound; a zero bound asks for a zero error"""
    err, bound = np.asarray(err, np.float64), np.broadcast_to(np.asarray(bound, np.float64), np.shape(err))
    r = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
    if r.size == 0:
        return 0.0
    worst = np.unravel_index(int(r.argmax()), r.shape)
    assert r[worst] <= 1.0, (what, f"ratio {r[worst]:.3f} at {worst}: error {err[worst]!r}, bound {bound[worst]!r}")
    return float(r[worst])


# ---- covariances ----------------------------------------------------------------------------------------------------------------

def _scm_launch(handle, c, arrays, seg_lo, nseg, what):
    """one launch over segments [seg_lo, seg_lo + nseg) of the case; returns their covariances [nseg][S + 1][F][49] after the
    ownership checks"""
    X, M, ov = arrays
    S, F = c["S"], c["F"]
    segs, per = c["seg_lo"] + c["nseg"], (S + 1) * F * R.NPACK
    out = handle.mvdr_host(0, X=X, masks=M, override=ov, scm=R.canary64(segs * per + SLACK), C=7, F=F, S=S, T=c["T"], hop=c["hop"],
                           nseg=nseg, seg_lo=seg_lo, stft_frames=c["stft_frames"], T_ld=c["T_ld"], mask_ld=c["mask_ld"])
    _kept(out[segs * per:], what + ": the slack")
    out = out[:segs * per].reshape(segs, S + 1, F, R.NPACK)
    _kept(out[:seg_lo], what + ": segments before seg_lo")
    _kept(out[seg_lo + nseg:], what + ": segments from seg_lo + nseg on")
    return out[seg_lo:seg_lo + nseg]


def _check_scm(handle, c, long_path):
    """the whole launch of a case against the reference; returns (covariances, worst ratio)"""
    arrays = R.scm_case_arrays(c)
    X, M, ov = arrays
    got = _scm_launch(handle, c, arrays, c["seg_lo"], c["nseg"], c["name"])
    assert np.isfinite(got).all(), (c["name"], "a non-finite covariance: a NaN plane or mask column was read")
    worst = 0.0
    for i in range(c["nseg"]):
        phi, bound = R.scm(X, c["F"], c["stft_frames"], M, c["S"], c["T"], c["hop"], c["seg_lo"] + i, ov, long_path)
        worst = max(worst, _ratio(np.abs(got[i].astype(R.LD) - phi), bound, f"{c['name']} segment {c['seg_lo'] + i}"))
        if c["planes"] == "silent":
            want = np.broadcast_to(np.where(np.arange(R.NPACK) < R.NC, R.DIAG, 0.0), got[i].shape)
            _same_bits(got[i], want, c["name"] + ": silent planes give 1e-15 on the diagonal and the word 0 elsewhere")
    if c["nseg"] == 3:
        alone = _scm_launch(handle, c, arrays, c["seg_lo"] + 1, 1, c["name"] + " alone")
        _same_bits(alone[0], got[1], c["name"] + ": the middle segment alone")
    return got, worst


@pytest.mark.parametrize("c", R.scm_cases(), ids=lambda c: c["name"])
def test_scm(handle, c):
    _, worst = _check_scm(handle, c, c["T"] > 512)
    print(f"covariances {c['name']} (S {c['S']} F {c['F']} hop {c['hop']} masks {c['masks']} planes {c['planes']} override "
          f"{c['override']}): worst error / bound {worst:.3f}")


def _forced_cases():
    return [c for c in R.scm_cases() if c["T"] in R.SCM_FORCED_T]


def _forced_child(out_dir):
    """in a process started with CSS_FORCE_LONG_PATH=1: the cases at the tuned lengths through scm_long_kernel, held to its
    bound; the covariances are left in out_dir for the parent"""
    assert os.environ.get("CSS_FORCE_LONG_PATH") == "1"
    sep = _open()
    try:
        worst = 0.0
        for c in _forced_cases():
            got, r = _check_scm(sep.handle, c, True)
            worst = max(worst, r)
            np.save(os.path.join(out_dir, f"scm_{c['name']}.npy"), got)
        print(f"covariances (any-length kernel at T {R.SCM_FORCED_T}): worst error / bound {worst:.3f}")
    finally:
        sep.close()


def test_scm_any_length_at_tuned_lengths(handle, tmp_path):
    out_dir = str(tmp_path)
    env = dict(os.environ, CSS_FORCE_LONG_PATH="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out_dir], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    differ, total, worst = 0, 0, 0.0
    for c in _forced_cases():
        arrays = R.scm_case_arrays(c)
        X, M, ov = arrays
        long_ = np.load(os.path.join(out_dir, f"scm_{c['name']}.npy"))
        tuned = _scm_launch(handle, c, arrays, c["seg_lo"], c["nseg"], c["name"])
        for i in range(c["nseg"]):
            args = (X, c["F"], c["stft_frames"], M, c["S"], c["T"], c["hop"], c["seg_lo"] + i, ov)
            both = R.scm(*args, False)[1] + R.scm(*args, True)[1]
            worst = max(worst, _ratio(np.abs(tuned[i] - long_[i]), both, c["name"] + ": tuned against any-length, sum of bounds"))
        differ += int((R.bits64(tuned) != R.bits64(long_)).sum())
        total += tuned.size
    print(f"tuned against any-length covariance kernel: worst difference / sum of bounds {worst:.3f}; differing doubles: {differ} of {total}")


# ---- solve ----------------------------------------------------------------------------------------------------------------------

def _solve_launch(handle, scm, S, F, seg_lo, nseg, what):
    """form 1 on the covariances scm [segs][S + 1][F][49]; returns W [nseg][S][F][7] complex128 after the ownership checks"""
    segs, per = scm.shape[0], S * F * 14
    out = handle.mvdr_host(1, scm=scm, bfw=R.canary64(segs * per + SLACK), C=7, F=F, S=S, T=64, hop=32, nseg=nseg, seg_lo=seg_lo)
    _kept(out[segs * per:], what + ": the slack")
    out = out[:segs * per].reshape(segs, S, F, R.NC, 2)
    _kept(out[:seg_lo], what + ": segments before seg_lo")
    _kept(out[seg_lo + nseg:], what + ": segments from seg_lo + nseg on")
    return out[seg_lo:seg_lo + nseg]


@pytest.mark.parametrize("c", R.solve_cases(), ids=lambda c: c["name"])
def test_solve(handle, c):
    S, F = c["S"], c["F"]
    scm = R.solve_case_scm(c, 3)
    raw = _solve_launch(handle, scm, S, F, 0, 3, c["name"])
    assert np.isfinite(raw).all(), (c["name"], "a non-finite weight")
    worst, n_judged, n = 0.0, 0, 0
    for seg in range(3):
        W, bound = R.solve(scm[seg], S, F)
        j = R.judged(W, bound)
        if c["complete"]:
            assert j.all(), (c["name"], "a well-conditioned system is not judged")
        err = np.abs(R.bfw_complex(raw[seg]).astype(R.CLD) - W).astype(np.float64)
        worst = max(worst, _ratio(np.where(j[..., None], err, 0.0), bound, f"{c['name']} segment {seg}"))
        n_judged, n = n_judged + int(j.sum()), n + j.size
    _same_bits(_solve_launch(handle, scm, S, F, 2, 1, c["name"] + " alone")[0], raw[2], c["name"] + ": segment 2 alone")
    one = handle.mvdr_host(2, scm=scm, bfw=R.canary64(raw.size + SLACK), sets=[(0, 3, 0, 0)], C=7, F=F, S=S, T=64, hop=32)
    _same_bits(one[:raw.size].reshape(raw.shape), raw, c["name"] + ": the multi launch of one set")
    _kept(one[raw.size:], c["name"] + ": the slack of the multi launch")
    print(f"solve {c['name']} (S {S} F {F}): judged {n_judged} of {n} systems, worst error / bound {worst:.4f}")


@pytest.mark.parametrize("nsegs", ((3, 1, 2), (3, 1, 2, 1, 1, 2, 3, 1, 2)), ids=("3_sets", "9_sets"))
def test_solve_multi(handle, nsegs):
    """sets of unequal length (more than MVDR_MULTI_MAX of them: the batching loop runs twice) against the single launches"""
    S, F = 2, 5
    fams = ("well", "pivot", "rank", "quiet_ref", "silent", "well", "rank", "well", "quiet_ref")
    per_s, per_w = (S + 1) * F * R.NPACK, S * F * 14
    sets, blocks, singles, s_off, w_off = [], [], [], 0, 0
    for i, n in enumerate(nsegs):
        seg_lo = i % 2                     # a set may start behind its first segment
        scm = np.stack([R.covariances(fams[i], S, F, 800 + 10 * i + s, winners_n=3) for s in range(seg_lo + n)])
        blocks.append(scm.reshape(-1))
        sets.append((seg_lo, n, s_off, w_off))
        singles.append((_solve_launch(handle, scm, S, F, seg_lo, n, f"set {i}"), w_off + seg_lo * per_w))
        s_off, w_off = s_off + scm.size + 7 * 8, w_off + (seg_lo + n) * per_w + 14      # gaps between the sets
        blocks.append(R.canary64(7 * 8))
    out = handle.mvdr_host(2, scm=np.concatenate(blocks), bfw=R.canary64(w_off + SLACK), sets=sets, C=7, F=F, S=S, T=64, hop=32)
    owned = np.zeros(out.size, bool)
    for (raw, at) in singles:
        _same_bits(out[at:at + raw.size].reshape(raw.shape), raw, "a set of the multi launch against its single launch")
        owned[at:at + raw.size] = True
    _kept(out[~owned], "the multi launch: between and behind the sets")


# ---- beamformer and power normalisation -------------------------------------------------------------------------------------------

BEAM_CASES = ("T16", "T63", "T64", "T65", "T128", "T191", "T513_tied_3seg")   # (T16: no valid frame; T63: silent microphone 0)


def _beam_inputs(name):
    c = {c["name"]: c for c in R.scm_cases()}[name]
    X, M, _ = R.scm_case_arrays(c)
    rng = np.random.default_rng(c["seed"])
    segs = c["seg_lo"] + c["nseg"]
    W = (rng.standard_normal((segs, c["S"], c["F"], R.NC)) + 1j * rng.standard_normal((segs, c["S"], c["F"], R.NC))) / 7
    return c, X, M, W


def _beam_launch(handle, c, X, M, W, floor, what):
    S, F, T = c["S"], c["F"], c["T"]
    segs, per = c["seg_lo"] + c["nseg"], S * F * T * 2
    bfw = None if W is None else np.stack([W.real, W.imag], axis=-1)
    out = handle.mvdr_host(3, X=X, masks=M, bfw=bfw, sep=R.canary(segs * per + SLACK), C=7, F=F, S=S, T=T, hop=c["hop"], nseg=c["nseg"],
                           seg_lo=c["seg_lo"], stft_frames=c["stft_frames"], T_ld=c["T_ld"], mask_ld=c["mask_ld"],
                           use_mvdr=int(W is not None), mask_floor=floor)
    _kept(out[segs * per:], what + ": the slack")
    out = out[:segs * per].reshape(segs, S, F, T, 2)
    _kept(out[:c["seg_lo"]], what + ": segments before seg_lo")
    return out[c["seg_lo"]:]


def test_beamform_plain(handle):
    for i, floor in itertools.product(BEAM_CASES, (0.0, 0.05, 0.3)):
        c, X, M, _ = _beam_inputs(i)
        got = _beam_launch(handle, c, X, M, None, floor, c["name"])
        for k in range(c["nseg"]):
            seg = c["seg_lo"] + k
            _same_bits(got[k], R.beamform_plain(X, c["F"], c["stft_frames"], M, c["S"], c["T"], c["hop"], seg, floor),
                       f"{c['name']} floor {floor} segment {seg}: x_0 max(mask, floor) in float32")
            tv = R.valid_frames(c["stft_frames"], seg, c["hop"], c["T"])
            assert not R.bits(got[k][:, :, tv:]).any(), (c["name"], "frames from tv on are not the word 0")


def _beam_mvdr(handle):
    """the worst error / bound over the MVDR cases"""
    worst = 0.0
    for i in BEAM_CASES:
        c, X, M, W = _beam_inputs(i)
        got = _beam_launch(handle, c, X, M, W, 0.05, c["name"])
        assert np.isfinite(got).all(), (c["name"], "a NaN plane was read")
        for k in range(c["nseg"]):
            seg = c["seg_lo"] + k
            ref, bound = R.beamform(X, c["F"], c["stft_frames"], M, c["S"], c["T"], c["hop"], seg, 0.05, W[seg])
            err = np.abs(got[k] - ref)
            worst = max(worst, float(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300)).max()))
            tv = R.valid_frames(c["stft_frames"], seg, c["hop"], c["T"])
            assert not R.bits(got[k][:, :, tv:]).any(), (c["name"], "frames from tv on are not the word 0")
    return worst


def test_beamform_mvdr(handle):
    """use_mvdr = 1 inside (14 u sum |W| |x| + U/2 |y|) m + U/2 |y m|: the float64 product y m rounded to float32 once"""
    r = _beam_mvdr(handle)
    print(f"beamformer (MVDR): worst error / bound {r:.3f}")
    assert r <= 1.0, r


def test_power_norm(handle):
    worst, judged, undefined = 0.0, 0, 0
    for i in BEAM_CASES:
        c, X, M, _ = _beam_inputs(i)
        S, F, T = c["S"], c["F"], c["T"]
        segs, per = c["seg_lo"] + c["nseg"], S * F * T * 2
        sep = R.canary(segs * per + SLACK)
        body = sep[:segs * per].reshape(segs, S, F, T, 2)
        for seg in range(c["seg_lo"], segs):
            body[seg] = R.beamform_plain(X, F, c["stft_frames"], M, S, T, c["hop"], seg, 0.05)
        out = handle.mvdr_host(4, X=X, sep=sep, C=7, F=F, S=S, T=T, hop=c["hop"], nseg=c["nseg"], seg_lo=c["seg_lo"],
                               stft_frames=c["stft_frames"], T_ld=c["T_ld"])
        _kept(out[segs * per:], c["name"] + ": the slack")
        got = out[:segs * per].reshape(segs, S, F, T, 2)
        _kept(got[:c["seg_lo"]], c["name"] + ": segments before seg_lo")
        for seg in range(c["seg_lo"], segs):
            ref, bound, g = R.power_norm(X, F, c["stft_frames"], body[seg], S, T, c["hop"], seg)
            if not np.isfinite(g):          # no valid frame, or silence: 0 / 0 in the reference's own formula (kernels.hpp)
                assert np.isnan(got[seg]).all(), (c["name"], seg, "a segment whose gain is 0 / 0 is not NaN throughout")
                undefined += 1
                continue
            worst = max(worst, _ratio(np.abs(got[seg] - ref), bound, f"{c['name']} segment {seg}"))
            judged += 1
    assert judged >= 10 and undefined >= 2, (judged, undefined)
    print(f"power normalisation: {judged} segments judged, worst error / bound {worst:.3f}; {undefined} segments with the gain 0 / 0 are NaN")


# ---- stitching costs ------------------------------------------------------------------------------------------------------------

def _costs_launch(handle, c, masks, sep, num_segments, lo, hi, what):
    S = c["S"]
    n = (num_segments - 1) * S * S
    out = handle.stitch_host(0, masks=masks if c["input"] == 0 else None, sep=sep if c["input"] == 1 else None,
                             costs=R.canary64(n + SLACK), S=S, F=c["F"], T=c["T"], hop=c["hop"], loss=c["loss"], input=c["input"],
                             num_segments=num_segments, mask_ld=masks.shape[1], lo=lo, hi=hi)
    _kept(out[n:], what + ": the slack")
    out = out[:n].reshape(num_segments - 1, S, S)
    _kept(out[:lo], what + ": boundaries before the range")
    _kept(out[hi:], what + ": boundaries behind the range")
    return out[lo:hi]


@pytest.mark.parametrize("c", R.pit_cases(), ids=lambda c: c["name"])
def test_pit_costs(handle, c):
    S, F, T, hop = c["S"], c["F"], c["T"], c["hop"]
    masks, sep = R.pit_inputs(S, F, T, 4, c["seed"], mask_ld=4 * T + (0, 3)[c["seed"] % 2])
    got = _costs_launch(handle, c, masks, sep, 4, 0, 3, c["name"])
    worst = 0.0
    for b in range(3):
        cost, bound = R.pit_costs(masks, sep, S, F, T, hop, b, c["loss"], c["input"])
        worst = max(worst, _ratio(np.abs(got[b].astype(R.LD) - cost), bound, f"{c['name']} boundary {b}"))
    for lo, hi in R.PIT_RANGES[1:]:
        _same_bits(_costs_launch(handle, c, masks, sep, 4, lo, hi, f"{c['name']} [{lo}, {hi})"), got[lo:hi],
                   f"{c['name']}: boundaries [{lo}, {hi}) against the whole range")
    print(f"costs {c['name']} (S {S} loss {c['loss']} input {c['input']}): worst error / bound {worst:.3f}")


@pytest.mark.parametrize("inp", (0, 1))
@pytest.mark.parametrize("counts", ((4, 1, 2), (4, 1, 2, 3, 1, 2, 2, 4, 3)), ids=("3_sessions", "9_sessions"))
def test_pit_costs_multi(handle, counts, inp):
    """sessions of unequal length, one with a single segment (no boundary), more than PIT_MULTI_MAX of them"""
    S, F, T, hop = 3, 5, 17, 5
    c = dict(S=S, F=F, T=T, hop=hop, loss=inp, input=inp)
    mask_ld = sum(counts) * T + 4
    masks = np.full((S * F, mask_ld), np.nan, np.float32)
    seps, sets, singles, col, s_off, c_off = [], [], [], 0, 0, 0
    for i, n in enumerate(counts):
        m, sp = R.pit_inputs(S, F, T, n, 900 + i)
        masks[:, col:col + n * T] = m
        seps.append(sp.reshape(-1))
        sets.append((n, col, s_off, c_off))
        if n > 1:
            singles.append((_costs_launch(handle, c, m, sp, n, 0, n - 1, f"session {i}"), c_off))
        col, s_off, c_off = col + n * T, s_off + sp.size, c_off + (n - 1) * S * S + 5
    out = handle.stitch_host(1, masks=masks if inp == 0 else None, sep=np.concatenate(seps) if inp == 1 else None,
                             costs=R.canary64(c_off + SLACK), sets=sets, S=S, F=F, T=T, hop=hop, loss=inp, input=inp, mask_ld=mask_ld)
    owned = np.zeros(out.size, bool)
    for raw, at in singles:
        _same_bits(out[at:at + raw.size].reshape(raw.shape), raw, "a session of the multi launch against its single launch")
        owned[at:at + raw.size] = True
    _kept(out[~owned], "the multi launch: between and behind the sessions")


# ---- permutation scan -----------------------------------------------------------------------------------------------------------

def _scan_launch(handle, costs, S, lo, hi, perms, what):
    """perms: the allocation [rows][S] before the launch (rows >= hi + 1); returns it after the launch, slack checked"""
    rows = perms.shape[0]
    out = handle.stitch_host(2, costs=costs, perms=np.concatenate([perms.reshape(-1), np.full(SLACK, PERM_CANARY, np.int32)]), S=S,
                             lo=lo, hi=hi)
    _kept(out[rows * S:], what + ": the slack")
    out = out[:rows * S].reshape(rows, S)
    _same_bits(out[:lo + (1 if lo else 0)], perms[:lo + (1 if lo else 0)], what + ": rows up to the one resumed from")
    _same_bits(out[hi + 1:], perms[hi + 1:], what + ": rows behind the range")
    return out


@pytest.mark.parametrize("S", (1, 2, 3, 4))
def test_pit_scan(handle, S):
    from scipy.optimize import linear_sum_assignment
    L = pkg("_lib")
    for n, kind in itertools.product(R.SCAN_N, ("random", "ties", "zero", "inf", "nan")):
        what = f"S {S} boundaries {n} costs {kind}"
        costs = R.scan_costs(kind, n, S, 1000 + n + S)
        host = L.pit_scan(costs, S)
        blank = np.full((n + 3, S), PERM_CANARY, np.int32)
        got = _scan_launch(handle, costs, S, 0, n, blank, what)
        _same_bits(got[:n + 1], host, what + ": the device scan against css_pit_scan")
        for b in sorted({0, n // 2, n - 1}):
            m = costs[b].reshape(S, S)[host[b]]
            if np.isfinite(m).all():
                assert (linear_sum_assignment(m)[1] == got[b + 1]).all(), (what, b, "scipy's assignment")
        for cut in sorted({1, n // 2, 4096} & set(range(1, n))):      # two calls, [0, cut) then [cut, n), against one
            first = _scan_launch(handle, costs, S, 0, cut, blank, what + f" [0, {cut})")
            second = _scan_launch(handle, costs, S, cut, n, first, what + f" [{cut}, {n})")
            _same_bits(second, got, what + f": a scan in two calls cut at {cut}")


def test_pit_scan_resume(handle):
    """a scan resumed at b_lo from every one of the 3! incoming permutations (index_of_perm), across the 4096-boundary chunk"""
    S, n = 3, 8193
    costs = R.scan_costs("ties", n, S, 1100)
    L = pkg("_lib")
    for b_lo, start in itertools.product((1, 4096, 4097), itertools.permutations(range(S))):
        perms = np.full((n + 1, S), PERM_CANARY, np.int32)
        perms[b_lo] = start
        got = _scan_launch(handle, costs, S, b_lo, n, perms, f"resume at {b_lo} from {start}")
        # the host scan of the tail, with the rows of its first boundary put in the incoming order, is the same chain
        tail = costs[b_lo:].reshape(-1, S, S).copy()
        tail[0] = tail[0][list(start)]
        want = L.pit_scan(tail.reshape(-1, S * S), S)
        _same_bits(got[b_lo + 1:], want[1:], f"resume at {b_lo} from {start}")


# ---- overlap-add and gate -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", R.ola_cases(), ids=lambda c: c["name"])
def test_overlap_add(handle, c):
    S, F, T, hop, n, TL = c["S"], c["F"], c["T"], c["hop"], c["num_segments"], c["T_long"]
    masks, sep, win, perms = R.ola_inputs(c, O.calc_segment_weight)
    KIp = -(-2 * F // 32) * 32 + c["KIp_extra"]
    common = dict(S=S, F=F, T=T, hop=hop, num_segments=n, T_long=TL)
    zero = (np.zeros((S, F, TL), np.float32), np.zeros((S, TL), np.float32), np.zeros((S, TL), np.uint8))
    act0 = R.ola_masks(masks, win, perms, S, F, T, hop, n, TL, 0.5, 0, TL, zero)[1]
    th = float(np.sort(act0.reshape(-1))[act0.size // 2])          # an attained activity value: >= differs from >
    full = R.ola_masks(masks, win, perms, S, F, T, hop, n, TL, th, 0, TL, zero)
    assert (full[1] == np.float32(th)).any() and full[2].any() and not full[2].all()
    gate = R.gates(S, TL, c["seed"])
    words = {(0, None): None}
    words.update({(1, w): w for w in R.LEVEL_WORDS})
    fullY = {k: R.ola_stft(sep, win, perms, gate, S, F, T, hop, n, TL, KIp, k[0], w, 0, TL, np.zeros((S, TL, KIp), np.float32))
             for k, w in words.items()}
    for lo, hi in R.OLA_RANGES:
        hi = TL if hi is None else hi
        if hi > TL:
            continue
        what = f"{c['name']} frames [{lo}, {hi})"
        st, act, act_b = handle.stitch_host(3, masks=masks, windows=win, perms=perms, mask_st=R.canary(S * F * TL + SLACK),
                                            activity=R.canary(S * TL + SLACK), act_b=R.canary8(S * TL + SLACK), mask_ld=n * T,
                                            activity_th=th, lo=lo, hi=hi, **common)
        for got, want, shape, name in ((st, full[0], (S, F, TL), "mask_st"), (act, full[1], (S, TL), "activity"), (act_b, full[2], (S, TL), "act_b")):
            _kept(got[want.size:], f"{what}: the slack of {name}")
            got = got[:want.size].reshape(shape)
            _kept(got[..., :lo], f"{what}: {name} before the range")
            _kept(got[..., hi:], f"{what}: {name} behind the range")
            _same_bits(got[..., lo:hi], want[..., lo:hi].astype(got.dtype), f"{what}: {name} against the float32 model")
        for (split, word), want in fullY.items():
            if (lo, hi) != (0, TL) and word not in (None, R.LEVEL_WORDS[1]):
                continue
            Y = handle.stitch_host(5, sep=sep, windows=win, perms=perms, act_final=gate, Y=R.canary(S * TL * KIp + SLACK), KIp=KIp,
                                   y_split=split, level=word, lo=lo, hi=hi, **common)
            _kept(Y[want.size:], f"{what}: the slack of Y")
            Y = Y[:want.size].reshape(S, TL, KIp)
            _kept(Y[:, :lo], f"{what}: Y before the range")
            _kept(Y[:, hi:], f"{what}: Y behind the range")
            _same_bits(Y[:, lo:hi], want[:, lo:hi], f"{what}: Y (split {split}, level {word}) against the float32 model")


def test_morphology(handle):
    for S, TL in ((1, 7), (3, 40), (4, 600)):
        act_b = R.gates(S, TL, 1200 + TL)
        for dil, ero in itertools.product((0, 1, 4, TL + 3), repeat=2):
            for lo, hi in ((0, TL), (0, 1), (TL - 1, TL), (2, min(6, TL)), (TL // 2, TL)):
                what = f"S {S} T_long {TL} dilation {dil} erosion {ero} frames [{lo}, {hi})"
                blank = (R.canary8(S * TL).reshape(S, TL), R.canary8(S * TL).reshape(S, TL))
                want_tmp, want_fin = R.morphology(act_b, S, TL, dil, ero, lo, hi, blank, O.dilate, O.erode)
                tmp, fin = handle.stitch_host(4, act_b=np.concatenate([act_b.reshape(-1), R.canary8(SLACK)]), act_tmp=R.canary8(S * TL + SLACK),
                                              act_final=R.canary8(S * TL + SLACK), S=S, T_long=TL, dilation=dil, erosion=ero, lo=lo, hi=hi)
                _kept(tmp[S * TL:], what + ": the slack of act_tmp")
                _kept(fin[S * TL:], what + ": the slack of act_final")
                _same_bits(tmp[:S * TL].reshape(S, TL), want_tmp, what + ": act_tmp (the canary outside the dilated range)")
                _same_bits(fin[:S * TL].reshape(S, TL), want_fin, what + ": act_final (the canary outside the range)")


# ---- refusals -------------------------------------------------------------------------------------------------------------------

def test_refusals(handle):
    L = pkg("_lib")

    def refused(fn, **kw):
        with pytest.raises(L.CssError) as e:
            fn(**kw)
        assert e.value.code == L.CSS_ERR_INVALID_ARG, e.value

    # a NULL descriptor with a real handle (the binding always builds one)
    import ctypes as C
    lib = L.load()
    assert lib.css_mvdr_host(handle.h, None, None, None, None, None, None, None) == L.CSS_ERR_INVALID_ARG
    assert b"css_mvdr_host: null argument" in lib.css_last_error(handle.h)
    assert lib.css_stitch_host(handle.h, None, *([None] * 11)) == L.CSS_ERR_INVALID_ARG
    assert b"css_stitch_host: null argument" in lib.css_last_error(handle.h)
    assert lib.css_mvdr_host(handle.h, C.byref(L.CssMvdrDesc(form=0)), None, None, None, None, None, None) == L.CSS_ERR_INVALID_ARG

    c = {c["name"]: c for c in R.scm_cases()}["T64"]
    X, M, _ = R.scm_case_arrays(c)
    S, F, T = c["S"], c["F"], c["T"]
    segs = c["seg_lo"] + c["nseg"]
    good = dict(X=X, masks=M, scm=R.canary64(segs * (S + 1) * F * 49), C=7, F=F, S=S, T=T, hop=c["hop"], nseg=c["nseg"], seg_lo=c["seg_lo"],
                stft_frames=c["stft_frames"], T_ld=c["T_ld"], mask_ld=c["mask_ld"])
    handle.mvdr_host(0, **good)
    for change in (dict(C=6), dict(S=0), dict(S=4), dict(T=0), dict(mask_ld=segs * T - 1), dict(T_ld=c["stft_frames"] - 1), dict(hop=0),
                   dict(nseg=0), dict(seg_lo=-1), dict(scm=good["scm"][:-1]), dict(X=X.reshape(-1)[:-1]), dict(masks=M.reshape(-1)[:-1]),
                   dict(scm=None), dict(override=np.zeros(segs * F * T - 1, np.uint8)), dict(override=np.full(segs * F * T, S + 1, np.uint8)),
                   dict(override=np.full(segs * F * T, 16, np.uint8))):
        refused(lambda **kw: handle.mvdr_host(0, **kw), **dict(good, **change))
    refused(lambda **kw: handle.mvdr_host(0, **kw), **dict(good, mask_ld=1 << 61))       # (products of these would wrap)
    refused(lambda **kw: handle.mvdr_host(0, **kw), **dict(good, T_ld=1 << 61))
    refused(lambda **kw: handle.mvdr_host(5, **kw), **good)
    bfw = R.canary64(segs * S * F * 14)
    refused(lambda **kw: handle.mvdr_host(1, **kw), scm=good["scm"], bfw=bfw[:-1], C=7, F=F, S=S, T=T, hop=1, nseg=c["nseg"], seg_lo=c["seg_lo"])
    refused(lambda **kw: handle.mvdr_host(2, **kw), scm=good["scm"], bfw=bfw, C=7, F=F, S=S, T=T, hop=1, sets=[(0, segs, 1, 0)])
    refused(lambda **kw: handle.mvdr_host(2, **kw), scm=good["scm"], bfw=bfw, C=7, F=F, S=S, T=T, hop=1, sets=[])
    sep = R.canary(segs * S * F * T * 2)
    beam = dict(good, scm=None, sep=sep, bfw=bfw)
    refused(lambda **kw: handle.mvdr_host(3, **kw), **dict(beam, use_mvdr=1, C=1))
    refused(lambda **kw: handle.mvdr_host(3, **kw), **dict(beam, sep=sep[:-1]))
    assert (R.bits(sep) == R.CANARY).all() and (R.bits64(bfw) == R.bits64(R.canary64(1))).all()

    S, F, T, hop, n = 3, 5, 17, 5, 4
    masks, sp = R.pit_inputs(S, F, T, n, 1)
    cost = dict(masks=masks, costs=R.canary64(3 * S * S), S=S, F=F, T=T, hop=hop, loss=0, input=0, num_segments=n, mask_ld=n * T, lo=0, hi=3)
    handle.stitch_host(0, **cost)
    for change in (dict(S=0), dict(S=5), dict(hop=0), dict(hop=T + 1), dict(hop=T), dict(hi=4), dict(lo=-1), dict(lo=2, hi=1), dict(mask_ld=n * T - 1),
                   dict(costs=cost["costs"][:-1]), dict(masks=masks.reshape(-1)[:-1]), dict(masks=None), dict(loss=2), dict(input=2)):
        refused(lambda **kw: handle.stitch_host(0, **kw), **dict(cost, **change))
    refused(lambda **kw: handle.stitch_host(0, **kw), **dict(cost, mask_ld=1 << 61))
    refused(lambda **kw: handle.stitch_host(1, **kw), **dict(cost, sets=[(n, 1, 0, 0)]))
    refused(lambda **kw: handle.stitch_host(1, **kw), **dict(cost, sets=[]))
    perms = np.tile(np.arange(S, dtype=np.int32), (4, 1))
    scan = dict(costs=np.zeros(3 * S * S), perms=perms, S=S, lo=1, hi=3)
    handle.stitch_host(2, **scan)
    refused(lambda **kw: handle.stitch_host(2, **kw), **dict(scan, perms=np.array([[0, 1, 2], [0, 0, 2], [0, 1, 2], [0, 1, 2]], np.int32)))
    refused(lambda **kw: handle.stitch_host(2, **kw), **dict(scan, perms=perms[:3]))
    refused(lambda **kw: handle.stitch_host(2, **kw), **dict(scan, hi=4))
    TL = R.coverage(n, T, hop)
    win = R.ola_windows("random", T, 2, O.calc_segment_weight)
    ola = dict(sep=sp, windows=win, perms=perms, act_final=np.ones(S * TL, np.uint8), Y=R.canary(S * TL * 32), KIp=32, S=S, F=F, T=T, hop=hop,
               num_segments=n, T_long=TL, lo=0, hi=TL)
    handle.stitch_host(5, **ola)
    bad_perm = perms.copy()
    bad_perm[2] = (0, 3, 1)
    for change in (dict(KIp=2 * F - 1), dict(KIp=48, y_split=1, Y=R.canary(S * TL * 48)), dict(T_long=TL + 1), dict(hi=TL + 1), dict(lo=-1), dict(perms=bad_perm),
                   dict(Y=ola["Y"][:-1]), dict(act_final=np.ones(S * TL - 1, np.uint8)), dict(sep=sp.reshape(-1)[:-1]), dict(num_segments=0)):
        refused(lambda **kw: handle.stitch_host(5, **kw), **dict(ola, **change))
    refused(lambda **kw: handle.stitch_host(4, **kw), act_b=np.ones(S * TL, np.uint8), act_tmp=R.canary8(S * TL), act_final=R.canary8(S * TL),
            S=S, T_long=TL, dilation=-1, erosion=0, lo=0, hi=TL)
    refused(lambda **kw: handle.stitch_host(6, **kw), **ola)


if __name__ == "__main__":
    _forced_child(sys.argv[1])
