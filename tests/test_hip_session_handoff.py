"""The hand-off of whole sessions on the MI355X (include/css_mi355_session_handoff.h; Handle.handoff_logmel_all,
run_enqueue_handoff, run_enqueue_pcm16_handoff): kept ranges and normalised log-mel of all three separated streams, found and
computed on the device -- synchronously after a pass, and behind the waveforms of queued sessions.  The reference is always
Handle.handoff_logmel per stream after run_device on the same handle; every comparison is np.array_equal."""
import ctypes as C

import numpy as np
import pytest

from conftest import pkg
from test_hip_stream_handoff import CONFIGS, _rec, _sep, _toggling_cfg

pytestmark = pytest.mark.gpu

HOP, FRAME = 256, 512
SENT = -7
LENGTHS = (6.0, 9.5, 13.0, 17.0, 20.0)       # seconds of the queue's five hand-off sessions; PLAIN: the plain one between them
PLAIN = 8.0


@pytest.fixture(scope="module")
def model():
    """the 2-block multi-channel model of test_hip_stream_handoff.py"""
    w = pkg("weights")
    desc = w.ModelDesc(num_blocks=2)
    return w.apply_golden_recipe(w.portable_state_dict(desc, 21)), desc


@pytest.fixture(scope="module")
def world(model):
    """one handle, the recordings, a configuration under which the gate toggles, and the references -- each computed once"""
    import torch
    css, L = pkg("css"), pkg("_lib")
    sep = _sep(model)
    recs = {s: L.pinned_copy(_rec(s, 40 + i)) for i, s in enumerate(LENGTHS + (PLAIN, 12.0))}
    cfg = _toggling_cfg(sep, recs[12.0])
    rc = css.make_run_cfg(cfg, 16000, 7)
    w = dict(sep=sep, h=sep.handle, recs=recs, cfg=cfg, rc=rc, wav={}, ref={}, dev={})

    def device_pass(x):
        """run_device on x -> (waveforms on the device, n_out); the handle's session is x's afterwards"""
        n_out = int(L.plan(sep.desc, rc, x.shape[0]).n_out)
        pcm = torch.from_numpy(np.asarray(x)).cuda()
        wav = torch.empty((3, n_out), dtype=torch.float32, device="cuda")
        w["h"].run_device(pcm.data_ptr(), x.shape[0], 7, rc, wav.data_ptr(), n_out)
        torch.cuda.synchronize()
        return wav, n_out

    def reference(sec, hcfg):
        """(run()'s waveforms, [(mel, ranges) per stream] of run_device + handoff_logmel) of recording `sec`"""
        key = (sec, tuple(sorted(hcfg.items())))
        if sec not in w["wav"]:
            w["wav"][sec] = w["h"].run(recs[sec], rc).copy()
        if key not in w["ref"]:
            wav, n_out = device_pass(recs[sec])
            assert np.array_equal(wav.cpu().numpy(), w["wav"][sec])
            w["ref"][key] = [w["h"].handoff_logmel(wav.data_ptr(), n_out, k, **hcfg) for k in range(3)]
        return w["wav"][sec], w["ref"][key]

    w["device_pass"], w["reference"] = device_pass, reference
    yield w
    sep.close()


def _same(ho, ref):
    for k in range(3):
        mel, ranges = ref[k]
        assert int(ho.n_frames[k]) == mel.shape[1] and int(ho.n_ranges[k]) == ranges.shape[0], k
        assert np.array_equal(ho.ranges[k], ranges), k
        assert ho.mel[k].dtype == np.float32 and np.array_equal(ho.mel[k], mel), k


class _Flat:
    """caller arrays of exactly the stated capacities with guard elements behind them, everything preset to a sentinel.
    pinned: page-locked arrays, which take the kernels' own stores (what every queued session's arrays do; the synchronous call
    fills pageable ones from a staging block on the host, so only page-locked arrays hold the kernels to their bounds)"""

    def __init__(self, L, n_mels, frames, ranges, guard=64, pinned=False):
        self.n_mels, self.frames, self.ranges_cap = n_mels, frames, ranges

        def full(n, dtype):
            a = L.pinned_empty((n,), dtype) if pinned else np.empty(n, dtype)
            a[:] = SENT
            return a

        self.mel = full(3 * n_mels * frames + guard, np.float32)
        self.reg = full(3 * ranges * 2 + guard, np.int64)
        self.nf = full(3 + guard, np.int64)
        self.nr = full(3 + guard, np.int32)
        self.c = L.CssSessionHandoffOut(self.mel.ctypes.data, frames, self.reg.ctypes.data, ranges, self.nf.ctypes.data, self.nr.ctypes.data)

    def check(self, ref):
        """the reference's values where the call writes, the sentinel everywhere else"""
        nm, F, R = self.n_mels, self.frames, self.ranges_cap
        mel = self.mel[:3 * nm * F].reshape(3, nm, F)
        reg = self.reg[:3 * R * 2].reshape(3, R, 2)
        for k in range(3):
            want_mel, want_reg = ref[k]
            nf, nr = int(self.nf[k]), int(self.nr[k])
            assert (nf, nr) == (want_mel.shape[1], want_reg.shape[0]), (k, nf, nr, want_mel.shape, want_reg.shape)
            assert np.array_equal(reg[k, :nr], want_reg) and (reg[k, nr:] == SENT).all(), k
            assert np.array_equal(mel[k, :, :nf], want_mel) and (mel[k, :, nf:] == SENT).all(), k
        for a, n in ((self.mel, 3 * nm * F), (self.reg, 3 * R * 2), (self.nf, 3), (self.nr, 3)):
            assert (a[n:] == SENT).all()


# ---- 1. real gates ------------------------------------------------------------------------------------------------------------------

def test_all_streams_equal_the_per_stream_calls_on_real_gates(world):
    L, h = pkg("_lib"), world["h"]
    wav, n_out = world["device_pass"](world["recs"][12.0])
    act = h.read(L.BUF_ACT_FINAL)
    assert 0 < act.mean() < 1 and all(np.abs(np.diff(act[k].astype(np.int8))).sum() >= 4 for k in range(3))   # the gate toggles
    for hcfg in CONFIGS:
        ref = [h.handoff_logmel(wav.data_ptr(), n_out, k, **hcfg) for k in range(3)]
        _same(h.handoff_logmel_all(wav.data_ptr(), n_out, **hcfg), ref)                       # pageable arrays
        frames, ranges = L.session_handoff_bounds(world["sep"].desc, world["rc"], L.handoff_cfg(**hcfg), world["recs"][12.0].shape[0])
        pinned = L.SessionHandoff(3, hcfg["n_mels"], frames, ranges, pinned=True)
        _same(h.handoff_logmel_all(wav.data_ptr(), n_out, out=pinned, **hcfg), ref)           # page-locked: the kernels' own stores


# ---- 2. hand-made gates -------------------------------------------------------------------------------------------------------------

def _runs(TL, *spans):
    g = np.zeros(TL, np.uint8)
    for a, b in spans:
        g[max(a, 0):min(b, TL)] = 1
    return g


def _gate_cases(TL):
    """(name, pad, gate [TL], expectation or None) for a stream of TL frames (TL >= 186)"""
    mid = TL // 2
    cases = [("all zero", 8, _runs(TL), dict(n_ranges=0, n_frames=0)),
             ("all one", 8, _runs(TL, (0, TL)), dict(n_ranges=1, n_frames=(TL + 1) * HOP // 160)),
             ("only frame 0", 8, _runs(TL, (0, 1)), dict(n_ranges=1, n_frames=10 * HOP // 160)),
             ("only frame 0, pad 0", 0, _runs(TL, (0, 1)), dict(n_ranges=1, n_frames=2 * HOP // 160)),
             ("only the last frame", 8, _runs(TL, (TL - 1, TL)), dict(n_ranges=1, n_frames=10 * HOP // 160)),
             ("only the last frame, pad 0", 0, _runs(TL, (TL - 1, TL)), dict(n_ranges=1, n_frames=2 * HOP // 160)),
             ("one frame in the middle, pad 0", 0, _runs(TL, (mid, mid + 1)), dict(n_ranges=1, n_frames=2 * HOP // 160)),
             ("one frame in the middle, pad > TL", TL + 5, _runs(TL, (mid, mid + 1)), dict(n_ranges=1, n_frames=(TL + 1) * HOP // 160))]
    for pad in (0, 3):
        a = 40
        for gap, n in ((2 * pad + 2, 1), (2 * pad + 3, 2)):
            # frames [a, a + 5) and [b, b + 4): the second run's first frame is `gap` frames behind the first run's last one
            # (2 pad + 3 is the densest gate's step: apart; one less: the kept blocks touch)
            b = a + 4 + gap
            cases.append((f"gap {gap} at pad {pad}", pad, _runs(TL, (a, a + 5), (b, b + 4)), dict(n_ranges=n)))
    for blocks, frames in ((19, 30), (20, 32), (21, 33)):    # the edges of the 32-frame mel tile
        cases.append((f"{blocks} blocks", 0, _runs(TL, (60, 60 + blocks - 1)), dict(n_ranges=1, n_frames=frames)))
        cases.append((f"{blocks} blocks in two runs", 0, _runs(TL, (20, 29), (100, 100 + blocks - 11)), dict(n_ranges=2, n_frames=frames)))
    return cases


def _run_cases(world, wav, n_out, TL, cases, n_mels=80):
    """three cases per write of the gate bytes (one per stream); both routes read the same bytes.  Returns the cases checked."""
    L, h = pkg("_lib"), world["h"]
    done = 0
    by_pad = {}
    for c in cases:
        by_pad.setdefault(c[1], []).append(c)
    for pad, group in by_pad.items():
        for i in range(0, len(group), 3):
            trio = group[i:i + 3]
            gates = np.zeros((3, TL), np.uint8)
            for k, c in enumerate(trio):
                gates[k] = c[2]
            h.write(L.BUF_ACT_FINAL, gates)
            assert np.array_equal(h.read(L.BUF_ACT_FINAL), gates)
            ref = [h.handoff_logmel(wav.data_ptr(), n_out, k, n_mels=n_mels, pad_frames=pad, drop_silence=True, max_regions=TL + 1)
                   for k in range(3)]
            bound_r = (TL - 1) // (2 * pad + 3) + 1
            hcfg = L.handoff_cfg(n_mels, pad, True)
            for pinned in (True, False):                     # the kernels' own stores; the staged copy into pageable arrays
                out = _Flat(L, n_mels, n_out // 160, bound_r, pinned=pinned)
                L.check(h.h, h.lib.css_handoff_logmel_all(h.h, C.c_void_p(wav.data_ptr()), n_out, C.byref(hcfg), C.byref(out.c)))
                out.check(ref)
                for k, c in enumerate(trio):
                    want = c[3] or {}
                    if "n_ranges" in want:
                        assert int(out.nr[k]) == want["n_ranges"], (c[0], pinned)
                    if "n_frames" in want:
                        assert int(out.nf[k]) == want["n_frames"], (c[0], pinned)
                    done += 1
    return done // 2


def test_hand_made_gates(world):
    L, h = pkg("_lib"), world["h"]
    x = world["recs"][6.0]
    wav, n_out = world["device_pass"](x)
    TL = int(h.get_plan().mix_frames)
    assert n_out == (TL + 1) * HOP and TL == (x.shape[0] - FRAME) // HOP + 1
    cases = _gate_cases(TL)
    for pad in (0, 1, 8):                                    # the densest gates: n_ranges == cap_ranges == the bound
        g = np.zeros(TL, np.uint8)
        g[::2 * pad + 3] = 1
        cases.append((f"densest at pad {pad}", pad, g, dict(n_ranges=(TL - 1) // (2 * pad + 3) + 1)))
    rs = np.random.RandomState(5)
    for pad in (0, 1, 8):
        cases.append((f"random at pad {pad}", pad, (rs.rand(TL) < 0.06).astype(np.uint8), None))
    assert len(cases) == 8 + 4 + 6 + 3 + 3
    assert _run_cases(world, wav, n_out, TL, cases) == len(cases)
    # the other filterbank and drop_silence = 0 on hand-made bytes
    assert _run_cases(world, wav, n_out, TL, cases[-3:], n_mels=128) == 3
    ref = [h.handoff_logmel(wav.data_ptr(), n_out, k, 80, 8, False) for k in range(3)]
    hcfg = L.handoff_cfg(80, 8, False)
    for pinned in (True, False):
        out = _Flat(L, 80, n_out // 160, 1, pinned=pinned)
        L.check(h.h, h.lib.css_handoff_logmel_all(h.h, C.c_void_p(wav.data_ptr()), n_out, C.byref(hcfg), C.byref(out.c)))
        out.check(ref)
        assert list(out.nr[:3]) == [1, 1, 1] and list(out.nf[:3]) == [n_out // 160] * 3


@pytest.mark.parametrize("extra", (-1, 0, 1, 4))
def test_scan_chunk_boundaries(world, extra):
    """streams of C - 1, C, C + 1 and C + 4 sample blocks (C: the keep-scan's step; C + 4 is the shortest stream in which a run
    can START on the first block of the second step with pad 0): runs that straddle the step, end on its last block, start on
    its first block, in the block domain (pad 0) and shifted by pad 8; and random gates, whose rows start at every alignment
    of the gate bytes (row k starts at byte k TL)"""
    L, h = pkg("_lib"), world["h"]
    Cn = L.SESSION_SCAN_CHUNK
    assert Cn == 1024
    TL = Cn + extra - 1
    x = _rec(((TL - 1) * HOP + FRAME) / 16000.0 + 0.01, 77)[:(TL - 1) * HOP + FRAME]
    wav, n_out = world["device_pass"](x)
    assert int(h.get_plan().mix_frames) == TL and n_out == (Cn + extra) * HOP
    rs = np.random.RandomState(100 + extra)
    cases = []
    for pad in (0, 8):
        # pad 0: active frames [a, b) keep blocks a .. b
        cases.append((f"straddles, pad {pad}", pad, _runs(TL, (Cn - 4, Cn + 2)), dict(n_ranges=1)))
        cases.append((f"ends on the last block of the step, pad {pad}", pad, _runs(TL, (Cn - 6 - pad, Cn - 1 - pad)), dict(n_ranges=1)))
        cases.append((f"starts on the step, pad {pad}", pad, _runs(TL, (min(Cn + pad, TL - 1), Cn + pad + 2)), dict(n_ranges=1)))
        cases.append((f"runs on both sides, pad {pad}", pad, _runs(TL, (3, 9), (Cn - 40, Cn - 30), (Cn - 3 - pad, TL)), None))
        cases.append((f"random, pad {pad}", pad, (rs.rand(TL) < 0.05).astype(np.uint8), None))
        cases.append((f"dense random, pad {pad}", pad, (rs.rand(TL) < 0.5).astype(np.uint8), None))
    assert len(cases) == 12
    if extra == 4:   # the three named runs are what their names say
        assert cases[1][2][Cn - 2] == 1 and cases[1][2][Cn - 1] == 0 and cases[2][2][Cn - 1] == 0 and cases[2][2][Cn] == 1
    assert _run_cases(world, wav, n_out, TL, cases) == 12


# ---- 3 / 4. the queue ---------------------------------------------------------------------------------------------------------------

HCFG = CONFIGS[0]


def _enqueue_six(world, pageable_wav=False):
    """five hand-off sessions (the fourth without waveforms) and a plain one in the middle -> [(seconds, wav view, hand-off)].
    The hand-off arrays are page-locked _Flat ones of exactly the bounds, preset to the sentinel with guards behind them: the
    kernels of a queued session store into them directly, and _Flat.check holds those stores to 'nothing else is written'."""
    L, h, rc = pkg("_lib"), world["h"], world["rc"]
    make = (lambda shape: np.empty(shape, np.float32)) if pageable_wav else (lambda shape: L.pinned_empty(shape, np.float32))
    order = list(LENGTHS[:2]) + [PLAIN] + list(LENGTHS[2:])
    sessions = []
    for sec in order:
        x = world["recs"][sec]
        n_out = int(L.plan(world["sep"].desc, rc, x.shape[0]).n_out)
        frames, ranges = L.session_handoff_bounds(world["sep"].desc, rc, L.handoff_cfg(**HCFG), x.shape[0])
        flat = None if sec == PLAIN else _Flat(L, HCFG["n_mels"], frames, ranges, pinned=True)
        if sec == PLAIN:
            out = L.pinned_empty((3, n_out), np.float32)
            out[:] = np.nan
            sessions.append((sec, h.run_enqueue(x, rc, out), None))
        elif sec == LENGTHS[3]:
            sessions.append((sec,) + h.run_enqueue_handoff(x, rc, None, handoff=flat, **HCFG))
        else:
            out = make((3, n_out))
            out[:] = np.nan
            sessions.append((sec,) + h.run_enqueue_handoff(x, rc, out, handoff=flat, **HCFG))
    return sessions


def _check_sessions(world, sessions):
    for sec, wav, ho in sessions:
        want_wav, ref = world["reference"](sec, HCFG)
        if wav is not None:
            assert np.array_equal(wav, want_wav), sec
        if ho is not None:
            ho.check(ref)                                    # the reference's values, and the sentinel everywhere else


def _references_first(world):
    for sec in LENGTHS + (PLAIN,):
        world["reference"](sec, HCFG)


def test_queue_of_handoff_and_plain_sessions(world):
    _references_first(world)
    sessions = _enqueue_six(world)
    assert sum(ho is not None for _, _, ho in sessions) == 5 and sum(w is None for _, w, _ in sessions) == 1
    world["h"].wait()
    _check_sessions(world, sessions)


def test_wait_sessions_makes_the_first_handoffs_valid(world):
    _references_first(world)
    sessions = _enqueue_six(world)
    world["h"].wait_sessions(2)
    _check_sessions(world, sessions[:2])
    world["h"].wait()
    _check_sessions(world, sessions)


def test_every_session_alone(world):
    _references_first(world)
    h = world["h"]
    h.set_queue_group(1)
    try:
        sessions = _enqueue_six(world)
        h.wait()
    finally:
        h.set_queue_group(8)
    _check_sessions(world, sessions)


def test_pageable_waveforms_with_page_locked_handoff(world):
    _references_first(world)
    sessions = _enqueue_six(world, pageable_wav=True)
    world["h"].wait()
    _check_sessions(world, sessions)


# ---- 5. filterbank switches -----------------------------------------------------------------------------------------------------------

def test_filterbank_switches_inside_one_queue(world):
    L, h, rc = pkg("_lib"), world["h"], world["rc"]
    plan = [(LENGTHS[0], 80), (LENGTHS[1], 128), (LENGTHS[2], 80), (LENGTHS[0], 128)]
    cfgs = {nm: dict(n_mels=nm, pad_frames=8, drop_silence=True) for nm in (80, 128)}
    refs = [world["reference"](sec, cfgs[nm]) for sec, nm in plan]
    got = [h.run_enqueue_handoff(world["recs"][sec], rc, None, **cfgs[nm])[1] for sec, nm in plan]
    h.wait()
    for ho, (_, ref), (sec, nm) in zip(got, refs, plan):
        assert ho.mel_all.shape[1] == nm
        _same(ho, ref)


# ---- 6. PCM16 -----------------------------------------------------------------------------------------------------------------------

def test_pcm16_twin(world):
    """PCM16 planes in, peak-normalised PCM16 streams out as run_pcm16 gives them, and the hand-off of the float waveforms
    before that normalisation: run_device on the same samples as float (q / 32768, the ingest's own scaling) + handoff_logmel"""
    L, h, rc = pkg("_lib"), world["h"], world["rc"]
    x = world["recs"][9.5]
    q = np.clip(np.round(np.asarray(x) * 32768.0), -32768, 32767).astype(np.int16)
    planes = [L.pinned_copy(np.ascontiguousarray(q[:, c])) for c in range(7)]
    want16, want_peaks = h.run_pcm16(planes, rc)
    xf = np.ascontiguousarray(q.astype(np.float32) / np.float32(32768.0))
    wav, n_out = world["device_pass"](xf)
    ref = [h.handoff_logmel(wav.data_ptr(), n_out, k, **HCFG) for k in range(3)]
    out16 = L.pinned_empty((3, n_out), np.int16)
    peaks = L.pinned_empty((3,), np.float32)
    out16[:] = 0
    peaks[:] = 0
    view, ho = h.run_enqueue_pcm16_handoff(planes, rc, out16, peaks, **HCFG)
    plain = L.pinned_empty((3, int(L.plan(world["sep"].desc, rc, world["recs"][PLAIN].shape[0]).n_out)), np.float32)
    plain_view = h.run_enqueue(world["recs"][PLAIN], rc, plain)
    h.wait()
    assert np.array_equal(view, want16) and np.array_equal(peaks, want_peaks)
    _same(ho, ref)
    assert np.array_equal(plain_view, world["reference"](PLAIN, HCFG)[0])


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------

def _refused(L, call, code):
    with pytest.raises(L.CssError) as e:
        call()
    assert e.value.code == code, (e.value.code, code)


def test_refusals_leave_the_queue_and_the_arrays_alone(world):
    L, h, rc, desc = pkg("_lib"), world["h"], world["rc"], world["sep"].desc
    x = world["recs"][6.0]
    n_out = int(L.plan(desc, rc, x.shape[0]).n_out)
    frames, ranges = L.session_handoff_bounds(desc, rc, L.handoff_cfg(**HCFG), x.shape[0])
    assert ranges >= 2
    wav = L.pinned_empty((3, n_out), np.float32)
    wav[:] = SENT

    def untouched(ho):
        assert (ho.mel_all == SENT).all() and (ho.ranges_all == SENT).all() and (ho.n_frames == SENT).all() and (ho.n_ranges == SENT).all()
        assert (wav == SENT).all()
        h.wait()                                             # nothing was queued, and waiting for nothing is fine
        assert (wav == SENT).all()

    good = lambda **kw: L.SessionHandoff(3, kw.get("n_mels", 80), kw.get("frames", frames), kw.get("ranges", ranges),
                                         pinned=kw.get("pinned", True), fill=SENT)
    n = 0
    # CSS_LINEAR_SPLIT_F16
    ho = good()
    h.set_linear_mode("split_f16")
    try:
        _refused(L, lambda: h.run_enqueue_handoff(x, rc, wav, handoff=ho, **HCFG), L.CSS_ERR_STATE)
    finally:
        h.set_linear_mode("exact_f32")
    untouched(ho)
    n += 1
    for kw, hcfg in ((dict(frames=frames - 1), HCFG), (dict(ranges=ranges - 1), HCFG), (dict(pinned=False), HCFG),
                     (dict(n_mels=64), dict(HCFG, n_mels=64)), (dict(), dict(HCFG, pad_frames=4097)), (dict(), dict(HCFG, pad_frames=-1))):
        ho = good(**kw)
        _refused(L, lambda: h.run_enqueue_handoff(x, rc, wav, handoff=ho, **hcfg), L.CSS_ERR_INVALID_ARG)
        untouched(ho)
        _refused(L, lambda: h.run_enqueue_handoff(x, rc, None, handoff=ho, **hcfg), L.CSS_ERR_INVALID_ARG)
        untouched(ho)
        n += 1
    assert n == 7
    # the synchronous form refuses short capacities too (it accepts pageable arrays)
    dwav, _ = world["device_pass"](x)
    for kw in (dict(frames=frames - 1), dict(ranges=ranges - 1)):
        ho = good(**kw)
        _refused(L, lambda: h.handoff_logmel_all(dwav.data_ptr(), n_out, out=ho, **HCFG), L.CSS_ERR_INVALID_ARG)
        assert (ho.mel_all == SENT).all() and (ho.n_frames == SENT).all()
    # and the queue still works
    ho = good()
    view, _ = h.run_enqueue_handoff(x, rc, wav, handoff=ho, **HCFG)
    h.wait()
    want_wav, ref = world["reference"](6.0, HCFG)
    assert np.array_equal(view, want_wav)
    _same(ho, ref)


def test_other_frame_geometry_is_refused(mc_state):
    L, CSS, SEP = pkg("_lib"), pkg("css"), pkg("separator")
    cfg = SEP.ConformerCssCfg(extractor_conf=SEP.ExtractorCfg(frame_len=400, frame_hop=160),
                              nnet_conf=SEP.NnetCfg(conformer_conf=SEP.ConformerCfg(attention_dim=512, attention_heads=8, num_blocks=18,
                                                                                  dropout_rate=0.0)))
    sep = SEP.HipSeparator(mc_state[0], cfg, device=0, max_batch_segments=16)
    try:
        assert (sep.desc.frame_len, sep.desc.frame_hop) == (400, 160)
        rc = CSS.make_run_cfg(CSS.CssCfg(show_progressbar=False), 16000, 7, 400, 160)
        x = L.pinned_copy(_rec(4.0, 3))
        n_out = int(L.plan(sep.desc, rc, x.shape[0]).n_out)
        wav = L.pinned_empty((3, n_out), np.float32)
        wav[:] = SENT
        ho = L.SessionHandoff(3, 80, n_out // 160 + 8, 64, pinned=True, fill=SENT)
        _refused(L, lambda: sep.handle.run_enqueue_handoff(x, rc, wav, handoff=ho), L.CSS_ERR_INVALID_ARG)
        sep.handle.wait()
        assert (wav == SENT).all() and (ho.mel_all == SENT).all() and (ho.n_ranges == SENT).all()
    finally:
        sep.close()


def test_open_stream_behaves_as_for_a_plain_enqueue(world):
    """with a stream open on the handle, the hand-off form is accepted or refused exactly as css_run_enqueue is"""
    L, h, rc = pkg("_lib"), world["h"], world["rc"]
    x = world["recs"][6.0]
    n_out = int(L.plan(world["sep"].desc, rc, x.shape[0]).n_out)
    want = world["reference"](6.0, HCFG)[0]
    s = pkg("stream").CssStream(world["sep"], world["cfg"])
    try:
        outcome = []
        for form in ("plain", "handoff"):
            wav = L.pinned_empty((3, n_out), np.float32)
            try:
                if form == "plain":
                    h.run_enqueue(x, rc, wav)
                else:
                    h.run_enqueue_handoff(x, rc, wav, **HCFG)
                h.wait()
                outcome.append(("ok", bool(np.array_equal(wav[:, :n_out], want))))
            except L.CssError as e:
                outcome.append(("refused", e.code))
                h.wait()
        assert outcome[0] == outcome[1], outcome
    finally:
        s.close()
