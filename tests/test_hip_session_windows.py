"""Encoder windows of whole sessions on the MI355X (include/css_mi355_session_window.h; Handle.handoff_windows_all,
run_enqueue_windows, run_enqueue_pcm16_windows): the windows and the whole padded log-mel written into device memory behind a
session's hand-off.  The rule is stream.session_windows over the session's normalised log-mel; every comparison is
np.array_equal, and every output buffer is preset to a sentinel with guard elements around it: "equal" means the rule's values
where the call writes and the sentinel everywhere else.

Two of the frame counts the hand-made gates were asked to produce cannot occur: the kept samples of a speaker are whole blocks
of 256, a kept run has at least two blocks, and J = floor(256 b / 160) for b kept blocks -- so J = 1 (b = 1) and J = 63
(39.375 <= b < 40) do not exist for any gate.  test_hand_made_gates takes J = 3 (the least frame count above zero) for the
first and reaches "stride - 1" and "stride + 1" at a second stride, (96, 63) with J = 62 and 64; J = 1 and J = stride - 1 at
stride 64 are covered on the numpy statement in tests/test_session_windows_host.py."""
import ctypes as C

import numpy as np
import pytest

from conftest import pkg
from test_hip_session_handoff import HCFG, LENGTHS, PLAIN, _Flat, _refused, _runs, model, world   # noqa: F401 (fixtures)
from test_hip_stream_handoff import CONFIGS, _Run, _rec

pytestmark = pytest.mark.gpu

SENT = -7.0                                            # (exact in float16; no log-mel value: those lie in [-1.5, 2.5])
GUARD = 64
SHAPES = ((3000, 3000, "float16", 3000, 0), (3000, 3000, "float32", 3008, 0), (96, 64, "float16", 97, 1), (100, 100, "float32", 101, 3),
          (64, 7, "float16", 64, 0))                   # (width, stride, dtype, ld, base offset in elements)


class _Dev:
    """device buffers of exactly the stated sizes for one call: windows [3][W][n_mels][ld] from element `off` of a flat tensor
    and -- mel_ld > 0 -- the whole log-mel [3][n_mels][mel_ld], both preset to the sentinel with guards on either side; the two
    count arrays, page-locked or pageable, with guards behind them"""

    def __init__(self, L, n_mels, width, stride, dtype, ld, off, W, mel_ld=0, pinned=True, windows=True):
        import torch
        self.n_mels, self.width, self.stride, self.dtype, self.ld, self.off, self.W, self.mel_ld = n_mels, width, stride, dtype, ld, off, W, mel_ld
        dt = getattr(torch, dtype)
        el = 2 if dtype == "float16" else 4
        self.n_win = 3 * W * n_mels * ld if windows else 0
        self.win = torch.full((GUARD + off + self.n_win + GUARD,), SENT, dtype=dt, device="cuda")
        self.whole = torch.full((GUARD + 3 * n_mels * mel_ld + GUARD,), SENT, dtype=dt, device="cuda")
        make = (lambda n, d: L.pinned_empty((n,), d)) if pinned else (lambda n, d: np.empty(n, d))
        self.nw, self.wm = make(3 + GUARD, np.int32), make(3 + GUARD, np.float32)
        self.nw[:] = int(SENT)
        self.wm[:] = SENT
        torch.cuda.synchronize()
        self.c = L.CssSessionWindows(width, stride, L.WINDOW_DTYPES[dtype], 0,
                                     self.win.data_ptr() + (GUARD + off) * el if windows else None, ld, W if windows else 0,
                                     self.whole.data_ptr() + GUARD * el if mel_ld else None, mel_ld, self.nw.ctypes.data, self.wm.ctypes.data)

    def expected(self, mels, M):
        """(windows buffer, whole buffer) by the rule, for the speakers' normalised log-mel `mels` and maxima `M`"""
        S = pkg("stream")
        dt = np.dtype(self.dtype)
        win = np.full(self.win.shape[0], SENT, dt)
        if self.n_win:
            view = win[GUARD + self.off:GUARD + self.off + self.n_win].reshape(3, self.W, self.n_mels, self.ld)
            for k in range(3):
                w = S.session_windows(mels[k], M[k], self.width, self.stride, self.dtype)
                assert w.shape[0] <= self.W
                view[k, :w.shape[0], :, :self.width] = w
        whole = np.full(self.whole.shape[0], SENT, dt)
        if self.mel_ld:
            view = whole[GUARD:GUARD + 3 * self.n_mels * self.mel_ld].reshape(3, self.n_mels, self.mel_ld)
            for k in range(3):
                J = mels[k].shape[1]
                if J:
                    view[k] = S.session_window_fill(M[k]).astype(dt)
                    view[k, :, :J] = mels[k].astype(dt)
        return win, whole

    def check(self, mels, M):
        """the rule's values where the call writes, the sentinel everywhere else; the counts"""
        import torch
        torch.cuda.synchronize()
        win, whole = self.expected(mels, M)
        assert np.array_equal(self.win.cpu().numpy(), win)
        assert np.array_equal(self.whole.cpu().numpy(), whole)
        for k in range(3):
            J = mels[k].shape[1]
            assert int(self.nw[k]) == -(-J // self.stride), (k, J)
            if J:
                assert self.wm[k] == np.float32(M[k]), (k, self.wm[k], M[k])
        assert (self.nw[3:] == int(SENT)).all() and (self.wm[3:] == SENT).all()

    def whole_view(self):
        return self.whole.cpu().numpy()[GUARD:GUARD + 3 * self.n_mels * self.mel_ld].reshape(3, self.n_mels, self.mel_ld)


def _stream_raw(world, x, hcfg):
    """the raw log-mel frames per speaker a finished CssStream with this hand-off configuration returned for recording x"""
    key = (x.shape[0], tuple(sorted(hcfg.items())))
    cache = world.setdefault("raw", {})
    if key not in cache:
        run = _Run(world["sep"], world["cfg"], hcfg)
        for n in range(0, x.shape[0], 24000):
            run.push(np.asarray(x[n:n + 24000]))
        run.finish()
        cache[key] = [run.total(k)[0] for k in range(3)]
        run.s.close()
    return cache[key]


def _maxima_of(mels, wm):
    """the maxima a call reported, held to the log-mel it normalised: the largest raw value is M itself, the clamp leaves it, so
    (M + 4) / 4 in float32 is the largest normalised value, and nothing lies below the clamp's floor"""
    M = []
    for k in range(3):
        m = np.float32(wm[k])
        if mels[k].shape[1]:
            assert (m + np.float32(4.0)) * np.float32(0.25) == mels[k].max(), k
            assert mels[k].min() >= (np.maximum(np.float32(-10.0), m - np.float32(8.0)) + np.float32(4.0)) * np.float32(0.25), k
        M.append(m)
    return M


# ---- 1. the synchronous call on real gates --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ci", range(len(CONFIGS)))
def test_synchronous_call_follows_the_rule(world, ci):
    L, S, h = pkg("_lib"), pkg("stream"), world["h"]
    hcfg = CONFIGS[ci]
    x = world["recs"][12.0]
    M = [np.float32(r.max()) for r in _stream_raw(world, x, hcfg)]      # from the streams: independent of the call under test
    wav, n_out = world["device_pass"](x)
    ref = h.handoff_logmel_all(wav.data_ptr(), n_out, **hcfg)
    mels = [m.copy() for m in ref.mel]
    assert all(m.shape[1] > 200 for m in mels)
    c_hcfg = L.handoff_cfg(**hcfg)
    for width, stride, dtype, ld, off in SHAPES:
        frames, ranges, W = L.session_window_bounds(world["sep"].desc, world["rc"], c_hcfg, width, stride, x.shape[0])
        assert frames == n_out // 160 and W == -(-frames // stride)
        for mel_ld in (frames, frames + 3000):
            for pinned, mel_host in ((True, True), (False, False)):
                if not pinned and mel_ld != frames:
                    continue
                dev = _Dev(L, hcfg["n_mels"], width, stride, dtype, ld, off, W, mel_ld, pinned=pinned)
                out = _Flat(L, hcfg["n_mels"], frames, ranges, pinned=pinned)
                keep = out.c.mel_host
                if not mel_host:
                    out.c.mel_host, out.c.cap_frames = None, 0
                L.check(h.h, h.lib.css_handoff_windows_all(h.h, C.c_void_p(wav.data_ptr()), n_out, C.byref(c_hcfg), C.byref(out.c), C.byref(dev.c)))
                dev.check(mels, M)
                if mel_host:
                    out.check(list(zip(ref.mel, ref.ranges)))
                else:
                    assert keep and (out.mel == -7).all()          # no log-mel went to the host
                    for k in range(3):
                        assert int(out.nf[k]) == mels[k].shape[1] and np.array_equal(out.reg[:3 * ranges * 2].reshape(3, ranges, 2)[k, :int(out.nr[k])], ref.ranges[k])
            if mel_ld == frames + 3000:
                # Whisper's segments: mel_dev[k][:, seek : seek + 3000] for seeks up to J_k
                whole = dev.whole_view()
                for k in range(3):
                    J = mels[k].shape[1]
                    fill = S.session_window_fill(M[k]).astype(dtype)
                    for seek in (0, J // 2, J - 1, J):
                        seg = whole[k][:, seek:seek + 3000]
                        assert seg.shape == (hcfg["n_mels"], 3000)
                        assert np.array_equal(seg[:, :J - seek], mels[k][:, seek:].astype(dtype)) and (seg[:, J - seek:] == fill).all()
                        if seek < J:
                            assert np.array_equal(seg, S.session_windows(mels[k][:, seek:], M[k], 3000, 3000, dtype)[0])
    # only the whole log-mel: windows_dev may be NULL
    dev = _Dev(L, hcfg["n_mels"], 3000, 3000, "float16", 3000, 0, 1, frames, windows=False)
    out = _Flat(L, hcfg["n_mels"], frames, ranges, pinned=True)
    L.check(h.h, h.lib.css_handoff_windows_all(h.h, C.c_void_p(wav.data_ptr()), n_out, C.byref(c_hcfg), C.byref(out.c), C.byref(dev.c)))
    dev.check(mels, M)


# ---- 2. hand-made gates -----------------------------------------------------------------------------------------------------------------

def test_hand_made_gates(world):
    """gate bytes written by hand (the mechanism of test_hip_session_handoff._run_cases: three cases per write, one per stream),
    pad 0: active frames [a, a + b - 1) keep the b blocks a .. a + b - 1, and J = 256 b // 160"""
    L, S, h = pkg("_lib"), pkg("stream"), world["h"]
    x = world["recs"][6.0]
    wav, n_out = world["device_pass"](x)
    TL = int(h.get_plan().mix_frames)
    frames = n_out // 160
    bound_r = (TL - 1) // 3 + 1
    hcfg = L.handoff_cfg(80, 0, True)
    blocks = {0: 0, 3: 2, 62: 39, 64: 40, 65: 41, 96: 60, 97: 61, 128: 80}      # J: kept blocks
    assert all(256 * b // 160 == J for J, b in blocks.items())
    seen = {}
    for width, stride, want in ((96, 64, (0, 3, 64, 65, 96, 97, 128)), (96, 63, (62, 64, 0))):
        W = -(-frames // stride)
        for i in range(0, len(want), 3):
            trio = (want[i:i + 3] + (0, 0))[:3]
            gates = np.stack([_runs(TL, (30, 30 + blocks[J] - 1)) if J else _runs(TL) for J in trio])
            h.write(L.BUF_ACT_FINAL, gates)
            ref = h.handoff_logmel_all(wav.data_ptr(), n_out, 80, 0, True)
            mels = [m.copy() for m in ref.mel]
            assert tuple(m.shape[1] for m in mels) == trio
            for dtype, pinned in (("float16", True), ("float32", False)):
                dev = _Dev(L, 80, width, stride, dtype, width + 1, 1, W, frames + 5, pinned=pinned)
                out = _Flat(L, 80, frames, bound_r, pinned=pinned)
                L.check(h.h, h.lib.css_handoff_windows_all(h.h, C.c_void_p(wav.data_ptr()), n_out, C.byref(hcfg), C.byref(out.c), C.byref(dev.c)))
                out.check(list(zip(ref.mel, ref.ranges)))
                M = _maxima_of(mels, dev.wm)
                dev.check(mels, M)
                view = dev.win.cpu().numpy()[GUARD + 1:GUARD + 1 + dev.n_win].reshape(3, W, 80, width + 1)
                for k, J in enumerate(trio):
                    n_w = -(-J // stride)
                    assert int(dev.nw[k]) == n_w
                    assert (view[k, n_w:] == SENT).all() and (view[k, :, :, width] == SENT).all()   # behind n_windows; behind the width
                    if J:
                        n_last = min(width, J - (n_w - 1) * stride)
                        fill = S.session_window_fill(M[k]).astype(dtype)
                        assert np.array_equal(view[k, n_w - 1, :, :n_last], mels[k][:, (n_w - 1) * stride:].astype(dtype))
                        assert (view[k, n_w - 1, :, n_last:width] == fill).all()
                    seen[(stride, J)] = n_w
    assert seen == {(64, 0): 0, (64, 3): 1, (64, 64): 1, (64, 65): 2, (64, 96): 2, (64, 97): 2, (64, 128): 2, (63, 62): 1, (63, 64): 2, (63, 0): 0}


# ---- 3. the maximum ---------------------------------------------------------------------------------------------------------------------

def test_window_max_is_the_maximum_of_the_raw_frames(world):
    L, S, h = pkg("_lib"), pkg("stream"), world["h"]
    x = world["recs"][12.0]
    raw = _stream_raw(world, x, HCFG)
    wav, n_out = world["device_pass"](x)
    ho, win = h.handoff_windows_all(wav.data_ptr(), n_out, 96, 64, "float32", **HCFG)
    for k in range(3):
        assert raw[k].shape[1] > 0 and win.window_max[k] == raw[k].max()
        assert np.array_equal(S.whisper_normalize(raw[k], win.window_max[k]), ho.mel[k])
        assert int(win.n_windows[k]) == -(-raw[k].shape[1] // 64)
        got = win.windows[k, :int(win.n_windows[k])].cpu().numpy()
        assert np.array_equal(got, S.session_windows(ho.mel[k], raw[k].max(), 96, 64, "float32"))


# ---- 4. the queue -----------------------------------------------------------------------------------------------------------------------

PARAMS = (dict(width=3000, stride=3000, dtype="float16", seek=True), dict(width=96, stride=64, dtype="float32", seek=False))
MEL_HOST = (True, False, False, True, False)           # of the five window sessions


def _window_args(world, sec, i, fill=SENT):
    """(SessionHandoff, SessionWindows) of exactly the bounds for window session i, everything preset to the sentinel"""
    import torch
    L, par = pkg("_lib"), PARAMS[i % 2]
    frames, ranges, W = L.session_window_bounds(world["sep"].desc, world["rc"], L.handoff_cfg(**HCFG), par["width"], par["stride"],
                                                world["recs"][sec].shape[0])
    dt = getattr(torch, par["dtype"])
    windows = torch.full((3, W, HCFG["n_mels"], par["width"] + 8), fill, dtype=dt, device="cuda")
    mel = torch.full((3, HCFG["n_mels"], frames + 3000), fill, dtype=dt, device="cuda") if par["seek"] else None
    ho = L.SessionHandoff(3, HCFG["n_mels"], frames, ranges, pinned=True, fill=int(fill))
    win = L.SessionWindows(0, 3, HCFG["n_mels"], par["width"], par["stride"], par["dtype"], windows=windows, mel=mel, fill=fill)
    return ho, win


def _sync_reference(world, sec, i):
    """the synchronous call's outputs for window session i of recording `sec`, into buffers preset like the queue's"""
    key = (sec, i % 2)
    cache = world.setdefault("winref", {})
    if key not in cache:
        par = PARAMS[i % 2]
        wav, n_out = world["device_pass"](world["recs"][sec])
        ho, win = _window_args(world, sec, i)
        world["h"].handoff_windows_all(wav.data_ptr(), n_out, par["width"], par["stride"], par["dtype"], out=ho, windows=win, **HCFG)
        cache[key] = (ho, win.windows.cpu().numpy(), None if win.mel is None else win.mel.cpu().numpy(), win.n_windows.copy(),
                      win.window_max.copy())
    return cache[key]


def _enqueue_seven(world):
    """the five lengths as window sessions, a plain hand-off session and a plain session between them"""
    L, h, rc = pkg("_lib"), world["h"], world["rc"]
    sessions = []

    def wav_out(sec):
        out = L.pinned_empty((3, int(L.plan(world["sep"].desc, rc, world["recs"][sec].shape[0]).n_out)), np.float32)
        out[:] = np.nan
        return out

    for i, sec in enumerate(LENGTHS):
        par = {k: v for k, v in PARAMS[i % 2].items() if k != "seek"}
        ho, win = _window_args(world, sec, i)
        view, _, _ = h.run_enqueue_windows(world["recs"][sec], rc, wav_out(sec) if i != 3 else None, mel_host=MEL_HOST[i], handoff=ho,
                                           windows=win, **par, **HCFG)
        sessions.append(("win", sec, i, view, ho, win))
        if i == 1:
            sessions.append(("plain", PLAIN, None, h.run_enqueue(world["recs"][PLAIN], rc, wav_out(PLAIN)), None, None))
        if i == 2:
            view, ho2 = h.run_enqueue_handoff(world["recs"][sec], rc, wav_out(sec), **HCFG)
            sessions.append(("handoff", sec, None, view, ho2, None))
    return sessions


def _check_sessions(world, sessions):
    for kind, sec, i, view, ho, win in sessions:
        want_wav, ref = world["reference"](sec, HCFG)
        if view is not None:
            assert np.array_equal(view, want_wav), (kind, sec)
        if kind == "handoff":
            for k in range(3):
                assert np.array_equal(ho.mel[k], ref[k][0]) and np.array_equal(ho.ranges[k], ref[k][1])
        if kind != "win":
            continue
        rho, rwin, rmel, rnw, rwm = _sync_reference(world, sec, i)
        assert np.array_equal(win.windows.cpu().numpy(), rwin), (sec, i)
        assert (win.mel is None) == (rmel is None) and (rmel is None or np.array_equal(win.mel.cpu().numpy(), rmel)), (sec, i)
        assert np.array_equal(win.n_windows, rnw) and np.array_equal(win.window_max, rwm)
        assert np.array_equal(ho.n_frames, rho.n_frames) and np.array_equal(ho.n_ranges, rho.n_ranges)
        for k in range(3):
            assert np.array_equal(ho.ranges[k], ref[k][1]) and int(ho.n_frames[k]) == ref[k][0].shape[1]
        if MEL_HOST[i]:
            assert np.array_equal(ho.mel_all, rho.mel_all)
            for k in range(3):
                assert np.array_equal(ho.mel[k], ref[k][0])
        else:
            assert (ho.mel_all == SENT).all()              # mel_host NULL: the array passed alongside keeps the sentinel


def test_queue_of_window_handoff_and_plain_sessions(world):
    h = world["h"]
    for i, sec in enumerate(LENGTHS):
        world["reference"](sec, HCFG)
        _sync_reference(world, sec, i)
    world["reference"](PLAIN, HCFG)
    for round_ in range(2):                                  # queued twice: the work buffers are reused
        launches0, sessions0 = h.session_window_stats()
        sessions = _enqueue_seven(world)
        assert len(sessions) == 7
        h.wait_sessions(3)
        _check_sessions(world, sessions[:3])                 # the first sessions' windows are valid
        h.wait()
        _check_sessions(world, sessions)
        launches1, sessions1 = h.session_window_stats()
        assert (launches1 - launches0, sessions1 - sessions0) == (5, 5)   # one launch per window session


# ---- 5. PCM16 ---------------------------------------------------------------------------------------------------------------------------

def test_pcm16_twin(world):
    L, h, rc = pkg("_lib"), world["h"], world["rc"]
    x = world["recs"][9.5]
    q = np.clip(np.round(np.asarray(x) * 32768.0), -32768, 32767).astype(np.int16)
    planes = [L.pinned_copy(np.ascontiguousarray(q[:, c])) for c in range(7)]
    n_out = int(L.plan(world["sep"].desc, rc, x.shape[0]).n_out)
    out16, peaks = L.pinned_empty((3, n_out), np.int16), L.pinned_empty((3,), np.float32)
    out16[:] = 0
    peaks[:] = 0
    want16, ho_ref = h.run_enqueue_pcm16_handoff(planes, rc, out16, peaks, **HCFG)
    h.wait()
    want16, want_peaks = want16.copy(), peaks.copy()
    xf = L.pinned_copy(np.ascontiguousarray(q.astype(np.float32) / np.float32(32768.0)))
    outf = L.pinned_empty((3, n_out), np.float32)
    _, ho_f, win_f = h.run_enqueue_windows(xf, rc, outf, 96, 64, "float16", seek=True, **HCFG)
    out16[:] = 0
    peaks[:] = 0
    view, ho, win = h.run_enqueue_pcm16_windows(planes, rc, out16, peaks, 96, 64, "float16", seek=True, **HCFG)
    h.wait()
    assert np.array_equal(view, want16) and np.array_equal(peaks, want_peaks)
    assert np.array_equal(win.n_windows, win_f.n_windows) and np.array_equal(win.window_max, win_f.window_max) and (win.n_windows > 0).all()
    for k in range(3):
        n = int(win.n_windows[k])
        assert np.array_equal(win.windows[k, :n].cpu().numpy(), win_f.windows[k, :n].cpu().numpy())
        assert np.array_equal(win.mel[k].cpu().numpy(), win_f.mel[k].cpu().numpy())
        assert np.array_equal(ho.mel[k], ho_f.mel[k]) and np.array_equal(ho.mel[k], ho_ref.mel[k]) and np.array_equal(ho.ranges[k], ho_ref.ranges[k])


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_queue_and_the_buffers_alone(world):
    import torch
    L, h, rc, desc = pkg("_lib"), world["h"], world["rc"], world["sep"].desc
    x = world["recs"][6.0]
    n_out = int(L.plan(desc, rc, x.shape[0]).n_out)
    c_hcfg = L.handoff_cfg(**HCFG)
    frames, ranges, W = L.session_window_bounds(desc, rc, c_hcfg, 96, 64, x.shape[0])
    world["reference"](6.0, HCFG)
    world["reference"](PLAIN, HCFG)
    _sync_reference(world, 6.0, 1)
    # two sessions are queued and stay queued while every refusal below happens
    first_ho, first_win = _window_args(world, 6.0, 1)
    launches_before = h.session_window_stats()[0]
    first_wav = L.pinned_empty((3, n_out), np.float32)
    h.run_enqueue_windows(x, rc, first_wav, 96, 64, "float32", mel_host=MEL_HOST[1], handoff=first_ho, windows=first_win, **HCFG)
    plain = L.pinned_empty((3, int(L.plan(desc, rc, world["recs"][PLAIN].shape[0]).n_out)), np.float32)
    h.run_enqueue(world["recs"][PLAIN], rc, plain)
    stats0 = h.session_window_stats()

    wav = L.pinned_empty((3, n_out), np.float32)
    wav[:] = SENT
    host = L.pinned_copy(np.full(3 * W * 80 * 97 + 64, SENT, np.float32))          # page-locked host memory: no device memory
    n = 0

    def attempt(code=L.CSS_ERR_INVALID_ARG, out_edit=None, hcfg=c_hcfg, null_win=False, pinned_counts=True, **edit):
        """one refused call per entry point; the status code, and every buffer keeps the sentinel"""
        nonlocal n
        for form in ("float", "pcm16"):
            dev = _Dev(L, 80, 96, 64, "float32", 97, 0, W, frames, pinned=pinned_counts)
            out = _Flat(L, 80, frames, ranges, pinned=True)
            for name, value in edit.items():
                setattr(dev.c, name, value(dev) if callable(value) else value)
            for name, value in (out_edit or {}).items():
                setattr(out.c, name, value)
            win_arg = None if null_win else C.byref(dev.c)
            if form == "float":
                rc_ = h.lib.css_run_enqueue_windows(h.h, x.ctypes.data_as(C.c_void_p), x.shape[0], 7, C.byref(rc.c), wav.ctypes.data_as(C.c_void_p),
                                                    n_out, C.byref(hcfg), C.byref(out.c), win_arg)
            else:
                rc_ = h.lib.css_run_enqueue_pcm16_windows(h.h, ptrs, x.shape[0], 7, C.byref(rc.c), w16.ctypes.data_as(C.c_void_p), n_out, None,
                                                          C.byref(hcfg), C.byref(out.c), win_arg)
            assert rc_ == code, (rc_, code, sorted(edit), out_edit, form)
            assert (dev.win == SENT).all() and (dev.whole == SENT).all() and (dev.nw == int(SENT)).all() and (dev.wm == SENT).all()
            assert (out.mel == -7).all() and (out.reg == -7).all() and (out.nf == -7).all() and (out.nr == -7).all()
            assert (wav == SENT).all() and (w16 == int(SENT)).all() and (host == SENT).all() and (pageable == SENT).all()
            assert h.session_window_stats() == stats0
        n += 1

    planes = [L.pinned_copy(np.zeros(x.shape[0], np.int16)) for _ in range(7)]
    ptrs = (C.c_void_p * 7)(*[p.ctypes.data for p in planes])
    w16 = L.pinned_empty((3, n_out), np.int16)
    w16[:] = int(SENT)
    pageable = np.full(host.shape[0], SENT, np.float32)
    attempt(null_win=True)
    attempt(n_windows=None)
    attempt(window_max=None)
    attempt(pinned_counts=False)                                                   # count arrays that are not page-locked
    attempt(windows_dev=None, mel_dev=None)
    for width, stride in ((0, 1), (3001, 64), (96, 0), (96, 97)):
        attempt(width=width, stride=stride)
    for dtype in (2, -1):
        attempt(dtype=dtype)
    attempt(ld=95)
    attempt(cap_windows=W - 1)
    attempt(mel_ld=frames - 1)
    attempt(windows_dev=host.ctypes.data)                                          # page-locked host memory is not device memory
    attempt(mel_dev=host.ctypes.data)
    attempt(windows_dev=pageable.ctypes.data)
    attempt(windows_dev=lambda d: d.win.data_ptr() + GUARD * 4 + 2)                # not aligned to the element
    attempt(mel_dev=lambda d: d.whole.data_ptr() + GUARD * 4 + 1)
    # everything css_run_enqueue_handoff refuses, with its codes
    for bad in (L.handoff_cfg(64, 8, True), L.handoff_cfg(80, 4097, True), L.handoff_cfg(80, -1, True)):
        attempt(hcfg=bad)
    attempt(out_edit=dict(cap_ranges=ranges - 1))
    attempt(out_edit=dict(cap_frames=frames - 1))
    attempt(out_edit=dict(ranges_host=None))
    attempt(out_edit=dict(n_frames=None))
    attempt(out_edit=dict(n_ranges=pageable.ctypes.data))                          # a hand-off array that is not page-locked
    assert n == 27
    # the queue still holds its two sessions, and finishes with the right results
    _refused(L, lambda: h.wait_sessions(3), L.CSS_ERR_INVALID_ARG)
    h.wait_sessions(2)
    h.wait()
    assert np.array_equal(first_wav, world["reference"](6.0, HCFG)[0]) and np.array_equal(plain, world["reference"](PLAIN, HCFG)[0])
    _check_sessions(world, [("win", 6.0, 1, None, first_ho, first_win)])
    assert h.session_window_stats() == (launches_before + 1, stats0[1])   # the queued session's one launch; no refusal counted
    # CSS_LINEAR_SPLIT_F16 (switching modes drains the queue, so a session is queued in that mode first)
    h.set_linear_mode("split_f16")
    try:
        stats0 = h.session_window_stats()
        h.run_enqueue(world["recs"][PLAIN], rc, plain)
        attempt(code=L.CSS_ERR_STATE)
        _refused(L, lambda: h.wait_sessions(2), L.CSS_ERR_INVALID_ARG)
        h.wait()
    finally:
        h.set_linear_mode("exact_f32")
    # the synchronous form refuses alike (a finished pass, nothing queued)
    dwav, _ = world["device_pass"](x)
    for edit in (dict(width=0), dict(stride=97), dict(dtype=5), dict(ld=95), dict(cap_windows=W - 1), dict(mel_ld=frames - 1),
                 dict(windows_dev=None, mel_dev=None), dict(windows_dev=host.ctypes.data), dict(n_windows=None)):
        dev = _Dev(L, 80, 96, 64, "float32", 97, 0, W, frames, pinned=False)
        out = _Flat(L, 80, frames, ranges, pinned=False)
        for name, value in edit.items():
            setattr(dev.c, name, value)
        assert h.lib.css_handoff_windows_all(h.h, C.c_void_p(dwav.data_ptr()), n_out, C.byref(c_hcfg), C.byref(out.c),
                                             C.byref(dev.c)) == L.CSS_ERR_INVALID_ARG, edit
        torch.cuda.synchronize()
        assert (dev.win == SENT).all() and (dev.whole == SENT).all() and (dev.nw == int(SENT)).all() and (dev.wm == SENT).all()
        assert (out.mel == -7).all() and (out.nf == -7).all() and (host == SENT).all()


def test_other_frame_geometry_is_refused(mc_state):
    L, CSS, SEP = pkg("_lib"), pkg("css"), pkg("separator")
    cfg = SEP.ConformerCssCfg(extractor_conf=SEP.ExtractorCfg(frame_len=400, frame_hop=160),
                              nnet_conf=SEP.NnetCfg(conformer_conf=SEP.ConformerCfg(attention_dim=512, attention_heads=8, num_blocks=18,
                                                                                  dropout_rate=0.0)))
    sep = SEP.HipSeparator(mc_state[0], cfg, device=0, max_batch_segments=16)
    try:
        rc = CSS.make_run_cfg(CSS.CssCfg(show_progressbar=False), 16000, 7, 400, 160)
        x = L.pinned_copy(_rec(4.0, 3))
        n_out = int(L.plan(sep.desc, rc, x.shape[0]).n_out)
        wav = L.pinned_empty((3, n_out), np.float32)
        wav[:] = SENT
        frames = n_out // 160 + 8
        dev = _Dev(L, 80, 96, 64, "float16", 96, 0, -(-frames // 64), frames)
        out = _Flat(L, 80, frames, 64, pinned=True)
        hcfg = L.handoff_cfg()
        rc_ = sep.handle.lib.css_run_enqueue_windows(sep.handle.h, x.ctypes.data_as(C.c_void_p), x.shape[0], 7, C.byref(rc.c),
                                                     wav.ctypes.data_as(C.c_void_p), n_out, C.byref(hcfg), C.byref(out.c), C.byref(dev.c))
        assert rc_ == L.CSS_ERR_INVALID_ARG
        sep.handle.wait()
        assert (wav == SENT).all() and (dev.win == SENT).all() and (dev.whole == SENT).all() and (dev.nw == int(SENT)).all() and (out.mel == -7).all()
    finally:
        sep.close()
