"""The hand-off of streamed sessions (css_stream_handoff_*), on the host: the rule that decides which samples a push
appends to a stream's concatenation, restated here and held to the oracle's active_regions; the pure entry points
(css_stream_handoff_final_frames, css_stream_handoff_bounds) against that rule; and the refusals.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import css_oracle as O
from conftest import pkg

FS, HOP, N = 16000, 256, 512
KNOBS = [dict(), dict(segment_size_sec=2.0, hop_size_sec=0.5), dict(activity_dilation_sec=0.6, activity_erosion_sec=0.1)]


def _desc():
    return pkg("weights").ModelDesc.mc_v1()


def _rc(knobs, ch=7):
    CSS = pkg("css")
    return CSS.make_run_cfg(CSS.CssCfg(**knobs), FS, ch)


def kept_ranges(act, t_known, pad, a, b, n_out):
    """sample ranges of [a, b) kept by the active frames below t_known: n is kept iff an active frame t has
    max(t - pad, 0) hop <= n < min((t + pad) hop + N, n_out)"""
    m = np.zeros(b - a, bool)
    for t in np.nonzero(act[:t_known])[0]:
        lo, hi = max(max(t - pad, 0) * HOP, a), min(min((t + pad) * HOP + N, n_out), b)
        if hi > lo:
            m[lo - a:hi - a] = True
    edges = np.flatnonzero(np.diff(np.concatenate([[0], m.astype(np.int8), [0]])))
    return [[a + int(s), a + int(e)] for s, e in zip(edges[::2], edges[1::2])]


def merged(ranges):
    out = []
    for a, b in ranges:
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return np.array(out, np.int64).reshape(-1, 2)


def test_incremental_ranges_equal_active_regions():
    """Random gate patterns, pad_frames 0 .. 11, gated-final frames growing in random steps: after a push the samples below
    D = max(t_g - pad, 0) hop are decided by the frames below t_g alone, and at finish all are; the ranges of all calls,
    touching ones merged, are the oracle's regions of the whole recording -- with and without an n_out that clips."""
    rng = np.random.default_rng(0)
    for trial in range(400):
        TL, pad = int(rng.integers(1, 400)), int(rng.integers(0, 12))
        p = rng.uniform(0.02, 0.5)
        act, t, on = np.zeros(TL, bool), 0, rng.random() < .5
        while t < TL:
            run = int(rng.geometric(p))
            act[t:t + run] = on
            on, t = not on, t + run
        n_out = max((TL - 1) * HOP + N - int(rng.integers(0, 3)) * 100, 1)
        want = O.active_regions(act, pad, n_out)
        ranges, t_g, D = [], 0, 0
        while t_g < TL:
            t_g = min(TL, t_g + int(rng.integers(1, 40)))
            D1 = n_out if t_g == TL else min(max(t_g - pad, 0) * HOP, n_out)
            if D1 > D:
                call = kept_ranges(act, t_g, pad, D, D1, n_out)
                # what a call returns is ascending and disjoint, and every end but the clip at n_out is a multiple of the hop
                assert all(x[1] <= y[0] for x, y in zip(call, call[1:]))
                assert all(e % HOP == 0 or e == n_out for _, e in call)
                # undecided frames cannot change it: the same call with every later frame active
                later = act.copy()
                later[t_g:] = True
                if t_g < TL:
                    assert kept_ranges(later, TL, pad, D, D1, n_out) == call
                ranges += call
                D = D1
        assert D == n_out
        assert np.array_equal(merged(ranges), want), (trial, pad)


def test_library_range_builder_incrementally():
    """css_handoff_kept_ranges -- the host function css_handoff_logmel and the streams share -- under the same random
    patterns: once over the whole recording (the offline call's use), and as a stream uses it: calls of one to three rounds,
    each round asking for [D before, D after) with the frames gated-final so far and a gate history trimmed to the frames
    from t_g - 2 pad - 3 on; a call's ranges merge where they touch.  Both equal the oracle's regions."""
    L = pkg("_lib")
    rng = np.random.default_rng(2)
    for trial in range(300):
        TL, pad = int(rng.integers(1, 400)), int(rng.integers(0, 12))
        p = rng.uniform(0.02, 0.5)
        act, t, on = np.zeros(TL, np.uint8), 0, rng.random() < .5
        while t < TL:
            run = int(rng.geometric(p))
            act[t:t + run] = on
            on, t = not on, t + run
        n_out = max((TL - 1) * HOP + N - int(rng.integers(0, 3)) * 100, 1)
        want = O.active_regions(act.astype(bool), pad, n_out)
        assert np.array_equal(L.handoff_kept_ranges(act, 0, TL, pad, 0, n_out, n_out), want)
        calls, t_g, D, base, hist, closing = [], 0, 0, 0, np.zeros(0, np.uint8), False
        while not closing:
            reg = None
            for _ in range(int(rng.integers(1, 4))):
                closing = t_g >= TL
                t1 = TL if closing else min(TL, t_g + int(rng.integers(1, 40)))
                D1 = n_out if closing else min(max(t1 - pad, 0) * HOP, n_out)
                hist = np.concatenate([hist, act[t_g:t1]])
                reg = L.handoff_kept_ranges(hist, base, t1, pad, D, max(D1, D), n_out if closing else 2 ** 62, reg)
                keep_from = max(t1 - 2 * pad - 3, base)
                hist, base, t_g, D = hist[keep_from - base:].copy(), keep_from, t1, max(D1, D)
                if closing:
                    break
            assert (reg[:, 0] < reg[:, 1]).all() and (reg[1:, 0] > reg[:-1, 1]).all()
            calls += reg.tolist()
        assert np.array_equal(merged(calls), want), (trial, pad)
    # a history that lacks a frame which can keep a sample of [a, b), too little room, bad arguments
    act = np.ones(100, np.uint8)
    for bad in (lambda: L.handoff_kept_ranges(act[50:], 50, 100, 8, 40 * HOP, 60 * HOP, 2 ** 62),
                lambda: L.handoff_kept_ranges(np.tile([1, 0, 0, 0], 25), 0, 100, 0, 0, 100 * HOP, 2 ** 62, cap=3),
                lambda: L.handoff_kept_ranges(act, 0, 100, -1, 0, 100, 100), lambda: L.handoff_kept_ranges(act, 0, 100, 0, 200, 100, 100)):
        with pytest.raises(L.CssError) as e:
            bad()
        assert e.value.code == L.CSS_ERR_INVALID_ARG


def test_block_rule_is_the_sample_rule():
    """the kernels decide whole 256-sample blocks: block q is kept iff an active frame t has t - pad <= q <= t + pad + 1"""
    rng = np.random.default_rng(1)
    for trial in range(100):
        TL, pad = int(rng.integers(1, 120)), int(rng.integers(0, 12))
        act = rng.random(TL) < rng.uniform(0.02, 0.4)
        n_out = (TL + 1) * HOP
        keep = np.zeros(TL + 1, bool)
        for t in np.nonzero(act)[0]:
            keep[max(t - pad, 0):min(t + pad + 1, TL) + 1] = True
        m = np.zeros(n_out, bool)
        for a, b in O.active_regions(act, pad, n_out):
            m[a:b] = True
        assert np.array_equal(np.repeat(keep, HOP), m)


@pytest.mark.parametrize("k", range(len(KNOBS)))
def test_final_frames_follow_the_final_samples(k):
    L = pkg("_lib")
    rc, desc = _rc(KNOBS[k]), _desc()
    h = L.handoff_cfg(80, 8, False)
    prev = 0
    ns = sorted(set(range(0, 6 * rc.c.segment_frames * HOP, 997)) | set(np.random.RandomState(k).randint(0, FS * 120, 300).tolist()))
    seen_positive = False
    for n in ns:
        fin = L.stream_final_samples(desc, rc, n)
        got = L.stream_handoff_final_frames(desc, rc, h, n)
        assert got == ((fin - 200) // 160 + 1 if fin >= 201 else 0), (n, fin, got)
        assert got >= prev
        prev, seen_positive = got, seen_positive or got > 0
    assert seen_positive
    with pytest.raises(L.CssError) as e:          # with the gate in play the count depends on the audio
        L.stream_handoff_final_frames(desc, rc, L.handoff_cfg(80, 8, True), 100000)
    assert e.value.code == L.CSS_ERR_INVALID_ARG


def _frames_of(n):
    return 0 if n < N else (n - N) // HOP + 1


def _t_g(rc, n):
    c = rc.c
    K = _frames_of(n)
    sd = (K - 1 - c.segment_frames) // c.hop_frames + 1 if K > c.segment_frames else 0
    return max(sd * c.hop_frames - c.dilation_frames - c.erosion_frames, 0)


def _emitted(A, closing):
    return A // 160 if closing else ((A - 200) // 160 + 1 if A >= 201 else 0)


@pytest.mark.parametrize("k", range(len(KNOBS)))
@pytest.mark.parametrize("drop,pad", [(False, 8), (True, 0), (True, 8), (True, 11)])
def test_bounds_cover_every_sample_kept(k, drop, pad):
    """css_stream_handoff_bounds for a sweep of chunk sizes against the counts of the rule when the gate keeps everything:
    frames, gate bits, and ranges (the worst case for ranges is every other block dropped)"""
    L = pkg("_lib")
    rc, desc = _rc(KNOBS[k]), _desc()
    h = L.handoff_cfg(80, pad, drop)
    p_eff = pad if drop else 0
    rs = np.random.RandomState(5 + k)
    for chunk in (1, 255, 256, 257, 4000, 24000, 32000, 100000, 700001):
        frames, ranges, activity = L.stream_handoff_bounds(desc, rc, h, chunk)
        n, A, J, D, tg = int(rs.randint(0, 70000)), 0, 0, 0, 0
        tg = _t_g(rc, n)
        D = max(tg - p_eff, 0) * HOP
        A = D
        J = _emitted(A, False)
        for _ in range(60):
            n += chunk
            tg1 = _t_g(rc, n)
            D1 = max(tg1 - p_eff, 0) * HOP
            A1 = A + (D1 - D)
            J1 = _emitted(A1, False)
            assert J1 - J <= frames and tg1 - tg <= activity, (chunk, n)
            assert (1 if not drop else ((D1 - D) // HOP + 1) // 2) <= ranges
            tg, D, A, J = tg1, D1, A1, J1
        # finish from here
        ff, fr, fa = L.stream_handoff_bounds(desc, rc, h, -1)
        TLf = max(_frames_of(n), rc.c.segment_frames)
        n_out = (TLf + 1) * HOP
        assert _emitted(A + n_out - D, True) - J <= ff and TLf - tg <= fa
        assert (1 if not drop else ((n_out - D) // HOP + 1) // 2) <= fr
    with pytest.raises(L.CssError):
        L.stream_handoff_bounds(desc, rc, h, -2)


def test_handoff_entry_points_fail_loudly():
    """bad arguments are CSS_ERR_INVALID_ARG; without a handle (no GPU: css_create fails) nothing is computed quietly"""
    L, CSS, W = pkg("_lib"), pkg("css"), pkg("weights")
    lib = L.load()
    rc, desc = _rc({}), _desc()
    for bad in (L.handoff_cfg(64, 8, True), L.handoff_cfg(80, -1, True), L.handoff_cfg(80, 5000, True)):
        with pytest.raises(L.CssError) as e:
            L.stream_handoff_bounds(desc, rc, bad, 1000)
        assert e.value.code == L.CSS_ERR_INVALID_ARG
        with pytest.raises(L.CssError) as e:
            L.stream_handoff_final_frames(desc, rc, bad, 1000)
        assert e.value.code == L.CSS_ERR_INVALID_ARG
    d400 = W.ModelDesc(num_blocks=1, frame_len=400, frame_hop=160)      # streams run 512 / 256 only
    with pytest.raises(L.CssError) as e:
        L.stream_handoff_bounds(d400, CSS.make_run_cfg(CSS.CssCfg(), FS, 7, 400, 160), L.handoff_cfg(), 1000)
    assert e.value.code == L.CSS_ERR_INVALID_ARG
    f = C.c_int64()
    assert lib.css_stream_handoff_final_frames(None, C.byref(rc.c), C.byref(L.handoff_cfg(80, 0, False)), 0, C.byref(f)) == L.CSS_ERR_INVALID_ARG
    assert lib.css_stream_handoff_open(None, 0, C.byref(L.handoff_cfg())) == L.CSS_ERR_INVALID_ARG
    assert lib.css_stream_handoff_bind(None, 0, None) == L.CSS_ERR_INVALID_ARG
    assert lib.css_stream_handoff_stats(None, None, None, None) == L.CSS_ERR_INVALID_ARG
    if lib.css_device_count() > 0:
        return
    SEP, S = pkg("separator"), pkg("stream")
    d1 = W.ModelDesc(num_blocks=1)
    sep = SEP.HipSeparator(W.portable_state_dict(d1, 0))
    with pytest.raises(L.CssError) as e:
        S.CssStream(sep, CSS.CssCfg(), handoff=dict(n_mels=80, pad_frames=8, drop_silence=True))
    assert e.value.code == L.CSS_ERR_NO_DEVICE


def test_whisper_normalize_is_the_offline_clamp():
    S = pkg("stream")
    rs = np.random.RandomState(0)
    raw = (rs.randn(80, 50) * 3 - 4).astype(np.float32)
    mx = np.float32(raw.max())
    want = (np.maximum(raw, mx - np.float32(8)) + np.float32(4)) * np.float32(0.25)
    assert np.array_equal(S.whisper_normalize(raw), want) and np.array_equal(S.whisper_normalize(raw, float(mx)), want)
    assert S.whisper_normalize(raw, 5.0).min() >= np.float32((5.0 - 8.0 + 4.0) / 4.0)
    assert S.whisper_normalize(np.empty((80, 0), np.float32)).shape == (80, 0)
