"""Encoder windows that reach the present on the MI355X (include/css_mi355_present_window.h; stream.py present_window /
present_windows).  The host accumulates acc[k] from the pushes' handoff.mel; with pv the preview_handoff of the SAME call,
J = acc[k].shape[1], P = pv.mel[k].shape[1], E = J + P, R = max(J - window_history, 0), a window (k, n, width, dtype) is
    a = max(E - n, R), used = E - a, whisper_window(concatenate([acc[k], pv.mel[k]], 1)[:, a:], width, dtype)
bit for bit, with first_frame = a, n_used = used, n_provisional = min(used, P), window_max = the span's maximum -- and the stream
is the stream it was.  Every comparison is np.array_equal.

The model, the recording (synth_meeting, 12 s, seed 2), the toggling gate and the chunk sizes are test_hip_stream_window.py's."""
import ctypes as C
import itertools
import types

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

CHUNKS = (0, 1, 255, 256, 257, 4000, 24000, 32000)
SEED = 2
SENTINEL = 77.0
UNTOUCHED = (-7, -7, -7, -7.0)


@pytest.fixture(scope="module")
def model():
    """the 2-block multi-channel model of test_hip_session.py's tiny_models"""
    w = pkg("weights")
    desc = w.ModelDesc(num_blocks=2)
    return w.apply_golden_recipe(w.portable_state_dict(desc, 21)), desc


def _sep(model):
    return pkg("separator").HipSeparator(model[0], None, device=0)


_RECS, _CFGS = {}, {}


def _rec(seconds=12.0, seed=SEED):
    if (seconds, seed) not in _RECS:
        x = pkg("synth").synth_meeting(float(seconds), 7, seed=seed)
        _RECS[(seconds, seed)] = np.ascontiguousarray(x[0] if x.ndim == 3 else x, dtype=np.float32)
    return _RECS[(seconds, seed)]


def _toggling_cfg(sep, x, key):
    """the recipe: a threshold at the 70th percentile of this model's activity on x, dilation 0.05 s, erosion 0.02 s"""
    css, L = pkg("css"), pkg("_lib")
    if key not in _CFGS:
        h = sep.handle
        h.run(x, css.make_run_cfg(css.CssCfg(activity_th=0.0, show_progressbar=False), 16000, x.shape[1]))
        _CFGS[key] = float(np.percentile(h.read(L.BUF_ACTIVITY), 70))
    return css.CssCfg(activity_th=_CFGS[key], show_progressbar=False, activity_dilation_sec=0.05, activity_erosion_sec=0.02)


def _cuts(total):
    out, n = [], 0
    for size in itertools.cycle(CHUNKS):
        if n >= total:
            return out
        n = min(n + size, total)
        out.append(n)


def _grow(acc, handoff):
    return [np.concatenate([a, m], axis=1) for a, m in zip(acc, handoff.mel)]


def _same(a, b):
    for k in range(3):
        assert np.array_equal(a.mel[k], b.mel[k]) and np.array_equal(a.ranges[k], b.ranges[k]) and np.array_equal(a.activity[k], b.activity[k])
    assert np.array_equal(a.raw_max, b.raw_max) and a.first_activity_frame == b.first_activity_frame


def _accepted(s):
    """preview(handoff=True) -> (waveforms, Handoff), or None where css_run refuses the prefix"""
    try:
        wav = np.stack(s.preview(handoff=True))
    except AssertionError:
        return None
    return wav, s.preview_handoff


def _present(h, parts, n_mels, edit=None):
    """ONE css_stream_present_windows.  parts: [(stream, [(k, n_frames, width, dtype), ...]), ...]; every window into a tensor
    [n_mels, width] of its own filled with SENTINEL, its out fields set to UNTOUCHED;
    `edit(items, tabs)` may change the items before the call.  -> rc, items, tabs, outs (torch), wavs, launches, stats; after
    CSS_OK every stream whose item's status is CSS_OK has its preview_handoff taken."""
    import torch
    L = pkg("_lib")
    items = (L.CssStreamPresentItem * max(len(parts), 1))()
    tabs, outs, wavs = [], [], []
    for it, (s, specs) in zip(items, parts):
        wav = np.full((s.num_spks, max(s.latency_samples, 1)), SENTINEL, np.float32)
        wavs.append(wav)
        it.ph.p.id, it.ph.p.out_host, it.ph.p.cap, it.ph.p.status, it.ph.p.n_out = s.id, wav.ctypes.data, wav.shape[1], -7, -7
        if s._hcfg is not None:
            ho, first_frame = s._preview_handoff_out()
            it.ph.ho, it.ph.first_frame = C.pointer(ho), first_frame.ctypes.data
        tab = (L.CssStreamPresentWindow * max(len(specs), 1))()
        mine = []
        for w, (k, n, width, dtype) in zip(tab, specs):
            t = torch.full((n_mels, width), SENTINEL, dtype=getattr(torch, dtype), device="cuda")
            mine.append(t)
            w.speaker, w.n_frames, w.width, w.dtype = k, n, width, L.WINDOW_DTYPES[dtype]
            w.out_dev, w.ld = t.data_ptr(), width
            w.first_frame, w.n_used, w.n_provisional, w.window_max = UNTOUCHED
        tabs.append(tab)
        outs.append(mine)
        it.windows, it.n_windows = tab, len(specs)
    if edit is not None:
        edit(items, tabs)
    torch.cuda.synchronize()
    stats, launches = L.CssStreamGroupStats(-7, -7), C.c_int32(-7)
    rc = h.lib.css_stream_present_windows(h.h, items, len(parts), C.byref(stats), C.byref(launches))
    if rc == L.CSS_OK:
        for it, (s, _) in zip(items, parts):
            s.preview_handoff = None
            if it.ph.p.status == L.CSS_OK:
                s._preview_handoff_take()
    return types.SimpleNamespace(rc=rc, items=items, tabs=tabs, outs=outs, wavs=wavs, launches=launches.value, stats=stats)


def _fields(w):
    return (w.first_frame, w.n_used, w.n_provisional, w.window_max)


def _expect(S, acc_k, pv_k, hist, n, width, dtype):
    """the rule -> (a, used, n_provisional, raw frames of the span, expected window or None)"""
    J, P = acc_k.shape[1], pv_k.shape[1]
    E, R = J + P, max(J - hist, 0)
    a = max(E - n, R)
    used = E - a
    raw = np.concatenate([acc_k, pv_k], axis=1)[:, a:]
    assert raw.shape[1] == used
    return a, used, min(used, P), raw, (S.whisper_window(raw, width, dtype) if used else None)


def _check(S, q_out, w, acc_k, pv_k, hist, spec):
    k, n, width, dtype = spec
    a, used, prov, raw, want = _expect(S, acc_k, pv_k, hist, n, width, dtype)
    assert used >= 1
    assert (w.first_frame, w.n_used, w.n_provisional) == (a, used, prov), (spec, _fields(w))
    assert w.window_max == raw.max()
    assert np.array_equal(q_out.cpu().numpy(), want), spec
    return a, used, prov


def test_spans_across_wrap_and_seam(model):
    """window_history = 96 (the ring turns over many times, and P_k, up to about 360 frames, may exceed it); at every cut at which
    a preview is accepted, for every speaker n_frames in {1, P, P + 1, P + 3, P + 96, 3000}: provisional frames only, exactly one
    ring frame across the seam, an unaligned seam, the whole ring, clamping; width = n_frames and n_frames + 5, both dtypes."""
    S, L = pkg("stream"), pkg("_lib")
    hcfg = dict(n_mels=80, pad_frames=8, drop_silence=False)
    sep = _sep(model)
    h = sep.handle
    x = _rec()
    cfg = _toggling_cfg(sep, x, ("mc", 12.0, SEED))
    acc = [np.zeros((80, 0), np.float32) for _ in range(3)]
    n, calls, checked, both, most_p = 0, 0, 0, 0, 0
    with S.CssStream(sep, cfg, handoff=hcfg, window_history=96) as s:
        for cut in _cuts(x.shape[0]):
            s.push(x[n:cut])
            n = cut
            acc = _grow(acc, s.handoff)
            pre = _accepted(s)
            if pre is None:
                continue
            specs = []
            for k in range(3):
                P = pre[1].mel[k].shape[1]
                most_p = max(most_p, P)
                for m in sorted({1, P, P + 1, P + 3, P + 96, 3000}):
                    if m >= 1:
                        for width, dtype in itertools.product(sorted({m, min(m + 5, 3000)}), ("float32", "float16")):
                            specs.append((k, m, width, dtype))
            kept = s.handoff
            r = _present(h, [(s, specs)], 80)
            assert r.rc == L.CSS_OK and r.items[0].ph.p.status == L.CSS_OK and r.launches == -(-len(specs) // L.WINDOW_TABLE)
            assert s.handoff is kept
            pv = s.preview_handoff
            _same(pv, pre[1])
            assert np.array_equal(pv.first_frame, pre[1].first_frame) and list(pv.first_frame) == [a.shape[1] for a in acc]
            assert np.array_equal(r.wavs[0][:, :r.items[0].ph.p.n_out], pre[0]) and r.items[0].ph.p.first_sample == s.preview_first_sample
            for spec, w, t in zip(specs, r.tabs[0], r.outs[0]):
                k = spec[0]
                a, used, prov = _check(S, t, w, acc[k], pv.mel[k], 96, spec)
                J = acc[k].shape[1]
                both += int(prov > 0 and a < J and a % 96 + (J - a) > 96)   # ring frames across the wrap AND provisional ones
                checked += 1
            calls += 1
        s.finish()
    print("present-window calls:", calls, "windows compared:", checked, "spans across wrap and seam:", both, "most provisional frames:", most_p)
    assert calls >= 10 and checked > 500 and both > 0 and most_p > 96
    sep.close()


def test_128_bands_large_history_and_the_offline_handoff(model):
    """n_mels = 128, window_history = 3000, drop_silence on: one window of 3000 frames per speaker at three cuts; at the last of
    them the window's frames are also Handle.handoff_logmel of css_run_device of the prefix."""
    import torch
    S, L, css = pkg("stream"), pkg("_lib"), pkg("css")
    hcfg = dict(n_mels=128, pad_frames=0, drop_silence=True)
    sep = _sep(model)
    h = sep.handle
    x = _rec()
    cfg = _toggling_cfg(sep, x, ("mc", 12.0, SEED))
    acc = [np.zeros((128, 0), np.float32) for _ in range(3)]
    cuts = _cuts(x.shape[0])
    at = [c for c in cuts if c >= 60000][::4][:3]
    assert len(at) == 3 and len(set(at)) == 3
    n, done, fulls = 0, 0, {}
    with S.CssStream(sep, cfg, handoff=hcfg, window_history=3000) as s:
        for cut in cuts:
            s.push(x[n:cut])
            n = cut
            acc = _grow(acc, s.handoff)
            if done == 3 or n != at[done]:
                continue
            done += 1
            for k, dtype in itertools.product(range(3), ("float16", "float32")):
                w = s.present_window(k, dtype=dtype)
                pv = s.preview_handoff
                a, used, prov, raw, want = _expect(S, acc[k], pv.mel[k], 3000, 3000, 3000, dtype)
                assert a == 0 and 0 < used < 3000 and prov == pv.mel[k].shape[1]
                assert tuple(w.shape) == (128, 3000) and w.is_cuda and str(w.dtype) == "torch." + dtype
                assert np.array_equal(w.cpu().numpy(), want)
                assert s.present_span == (a, used, prov) and s.window_max == raw.max()
                if done == 3 and dtype == "float32":
                    fulls[k] = w.cpu().numpy()[:, :used]
            if done == 3:
                # the span is everything there is: the offline hand-off of the prefix, which normalises over the whole of it
                rc = css.make_run_cfg(cfg, 16000, x.shape[1])
                n_out = int(L.plan(sep.desc, rc, n).n_out)
                pcm = torch.from_numpy(np.ascontiguousarray(x[:n])).cuda()
                wav = torch.empty((3, n_out), dtype=torch.float32, device="cuda")
                h.run_device(pcm.data_ptr(), n, x.shape[1], rc, wav.data_ptr(), n_out)
                torch.cuda.synchronize()
                for k in range(3):
                    mel, _ = h.handoff_logmel(wav.data_ptr(), n_out, k, **hcfg)
                    assert np.array_equal(fulls[k], mel), k
        assert done == 3
    sep.close()


def test_empty_span(model):
    """activity_th = 2.0 with drop_silence: no frame is ever kept, J_k = P_k = 0 -- nothing is written, window_max keeps its value"""
    S, L, css = pkg("stream"), pkg("_lib"), pkg("css")
    hcfg = dict(n_mels=80, pad_frames=8, drop_silence=True)
    sep = _sep(model)
    h = sep.handle
    x = _rec()
    cfg = css.CssCfg(activity_th=2.0, show_progressbar=False)
    acc = [np.zeros((80, 0), np.float32) for _ in range(3)]
    with S.CssStream(sep, cfg, handoff=hcfg, window_history=96) as s:
        for lo in range(0, 96000, 32000):
            s.push(x[lo:lo + 32000])
            acc = _grow(acc, s.handoff)
        specs = [(k, m, m + 5, dtype) for k in range(3) for m in (1, 96, 2995) for dtype in ("float32", "float16")]
        r = _present(h, [(s, specs)], 80)
        assert r.rc == L.CSS_OK and r.items[0].ph.p.status == L.CSS_OK and r.items[0].ph.p.n_out > 0
        pv = s.preview_handoff
        for k in range(3):
            assert pv.mel[k].shape[1] == 0 == acc[k].shape[1]
        for w, t in zip(r.tabs[0], r.outs[0]):
            assert _fields(w) == (0, 0, 0, -7.0)
            assert bool((t == SENTINEL).all())
        assert r.launches == 1
        assert s.present_window(0) is None and s.present_span == (0, 0, 0)
    sep.close()


@pytest.mark.parametrize("dtype", ["float16", "float32"])
def test_destination_layout(dtype, model):
    """ld = 3001 at an element offset of 1 (2 bytes / 4 bytes off a 16-byte boundary): every row starts at another alignment, and
    nothing around the windows is written"""
    import torch
    S = pkg("stream")
    hcfg = dict(n_mels=80, pad_frames=8, drop_silence=True)
    sep = _sep(model)
    x = _rec()
    cfg = _toggling_cfg(sep, x, ("mc", 12.0, SEED))
    acc = [np.zeros((80, 0), np.float32) for _ in range(3)]
    with S.CssStream(sep, cfg, handoff=hcfg, window_history=3000) as s:
        for lo in range(0, 128000, 32000):
            s.push(x[lo:lo + 32000])
            acc = _grow(acc, s.handoff)
        per = 1 + 80 * 3001 + 7
        flat = torch.full((3 * per,), SENTINEL, dtype=getattr(torch, dtype), device="cuda")
        assert flat.data_ptr() % 16 == 0
        spans = []
        for k in range(3):
            view = flat[k * per + 1:k * per + 1 + 80 * 3001].view(80, 3001)[:, :3000]
            assert view.data_ptr() == flat.data_ptr() + (k * per + 1) * flat.element_size() and view.stride(0) == 3001
            got = s.present_window(k, dtype=dtype, out=view)
            assert got.data_ptr() == view.data_ptr()
            spans.append((s.present_span, s.preview_handoff.mel[k]))
        host = flat.cpu().numpy()
        for k in range(3):
            a, used, prov, raw, want = _expect(S, acc[k], spans[k][1], 3000, 3000, 3000, dtype)
            assert spans[k][0] == (a, used, prov) and prov > 0 and used > prov
            part = host[k * per:(k + 1) * per]
            body = part[1:1 + 80 * 3001].reshape(80, 3001)
            assert np.array_equal(body[:, :3000], want)
            assert part[0] == SENTINEL and np.all(body[:, 3000] == SENTINEL) and np.all(part[1 + 80 * 3001:] == SENTINEL)
    sep.close()


def test_the_stream_does_not_move(model):
    """A twin that never calls the new entry point: identical pushes, hand-off outputs, window_range and window() tensors over the
    whole ring after every present-window call and after finish."""
    S, L = pkg("stream"), pkg("_lib")
    hcfg = dict(n_mels=80, pad_frames=8, drop_silence=True)
    sep = _sep(model)
    h = sep.handle
    x = _rec()
    cfg = _toggling_cfg(sep, x, ("mc", 12.0, SEED))
    a = S.CssStream(sep, cfg, handoff=hcfg, window_history=96)
    b = S.CssStream(sep, cfg, handoff=hcfg, window_history=96)

    def rings_agree():
        fa, ea = a.window_range()
        fb, eb = b.window_range()
        assert np.array_equal(fa, fb) and np.array_equal(ea, eb)
        for k in range(3):
            if ea[k] > fa[k]:
                wa = a.window(k, width=96, dtype="float32").cpu().numpy()
                assert np.array_equal(wa, b.window(k, width=96, dtype="float32").cpu().numpy()) and a.window_max == b.window_max

    n, calls = 0, 0
    for cut in _cuts(x.shape[0]):
        wa, wb = np.stack(a.push(x[n:cut])), np.stack(b.push(x[n:cut]))
        n = cut
        assert np.array_equal(wa, wb)
        _same(a.handoff, b.handoff)
        before = (a.info().n_pushed, a.info().n_emitted, a.info().finished, a.info().device_bytes)
        kept = a.handoff
        r = _present(h, [(a, [(k, m, 3000, "float16") for k in range(3) for m in (50, 3000)])], 80)
        assert r.rc == L.CSS_OK
        calls += int(r.items[0].ph.p.status == L.CSS_OK)
        assert a.handoff is kept
        after = (a.info().n_pushed, a.info().n_emitted, a.info().finished, a.info().device_bytes)
        assert before[:3] == after[:3] and b.info().n_pushed == after[0]
        rings_agree()
    assert calls >= 10
    assert np.array_equal(np.stack(a.finish()), np.stack(b.finish()))
    _same(a.handoff, b.handoff)
    rings_agree()
    a.close()
    b.close()
    sep.close()


def test_grouped(model):
    """Three streams at different phases -- one before its first accepted preview, one with window_history = 96, one with 3000
    -- and 70 windows in ONE call: 3 window launches, the hand-off's launches of css_stream_preview_handoff_many on the same
    items, every window its single-stream call's; the refused stream's windows and out fields stay.  Then, on the stream with 96
    frames of history, css_stream_present_windows (3 windows), css_stream_windows (40: two launches) and the first again -- the
    two calls share one result staging: after each, every window is whisper_window of the host's frames and every out field the rule's."""
    import torch
    S, L = pkg("stream"), pkg("_lib")
    hcfg = dict(n_mels=80, pad_frames=8, drop_silence=True)
    sep = _sep(model)
    h = sep.handle
    x = _rec()
    cfg = _toggling_cfg(sep, x, ("mc", 12.0, SEED))
    early = S.CssStream(sep, cfg, handoff=hcfg, window_history=96)
    small = S.CssStream(sep, cfg, handoff=hcfg, window_history=96)
    large = S.CssStream(sep, cfg, handoff=hcfg, window_history=3000)
    y = np.ascontiguousarray(np.roll(x, 48000, axis=0))
    group = S.CssStreamGroup([early, small, large])
    acc = [np.zeros((80, 0), np.float32) for _ in range(3)]   # the frames `small` has handed off
    group.push([x[:20000], x[:32000], y[:32000]])
    acc = _grow(acc, small.handoff)
    group.push([None, x[32000:64000], y[32000:64000]])
    acc = _grow(acc, small.handoff)
    group.push([None, x[64000:100000], y[64000:96000]])
    acc = _grow(acc, small.handoff)
    group.push([None, None, y[96000:150000]])
    widths = (3000, 200, 101)
    specs = {early: [(k, 40, 45, "float16") for k in range(3)] + [(0, 1, 1, "float32")],
             small: [(k, m, w, d) for k in range(3) for m, w, d in ((3000, 3000, "float16"), (97, 101, "float32"), (1, 200, "float16"),
                     (200, 200, "float32"), (150, 200, "float16"), (100, 101, "float16"), (60, 101, "float32"), (33, 200, "float32"),
                     (7, 101, "float16"), (180, 200, "float16"), (2, 101, "float32"))],
             large: [(k, m, w, d) for k in range(3) for m, w, d in ((3000, 3000, "float16"), (3000, 3000, "float32"), (1, 200, "float16"),
                     (200, 200, "float32"), (150, 200, "float16"), (100, 101, "float16"), (60, 101, "float32"), (33, 200, "float32"),
                     (7, 101, "float16"), (180, 200, "float16"), (2, 101, "float32"))]}
    parts = [(s, specs[s]) for s in (early, small, large)]
    assert sum(len(v) for _, v in parts) == 70 and all(w in widths or s is early for s, v in parts for _, _, w, _ in v)
    # the hand-off's launches of the plain grouped preview on the same items
    group.preview(handoff=True)
    ref_stats = h.stream_handoff_stats()
    ref_batches = (group.stats.estimator_batches, group.stats.estimator_segments)
    assert early.preview_handoff is None and small.preview_handoff is not None
    r = _present(h, parts, 80)
    assert r.rc == L.CSS_OK and r.launches == 3 == -(-70 // L.WINDOW_TABLE)
    assert h.stream_handoff_stats() == ref_stats and ref_stats[0] == 3
    assert (r.stats.estimator_batches, r.stats.estimator_segments) == ref_batches
    assert [it.ph.p.status for it in r.items] == [L.CSS_ERR_ZERO_WEIGHT, L.CSS_OK, L.CSS_OK]
    assert r.items[0].ph.p.n_out == 0 and bool((r.wavs[0] == SENTINEL).all())
    for w, t in zip(r.tabs[0], r.outs[0]):
        assert _fields(w) == UNTOUCHED and bool((t == SENTINEL).all())
    seen = set()
    for i, s in ((1, small), (2, large)):
        for spec, w, t in zip(specs[s], r.tabs[i], r.outs[i]):
            k, m, width, dtype = spec
            single = s.present_window(k, m, width, dtype)
            assert np.array_equal(t.cpu().numpy(), single.cpu().numpy()), (i, spec)
            assert s.present_span == _fields(w)[:3] and s.window_max == w.window_max and w.n_used >= 1
            seen.add((i, w.first_frame, w.n_used, w.n_provisional))
    assert len(seen) > 20
    # the Python group: the same call through present_windows, into a slice of a caller's tensor
    reqs = [(s, k, m) for s in (small, large) for k, m, w, d in specs[s] if w == 200 and d == "float16"]
    big = torch.full((len(reqs) + 2, 80, 200), SENTINEL, dtype=torch.float16, device="cuda")
    got, spans, maxima = group.present_windows(reqs + [(early, 1, 40)], width=200, dtype="float16", out=big[1:])
    assert got.data_ptr() == big[1:].data_ptr() and group.window_launches == 1
    host = big.cpu().numpy()
    assert np.all(host[0] == SENTINEL) and np.all(host[-1] == SENTINEL)
    assert tuple(spans[-1]) == (-1, 0, 0) and np.isnan(maxima[-1]) and early.preview_handoff is None
    for i, (s, k, m) in enumerate(reqs):
        single = s.present_window(k, m, 200, "float16")
        assert np.array_equal(host[1 + i], single.cpu().numpy()) and tuple(spans[i]) == s.present_span and maxima[i] == np.float32(s.window_max)
    # the calls alternate on one stream, with different counts
    first, end = small.window_range()
    assert [int(e) for e in end] == [a.shape[1] for a in acc]
    live = [k for k in range(3) if end[k] > first[k]]
    assert live
    plain = []
    for i in range(40):
        k = live[i % len(live)]
        f, n = int(first[k]), int(end[k] - first[k])
        a = f + i * 7 % n
        m = 1 + i * 5 % (f + n - a)
        plain.append((k, a, m, m + 5 * (i & 1), ("float16", "float32")[i >> 1 & 1]))
    three = [(k, 50 + 40 * k, 131, ("float16", "float32")[k & 1]) for k in range(3)]
    for call in ("present", "plain", "present"):
        if call == "present":
            r = _present(h, [(small, three)], 80)
            assert r.rc == L.CSS_OK and r.items[0].ph.p.status == L.CSS_OK and r.launches == 1 == -(-3 // L.WINDOW_TABLE)
            for spec, w, t in zip(three, r.tabs[0], r.outs[0]):
                _check(S, t, w, acc[spec[0]], small.preview_handoff.mel[spec[0]], 96, spec)
            continue
        items = (L.CssStreamWindow * 40)()
        outs = [torch.full((80, width), SENTINEL, dtype=getattr(torch, dtype), device="cuda") for _, _, _, width, dtype in plain]
        for it, t, (k, a, m, width, dtype) in zip(items, outs, plain):
            it.id, it.speaker, it.first_frame, it.n_frames, it.width = small.id, k, a, m, width
            it.dtype, it.out_dev, it.ld, it.window_max = L.WINDOW_DTYPES[dtype], t.data_ptr(), width, -7.0
        torch.cuda.synchronize()
        launches = C.c_int32(-7)
        assert h.lib.css_stream_windows(h.h, items, 40, C.byref(launches)) == L.CSS_OK and launches.value == 2 == -(-40 // L.WINDOW_TABLE)
        for it, t, (k, a, m, width, dtype) in zip(items, outs, plain):
            raw = acc[k][:, a:a + m]
            assert np.array_equal(t.cpu().numpy(), S.whisper_window(raw, width, dtype)), (k, a, m, width, dtype)
            assert it.window_max == raw.max() and (it.first_frame, it.n_frames) == (a, m)
    for s in (early, small, large):
        s.close()
    sep.close()


def test_refusals_change_nothing(model):
    """Every refusal: the return code, css_last_error naming the item (and the window), every tensor at its sentinel, every out
    field untouched -- and the next push that of a twin that was never asked."""
    import torch
    S, L = pkg("stream"), pkg("_lib")
    hcfg = dict(n_mels=80, pad_frames=8, drop_silence=False)
    sep = _sep(model)
    h = sep.handle
    x = _rec()
    cfg = _toggling_cfg(sep, x, ("mc", 12.0, SEED))
    s = S.CssStream(sep, cfg, handoff=hcfg, window_history=96)
    twin = S.CssStream(sep, cfg, handoff=hcfg, window_history=96)
    other = S.CssStream(sep, cfg, handoff=hcfg, window_history=96)
    no_hist = S.CssStream(sep, cfg, handoff=hcfg)
    plain = S.CssStream(sep, cfg)
    done = S.CssStream(sep, cfg, handoff=hcfg, window_history=96)
    for st in (s, twin, other, no_hist, plain, done):
        st.push(x[:96000])
    done.finish()
    acc = _grow([np.zeros((80, 0), np.float32) for _ in range(3)], s.handoff)
    good = [(0, 96, 100, "float16"), (1, 3000, 3000, "float32")]
    buf = torch.full((80 * 100 + 8,), SENTINEL, dtype=torch.float32, device="cuda")

    def refused(code, edit, text=(), parts=None):
        parts = parts if parts is not None else [(other, good), (s, good)]
        r = _present(h, parts, 80, edit=edit)
        msg = h.lib.css_last_error(h.h).decode()
        assert r.rc == code, (r.rc, msg)
        assert all(t in msg for t in text), msg
        assert r.launches == -7 and (r.stats.estimator_batches, r.stats.estimator_segments) == (-7, -7)
        for it, tab, outs, wav in zip(r.items, r.tabs, r.outs, r.wavs):
            assert (it.ph.p.status, it.ph.p.n_out) == (-7, -7) and bool((wav == SENTINEL).all())
            for w, t in zip(tab, outs):
                assert _fields(w) == UNTOUCHED and bool((t == SENTINEL).all())
        assert bool((buf == SENTINEL).all())

    def win(**kw):
        def edit(items, tabs):
            for name, v in kw.items():
                setattr(tabs[1][1], name, v)
        return edit

    def item(**kw):
        def edit(items, tabs):
            for name, v in kw.items():
                setattr(items[1], name, v)
        return edit

    def small_caps(items, tabs):
        ho = items[1].ph.ho.contents
        small_caps.kept = ho.cap_frames
        ho.cap_frames = 1

    def small_wave(items, tabs):
        items[1].ph.p.cap = 1

    def other_id(i):
        def edit(items, tabs):
            items[1].ph.p.id = i
        return edit

    INV, STATE = L.CSS_ERR_INVALID_ARG, L.CSS_ERR_STATE
    # what css_stream_preview_handoff_many refuses
    refused(INV, other_id(40), ("item 1", "no open stream"))
    refused(INV, other_id(other.id), ("item 1", "twice"))
    refused(STATE, other_id(done.id), ("item 1", "finished"))
    refused(INV, small_caps, ("item 1", "capacities"))
    s._preview_handoff_out()[0].cap_frames = small_caps.kept
    refused(INV, small_wave, ("item 1", "capacity"))
    refused(INV, lambda items, tabs: setattr(items[1].ph, "first_frame", None), ("item 1", "first_frame"))
    # a stream without a history; with the hand-off off
    refused(STATE, None, ("item 1", "history"), parts=[(other, good), (no_hist, good)])
    refused(STATE, None, ("item 1",), parts=[(other, good), (plain, good)])
    # the item's window table
    refused(INV, item(n_windows=-1), ("item 1", "n_windows"))
    refused(INV, item(windows=None), ("item 1", "windows"))
    refused(INV, lambda items, tabs: setattr(items[1].ph, "ho", None), ("item 1",))
    # the windows
    refused(INV, win(speaker=3), ("item 1", "window 1", "speaker"))
    refused(INV, win(speaker=-1), ("item 1", "window 1", "speaker"))
    refused(INV, win(n_frames=0), ("item 1", "window 1"))
    refused(INV, win(n_frames=3000, width=2999, ld=3000), ("item 1", "window 1"))
    refused(INV, win(n_frames=3001, width=3001, ld=3001), ("item 1", "window 1"))
    refused(INV, win(ld=2999), ("item 1", "window 1", "ld"))
    refused(INV, win(dtype=2), ("item 1", "window 1", "dtype"))
    refused(INV, win(out_dev=None), ("item 1", "window 1", "out_dev"))
    refused(INV, win(out_dev=buf.data_ptr() + 2, n_frames=96, width=100, ld=100), ("item 1", "window 1", "out_dev"))   # float32 at 2 mod 4
    refused(INV, win(dtype=1, out_dev=buf.data_ptr() + 1, n_frames=96, width=100, ld=100), ("item 1", "window 1", "out_dev"))
    # the call itself
    assert h.lib.css_stream_present_windows(h.h, None, 1, None, None) == INV
    r = _present(h, [], 80)
    assert r.rc == INV and r.launches == -7
    # later calls work, and the stream went on undisturbed
    r = _present(h, [(other, good), (s, good)], 80)
    assert r.rc == L.CSS_OK and r.launches == 1
    pv = s.preview_handoff
    for spec, w, t in zip(good, r.tabs[1], r.outs[1]):
        _check(S, t, w, acc[spec[0]], pv.mel[spec[0]], 96, spec)
    for lo in (96000, 128000):
        assert np.array_equal(np.stack(s.push(x[lo:lo + 32000])), np.stack(twin.push(x[lo:lo + 32000])))
        _same(s.handoff, twin.handoff)
    assert np.array_equal(np.stack(s.finish()), np.stack(twin.finish()))
    _same(s.handoff, twin.handoff)
    for k in range(3):
        assert np.array_equal(s.window(k, width=96).cpu().numpy(), twin.window(k, width=96).cpu().numpy())
    for st in (s, twin, other, no_hist, plain, done):
        st.close()
    sep.close()
