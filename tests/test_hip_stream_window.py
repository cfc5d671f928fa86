"""Encoder windows out of a stream's frame history on the MI355X (include/css_mi355_window.h; stream.py window / windows): a
window is, bit for bit, whisper_window of the raw frames the stream's own pushes returned, accumulated on the host -- for any
first frame, any wrap position of the ring, any width, both dtypes and any destination layout -- and a stream with a history
returns and holds, apart from the history, what its twin without one does.  Every comparison is np.array_equal.

The model, the recording (synth_meeting, 12 s, seed 2), the toggling gate and the chunk sizes are
test_hip_stream_preview_handoff.py's."""
import ctypes as C
import itertools

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

CHUNKS = (0, 1, 255, 256, 257, 4000, 24000, 32000)
SEED = 2
SENTINEL = 77.0


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


def _raw_windows(s, specs, n_mels):
    """ONE css_stream_windows for specs (k, first_frame, n_frames, width, dtype), each into a tensor of its own -> (rc, arrays, maxima)"""
    import torch
    L = pkg("_lib")
    h = s._h
    items = (L.CssStreamWindow * len(specs))()
    outs = []
    for it, (k, first, n, width, dtype) in zip(items, specs):
        t = torch.full((n_mels, width), SENTINEL, dtype=getattr(torch, dtype), device="cuda")
        outs.append(t)
        it.id, it.speaker, it.first_frame, it.n_frames, it.width = s.id, k, first, n, width
        it.dtype, it.out_dev, it.ld, it.window_max = L.WINDOW_DTYPES[dtype], t.data_ptr(), width, -7.0
    torch.cuda.synchronize()
    launches = C.c_int32(-7)
    rc = h.lib.css_stream_windows(h.h, items, len(specs), C.byref(launches))
    assert rc != L.CSS_OK or launches.value == -(-len(specs) // L.WINDOW_TABLE)
    return rc, [t.cpu().numpy() for t in outs], [it.window_max for it in items]


def _check_spans(S, s, acc, hist, n_mels):
    """window_range is [max(J - hist, 0), J); the issue's spans of it, each with width = n and n + 5, in both dtypes"""
    first, end = s.window_range()
    specs = []
    for k in range(3):
        J = acc[k].shape[1]
        assert (first[k], end[k]) == (max(J - hist, 0), J)
        f, n = int(first[k]), int(end[k] - first[k])
        if n == 0:
            continue
        spans = [(f, n), (f, 1), (f + n - 1, 1), (f + 1, n - 1), (f + 3, n - 3)]
        for (a, m), pad, dtype in itertools.product(spans, (0, 5), ("float32", "float16")):
            if m >= 1:
                specs.append((k, a, m, m + pad, dtype))
    if not specs:
        return 0
    rc, got, mx = _raw_windows(s, specs, n_mels)
    assert rc == 0
    for (k, a, m, width, dtype), w, top in zip(specs, got, mx):
        raw = acc[k][:, a:a + m]
        assert np.array_equal(w, S.whisper_window(raw, width, dtype)), (k, a, m, width, dtype)
        assert top == raw.max()
    return len(specs)


def test_history_smaller_than_a_round(model):
    """window_history = 96: a 32 000-sample push completes about 200 frames, more than the ring holds, and the ring turns over
    many times in 12 s, so the spans start at every alignment and cross the wrap."""
    S = pkg("stream")
    hcfg = dict(n_mels=80, pad_frames=8, drop_silence=False)
    sep = _sep(model)
    x = _rec()
    cfg = _toggling_cfg(sep, x, ("mc", 12.0, SEED))
    acc = [np.zeros((80, 0), np.float32) for _ in range(3)]
    n, checked, most, wrapped = 0, 0, 0, 0
    with S.CssStream(sep, cfg, handoff=hcfg, window_history=96) as s:
        assert _check_spans(S, s, acc, 96, 80) == 0
        for cut in _cuts(x.shape[0]):
            s.push(x[n:cut])
            n = cut
            most = max(most, max(m.shape[1] for m in s.handoff.mel))
            acc = _grow(acc, s.handoff)
            checked += _check_spans(S, s, acc, 96, 80)
            f, e = s.window_range()
            wrapped += int(any(f[k] > 0 and f[k] % 96 + (e[k] - f[k]) > 96 for k in range(3)))
        s.finish()
        assert s.info().finished
        acc = _grow(acc, s.handoff)
        checked += _check_spans(S, s, acc, 96, 80)
    print("windows compared:", checked, "most frames of a call:", most, "pushes after which a retained range crossed the wrap:", wrapped)
    assert most > 96 and wrapped > 0 and checked > 500
    sep.close()


def test_whole_recording_128_bands(model):
    """n_mels = 128, drop_silence on, pad 0, a history that holds everything: after finish, stream.window(k) with its defaults"""
    S = pkg("stream")
    hcfg = dict(n_mels=128, pad_frames=0, drop_silence=True)
    sep = _sep(model)
    x = _rec()
    cfg = _toggling_cfg(sep, x, ("mc", 12.0, SEED))
    acc = [np.zeros((128, 0), np.float32) for _ in range(3)]
    n = 0
    with S.CssStream(sep, cfg, handoff=hcfg, window_history=3000) as s:
        for cut in _cuts(x.shape[0]):
            s.push(x[n:cut])
            n = cut
            acc = _grow(acc, s.handoff)
        s.finish()
        acc = _grow(acc, s.handoff)
        first, end = s.window_range()
        for k in range(3):
            J = acc[k].shape[1]
            assert 0 < J < 3000 and (first[k], end[k]) == (0, J)
            w = s.window(k)
            assert tuple(w.shape) == (128, 3000) and str(w.dtype) == "torch.float16" and w.is_cuda
            assert np.array_equal(w.cpu().numpy(), S.whisper_window(acc[k], 3000, "float16"))
            assert s.window_max == acc[k].max()
    sep.close()


@pytest.mark.parametrize("dtype", ["float16", "float32"])
def test_destination_layout(dtype, model):
    """ld = 3001 at an element offset of 1: every row starts at another alignment, and nothing around the windows is written"""
    import torch
    S = pkg("stream")
    hcfg = dict(n_mels=80, pad_frames=8, drop_silence=True)
    sep = _sep(model)
    x = _rec()
    cfg = _toggling_cfg(sep, x, ("mc", 12.0, SEED))
    acc = [np.zeros((80, 0), np.float32) for _ in range(3)]
    with S.CssStream(sep, cfg, handoff=hcfg, window_history=3000) as s:
        for lo in range(0, x.shape[0], 32000):
            s.push(x[lo:lo + 32000])
            acc = _grow(acc, s.handoff)
        s.finish()
        acc = _grow(acc, s.handoff)
        per = 1 + 80 * 3001 + 7
        flat = torch.full((3 * per,), SENTINEL, dtype=getattr(torch, dtype), device="cuda")
        for k in range(3):
            view = flat[k * per + 1:k * per + 1 + 80 * 3001].view(80, 3001)[:, :3000]
            assert view.data_ptr() == flat.data_ptr() + (k * per + 1) * flat.element_size() and view.stride(0) == 3001
            got = s.window(k, dtype=dtype, out=view)
            assert got.data_ptr() == view.data_ptr()
        host = flat.cpu().numpy()
        for k in range(3):
            part = host[k * per:(k + 1) * per]
            body = part[1:1 + 80 * 3001].reshape(80, 3001)
            assert np.array_equal(body[:, :3000], S.whisper_window(acc[k], 3000, dtype))
            assert part[0] == SENTINEL and np.all(body[:, 3000] == SENTINEL) and np.all(part[1 + 80 * 3001:] == SENTINEL)
    sep.close()


def test_many_windows_many_streams(model):
    """three streams of a group, 3 x 3 speakers x 2 spans = 18 requests in ONE call: the 18 single calls, in at most 2 ceil(18 / table) launches"""
    S, L = pkg("stream"), pkg("_lib")
    hcfg = dict(n_mels=80, pad_frames=8, drop_silence=True)
    sep = _sep(model)
    x = _rec()
    cfg = _toggling_cfg(sep, x, ("mc", 12.0, SEED))
    recs = [x, np.ascontiguousarray(np.roll(x, 48000, axis=0)), np.ascontiguousarray(x[::-1])]
    streams = [S.CssStream(sep, cfg, handoff=hcfg, window_history=400) for _ in range(3)]
    group = S.CssStreamGroup(streams)
    for lo in range(0, x.shape[0], 32000):
        group.push([r[lo:lo + 32000] for r in recs])
    requests = []
    for s in streams:
        first, end = s.window_range()
        for k in range(3):
            assert end[k] - first[k] > 60
            requests += [(s, k), (s, k, int(first[k]) + 2, 50)]
    assert len(requests) == 18 > 16
    got = group.windows(requests, width=3000, dtype="float16")
    assert tuple(got.shape) == (18, 80, 3000)
    assert 1 <= group.window_launches <= 2 * -(-18 // L.WINDOW_TABLE)
    got = got.cpu().numpy()
    for i, r in enumerate(requests):
        single = r[0].window(*r[1:], width=3000, dtype="float16").cpu().numpy()
        assert np.array_equal(got[i], single), i
    assert len({got[i].tobytes() for i in range(18)}) == 18
    # ... and into a slice of a caller's tensor, in float32
    import torch
    big = torch.full((20, 80, 3000), SENTINEL, dtype=torch.float32, device="cuda")
    group.windows(requests, width=3000, dtype="float32", out=big[1:19])
    big = big.cpu().numpy()
    assert np.all(big[0] == SENTINEL) and np.all(big[19] == SENTINEL)
    for i, r in enumerate(requests):
        assert np.array_equal(big[1 + i].astype(np.float16), got[i])
    for s in streams:
        s.close()
    sep.close()


def test_nothing_else_moved(model):
    """A twin without window_history, pushed the same chunks: the same waveforms and Handoff, the same hand-off launches per call,
    device_bytes apart by exactly the ring and the per-frame maxima; a preview with hand-off writes nothing into the history."""
    S = pkg("stream")
    hcfg = dict(n_mels=80, pad_frames=8, drop_silence=True)
    sep = _sep(model)
    h = sep.handle
    x = _rec()
    cfg = _toggling_cfg(sep, x, ("mc", 12.0, SEED))
    a = S.CssStream(sep, cfg, handoff=hcfg, window_history=96)
    b = S.CssStream(sep, cfg, handoff=hcfg)
    ring = 3 * 80 * 96 * 4 + 3 * 96 * 4
    assert a.info().device_bytes - b.info().device_bytes == ring
    n, previews = 0, 0
    for cut in _cuts(x.shape[0]):
        wa = np.stack(a.push(x[n:cut]))
        la = h.stream_handoff_stats()
        wb = np.stack(b.push(x[n:cut]))
        lb = h.stream_handoff_stats()
        assert np.array_equal(wa, wb) and la == lb and la[0] == (3 if wa.shape[1] else 0)
        _same(a.handoff, b.handoff)
        assert a.info().device_bytes - b.info().device_bytes == ring
        n = cut
        first, end = a.window_range()
        if n >= 100000 and previews < 3 and (end > first).all():
            before = [a.window(k, width=96, dtype="float32").cpu().numpy() for k in range(3)]
            kept = a.handoff
            a.preview(handoff=True)
            assert a.handoff is kept and sum(m.shape[1] for m in a.preview_handoff.mel) > 0
            f2, e2 = a.window_range()
            assert np.array_equal(first, f2) and np.array_equal(end, e2)
            for k in range(3):
                assert np.array_equal(a.window(k, width=96, dtype="float32").cpu().numpy(), before[k])
            previews += 1
    assert previews == 3
    assert np.array_equal(np.stack(a.finish()), np.stack(b.finish())) and h.stream_handoff_stats()[0] == 3
    _same(a.handoff, b.handoff)
    a.close()
    b.close()
    sep.close()


def test_refusals(model):
    """Every refusal of css_stream_windows names the item, writes nothing and leaves later calls working; css_stream_window_open
    after the first sample, twice, and on a stream without hand-off is refused."""
    import torch
    S, L = pkg("stream"), pkg("_lib")
    hcfg = dict(n_mels=80, pad_frames=8, drop_silence=False)
    sep = _sep(model)
    h = sep.handle
    x = _rec()
    cfg = _toggling_cfg(sep, x, ("mc", 12.0, SEED))
    s = S.CssStream(sep, cfg, handoff=hcfg, window_history=96)
    no_hist = S.CssStream(sep, cfg, handoff=hcfg)
    plain = S.CssStream(sep, cfg)
    opened = lambda st, n: h.lib.css_stream_window_open(h.h, st.id, n)
    assert opened(s, 96) == L.CSS_ERR_STATE                                    # twice
    assert opened(plain, 96) == L.CSS_ERR_STATE                                # no hand-off
    assert opened(no_hist, 31) == opened(no_hist, (1 << 20) + 1) == L.CSS_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        S.CssStream(sep, cfg, window_history=96)
    acc = [np.zeros((80, 0), np.float32) for _ in range(3)]
    for st in (s, no_hist, plain):
        st.push(x[:96000])
    acc = _grow(acc, s.handoff)
    assert opened(no_hist, 96) == L.CSS_ERR_STATE                              # after the first sample
    first, end = s.window_range()
    assert (first > 0).all() and (end - first == 96).all()                     # the ring has turned over
    f0, e0 = int(first[0]), int(end[0])
    good = dict(id=s.id, speaker=0, first_frame=f0, n_frames=96, width=100, dtype=1, ld=100)
    buf = torch.full((80 * 100 + 8,), SENTINEL, dtype=torch.float32, device="cuda")   # (room for either dtype)

    def call(items_kw):
        items = (L.CssStreamWindow * len(items_kw))()
        for it, kw in zip(items, items_kw):
            kw = dict(good, out_dev=buf.data_ptr(), **kw) if "out_dev" not in kw else dict(good, **kw)
            for name, v in kw.items():
                setattr(it, name, v)
            it.window_max = -7.0
        launches = C.c_int32(-7)
        rc = h.lib.css_stream_windows(h.h, items, len(items), C.byref(launches))
        return rc, items, launches.value

    def refused(kw, text=()):
        rc, items, launches = call([{}, kw])
        assert rc == L.CSS_ERR_INVALID_ARG and launches == -7 and all(it.window_max == -7.0 for it in items)
        msg = h.lib.css_last_error(h.h).decode()
        assert "item 1" in msg and all(t in msg for t in text), msg
        assert bool((buf == SENTINEL).all())
        rc, items, launches = call([{}])                                       # later calls work
        assert rc == L.CSS_OK and launches == 1 and items[0].window_max == acc[0][:, f0:e0].max()
        got = buf.view(torch.float16)[:80 * 100].view(80, 100).cpu().numpy()
        assert np.array_equal(got, S.whisper_window(acc[0][:, f0:e0], 100, "float16"))
        buf.fill_(SENTINEL)

    refused(dict(id=no_hist.id), ("history",))
    refused(dict(id=plain.id), ("history",))
    refused(dict(id=40), ("no open stream",))
    refused(dict(speaker=3), ("speaker",))
    refused(dict(speaker=-1), ("speaker",))
    refused(dict(first_frame=f0 - 1), ("css_stream_window_range",))           # one below the retained range
    refused(dict(first_frame=f0 + 1), ("css_stream_window_range",))           # one past its end
    refused(dict(first_frame=e0, n_frames=1, width=1), ("css_stream_window_range",))
    refused(dict(n_frames=0))
    refused(dict(n_frames=96, width=95))
    refused(dict(width=3001, ld=3001))
    refused(dict(ld=99), ("ld",))
    refused(dict(dtype=2), ("dtype",))
    refused(dict(out_dev=None), ("out_dev",))
    refused(dict(out_dev=buf.data_ptr() + 1), ("out_dev",))                    # float16 at an odd address
    refused(dict(dtype=0, out_dev=buf.data_ptr() + 2), ("out_dev",))           # float32 at 2 mod 4
    assert h.lib.css_stream_window_range(h.h, no_hist.id, first.ctypes.data_as(C.POINTER(C.c_int64)),
                                         end.ctypes.data_as(C.POINTER(C.c_int64))) == L.CSS_ERR_STATE
    # the stream went on undisturbed: a finished stream still serves windows
    s.push(x[96000:])
    acc = _grow(acc, s.handoff)
    s.finish()
    acc = _grow(acc, s.handoff)
    for k in range(3):
        J = acc[k].shape[1]
        assert np.array_equal(s.window(k, width=96).cpu().numpy(), S.whisper_window(acc[k][:, J - 96:], 96, "float16"))
    for st in (s, no_hist, plain):
        st.close()
    sep.close()
