"""Previews of streamed sessions on the MI355X (include/css_mi355_preview.h; stream.py CssStream.preview, CssStreamGroup.preview):
after n pushed samples a preview is css_run of those n samples from the stream's first unemitted sample on, bit for bit, and the
stream afterwards behaves as if it had never been previewed.  Every comparison is np.array_equal."""
import ctypes as C

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

CHUNKS = (1, 255, 256, 257, 4000, 24000)
ZERO_WEIGHT_TEXT = "zero weights found"


def _sep(state, **kw):
    st, _ = state
    return pkg("separator").HipSeparator(st, None, device=0, **kw)


def _clip(mix60, seconds, ch=7, start=0):
    x = mix60[0] if mix60.ndim == 3 else mix60
    return np.ascontiguousarray(x[start:start + int(16000 * seconds), :ch], dtype=np.float32)


def _offline(sep, x, cfg):
    rc = pkg("css").make_run_cfg(cfg, 16000, x.shape[1])
    return sep.handle.run(np.ascontiguousarray(x, np.float32), rc).copy()


def _try(fn):
    """((exception type, css_status or text), None) of a call that raises, ((None, None), value) of one that returns"""
    L = pkg("_lib")
    try:
        return (None, None), fn()
    except L.CssError as e:
        return (L.CssError, e.code), None
    except AssertionError as e:   # CSS_ERR_ZERO_WEIGHT raises the reference's assert (_lib.check)
        return (AssertionError, str(e)), None


def _frames(cfg, ch=7):
    c = pkg("css").make_run_cfg(cfg, 16000, ch).c
    return c.segment_frames, c.hop_frames, c.dilation_frames + c.erosion_frames


def _first_rebase_length(cfg):
    """the shortest prefix whose frames no longer fit the window a stream opens with (api_stream.hip css_stream_open: WF), so
    that the push reaching it moves the window"""
    T, hop, halo = _frames(cfg)
    wf = (2 * T + 2 * halo + 3 * hop + 8 * hop + 16 + 3) // 4 * 4
    return wf * 256 + 512


def _seeded_cuts(seed, total, forced=()):
    rs = np.random.RandomState(seed)
    cuts, n = set(int(f) for f in forced if 0 < f <= total), 0
    while n < total:
        n = min(total, n + int(CHUNKS[rs.randint(0, len(CHUNKS))]))
        cuts.add(n)
    return sorted(cuts)


def _preview_is_css_run(sep, s, x, n, cfg):
    """the stream holds x[:n]: its preview against css_run of x[:n]; True when both succeeded"""
    before = s.info()
    ref_status, want = _try(lambda: _offline(sep, x[:n], cfg))
    got_status, got = _try(s.preview)
    assert got_status == ref_status, (n, got_status, ref_status)
    after = s.info()
    assert (after.n_pushed, after.n_emitted, after.finished) == (before.n_pushed, before.n_emitted, 0) and before.n_pushed == n
    if ref_status != (None, None):
        assert ref_status[0] is AssertionError and ZERO_WEIGHT_TEXT in ref_status[1]
        return False
    got = np.stack(got)
    em = after.n_emitted
    assert got.shape == want[:, em:].shape and got.shape[1] <= s.latency_samples, (n, got.shape, want.shape, em)
    assert np.array_equal(got, want[:, em:]), n
    assert s.preview_first_sample == em and s.preview_samples(n) == (em, got.shape[1])
    return True


def _push_preview_compare(sep, x, cfg, cuts, at_zero=True):
    """pushes x up to every cut, previews after every push and compares; the pushes' and finish's outputs are css_run's too.
    -> the cuts at which a preview existed"""
    S = pkg("stream")
    ok, outs = [], []
    with S.CssStream(sep, cfg, num_channels=x.shape[1]) as s:
        if at_zero and _preview_is_css_run(sep, s, x, 0, cfg):
            ok.append(0)
        n = 0
        for cut in cuts:
            outs.append(np.stack(s.push(x[n:cut])))
            n = cut
            if _preview_is_css_run(sep, s, x, n, cfg):
                ok.append(n)
        if n < x.shape[0]:
            outs.append(np.stack(s.push(x[n:])))
        outs.append(np.stack(s.finish()))
    assert np.array_equal(np.concatenate(outs, axis=1), _offline(sep, x, cfg))
    return ok


@pytest.mark.parametrize("m0", [0.15, 0.0])
def test_preview_is_css_run_of_the_prefix(m0, mc_state, mix60):
    """Seeded chunks and the forced prefix lengths: none, less than a frame, less than a segment, one sample short of / exactly
    one segment plus a frame, the same around the second segment.  With the default windows css_run refuses every prefix of at
    most one segment and so does the preview; with seg_weight_m0_sec = 0 every prefix of at least one frame has one."""
    cfg = pkg("css").CssCfg(seg_weight_m0_sec=m0)
    T, hop, _ = _frames(cfg)
    forced = (300, 16000, T * 256 + 511, T * 256 + 512, (T + hop) * 256 + 511, (T + hop) * 256 + 512)
    x = _clip(mix60, 6.0)
    assert forced[-1] < x.shape[0]
    sep = _sep(mc_state)
    cuts = _seeded_cuts(3, x.shape[0], forced)
    assert set(forced) <= set(cuts)
    ok = _push_preview_compare(sep, x, cfg, cuts)
    if m0:
        assert ok == [n for n in cuts if n >= T * 256 + 512] and len(ok) >= 3
    else:
        assert [n for n in ok if n >= 512] == [n for n in cuts if n >= 512]
    sep.close()


@pytest.mark.parametrize("case", ["default_30s", "seg2_14s"])
def test_preview_past_the_first_window_rebase(case, mc_state, mix60):
    """The window moves for the first time when the transformed frames no longer fit it: after more than 24 s with the default
    segmentation (run once, in 1.5 s ticks), after 10 s with 2 s / 0.5 s segments (seeded chunks).  Prefixes one sample short of
    that push and exactly at it are forced."""
    CSS, S = pkg("css"), pkg("stream")
    sep = _sep(mc_state)
    if case == "default_30s":
        cfg, x = CSS.CssCfg(), _clip(mix60, 30.0)
    else:
        cfg, x = CSS.CssCfg(segment_size_sec=2.0, hop_size_sec=0.5), _clip(mix60, 14.0)
    n_rb = _first_rebase_length(cfg)
    assert n_rb + 24000 < x.shape[0], n_rb
    if case == "default_30s":
        cuts = sorted(set(list(range(24000, x.shape[0] + 1, 24000)) + [n_rb - 1, n_rb]))
    else:
        cuts = _seeded_cuts(5, x.shape[0], (n_rb - 1, n_rb))
    ok = _push_preview_compare(sep, x, cfg, cuts, at_zero=False)
    assert n_rb - 1 in ok and n_rb in ok and max(ok) > n_rb
    sep.close()


def test_the_stream_does_not_move(mc_state, mix60):
    """Twin streams on one handle, one of them previewed after every push (once twice in a row, once with a css_run on the handle
    between the push and the preview): every push returns the same samples, the counters agree, both are css_run of the clip."""
    CSS, S = pkg("css"), pkg("stream")
    cfg = CSS.CssCfg()
    x, other = _clip(mix60, 12.0), _clip(mix60, 4.0, start=16000 * 20)
    sep = _sep(mc_state)
    ref, ref_other = _offline(sep, x, cfg), _offline(sep, other, cfg)
    cuts = _seeded_cuts(7, x.shape[0])
    twice_at, run_at = cuts[len(cuts) // 2], cuts[2 * len(cuts) // 3]
    a, b = S.CssStream(sep, cfg), S.CssStream(sep, cfg)
    oa, ob, n, previews = [], [], 0, 0
    for cut in cuts:
        ga, gb = np.stack(a.push(x[n:cut])), np.stack(b.push(x[n:cut]))
        n = cut
        assert np.array_equal(ga, gb)
        oa.append(ga); ob.append(gb)
        if cut == run_at:
            assert np.array_equal(_offline(sep, other, cfg), ref_other)
            assert _preview_is_css_run(sep, a, x, n, cfg)
        status, p1 = _try(a.preview)
        if cut == twice_at:
            status2, p2 = _try(a.preview)
            assert status2 == status == (None, None) and all(np.array_equal(u, v) for u, v in zip(p1, p2))
        previews += status == (None, None)
        ia, ib = a.info(), b.info()
        assert (ia.n_pushed, ia.n_emitted, ia.finished) == (ib.n_pushed, ib.n_emitted, ib.finished) == (n, a.final_samples(n), 0)
    assert previews >= len(cuts) // 2
    oa.append(np.stack(a.finish())); ob.append(np.stack(b.finish()))
    assert a.info().finished == b.info().finished == 1
    assert np.array_equal(np.concatenate(oa, axis=1), ref) and np.array_equal(np.concatenate(ob, axis=1), ref)
    a.close(); b.close()
    sep.close()


@pytest.mark.parametrize("knob", ["sc", "normalize", "sep_mse", "th03", "sqrt_hann"])
def test_preview_knobs_and_models(knob, mc_state, sc_state, mix60):
    CSS = pkg("css")
    x = _clip(mix60, 12.0)
    cfg = CSS.CssCfg()
    state = mc_state
    if knob == "sc":
        state, x = sc_state, np.ascontiguousarray(x[:, :1])
    elif knob == "normalize":
        cfg.normalize_segment_power = True
    elif knob == "sep_mse":
        cfg.stitching_input, cfg.stitching_loss = "separation_result", "mse"
    elif knob == "th03":
        cfg.activity_th = 0.3
    sep = _sep(state)
    if knob == "sqrt_hann":
        sep.handle.set_analysis_window("sqrt_hann")
    T = _frames(cfg, x.shape[1])[0]
    cuts = [T * 256 + 512, 100001, 150000, x.shape[0]]
    assert _push_preview_compare(sep, x, cfg, cuts, at_zero=False) == cuts
    sep.close()


def _raw_preview_many(sep, streams, caps=None, canary=7.5):
    """one css_stream_preview_many with canary-filled buffers -> (return code, items, buffers, stats)"""
    L = pkg("_lib")
    h = sep.handle
    items = (L.CssStreamPreview * len(streams))()
    bufs = []
    for i, (it, s) in enumerate(zip(items, streams)):   # (a bare int: an id no stream has)
        cap = s.latency_samples if caps is None else caps[i]
        buf = np.full((sep.desc.num_spks, max(cap, 1)), canary, np.float32)
        bufs.append(buf)
        it.id, it.out_host, it.cap, it.n_out, it.first_sample, it.status = (s if isinstance(s, int) else s.id), buf.ctypes.data, cap, -7, -7, 77
    stats = L.CssStreamGroupStats(-7, -7)
    rc = h.lib.css_stream_preview_many(h.h, items, len(streams), C.byref(stats))
    return rc, items, bufs, stats


def test_grouped_preview(mc_state, mix60):
    """18 streams of one separator (the table launches take 16 entries) at different lengths: one shorter than a segment plus a
    frame, two pushed as int16, two at 48 kHz.  One css_stream_preview_many: every item is the stream's own css_stream_preview
    and css_run of its prefix, the pending segments were one estimator batch, and the streams go on to css_run of their recordings."""
    L, CSS, S = pkg("_lib"), pkg("css"), pkg("stream")
    cfg = CSS.CssCfg()
    sep = _sep(mc_state)
    h = sep.handle
    N, total = 18, 96000
    streams, recs, inputs, pre, kinds = [], [], [], [], []
    for i in range(N):
        kind = "f32" if i not in (1, 2, 3, 4) else ("i16" if i < 3 else "r48")
        if kind == "r48":
            u = _clip(mix60, 3 * total / 16000, start=8000 * i)          # any samples, taken as 48 kHz
            s = S.CssStream(sep, cfg, input_rate=48000)
            rec, n_i = h.resample(u, 48000), (170000, 200001)[i - 3]
            x_pre = h.resample(u[:n_i], 48000)
        else:
            u = _clip(mix60, total / 16000, start=16000 * i)
            s = S.CssStream(sep, cfg)
            n_i = 40000 if i == 0 else 50000 + 2500 * i
            if kind == "i16":
                u = np.clip(np.round(u * 32767.0), -32768, 32767).astype(np.int16)
                rec = u.astype(np.float32) / np.float32(32768.0)
            else:
                rec = u
            x_pre = rec[:n_i]
        streams.append(s); recs.append(rec); inputs.append((u, n_i)); pre.append(x_pre); kinds.append(kind)
    T = _frames(cfg)[0]
    assert pre[0].shape[0] < T * 256 + 512 <= min(p.shape[0] for p in pre[1:])
    outs = [[] for _ in range(N)]
    for s, (u, n_i), o, kind in zip(streams, inputs, outs, kinds):
        o.append(np.stack(s.push_pcm16(u[:n_i]) if kind == "i16" else s.push(u[:n_i])))
    infos = [s.info() for s in streams]
    assert [inf.n_pushed for inf in infos[:3]] == [40000, 52500, 55000]
    rc, items, bufs, stats = _raw_preview_many(sep, streams)
    assert rc == L.CSS_OK
    assert (stats.estimator_batches, stats.estimator_segments) == (1, N - 1)
    assert (items[0].status, items[0].n_out) == (L.CSS_ERR_ZERO_WEIGHT, 0) and np.all(bufs[0] == 7.5)
    wrapped = S.CssStreamGroup(streams).preview()
    assert wrapped[0] is None
    for i in range(1, N):
        s, it, em = streams[i], items[i], infos[i].n_emitted
        assert (it.status, it.first_sample) == (L.CSS_OK, em)
        got = bufs[i][:, :it.n_out]
        assert np.all(bufs[i][:, it.n_out:] == 7.5)
        own = np.stack(s.preview())
        want = _offline(sep, pre[i], cfg)
        assert got.shape == own.shape == want[:, em:].shape, (i, kinds[i])
        assert np.array_equal(got, own) and np.array_equal(got, want[:, em:]), (i, kinds[i])
        assert np.array_equal(np.stack(wrapped[i]), got)
        after = s.info()
        assert (after.n_pushed, after.n_emitted, after.finished) == (infos[i].n_pushed, em, 0)
    for s, (u, n_i), o, kind, rec in zip(streams, inputs, outs, kinds, recs):
        o.append(np.stack(s.push_pcm16(u[n_i:]) if kind == "i16" else s.push(u[n_i:])))
        o.append(np.stack(s.finish()))
        assert np.array_equal(np.concatenate(o, axis=1), _offline(sep, rec, cfg)), kind
        s.close()
    sep.close()


def _toggling_cfg(sep, x, percentile=70):
    """test_hip_stream_handoff.py's recipe: a threshold at the 70th percentile of this model's activity on x, short dilation and
    erosion, so that the gate really toggles"""
    css, L = pkg("css"), pkg("_lib")
    h = sep.handle
    h.run(x, css.make_run_cfg(css.CssCfg(activity_th=0.0, show_progressbar=False), 16000, 7))
    th = float(np.percentile(h.read(L.BUF_ACTIVITY), percentile))
    return css.CssCfg(activity_th=th, show_progressbar=False, activity_dilation_sec=0.05, activity_erosion_sec=0.02)


def test_handoff_twin(mc_state, mix60):
    """Two streams with the hand-off on, one previewed after every push: every call's Handoff is equal, and the whole is
    Handle.handoff_logmel of the recording (as test_hip_stream_handoff.py states it)."""
    import torch
    CSS, S, L = pkg("css"), pkg("stream"), pkg("_lib")
    hcfg = dict(n_mels=80, pad_frames=8, drop_silence=True)
    x = _clip(mix60, 10.0)
    sep = _sep(mc_state)
    h = sep.handle
    cfg = _toggling_cfg(sep, x)
    a, b = S.CssStream(sep, cfg, handoff=hcfg), S.CssStream(sep, cfg, handoff=hcfg)
    calls, wav, previews = [], [], 0

    def same(p, q):
        for k in range(3):
            assert np.array_equal(p.mel[k], q.mel[k]) and np.array_equal(p.ranges[k], q.ranges[k]) and np.array_equal(p.activity[k], q.activity[k])
        assert np.array_equal(p.raw_max, q.raw_max) and p.first_activity_frame == q.first_activity_frame

    n = 0
    for cut in _seeded_cuts(11, x.shape[0], (24000, 48000, 72000, 96000, 120000, 144000)):
        ga, gb = np.stack(a.push(x[n:cut])), np.stack(b.push(x[n:cut]))
        n = cut
        assert np.array_equal(ga, gb)
        same(a.handoff, b.handoff)
        calls.append(a.handoff); wav.append(ga)
        kept = a.handoff
        previews += _try(a.preview)[0] == (None, None)
        assert a.handoff is kept                      # (a preview hands nothing off)
    assert previews >= 3
    ga, gb = np.stack(a.finish()), np.stack(b.finish())
    assert np.array_equal(ga, gb)
    same(a.handoff, b.handoff)
    calls.append(a.handoff); wav.append(ga)
    a.close(); b.close()
    # the whole against the offline call
    rc = CSS.make_run_cfg(cfg, 16000, 7)
    n_out = int(L.plan(sep.desc, rc, x.shape[0]).n_out)
    pcm = torch.from_numpy(x).cuda()
    dev = torch.empty((3, n_out), dtype=torch.float32, device="cuda")
    h.run_device(pcm.data_ptr(), x.shape[0], 7, rc, dev.data_ptr(), n_out)
    torch.cuda.synchronize()
    act = h.read(L.BUF_ACT_FINAL).copy()
    assert np.array_equal(np.concatenate(wav, axis=1), dev.cpu().numpy())
    for k in range(3):
        mel, regions = h.handoff_logmel(dev.data_ptr(), n_out, k, **hcfg)
        raw = np.concatenate([c.mel[k] for c in calls], axis=1)
        merged = []
        for lo, hi in np.concatenate([c.ranges[k] for c in calls]):
            if merged and lo <= merged[-1][1]:
                merged[-1][1] = max(merged[-1][1], int(hi))
            else:
                merged.append([int(lo), int(hi)])
        assert np.array_equal(np.array(merged, np.int64).reshape(-1, 2), regions)
        assert np.array_equal(np.concatenate([c.activity[k] for c in calls]), act[k])
        assert np.array_equal(S.whisper_normalize(raw, calls[-1].raw_max[k]), mel), k
    sep.close()


def test_refusals_change_nothing(mc_state, mix60):
    """cap one below the count, an id named twice, an unknown id, a finished stream, a queued session outstanding: the status,
    the buffers as they were, the stream as it was, and the next push equal to an unpreviewed twin's."""
    L, CSS, S = pkg("_lib"), pkg("css"), pkg("stream")
    cfg = CSS.CssCfg()
    x = _clip(mix60, 8.0)
    sep = _sep(mc_state)
    h = sep.handle
    a, b, done = S.CssStream(sep, cfg), S.CssStream(sep, cfg), S.CssStream(sep, cfg)
    n = 72000
    for s in (a, b, done):
        s.push(x[:n])
    done.finish()
    first, count = a.preview_samples(n)
    assert first == a.info().n_emitted and 0 < count <= a.latency_samples

    def state(s):
        inf = s.info()
        return inf.n_pushed, inf.n_emitted, inf.finished, inf.device_bytes

    def refused(streams, code, caps=None, text=None):
        before = state(a)
        rc, items, bufs, stats = _raw_preview_many(sep, streams, caps)
        assert rc == code
        assert all(np.all(buf == 7.5) for buf in bufs) and all((it.n_out, it.first_sample, it.status) == (-7, -7, 77) for it in items)
        assert state(a) == before
        if text is not None:
            msg = h.lib.css_last_error(h.h).decode()
            assert all(t in msg for t in text), msg

    free_id = next(i for i in range(L.MAX_STREAMS) if i not in (a.id, b.id, done.id))
    refused([a], L.CSS_ERR_INVALID_ARG, caps=[count - 1], text=("item 0", f"stream {a.id}"))
    refused([a, a], L.CSS_ERR_INVALID_ARG, text=("item 1", f"stream {a.id}"))
    refused([a, free_id], L.CSS_ERR_INVALID_ARG, caps=[a.latency_samples, 1000], text=("item 1", f"stream {free_id}"))
    refused([a, done], L.CSS_ERR_STATE, text=("item 1", f"stream {done.id}"))
    # the single form: the same refusals, its outputs untouched; exactly the count is enough
    buf = np.full((3, count), 7.5, np.float32)
    n_out, fs = C.c_int64(-7), C.c_int64(-7)
    ptr = buf.ctypes.data_as(C.c_void_p)
    assert h.lib.css_stream_preview(h.h, a.id, ptr, count - 1, C.byref(n_out), C.byref(fs)) == L.CSS_ERR_INVALID_ARG
    assert h.lib.css_stream_preview(h.h, a.id, None, count, C.byref(n_out), C.byref(fs)) == L.CSS_ERR_INVALID_ARG
    assert h.lib.css_stream_preview(h.h, a.id, ptr, count, None, C.byref(fs)) == L.CSS_ERR_INVALID_ARG
    assert h.lib.css_stream_preview(h.h, a.id, ptr, count, C.byref(n_out), None) == L.CSS_ERR_INVALID_ARG
    assert h.lib.css_stream_preview(h.h, done.id, ptr, count, C.byref(n_out), C.byref(fs)) == L.CSS_ERR_STATE
    assert (n_out.value, fs.value) == (-7, -7) and np.all(buf == 7.5)
    # a queued session outstanding
    rc_ = CSS.make_run_cfg(cfg, 16000, 7)
    q_in = L.pinned_copy(np.ascontiguousarray(x[:64000]))
    q_out = L.pinned_empty((3, L.plan(sep.desc, rc_, q_in.shape[0]).n_out))
    h.run_enqueue(q_in, rc_, q_out)
    refused([a], L.CSS_ERR_STATE)
    assert h.lib.css_stream_preview(h.h, a.id, ptr, count, C.byref(n_out), C.byref(fs)) == L.CSS_ERR_STATE
    assert (n_out.value, fs.value) == (-7, -7) and np.all(buf == 7.5)
    h.wait()
    assert h.lib.css_stream_preview(h.h, a.id, ptr, count, C.byref(n_out), C.byref(fs)) == L.CSS_OK
    assert (n_out.value, fs.value) == (count, first)
    assert np.array_equal(buf, _offline(sep, x[:n], cfg)[:, first:])
    for lo, hi in ((n, n + 24000), (n + 24000, x.shape[0])):
        assert np.array_equal(np.stack(a.push(x[lo:hi])), np.stack(b.push(x[lo:hi])))
    assert np.array_equal(np.stack(a.finish()), np.stack(b.finish()))
    for s in (a, b, done):
        s.close()
    sep.close()
