"""Previews with hand-off on the MI355X (include/css_mi355_preview_handoff.h; stream.py preview(handoff=True)): after n pushed
samples the preview returns what finish would return at this moment -- the waveforms and the hand-off's log-mel frames, kept
ranges and gate bits -- which, with everything the pushes returned, is css_handoff_logmel after css_run_device of the prefix;
and the stream afterwards is the stream it was.  Every comparison is np.array_equal.

The model is the 2-block multi-channel one of the stream tests, the recordings are synth_meeting's, and the gate follows the
hand-off tests' recipe: a threshold at the 70th percentile of the model's activity on the recording, dilation 0.05 s, erosion
0.02 s.  Recording seed 2 (12 s) was chosen because with this recipe the gate leaves a pause longer than 2 * 8 + 2 frames inside
the undecided span of most prefixes, so the pad-8 configuration has two provisional ranges there (asserted below)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

CHUNKS = (0, 1, 255, 256, 257, 4000, 24000, 32000)     # test_hip_stream_handoff.py's
CONFIGS = (dict(n_mels=80, pad_frames=8, drop_silence=True), dict(n_mels=128, pad_frames=0, drop_silence=True),
           dict(n_mels=80, pad_frames=8, drop_silence=False))
ZERO_WEIGHT_TEXT = "zero weights found"
SEED = 2


@pytest.fixture(scope="module")
def model():
    """the 2-block multi-channel model of test_hip_session.py's tiny_models"""
    w = pkg("weights")
    desc = w.ModelDesc(num_blocks=2)
    return w.apply_golden_recipe(w.portable_state_dict(desc, 21)), desc


def _sep(model):
    return pkg("separator").HipSeparator(model[0], None, device=0)


_RECS, _CFGS, _OFFLINE = {}, {}, {}


def _rec(seconds, seed):
    if (seconds, seed) not in _RECS:
        x = pkg("synth").synth_meeting(float(seconds), 7, seed=seed)
        _RECS[(seconds, seed)] = np.ascontiguousarray(x[0] if x.ndim == 3 else x, dtype=np.float32)
    return _RECS[(seconds, seed)]


def _toggling_cfg(sep, x, key, **kw):
    """the recipe: a threshold at the 70th percentile of this model's activity on x, dilation 0.05 s, erosion 0.02 s"""
    css, L = pkg("css"), pkg("_lib")
    if key not in _CFGS:
        h = sep.handle
        h.run(x, css.make_run_cfg(css.CssCfg(activity_th=0.0, show_progressbar=False, **kw), 16000, x.shape[1]))
        _CFGS[key] = float(np.percentile(h.read(L.BUF_ACTIVITY), 70))
    return css.CssCfg(activity_th=_CFGS[key], show_progressbar=False, activity_dilation_sec=0.05, activity_erosion_sec=0.02, **kw)


def _frames(cfg, ch=7):
    c = pkg("css").make_run_cfg(cfg, 16000, ch).c
    return c.segment_frames, c.hop_frames, c.dilation_frames + c.erosion_frames


def _offline(sep, x, cfg, key, configs=CONFIGS):
    """css_run_device on x -> (waveforms, gate bits, [per config: [(mel, regions) per stream]]); computed once per key"""
    import torch
    css, L = pkg("css"), pkg("_lib")
    if key not in _OFFLINE:
        h = sep.handle
        ch = x.shape[1]
        rc = css.make_run_cfg(cfg, 16000, ch)
        n_out = int(L.plan(sep.desc, rc, x.shape[0]).n_out)
        pcm = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        wav = torch.empty((3, n_out), dtype=torch.float32, device="cuda")
        h.run_device(pcm.data_ptr(), x.shape[0], ch, rc, wav.data_ptr(), n_out)
        torch.cuda.synchronize()
        act = h.read(L.BUF_ACT_FINAL).copy()
        res = [[h.handoff_logmel(wav.data_ptr(), n_out, k, **c) for k in range(3)] for c in configs]
        _OFFLINE[key] = (wav.cpu().numpy(), act, res)
    return _OFFLINE[key]


def _merged(ranges):
    out = []
    for a, b in ranges:
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], int(b))
        else:
            out.append([int(a), int(b)])
    return np.array(out, np.int64).reshape(-1, 2)


def _same(a, b):
    for k in range(3):
        assert np.array_equal(a.mel[k], b.mel[k]) and np.array_equal(a.ranges[k], b.ranges[k]) and np.array_equal(a.activity[k], b.activity[k])
    assert np.array_equal(a.raw_max, b.raw_max) and a.first_activity_frame == b.first_activity_frame


def _cuts(total, stops=()):
    """the chunk sizes cycled (the empty push included); a push that would pass one of `stops` ends there, so that the stream
    holds exactly that prefix once, and the cycle goes on"""
    out, n = [], 0
    for size in itertools.cycle(CHUNKS):
        if n >= total:
            return out
        nxt = min(n + size, total)
        for s in sorted(stops):
            if n < s < nxt:
                nxt = s
                break
        out.append(nxt)
        n = nxt


def _preview(s):
    """preview(handoff=True) -> (waveforms [S, n], Handoff), or None where css_run refuses the prefix; the last push's Handoff stays"""
    kept = s.handoff
    try:
        wav = np.stack(s.preview(handoff=True))
    except AssertionError as e:
        assert ZERO_WEIGHT_TEXT in str(e)
        assert s.handoff is kept
        return None
    assert s.handoff is kept
    return wav, s.preview_handoff


def _state(s):
    inf = s.info()
    return inf.n_pushed, inf.n_emitted, inf.finished, inf.device_bytes


def _against_offline(S, calls, wav_calls, pv_wav, pv, off, ci, hcfg, n_out):
    """what the pushes returned (calls) and the preview pv, against the offline call on the prefix -> most provisional ranges"""
    wav, act, res = off
    assert wav.shape[1] == n_out
    em = sum(w.shape[1] for w in wav_calls)
    assert np.array_equal(np.concatenate(wav_calls + [pv_wav], axis=1), wav)
    t_g = sum(c.activity[0].shape[0] for c in calls)
    assert pv.first_activity_frame == t_g and em == t_g * 256
    pad = hcfg["pad_frames"] if hcfg["drop_silence"] else 0
    D = max(t_g - pad, 0) * 256
    most = 0
    for k in range(3):
        mel, regions = res[ci][k]
        assert np.array_equal(np.concatenate([c.activity[k] for c in calls] + [pv.activity[k]]), act[k])
        r = pv.ranges[k]
        assert (r[:, 0] < r[:, 1]).all() and (r[1:, 0] > r[:-1, 1]).all() and (r.size == 0 or (r[0, 0] >= D and r[-1, 1] <= n_out))
        if not hcfg["drop_silence"]:
            assert np.array_equal(r, np.array([[D, n_out]], np.int64))
        assert np.array_equal(_merged(np.concatenate([c.ranges[k] for c in calls] + [r])), regions)
        raw = np.concatenate([c.mel[k] for c in calls] + [pv.mel[k]], axis=1)
        assert pv.first_frame[k] == sum(c.mel[k].shape[1] for c in calls)
        assert raw.shape[1] == int((regions[:, 1] - regions[:, 0]).sum()) // 160 == mel.shape[1]
        if raw.size:
            assert pv.raw_max[k] == raw.max()
        assert np.array_equal(S.whisper_normalize(raw, pv.raw_max[k]), mel), (ci, k)
        most = max(most, len(r))
    return most


@pytest.mark.parametrize("ci", range(len(CONFIGS)))
def test_equals_the_offline_handoff_of_the_prefix(ci, model):
    """The chunk sizes cycled, a preview with hand-off after every push; at the first prefix with K > T, one mid-segment, a
    segment boundary - 1 / the boundary / + 1 sample, and the last push: pushes + preview = run_device + handoff_logmel of
    recording[:n].  In the drop configurations at least one compared preview has two provisional ranges for some stream, that is
    a dropped block inside [D, n_out)."""
    S = pkg("stream")
    hcfg = CONFIGS[ci]
    sep = _sep(model)
    x = _rec(12.0, SEED)
    cfg = _toggling_cfg(sep, x, ("mc", 12.0, SEED))
    T, hop, _ = _frames(cfg)
    first, mid, bound = T * 256 + 512, (T + hop) * 256 + 512 + hop * 128, (T + 3 * hop) * 256 + 512
    compared = (first, mid, bound - 1, bound, bound + 1, x.shape[0])
    cuts = _cuts(x.shape[0], compared)
    assert set(compared) <= set(cuts) and 0 in cuts
    most, n, calls, wavs, done = 0, 0, [], [], []
    with S.CssStream(sep, cfg, handoff=hcfg) as s:
        for cut in cuts:
            wavs.append(np.stack(s.push(x[n:cut])))
            calls.append(s.handoff)
            n = cut
            before = _state(s)
            got = _preview(s)
            assert _state(s)[:3] == before[:3]
            assert (got is None) == (n < first), n
            if n in compared and n not in done:
                done.append(n)
                off = _offline(sep, x[:n], cfg, ("mc", 12.0, SEED, n))
                most = max(most, _against_offline(S, calls, wavs, got[0], got[1], off, ci, hcfg, off[0].shape[1]))
    assert tuple(done) == compared
    print(hcfg, "most provisional ranges of a stream in a compared preview:", most)
    if hcfg["drop_silence"]:
        assert most >= 2
    sep.close()


def test_equals_finish(model):
    """At three prefixes a twin pushed identically and then finished returns, in its Handoff, the previewed stream's
    preview_handoff, and the same waveforms."""
    S = pkg("stream")
    hcfg = CONFIGS[0]
    sep = _sep(model)
    x = _rec(12.0, SEED)
    cfg = _toggling_cfg(sep, x, ("mc", 12.0, SEED))
    T, hop, _ = _frames(cfg)
    at = ((T + hop) * 256 + 512 + hop * 128, (T + 3 * hop) * 256 + 512, x.shape[0])
    cuts = _cuts(x.shape[0], at)
    seen, n = {}, 0
    with S.CssStream(sep, cfg, handoff=hcfg) as s:
        for cut in cuts:
            s.push(x[n:cut])
            n = cut
            got = _preview(s)
            if n in at:
                seen[n] = got
    assert sorted(seen) == sorted(at)
    for stop in at:
        with S.CssStream(sep, cfg, handoff=hcfg) as twin:
            n = 0
            for cut in cuts:
                if cut > stop:
                    break
                twin.push(x[n:cut])
                n = cut
            assert n == stop
            wav = np.stack(twin.finish())
            pv_wav, pv = seen[stop]
            assert np.array_equal(wav, pv_wav)
            _same(twin.handoff, pv)
            assert sum(m.shape[1] for m in pv.mel) > 0 and pv.activity[0].shape[0] > 0
    sep.close()


def _twins(sep, x, cfg, hcfg, cuts, check_from=None, key=None, ci=0):
    """a stream previewed with hand-off after every push against its never-previewed twin, push by push and at finish; the
    whole against the offline call on the recording.  check_from: previews at prefixes from there on also against the offline
    call of the prefix (at most two of them)."""
    S = pkg("stream")
    a, b = S.CssStream(sep, cfg, handoff=hcfg), S.CssStream(sep, cfg, handoff=hcfg)
    calls, wavs, n, previews, settled, checked = [], [], 0, 0, None, 0
    for cut in cuts:
        ga, gb = np.stack(a.push(x[n:cut])), np.stack(b.push(x[n:cut]))
        n = cut
        assert np.array_equal(ga, gb)
        _same(a.handoff, b.handoff)
        calls.append(a.handoff); wavs.append(ga)
        got = _preview(a)
        assert _state(a)[:3] == _state(b)[:3]
        if got is not None:
            previews += 1
            if settled is None:
                settled = _state(a)[3]                       # (the output buffer may have grown to the preview's length, once)
            assert _state(a)[3] == settled
            if check_from is not None and n >= check_from and checked < 2 and cut != cuts[-1]:
                off = _offline(sep, x[:n], cfg, key + (n,), (hcfg,))
                _against_offline(S, calls, wavs, got[0], got[1], off, 0, hcfg, off[0].shape[1])
                checked += 1
    assert previews >= len(cuts) // 2 and (check_from is None or checked == 2)
    ga, gb = np.stack(a.finish()), np.stack(b.finish())
    assert np.array_equal(ga, gb)
    _same(a.handoff, b.handoff)
    calls.append(a.handoff); wavs.append(ga)
    assert _state(a)[:3] == _state(b)[:3] and a.info().finished == 1
    a.close(); b.close()
    return calls, wavs


@pytest.mark.parametrize("ci", range(len(CONFIGS)))
def test_the_stream_does_not_move(ci, model):
    S = pkg("stream")
    hcfg = CONFIGS[ci]
    sep = _sep(model)
    x = _rec(12.0, SEED)
    cfg = _toggling_cfg(sep, x, ("mc", 12.0, SEED))
    calls, wavs = _twins(sep, x, cfg, hcfg, _cuts(x.shape[0]))
    wav, act, res = _offline(sep, x, cfg, ("mc", 12.0, SEED, x.shape[0]))
    assert np.array_equal(np.concatenate(wavs, axis=1), wav)
    for k in range(3):
        mel, regions = res[ci][k]
        raw = np.concatenate([c.mel[k] for c in calls], axis=1)
        assert np.array_equal(np.concatenate([c.activity[k] for c in calls]), act[k])
        assert np.array_equal(_merged(np.concatenate([c.ranges[k] for c in calls])), regions)
        assert np.array_equal(S.whisper_normalize(raw, calls[-1].raw_max[k]), mel), k
    sep.close()


def test_past_a_window_rebase(model):
    """2 s / 0.5 s segments, 34 s: the window has moved many times (first after 10 s) when the previews after 30 s are compared
    with the offline call of their prefixes; the twin never sees a difference, and the whole is the offline call."""
    S = pkg("stream")
    hcfg = CONFIGS[0]
    sep = _sep(model)
    x = _rec(34.0, SEED)
    cfg = _toggling_cfg(sep, x, ("mc-2s", 34.0, SEED), segment_size_sec=2.0, hop_size_sec=0.5)
    T, hop, halo = _frames(cfg)
    assert ((2 * T + 2 * halo + 11 * hop + 16 + 3) // 4 * 4) * 256 + 512 < 11 * 16000      # the window a stream opens with
    cuts = sorted(set(list(range(24000, x.shape[0], 24000)) + [30 * 16000 + 257, 31 * 16000 + 4001, x.shape[0]]))
    calls, wavs = _twins(sep, x, cfg, hcfg, cuts, check_from=30 * 16000, key=("mc-2s", 34.0, SEED))
    wav, act, res = _offline(sep, x, cfg, ("mc-2s", 34.0, SEED, x.shape[0]), (hcfg,))
    assert np.array_equal(np.concatenate(wavs, axis=1), wav)
    for k in range(3):
        mel, regions = res[0][k]
        raw = np.concatenate([c.mel[k] for c in calls], axis=1)
        assert np.array_equal(np.concatenate([c.activity[k] for c in calls]), act[k])
        assert np.array_equal(_merged(np.concatenate([c.ranges[k] for c in calls])), regions)
        assert np.array_equal(S.whisper_normalize(raw, calls[-1].raw_max[k]), mel), k
    sep.close()


def _raw_out(n_mels, caps, S_=3):
    L = pkg("_lib")
    keep = dict(mel=np.full((S_, n_mels, max(caps[0], 1)), 7.5, np.float32), ranges=np.full((S_, max(caps[1], 1), 2), -7, np.int64),
                act=np.full((S_, max(caps[2], 1)), 9, np.uint8), nf=np.full(S_, -7, np.int64), nr=np.full(S_, -7, np.int32),
                mx=np.full(S_, 7.5, np.float32), first=np.full(S_, -7, np.int64))
    o = L.CssStreamHandoffOut()
    o.mel_host, o.cap_frames = keep["mel"].ctypes.data, caps[0]
    o.ranges_host, o.cap_ranges = keep["ranges"].ctypes.data, caps[1]
    o.activity_host, o.cap_activity = keep["act"].ctypes.data, caps[2]
    o.n_frames, o.n_ranges, o.raw_max = keep["nf"].ctypes.data, keep["nr"].ctypes.data, keep["mx"].ctypes.data
    o.n_activity, o.first_activity_frame = -7, -7
    return o, keep


def _untouched(o, keep):
    return bool(np.all(keep["mel"] == 7.5) and np.all(keep["ranges"] == -7) and np.all(keep["act"] == 9) and np.all(keep["nf"] == -7) and
                np.all(keep["nr"] == -7) and np.all(keep["mx"] == 7.5) and np.all(keep["first"] == -7) and
                (o.n_activity, o.first_activity_frame) == (-7, -7))


def _raw_many(sep, entries):
    """one css_stream_preview_handoff_many; entries: (stream, hand-off outputs (o, keep) or None, first_frame given) ->
    (return code, items, waveform buffers, stats)"""
    L = pkg("_lib")
    h = sep.handle
    items = (L.CssStreamPreviewHandoff * len(entries))()
    bufs = []
    for it, (s, ho, with_first) in zip(items, entries):
        buf = np.full((3, max(s.latency_samples, 1)), 7.5, np.float32)
        bufs.append(buf)
        it.p.id, it.p.out_host, it.p.cap, it.p.n_out, it.p.first_sample, it.p.status = s.id, buf.ctypes.data, buf.shape[1], -7, -7, 77
        if ho is not None:
            it.ho = C.pointer(ho[0])
            it.first_frame = ho[1]["first"].ctypes.data if with_first else None
    stats = L.CssStreamGroupStats(-7, -7)
    rc = h.lib.css_stream_preview_handoff_many(h.h, items, len(entries), C.byref(stats))
    return rc, items, bufs, stats


def _as_handoff(S, o, keep):
    nf, nr, na = keep["nf"], keep["nr"], int(o.n_activity)
    return S.Handoff([keep["mel"][k, :, :nf[k]] for k in range(3)], [keep["ranges"][k, :nr[k]] for k in range(3)],
                     [keep["act"][k, :na] for k in range(3)], keep["mx"], int(o.first_activity_frame), keep["first"])


def test_grouped(model):
    """18 streams of one handle in one call: sixteen served with hand-off outputs (two of them pushed as int16, one at 48 kHz),
    one with the hand-off off and ho == NULL, one with the hand-off on that is still too short to preview.  Every item is its own
    single call; one estimator batch of 17 segments; 3 hand-off launches, one of them the product."""
    L, S = pkg("_lib"), pkg("stream")
    sep = _sep(model)
    h = sep.handle
    base = [_rec(12.0, SEED), _rec(12.0, SEED + 1)]
    cfg = _toggling_cfg(sep, base[0], ("mc", 12.0, SEED))
    T = _frames(cfg)[0]
    variants = [CONFIGS[0], CONFIGS[1], CONFIGS[2], dict(n_mels=128, pad_frames=3, drop_silence=True)]
    N, OFF, SHORT, I16, R48 = 18, 7, 0, (1, 2), 3
    streams, hcfgs = [], []
    for i in range(N):
        hcfg = None if i == OFF else variants[i % 4]
        s = S.CssStream(sep, cfg, handoff=hcfg, input_rate=48000 if i == R48 else None)
        x = base[i % 2]
        if i == R48:
            u = x[:170001]                                          # any samples, taken as 48 kHz: 56667 at the model rate
        else:
            start = 4000 * i
            u = x[start:start + (40000 if i == SHORT else 50000 + 2500 * i)]
        if i in I16:
            s.push_pcm16(np.clip(np.round(u * 32767.0), -32768, 32767).astype(np.int16))
        else:
            s.push(u)
        streams.append(s); hcfgs.append(hcfg)
    assert streams[SHORT].info().n_pushed < T * 256 + 512 <= min(s.info().n_pushed for s in streams[1:])
    outs = [None if c is None else _raw_out(c["n_mels"], s.handoff_bounds(-1)) for s, c in zip(streams, hcfgs)]
    before = [_state(s) for s in streams]
    last = [s.handoff for s in streams]
    rc, items, bufs, stats = _raw_many(sep, [(s, o, True) for s, o in zip(streams, outs)])
    assert rc == L.CSS_OK
    assert (stats.estimator_batches, stats.estimator_segments) == (1, N - 1)
    launches, products, frames = h.stream_handoff_stats()
    assert (launches, products) == (3, 1) and frames > 0
    assert (items[SHORT].p.status, items[SHORT].p.n_out) == (L.CSS_ERR_ZERO_WEIGHT, 0)
    assert np.all(bufs[SHORT] == 7.5) and _untouched(*outs[SHORT])
    wrapped = S.CssStreamGroup(streams).preview(handoff=True)
    group_pv = [s.preview_handoff for s in streams]
    assert wrapped[SHORT] is None and group_pv[SHORT] is None and group_pv[OFF] is None
    emitted = 0
    for i in range(1, N):
        s, it = streams[i], items[i]
        assert (it.p.status, it.p.first_sample) == (L.CSS_OK, before[i][1])
        got = bufs[i][:, :it.p.n_out]
        assert np.all(bufs[i][:, it.p.n_out:] == 7.5)
        assert np.array_equal(np.stack(wrapped[i]), got)
        if i == OFF:
            assert np.array_equal(np.stack(s.preview()), got)
            with pytest.raises(ValueError):
                s.preview(handoff=True)
        else:
            own = np.stack(s.preview(handoff=True))
            assert np.array_equal(own, got)
            mine = _as_handoff(S, *outs[i])
            _same(mine, s.preview_handoff)
            _same(mine, group_pv[i])
            assert np.array_equal(mine.first_frame, s.preview_handoff.first_frame) and np.array_equal(mine.first_frame, group_pv[i].first_frame)
            assert np.array_equal(mine.first_frame, [sum(m.shape[1] for m in [last[i].mel[k]]) for k in range(3)])   # (one push so far)
            emitted += sum(m.shape[1] for m in mine.mel)
        assert _state(s)[:3] == before[i][:3] and s.handoff is last[i]
    assert emitted > 0
    for s in streams:
        s.close()
    sep.close()


def test_refusals_change_nothing(model):
    """Each refused call leaves its outputs and the stream as they were, and the push that follows equals the twin's."""
    L, CSS, S = pkg("_lib"), pkg("css"), pkg("stream")
    hcfg = CONFIGS[0]
    sep = _sep(model)
    h = sep.handle
    x = _rec(12.0, SEED)
    cfg = _toggling_cfg(sep, x, ("mc", 12.0, SEED))
    a, b, done = (S.CssStream(sep, cfg, handoff=hcfg) for _ in range(3))
    plain = S.CssStream(sep, cfg)
    n = 72000
    for s in (a, b, done, plain):
        s.push(x[:n])
    done.finish()
    need = a.handoff_bounds(-1)
    pos = [n]

    def next_push_equals_the_twins():
        lo, hi = pos[0], pos[0] + 8000
        assert np.array_equal(np.stack(a.push(x[lo:hi])), np.stack(b.push(x[lo:hi])))
        _same(a.handoff, b.handoff)
        pos[0] = hi

    def refused(entries, code, text=None):
        before = [_state(e[0]) for e in entries]
        rc, items, bufs, stats = _raw_many(sep, entries)
        assert rc == code
        assert all(np.all(buf == 7.5) for buf in bufs) and all((it.p.n_out, it.p.first_sample, it.p.status) == (-7, -7, 77) for it in items)
        assert all(e[1] is None or _untouched(*e[1]) for e in entries)
        assert [_state(e[0]) for e in entries] == before
        if text is not None:
            msg = h.lib.css_last_error(h.h).decode()
            assert all(t in msg for t in text), msg
        next_push_equals_the_twins()

    # hand-off outputs for a stream whose hand-off is off
    refused([(a, _raw_out(80, need), True), (plain, _raw_out(80, need), True)], L.CSS_ERR_STATE, ("item 1", f"stream {plain.id}"))
    # one frame / one range / one gate byte below the bound of finish
    for short in range(3):
        caps = [c - (1 if i == short else 0) for i, c in enumerate(need)]
        refused([(a, _raw_out(80, caps), True)], L.CSS_ERR_INVALID_ARG, ("item 0", f"stream {a.id}", "css_stream_handoff_bounds"))
    # an id named twice; a finished stream; no first_frame; a required array missing
    refused([(a, _raw_out(80, need), True), (a, _raw_out(80, need), True)], L.CSS_ERR_INVALID_ARG, ("item 1", f"stream {a.id}"))
    refused([(a, _raw_out(80, need), True), (done, _raw_out(80, need), True)], L.CSS_ERR_STATE, ("item 1", f"stream {done.id}"))
    refused([(a, _raw_out(80, need), False)], L.CSS_ERR_INVALID_ARG, ("item 0", "first_frame"))
    o, keep = _raw_out(80, need)
    o.raw_max = None
    refused([(a, (o, keep), True)], L.CSS_ERR_INVALID_ARG, ("item 0",))
    # the single form: NULL hand-off outputs / first_frame
    o, keep = _raw_out(80, need)
    buf = np.full((3, a.latency_samples), 7.5, np.float32)
    n_out, fs = C.c_int64(-7), C.c_int64(-7)
    ptr, ff = buf.ctypes.data_as(C.c_void_p), keep["first"].ctypes.data_as(C.c_void_p)
    single = lambda ho, first: h.lib.css_stream_preview_handoff(h.h, a.id, ptr, buf.shape[1], C.byref(n_out), C.byref(fs), ho, first)
    assert single(C.byref(o), None) == L.CSS_ERR_INVALID_ARG and single(None, ff) == L.CSS_ERR_INVALID_ARG
    assert (n_out.value, fs.value) == (-7, -7) and np.all(buf == 7.5) and _untouched(o, keep)
    next_push_equals_the_twins()
    # queued sessions outstanding
    rc_ = CSS.make_run_cfg(cfg, 16000, 7)
    q_in = L.pinned_copy(np.ascontiguousarray(x[:64000]))
    q_out = L.pinned_empty((3, L.plan(sep.desc, rc_, q_in.shape[0]).n_out))
    h.run_enqueue(q_in, rc_, q_out)
    before = _state(a)
    rc, items, bufs, stats = _raw_many(sep, [(a, (o, keep), True)])
    assert rc == L.CSS_ERR_STATE and np.all(bufs[0] == 7.5) and _untouched(o, keep) and _state(a) == before
    assert single(C.byref(o), ff) == L.CSS_ERR_STATE and _untouched(o, keep)
    h.wait()
    next_push_equals_the_twins()
    # exactly the bound is enough, and a stream with the hand-off on is served without outputs as css_stream_preview serves it
    assert single(C.byref(o), ff) == L.CSS_OK and n_out.value > 0 and fs.value == a.info().n_emitted
    assert np.array_equal(buf[:, :n_out.value], np.stack(a.preview(handoff=True)))
    _same(_as_handoff(S, o, keep), a.preview_handoff)
    rc, items, bufs, stats = _raw_many(sep, [(a, None, True)])
    assert rc == L.CSS_OK and np.array_equal(bufs[0][:, :items[0].p.n_out], np.stack(a.preview()))
    while pos[0] < x.shape[0]:
        next_push_equals_the_twins()
    assert np.array_equal(np.stack(a.finish()), np.stack(b.finish()))
    _same(a.handoff, b.handoff)
    for s in (a, b, done, plain):
        s.close()
    sep.close()


def test_single_channel_model():
    """the 1-block single-channel model of test_hip_session.py's tiny_models, one prefix"""
    w, S = pkg("weights"), pkg("stream")
    desc = w.ModelDesc(num_mics=1, in_features=257, num_blocks=1)
    sep = pkg("separator").HipSeparator(w.portable_state_dict(desc, 22), None, device=0)
    hcfg = CONFIGS[1]
    x = np.ascontiguousarray(_rec(12.0, SEED)[:, :1])
    cfg = _toggling_cfg(sep, x, ("sc", 12.0, SEED))
    n, calls, wavs = 0, [], []
    with S.CssStream(sep, cfg, num_channels=1, handoff=hcfg) as s:
        for cut in (24000, 72001, 130000):
            wavs.append(np.stack(s.push(x[n:cut])))
            calls.append(s.handoff)
            n = cut
        got = _preview(s)
        off = _offline(sep, x[:n], cfg, ("sc", 12.0, SEED, n), (hcfg,))
        _against_offline(S, calls, wavs, got[0], got[1], off, 0, hcfg, off[0].shape[1])
    sep.close()


def test_no_drop_ignores_pad_frames(model):
    """drop_silence off with pad_frames = 64: nothing waits for the gate, so D = t_g * 256 and the one provisional range is
    [D, n_out) (asserted in _against_offline with pad taken as 0), one prefix"""
    S = pkg("stream")
    hcfg = dict(n_mels=128, pad_frames=64, drop_silence=False)
    sep = _sep(model)
    x = _rec(12.0, SEED)
    cfg = _toggling_cfg(sep, x, ("mc", 12.0, SEED))
    n, calls, wavs = 0, [], []
    with S.CssStream(sep, cfg, handoff=hcfg) as s:
        for cut in (24000, 72001, 130000):
            wavs.append(np.stack(s.push(x[n:cut])))
            calls.append(s.handoff)
            n = cut
        got = _preview(s)
        off = _offline(sep, x[:n], cfg, ("mc", 12.0, SEED, n, "nodrop64"), (hcfg,))
        _against_offline(S, calls, wavs, got[0], got[1], off, 0, hcfg, off[0].shape[1])
        assert got[1].ranges[0][0, 0] == s.info().n_emitted
    sep.close()
