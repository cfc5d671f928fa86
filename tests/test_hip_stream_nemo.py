"""The NeMo hand-off of streamed sessions on the MI355X (css_stream_nemo_*, stream.py CssStream(nemo=...)): with every push a stream
returns the raw NeMo log-mel frames, the kept sample ranges and the gate bits that became final, and what the calls returned, put
together, is what css_handoff_nemo_all(normalize = 0) returns after css_run_device on the whole recording -- bit for bit, over any
cutting into pushes.  Every comparison is np.array_equal unless it says otherwise.  The 2-block model and the toggling-gate recipe
are tests/test_hip_stream_handoff.py's."""
import ctypes as C
import itertools

import numpy as np
import pytest

import nemo_reference as N
from conftest import pkg

pytestmark = pytest.mark.gpu

CHUNKS = (0, 1, 255, 256, 257, 4000, 24000, 32000)
CONFIGS = (dict(n_mels=80, pad_frames=8, drop_silence=True, preemphasis=0.97), dict(n_mels=128, pad_frames=0, drop_silence=True, preemphasis=0.97),
           dict(n_mels=80, pad_frames=8, drop_silence=False, preemphasis=0.97))


@pytest.fixture(scope="module")
def model():
    w = pkg("weights")
    desc = w.ModelDesc(num_blocks=2)
    return w.apply_golden_recipe(w.portable_state_dict(desc, 21)), desc


@pytest.fixture(scope="module")
def sep(model):
    s = pkg("separator").HipSeparator(model[0], None, device=0)
    yield s
    s.close()


def _rec(seconds, seed):
    x = pkg("synth").synth_meeting(float(seconds), 7, seed=seed)
    return np.ascontiguousarray(x[0] if x.ndim == 3 else x, dtype=np.float32)


def _toggling_cfg(sep, x, percentile=95):
    """a threshold at a percentile of this model's activity on x, dilation 0.05 s, erosion 0.02 s: the gate really toggles, and at
    the 95th percentile its pauses outlast 2 pad + 2 frames, so that the padded configurations drop too"""
    css, L = pkg("css"), pkg("_lib")
    h = sep.handle
    h.run(x, css.make_run_cfg(css.CssCfg(activity_th=0.0, show_progressbar=False), 16000, 7))
    th = float(np.percentile(h.read(L.BUF_ACTIVITY), percentile))
    return css.CssCfg(activity_th=th, show_progressbar=False, activity_dilation_sec=0.05, activity_erosion_sec=0.02)


_SHARED = {}


def _main(sep):
    """the main recording (10 s), its configuration and the offline results, computed once: (x, cfg, wav, act, {ci: NemoHandoff})"""
    if "main" not in _SHARED:
        import torch
        css, L = pkg("css"), pkg("_lib")
        x = _rec(10.0, 12)
        cfg = _toggling_cfg(sep, x)
        h = sep.handle
        rc = css.make_run_cfg(cfg, 16000, 7)
        n_out = int(L.plan(sep.desc, rc, x.shape[0]).n_out)
        pcm = torch.from_numpy(x).cuda()
        wav = torch.empty((3, n_out), dtype=torch.float32, device="cuda")
        h.run_device(pcm.data_ptr(), x.shape[0], 7, rc, wav.data_ptr(), n_out)
        torch.cuda.synchronize()
        act = h.read(L.BUF_ACT_FINAL).copy()
        off = {}
        for ci, c in enumerate(CONFIGS):
            o = h.handoff_nemo_all(wav.data_ptr(), n_out, normalize=False, **c)
            off[ci] = ([m.copy() for m in o.mel], [r.copy() for r in o.ranges])
        w = wav.cpu().numpy()
        for a in [x, w, act]:
            a.setflags(write=False)
        _SHARED["main"] = (x, cfg, w, act, off)
    return _SHARED["main"]


def _merged(ranges):
    out = []
    for a, b in ranges:
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], int(b))
        else:
            out.append([int(a), int(b)])
    return np.array(out, np.int64).reshape(-1, 2)


class _Run:
    """one stream with the NeMo hand-off on: pushes, keeps every call's results, checks what holds for every call"""

    def __init__(self, sep, cfg, ncfg, **kw):
        self.s = pkg("stream").CssStream(sep, cfg, nemo=ncfg, **kw)
        self.ncfg, self.calls, self.wav, self.n = ncfg, [], [], 0

    def took(self, wav, n, finished=False):
        h = self.s.nemo
        self.n += n
        assert self.s.handoff is None and h.raw_max is None
        for k in range(3):
            assert h.mel[k].shape[0] == self.ncfg["n_mels"] and h.mel[k].dtype == np.float32 and np.isfinite(h.mel[k]).all()
            r = h.ranges[k]
            assert (r[:, 0] < r[:, 1]).all() and (r[1:, 0] > r[:-1, 1]).all()
            assert h.first_frame[k] == sum(c.mel[k].shape[1] for c in self.calls)
        assert h.first_activity_frame == sum(c.activity[0].shape[0] for c in self.calls)
        if not self.ncfg["drop_silence"] and not finished:
            assert sum(c.mel[0].shape[1] for c in self.calls) + h.mel[0].shape[1] == self.s.nemo_final_frames(self.n)
        self.calls.append(h)
        self.wav.append(np.stack(wav))

    def push(self, chunk):
        self.took(self.s.push(chunk), chunk.shape[0])

    def finish(self):
        self.took(self.s.finish(), 0, True)

    def feed(self, x, sizes):
        n = 0
        for size in sizes:
            if n >= x.shape[0]:
                break
            self.push(x[n:n + size])
            n += size
        self.finish()
        return self

    def total(self, k):
        return (np.concatenate([c.mel[k] for c in self.calls], axis=1), _merged(np.concatenate([c.ranges[k] for c in self.calls])),
                np.concatenate([c.activity[k] for c in self.calls]))


def _same(a, b):
    for k in range(3):
        assert np.array_equal(a.mel[k], b.mel[k]) and np.array_equal(a.ranges[k], b.ranges[k]) and np.array_equal(a.activity[k], b.activity[k])
        assert a.first_frame[k] == b.first_frame[k]
    assert a.first_activity_frame == b.first_activity_frame


def _same_runs(a, b):
    assert len(a.calls) == len(b.calls)
    for ca, cb, wa, wb in zip(a.calls, b.calls, a.wav, b.wav):
        _same(ca, cb)
        assert np.array_equal(wa, wb)


# ---- 1. the main comparison ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ci", range(3), ids=lambda ci: "-".join(f"{v}" for v in CONFIGS[ci].values()))
@pytest.mark.parametrize("cut", ("cycled", "ticks"))
def test_streamed_equals_offline(sep, ci, cut):
    x, cfg, wav, act, off = _main(sep)
    ncfg = CONFIGS[ci]
    mel, regions = off[ci]
    n_out = wav.shape[1]
    assert 0.02 < act.astype(bool).mean() < 0.95
    print(ncfg, "ranges per speaker", [len(r) for r in regions], "kept share", [float((r[:, 1] - r[:, 0]).sum()) / n_out for r in regions])
    if ncfg["drop_silence"]:
        assert max(len(r) for r in regions) >= 3      # the seam path is on: a speaker's concatenation has at least two seams
    run = _Run(sep, cfg, ncfg).feed(x, itertools.cycle(CHUNKS) if cut == "cycled" else itertools.repeat(24000))
    run.s.close()
    assert np.array_equal(np.concatenate(run.wav, axis=1), wav)
    for k in range(3):
        raw, ranges, a = run.total(k)
        assert np.array_equal(a, act[k])
        assert np.array_equal(ranges, regions[k])
        assert raw.shape[1] == int((regions[k][:, 1] - regions[k][:, 0]).sum()) // 160 == mel[k].shape[1]
        assert np.array_equal(raw, mel[k]), (ci, cut, k)
    assert sum(m.shape[1] for m in mel) > 0


# ---- 2. the frames against the definition -------------------------------------------------------------------------------------------

def test_frames_against_the_float64_definition(sep):
    """the drop-silence configuration's concatenated frames within tests/nemo_reference.py's counted bound of the float64
    definition on the stream's own kept samples; no element is left out"""
    x, cfg, wav, act, off = _main(sep)
    ncfg = CONFIGS[0]
    run = _Run(sep, cfg, ncfg).feed(x, itertools.repeat(24000))
    run.s.close()
    seen = 0
    for k in range(3):
        raw, ranges, _ = run.total(k)
        ref = N.reference(wav[k], ranges, ncfg["n_mels"], ncfg["preemphasis"], normalize=False)
        assert ref.raw.shape == raw.shape
        if raw.size == 0:
            continue
        err = np.abs(raw.astype(np.float64) - ref.raw)
        print("speaker", k, "frames", raw.shape[1], "largest error / bound", float((err / ref.bound).max()))
        assert (err <= ref.bound).all()
        seen += raw.size
    assert seen > 0


# ---- 3. groups ----------------------------------------------------------------------------------------------------------------------

def test_group_of_three_kinds(sep):
    """one NeMo, one Whisper and one plain stream in one group: each call returns what the stream's solo twin returns, and a round
    costs 3 hand-off launches per format present"""
    S = pkg("stream")
    x, cfg, wav, act, off = _main(sep)
    whisper = dict(n_mels=80, pad_frames=3, drop_silence=True)
    mk = lambda: (S.CssStream(sep, cfg, nemo=CONFIGS[1]), S.CssStream(sep, cfg, handoff=whisper), S.CssStream(sep, cfg))
    grouped, solo = mk(), mk()
    group = S.CssStreamGroup(grouped)
    formats_seen = set()
    for n in range(0, x.shape[0], 24000):
        chunk = x[n:n + 24000]
        # (the Whisper stream sits out one tick, the NeMo stream another: rounds with one format and with both)
        part = [None if (i == 1 and n == 48000) or (i == 0 and n == 72000) else chunk for i in range(3)]
        res = group.push(part)
        launches, products, _ = sep.handle.stream_handoff_stats()
        took = [(grouped[0].nemo if part[0] is not None else None), (grouped[1].handoff if part[1] is not None else None)]
        n_formats = sum(1 for t in took if t is not None and t.activity[0].shape[0] > 0)
        # a tick of 1.5 s is one round: 3 launches per format that has a stream in its hand-off, one of them the product
        assert (launches, products) == (3 * n_formats, n_formats), (n, launches, products, n_formats)
        formats_seen.add(n_formats)
        for i in range(3):
            if part[i] is None:
                continue
            alone = solo[i].push(chunk)
            assert np.array_equal(np.stack(res[i]), np.stack(alone))
            if i == 0:
                _same(grouped[0].nemo, solo[0].nemo)
            if i == 1:
                a, b = grouped[1].handoff, solo[1].handoff
                assert all(np.array_equal(a.mel[k], b.mel[k]) and np.array_equal(a.ranges[k], b.ranges[k]) for k in range(3))
                assert np.array_equal(a.raw_max, b.raw_max)
    assert 2 in formats_seen and 1 in formats_seen
    for g, s_ in zip(grouped, solo):
        assert np.array_equal(np.stack(g.finish()), np.stack(s_.finish()))
    _same(grouped[0].nemo, solo[0].nemo)
    for s_ in grouped + solo:
        s_.close()


def test_one_round_costs_three_launches_per_format(sep):
    """No clock: one grouped tick (one round) of 4 NeMo + 2 Whisper + 1 plain stream costs 6 hand-off launches, 2 of them products;
    of NeMo streams alone 3 and 1, for 17 streams (two tables) 5 and 1"""
    CSS, S = pkg("css"), pkg("stream")
    x = _rec(4.0, 40)[:50000]
    cfg = CSS.CssCfg()

    def tick(n_nemo, n_whisper, n_plain):
        streams = ([S.CssStream(sep, cfg, nemo=CONFIGS[i % 3]) for i in range(n_nemo)] +
                   [S.CssStream(sep, cfg, handoff=dict(n_mels=80, pad_frames=8, drop_silence=True)) for _ in range(n_whisper)] +
                   [S.CssStream(sep, cfg) for _ in range(n_plain)])
        S.CssStreamGroup(streams).push([x] * len(streams))
        assert all(s.nemo.activity[0].shape[0] > 0 for s in streams[:n_nemo])
        stats = sep.handle.stream_handoff_stats()
        for s in streams:
            s.close()
        return stats
    assert tick(4, 2, 1)[:2] == (6, 2)
    assert tick(4, 0, 0)[:2] == (3, 1)
    assert tick(0, 2, 1)[:2] == (3, 1)
    assert tick(17, 0, 0)[:2] == (5, 1)


def test_seventeen_nemo_streams_in_one_group(sep):
    """17 NeMo streams of 3.2 s (two tables per kernel; the shortest recording css_run's default windows accept is just above one
    segment of 3 s) pushed as a group: each equals its solo twin, call by call"""
    S = pkg("stream")
    recs = [_rec(3.2, 800 + i) for i in range(17)]
    cfg = _main(sep)[1]
    n_in = recs[0].shape[0]
    variants = [CONFIGS[0], CONFIGS[1], CONFIGS[2], dict(n_mels=128, pad_frames=3, drop_silence=True, preemphasis=0.0)]
    streams = [S.CssStream(sep, cfg, nemo=variants[i % 4]) for i in range(17)]
    group = S.CssStreamGroup(streams)
    got = [[] for _ in range(17)]
    for n in range(0, n_in, 16000):
        res = group.push([r[n:n + 16000] for r in recs])
        for i, s in enumerate(streams):
            got[i].append((np.stack(res[i]), s.nemo))
    for i, s in enumerate(streams):
        got[i].append((np.stack(s.finish()), s.nemo))
        s.close()
    emitted = 0
    for i in range(17):
        with S.CssStream(sep, cfg, nemo=variants[i % 4]) as s:
            alone = [(np.stack(s.push(recs[i][n:n + 16000])), s.nemo) for n in range(0, n_in, 16000)]
            alone.append((np.stack(s.finish()), s.nemo))
        assert len(alone) == len(got[i])
        for (wg, hg), (ws, hs) in zip(got[i], alone):
            assert np.array_equal(wg, ws)
            _same(hg, hs)
            emitted += sum(m.shape[1] for m in hg.mel)
    assert emitted > 0


# ---- 4. PCM16 -----------------------------------------------------------------------------------------------------------------------

def test_pcm16_pushes_equal_float_pushes(sep):
    x, cfg, *_ = _main(sep)
    q = np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16)
    xf = q.astype(np.float32) / np.float32(32768.0)
    a, b = _Run(sep, cfg, CONFIGS[0]), _Run(sep, cfg, CONFIGS[0])
    sizes = (24000, 1, 4097, 32000)
    n = 0
    for size in itertools.cycle(sizes):
        if n >= q.shape[0]:
            break
        a.took(a.s.push_pcm16(q[n:n + size]), q[n:n + size].shape[0])
        b.push(xf[n:n + size])
        n += size
    a.finish()
    b.finish()
    _same_runs(a, b)
    assert sum(c.mel[k].shape[1] for c in a.calls for k in range(3)) > 0
    a.s.close()
    b.s.close()


# ---- 5. rate and output format ------------------------------------------------------------------------------------------------------

def test_capture_rate_and_output_format(sep):
    """a 48 kHz stream with a 48 kHz int16 output equals, in its NeMo results, a 16 kHz float twin fed handle.resample(recording)"""
    S = pkg("stream")
    rec48 = _rec(30.0, 77)                       # (480000 samples: 10 s at 48 kHz)
    x16 = sep.handle.resample(rec48, 48000)
    cfg = _toggling_cfg(sep, x16)
    fast = _Run(sep, cfg, CONFIGS[0], input_rate=48000, output=dict(rate=48000, dtype="int16"))
    twin = _Run(sep, cfg, CONFIGS[0])
    for n in range(0, rec48.shape[0], 72000):
        fast.s.push(rec48[n:n + 72000])
        fast.calls.append(fast.s.nemo)
    fast.s.finish()
    fast.calls.append(fast.s.nemo)
    twin.feed(x16, itertools.repeat(24000))
    assert sum(m.shape[1] for m in twin.calls[-1].mel) + sum(c.mel[k].shape[1] for c in twin.calls[:-1] for k in range(3)) > 0
    # (the resampler's lag moves samples between calls: the totals are compared)
    for k in range(3):
        for i in range(3):
            assert np.array_equal(fast.total(k)[i], twin.total(k)[i]), (k, i)
    assert max(len(twin.total(k)[1]) for k in range(3)) >= 2
    fast.s.close()
    twin.s.close()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------

def _raw_out(S_, n_mels, frames, ranges, activity, raw_max=False):
    L = pkg("_lib")
    keep = dict(mel=np.empty((S_, n_mels, max(frames, 1)), np.float32), ranges=np.empty((S_, max(ranges, 1), 2), np.int64),
                act=np.empty((S_, max(activity, 1)), np.uint8), nf=np.zeros(S_, np.int64), nr=np.zeros(S_, np.int32), mx=np.full(S_, 7.0, np.float32))
    o = L.CssStreamHandoffOut()
    o.mel_host, o.cap_frames = keep["mel"].ctypes.data, frames
    o.ranges_host, o.cap_ranges = keep["ranges"].ctypes.data, ranges
    o.activity_host, o.cap_activity = keep["act"].ctypes.data, activity
    o.n_frames, o.n_ranges = keep["nf"].ctypes.data, keep["nr"].ctypes.data
    o.raw_max = keep["mx"].ctypes.data if raw_max else None
    return o, keep


def test_refusals_leave_the_stream_unchanged(sep):
    L, CSS, S = pkg("_lib"), pkg("css"), pkg("stream")
    h = sep.handle
    x, cfg, *_ = _main(sep)
    info = lambda s: (s.info().n_pushed, s.info().n_emitted, s.info().finished, s.info().device_bytes)
    err = lambda: h.lib.css_last_error(h.h).decode()
    # ---- open: bad values, after the first sample, twice, on a Whisper stream, Whisper on a NeMo stream
    plain = S.CssStream(sep, cfg)
    bytes_off = plain.info().device_bytes
    for bad in (L.stream_nemo_cfg(64), L.stream_nemo_cfg(80, -1), L.stream_nemo_cfg(80, 4097), L.stream_nemo_cfg(80, 8, True, 1.0),
                L.stream_nemo_cfg(80, 8, True, -0.1), L.stream_nemo_cfg(80, 8, True, float("nan"))):
        assert h.lib.css_stream_nemo_open(h.h, plain.id, C.byref(bad)) == L.CSS_ERR_INVALID_ARG
    assert h.lib.css_stream_nemo_open(h.h, plain.id, None) == L.CSS_ERR_INVALID_ARG
    assert plain.info().device_bytes == bytes_off
    plain.push(x[:1000])
    assert h.lib.css_stream_nemo_open(h.h, plain.id, C.byref(L.stream_nemo_cfg())) == L.CSS_ERR_STATE
    plain.close()
    with S.CssStream(sep, cfg, handoff=dict(n_mels=80, pad_frames=8, drop_silence=True)) as w:
        assert h.lib.css_stream_nemo_open(h.h, w.id, C.byref(L.stream_nemo_cfg())) == L.CSS_ERR_STATE
    for kw in (dict(handoff=dict(n_mels=80)), dict(window_history=3000)):
        with pytest.raises(ValueError):
            S.CssStream(sep, cfg, nemo=CONFIGS[0], **kw)
    s, twin = (S.CssStream(sep, cfg, nemo=CONFIGS[0]) for _ in range(2))
    assert s.info().device_bytes > bytes_off                                  # the NeMo buffers are counted
    assert h.lib.css_stream_nemo_open(h.h, s.id, C.byref(L.stream_nemo_cfg())) == L.CSS_ERR_STATE
    assert h.lib.css_stream_handoff_open(h.h, s.id, C.byref(L.handoff_cfg())) == L.CSS_ERR_STATE
    assert h.lib.css_stream_window_open(h.h, s.id, 3000) == L.CSS_ERR_STATE and "NeMo" in err()
    first = x[:60000]
    assert np.array_equal(np.stack(s.push(first)), np.stack(twin.push(first)))
    _same(s.nemo, twin.nemo)
    bytes_on = s.info().device_bytes
    # ---- nothing bound: CSS_ERR_STATE, for a push and for finish
    chunk = x[60000:60000 + 40000]
    out = np.empty((3, chunk.shape[0] + s.latency_samples), np.float32)
    n_out = C.c_int64()
    push = lambda: h.lib.css_stream_push(h.h, s.id, chunk.ctypes.data_as(C.c_void_p), chunk.shape[0], out.ctypes.data_as(C.c_void_p),
                                         out.shape[1], C.byref(n_out))
    before = info(s)
    assert h.lib.css_stream_handoff_bind(h.h, s.id, None) == L.CSS_OK
    assert push() == L.CSS_ERR_STATE and info(s) == before
    assert h.lib.css_stream_finish(h.h, s.id, out.ctypes.data_as(C.c_void_p), out.shape[1], C.byref(n_out)) == L.CSS_ERR_STATE and info(s) == before
    # ---- one frame / one range / one gate byte below the bound: CSS_ERR_INVALID_ARG, the stream unchanged
    need = s.nemo_bounds(chunk.shape[0])
    for short in range(3):
        caps = [n - (1 if i == short else 0) for i, n in enumerate(need)]
        o, keep = _raw_out(3, 80, *caps)
        assert h.lib.css_stream_handoff_bind(h.h, s.id, C.byref(o)) == L.CSS_OK
        assert push() == L.CSS_ERR_INVALID_ARG and info(s) == before
    # ---- a refused item of a group leaves the other streams of the call unchanged too
    items = (L.CssStreamPush * 2)()
    out2 = np.empty_like(out)
    twin._handoff_bind(chunk.shape[0])
    for it, st, buf in ((items[0], twin, out2), (items[1], s, out)):
        it.id, it.pcm_host, it.n_samples, it.out_host, it.cap = st.id, chunk.ctypes.data, chunk.shape[0], buf.ctypes.data, buf.shape[1]
    tb = info(twin)
    assert h.lib.css_stream_push_many(h.h, items, 2, None) == L.CSS_ERR_INVALID_ARG and info(twin) == tb and info(s) == before
    assert "item 1" in err()
    # ---- a preview with hand-off, windows up to the present: CSS_ERR_STATE with a message; a plain preview works
    pv = np.empty((3, max(s.latency_samples, 1)), np.float32)
    o, keep = _raw_out(3, 80, *s.nemo_bounds(-1), raw_max=True)
    first_frame = np.zeros(3, np.int64)
    n_pv, first_sample = C.c_int64(), C.c_int64()
    assert h.lib.css_stream_preview_handoff(h.h, s.id, pv.ctypes.data_as(C.c_void_p), pv.shape[1], C.byref(n_pv), C.byref(first_sample), C.byref(o),
                                            first_frame.ctypes.data_as(C.c_void_p)) == L.CSS_ERR_STATE
    assert "NeMo" in err() and info(s) == before
    item = (L.CssStreamPresentItem * 1)()
    item[0].ph.p.id, item[0].ph.p.out_host, item[0].ph.p.cap = s.id, pv.ctypes.data, pv.shape[1]
    item[0].ph.ho, item[0].ph.first_frame = C.pointer(o), first_frame.ctypes.data
    launches = C.c_int32()
    assert h.lib.css_stream_present_windows(h.h, item, 1, None, C.byref(launches)) == L.CSS_ERR_STATE
    assert "NeMo" in err() and info(s) == before
    with pytest.raises(ValueError):
        s.preview(handoff=True)
    got = s.preview()
    assert len(got) == 3 and got[0].shape[0] > 0 and info(s) == before and (keep["mx"] == 7.0).all()
    # ---- raw_max may be NULL, and is never written where it is not
    o, keep = _raw_out(3, 80, *need, raw_max=True)
    s2 = S.CssStream(sep, cfg, nemo=CONFIGS[0])
    assert h.lib.css_stream_handoff_bind(h.h, s2.id, C.byref(o)) == L.CSS_OK
    out3 = np.empty((3, 40000 + s2.latency_samples), np.float32)
    assert h.lib.css_stream_push(h.h, s2.id, x[:40000].ctypes.data_as(C.c_void_p), 40000, out3.ctypes.data_as(C.c_void_p), out3.shape[1],
                                 C.byref(n_out)) == L.CSS_OK
    assert (keep["mx"] == 7.0).all()
    s2.close()
    # ---- the same pushes with enough room return what the undisturbed twin returns, to the end; the device bytes stay
    sizes = [2000] * 50
    n = 60000
    for size in sizes:
        assert np.array_equal(np.stack(s.push(x[n:n + size])), np.stack(twin.push(x[n:n + size])))
        _same(s.nemo, twin.nemo)
        n += size
    assert n > 60000 + 40000 and s.info().device_bytes == bytes_on == twin.info().device_bytes
    assert np.array_equal(np.stack(s.finish()), np.stack(twin.finish()))
    _same(s.nemo, twin.nemo)
    s.close()
    twin.close()
