"""PCM16 stream pushes on the MI355X (css_stream_push_pcm16, css_stream_push_many_pcm16; stream.py push_pcm16): int16 samples,
interleaved or planar, cross to the device as they are and one kernel launch per round de-interleaves and scales them into the
streams' windows.  The call is the float push of q.astype(float32) / 32768, so everything a stream returns -- the samples, the
counts, the hand-off, the group statistics, the refusals -- is the float push's, hence css_run's, bit for bit.  Every comparison
here is np.array_equal.  Input: synth_meeting, quantised as test_frame_sizes.py does (clip(rint(x * 0.2 * 32768))), with a few
samples forced to -32768 and 32767."""
import ctypes as C

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

CHUNKS = (1, 255, 256, 257, 4000, 24000, 32000)
HANDOFF = dict(n_mels=80, pad_frames=8, drop_silence=True)


def _sep(state, **kw):
    st, _ = state
    return pkg("separator").HipSeparator(st, None, device=0, **kw)


def _quantise(x, seed=0):
    """float [n, C] -> int16 [n, C] with both ends of the range present in every channel"""
    q = np.clip(np.rint(np.asarray(x, np.float64) * 0.2 * 32768.0), -32768, 32767).astype(np.int16)
    rs = np.random.RandomState(seed)
    for c in range(q.shape[1]):
        at = rs.choice(q.shape[0], 6, replace=False)
        q[at[:3], c] = -32768
        q[at[3:], c] = 32767
    q[0, 0], q[-1, -1] = 32767, -32768
    return np.ascontiguousarray(q)


def _dequantise(q):
    return np.ascontiguousarray(q.astype(np.float32) / np.float32(32768.0))


def _rec16(seconds, seed):
    x = pkg("synth").synth_meeting(float(seconds), 7, seed=seed)
    return _quantise(x[0] if x.ndim == 3 else x, seed)


def _offline(sep, q, cfg):
    """css_run of the dequantised recording"""
    x = _dequantise(q)
    return sep.handle.run(x, pkg("css").make_run_cfg(cfg, 16000, x.shape[1])).copy()


def _seeded_sizes(seed, n=64):
    rs = np.random.RandomState(seed)
    return [int(CHUNKS[j]) for j in rs.randint(0, len(CHUNKS), n)]


def _info(s):
    i = s.info()
    return (i.n_pushed, i.n_emitted, i.max_lag, i.device_bytes, i.finished)


def _stream(sep, n_total, cfg, sizes, ref, push, num_channels=7, **kw):
    """push(stream, a, b, call index) feeds samples [a, b); after every push the emitted prefix is css_run's and its length
    final_samples(n_pushed); returns everything the stream returned"""
    S = pkg("stream")
    outs, em = [], 0
    with S.CssStream(sep, cfg, num_channels=num_channels, **kw) as s:
        n, i = 0, 0
        while n < n_total:
            k = min(sizes[i % len(sizes)], n_total - n)
            got = np.stack(push(s, n, n + k, i))
            n += k
            i += 1
            assert got.shape[1] == s.final_samples(n) - em
            assert np.array_equal(got, ref[:, em:em + got.shape[1]])
            em += got.shape[1]
            inf = s.info()
            assert (inf.n_pushed, inf.n_emitted) == (n, em) and em == s.final_samples(n)
            outs.append(got)
        outs.append(np.stack(s.finish()))
        assert s.info().finished == 1
    return np.concatenate(outs, axis=1)


def test_pcm16_stream_is_bit_identical_to_css_run(mc_state, mix60):
    """60 s, 7 channels, seeded chunk sizes: interleaved, the planar view of the same samples, and the whole recording in one push"""
    sep = _sep(mc_state)
    cfg = pkg("css").CssCfg()
    q = _quantise(mix60[0] if mix60.ndim == 3 else mix60)
    assert q.shape == (960000, 7) and q.min() == -32768 and q.max() == 32767
    planes = np.ascontiguousarray(q.T)
    ref = _offline(sep, q, cfg)
    n = q.shape[0]
    got = _stream(sep, n, cfg, _seeded_sizes(0), ref, lambda s, a, b, i: s.push_pcm16(q[a:b]))
    assert got.shape == ref.shape and np.array_equal(got, ref)
    got = _stream(sep, n, cfg, _seeded_sizes(0), ref, lambda s, a, b, i: s.push_pcm16(planes[:, a:b].T))
    assert got.shape == ref.shape and np.array_equal(got, ref)
    for whole in (q, planes.T):   # many pieces in one call
        got = _stream(sep, n, cfg, [n], ref, lambda s, a, b, i: s.push_pcm16(whole[a:b]))
        assert np.array_equal(got, ref)
    sep.close()


def test_short_pieces_at_arbitrary_destination_columns(mc_state):
    """4 s, 7 channels, pieces of 1, 7, 8, 9, 63, 1023, 1024, 1025 and 2049 samples and then the rest, interleaved and planar: the
    pieces begin at destination columns 0, 1, 8, 16, 25, 88, 1111, 2135, 3160 and 5209 -- on, one past and well off the edges of
    the ingest kernel's 16-byte spans -- and their lengths sit on either side of the span and of its tile."""
    sep = _sep(mc_state)
    cfg = pkg("css").CssCfg()
    q = _rec16(4.0, 960)
    n = q.shape[0]
    assert q.shape == (64000, 7)
    planes = np.ascontiguousarray(q.T)
    ref = _offline(sep, q, cfg)
    sizes = [1, 7, 8, 9, 63, 1023, 1024, 1025, 2049, n]
    got = _stream(sep, n, cfg, sizes, ref, lambda s, a, b, i: s.push_pcm16(q[a:b]))
    assert got.shape == ref.shape and np.array_equal(got, ref)
    got = _stream(sep, n, cfg, sizes, ref, lambda s, a, b, i: s.push_pcm16(planes[:, a:b].T))
    assert got.shape == ref.shape and np.array_equal(got, ref)
    sep.close()


def test_float_and_pcm16_pushes_alternate_on_one_stream(mc_state, mix60):
    sep = _sep(mc_state)
    cfg = pkg("css").CssCfg()
    q = _quantise((mix60[0] if mix60.ndim == 3 else mix60)[:16000 * 30], 1)
    x = _dequantise(q)
    planes = np.ascontiguousarray(q.T)
    ref = _offline(sep, q, cfg)

    def push(s, a, b, i):
        if i % 3 == 0:
            return s.push(x[a:b])
        return s.push_pcm16(q[a:b] if i % 3 == 1 else planes[:, a:b].T)

    got = _stream(sep, q.shape[0], cfg, _seeded_sizes(2), ref, push)
    assert got.shape == ref.shape and np.array_equal(got, ref)
    sep.close()


def test_single_channel_model(sc_state, mix60):
    sep = _sep(sc_state)
    cfg = pkg("css").CssCfg()
    q = _quantise((mix60[0] if mix60.ndim == 3 else mix60)[:16000 * 24, :1], 2)
    ref = _offline(sep, q, cfg)
    got = _stream(sep, q.shape[0], cfg, _seeded_sizes(1), ref, lambda s, a, b, i: s.push_pcm16(q[a:b] if i % 2 else q[a:b, 0]),
                  num_channels=1)
    assert got.shape == ref.shape and np.array_equal(got, ref)
    sep.close()


class _Feed:
    """One stream with its int16 recording and css_run's output: hands out slices in the layout asked for, checks every piece."""

    def __init__(self, stream, q, ref, planar=False):
        self.s, self.q, self.ref, self.n, self.em, self.outs = stream, q, ref, 0, 0, []
        self.planes = np.ascontiguousarray(q.T) if planar else None

    def take(self, k, kind="pcm16"):
        a, b = self.n, min(self.n + k, self.q.shape[0])
        self.n = b
        if kind == "float":
            return _dequantise(self.q[a:b])
        return self.planes[:, a:b].T if self.planes is not None else self.q[a:b]

    def check(self, got):
        got = np.stack(got)
        assert got.shape[1] == self.s.final_samples(self.n) - self.em
        assert np.array_equal(got, self.ref[:, self.em:self.em + got.shape[1]])
        self.em += got.shape[1]
        self.outs.append(got)
        assert _info(self.s)[:2] == (self.n, self.em)
        return got

    def finish(self):
        self.outs.append(np.stack(self.s.finish()))
        got = np.concatenate(self.outs, axis=1)
        assert got.shape == self.ref.shape and np.array_equal(got, self.ref)


def test_grouped_equals_single_equals_offline(mc_state):
    """Five streams at different offsets of different recordings, interleaved and planar items in one call: per tick the grouped
    PCM16 push returns what the per-stream PCM16 pushes return and what css_run gives, and shares the estimator's batches
    exactly as a float group fed the same audio does."""
    CSS, S = pkg("css"), pkg("stream")
    cfg = CSS.CssCfg()
    sep = _sep(mc_state)
    offsets = (0, 1, 255, 4000, 12345)
    qs = [_rec16(22.0, 700 + i)[o:] for i, o in enumerate(offsets)]
    refs = [_offline(sep, q, cfg) for q in qs]
    grouped = [_Feed(S.CssStream(sep, cfg), q, r, planar=bool(i % 2)) for i, (q, r) in enumerate(zip(qs, refs))]
    single = [_Feed(S.CssStream(sep, cfg), q, r, planar=not i % 2) for i, (q, r) in enumerate(zip(qs, refs))]
    floats = [_Feed(S.CssStream(sep, cfg), q, r) for q, r in zip(qs, refs)]
    g16, gf = S.CssStreamGroup([f.s for f in grouped]), S.CssStreamGroup([f.s for f in floats])
    rs = np.random.RandomState(5)
    shared = 0
    while any(f.n < f.q.shape[0] for f in grouped):
        sizes = [int(rs.choice((24000, 24000, 32000, 257))) for _ in grouped]
        part = [f.n < f.q.shape[0] and rs.rand() > 0.1 for f in grouped]
        res16 = g16.push_pcm16([f.take(k) if p else None for f, k, p in zip(grouped, sizes, part)])
        resf = gf.push([f.take(k, "float") if p else None for f, k, p in zip(floats, sizes, part)])
        assert (g16.stats.estimator_batches, g16.stats.estimator_segments) == (gf.stats.estimator_batches, gf.stats.estimator_segments)
        shared += g16.stats.estimator_segments - g16.stats.estimator_batches
        for f, o, ff, k, p, a, b in zip(grouped, single, floats, sizes, part, res16, resf):
            if not p:
                assert all(v.size == 0 for v in a)
                continue
            a = f.check(a)
            assert np.array_equal(a, o.check(o.s.push_pcm16(o.take(k))))
            assert np.array_equal(a, ff.check(b))
    assert shared > 0   # (some batch held several streams' segments)
    for f in grouped + single + floats:
        f.finish()
        f.s.close()
    sep.close()


def test_more_than_sixteen_streams(mc_state):
    """20 streams in one call: two tables of the ingest launch"""
    CSS, S = pkg("css"), pkg("stream")
    cfg = CSS.CssCfg()
    sep = _sep(mc_state)
    base = [_rec16(14.0, 800 + i) for i in range(4)]
    qs = [np.ascontiguousarray(base[i % 4][i * 997:i * 997 + 16000 * 9]) for i in range(20)]
    feeds = [_Feed(S.CssStream(sep, cfg), q, _offline(sep, q, cfg), planar=i % 3 == 0) for i, q in enumerate(qs)]
    group = S.CssStreamGroup([f.s for f in feeds])
    while feeds[0].n < qs[0].shape[0]:
        res = group.push_pcm16({f.s: f.take(24000) for f in feeds})
        for f, got in zip(feeds, res):
            f.check(got)
    for f in feeds:
        f.finish()
        f.s.close()
    sep.close()


def test_handoff_equals_a_float_pushed_twin():
    """Hand-off on (80 bands, pad 8, drop silence): mel, ranges, activity and raw_max of every call equal those of a twin stream
    that is pushed the dequantised floats in the same chunks (the 2-block model and the toggling gate of test_hip_stream_handoff.py)."""
    w, CSS, S, L = pkg("weights"), pkg("css"), pkg("stream"), pkg("_lib")
    desc = w.ModelDesc(num_blocks=2)
    sep = pkg("separator").HipSeparator(w.apply_golden_recipe(w.portable_state_dict(desc, 21)), None, device=0)
    q = _rec16(30.0, 31)
    x = _dequantise(q)
    planes = np.ascontiguousarray(q.T)
    sep.handle.run(x, CSS.make_run_cfg(CSS.CssCfg(activity_th=0.0, show_progressbar=False), 16000, 7))
    th = float(np.percentile(sep.handle.read(L.BUF_ACTIVITY), 70))
    cfg = CSS.CssCfg(activity_th=th, show_progressbar=False, activity_dilation_sec=0.05, activity_erosion_sec=0.02)
    a, b = S.CssStream(sep, cfg, handoff=HANDOFF), S.CssStream(sep, cfg, handoff=HANDOFF)
    sizes = _seeded_sizes(3)
    n, i, frames, ranges = 0, 0, 0, 0

    def same():
        ha, hb = a.handoff, b.handoff
        assert ha.first_activity_frame == hb.first_activity_frame and np.array_equal(ha.raw_max, hb.raw_max)
        for k in range(3):
            assert ha.mel[k].shape == hb.mel[k].shape and np.array_equal(ha.mel[k], hb.mel[k])
            assert np.array_equal(ha.ranges[k], hb.ranges[k]) and np.array_equal(ha.activity[k], hb.activity[k])
        return sum(m.shape[1] for m in ha.mel), sum(len(r) for r in ha.ranges)

    while n < q.shape[0]:
        k = min(sizes[i % len(sizes)], q.shape[0] - n)
        ga = a.push_pcm16(q[n:n + k] if i % 2 else planes[:, n:n + k].T)
        gb = b.push(x[n:n + k])
        assert np.array_equal(np.stack(ga), np.stack(gb))
        f, r = same()
        frames, ranges = frames + f, ranges + r
        n, i = n + k, i + 1
    assert np.array_equal(np.stack(a.finish()), np.stack(b.finish()))
    f, r = same()
    assert frames + f > 100 and ranges + r > 3, (frames + f, ranges + r)   # (the gate toggled: there was something to compare)
    a.close()
    b.close()
    sep.close()


def _raw_many(h, entries):
    """css_stream_push_many_pcm16 with explicit fields: entries = (id, address or None, n, sample_stride, channel_stride, out or None, cap)"""
    L = pkg("_lib")
    items = (L.CssStreamPushPcm16 * max(len(entries), 1))()
    for it, (sid, ptr, n, ss, cs, out, cap) in zip(items, entries):
        it.id, it.pcm16_host, it.n_samples, it.sample_stride, it.channel_stride = sid, ptr, n, ss, cs
        it.out_host, it.cap, it.n_out = (out.ctypes.data if out is not None else None), cap, -1
    stats = L.CssStreamGroupStats()
    return h.lib.css_stream_push_many_pcm16(h.h, items, len(entries), C.byref(stats)), items, stats


def test_refusals_change_nothing(mc_state):
    """Every refused call returns its status and leaves css_stream_info of EVERY stream of the call as it was -- device_bytes
    included: a refused first PCM16 push allocates nothing -- and the streams then go on to css_run's output."""
    L, CSS, S = pkg("_lib"), pkg("css"), pkg("stream")
    cfg = CSS.CssCfg()
    sep = _sep(mc_state)
    h = sep.handle
    qs = [_rec16(16.0, 900 + i) for i in range(3)]
    feeds = [_Feed(S.CssStream(sep, cfg), q, _offline(sep, q, cfg), planar=i == 1) for i, q in enumerate(qs)]
    group = S.CssStreamGroup([f.s for f in feeds])
    step = 32000
    lat = feeds[0].s.latency_samples
    bufs = [np.empty((3, step + lat), np.float32) for _ in feeds]
    q8 = np.ascontiguousarray(qs[0][:16000 * 8])
    p8 = np.ascontiguousarray(q8.T)
    big = np.empty((3, q8.shape[0] + lat), np.float32)
    n8 = q8.shape[0]

    def good():
        out = []
        for f, b in zip(feeds, bufs):
            c = f.q[f.n:f.n + step]
            out.append((f.s.id, c.ctypes.data, c.shape[0], 7, 1, b, b.shape[1]))
        return out

    def refused(bad, want, at=1, streams=()):
        """the good items with `bad` inserted at `at`: refused with `want`, nothing moves; the single call is refused alike"""
        entries = good()
        entries.insert(at, bad)
        before = [_info(f.s) for f in feeds] + [_info(s) for s in streams]
        rc, _, _ = _raw_many(h, entries)
        assert rc == want, (rc, want)
        assert f"item {at} (stream {bad[0]})" in h.lib.css_last_error(h.h).decode()
        assert [_info(f.s) for f in feeds] + [_info(s) for s in streams] == before
        if bad[0] not in [f.s.id for f in feeds]:
            sid, ptr, n, ss, cs, out, cap = bad
            n_out = C.c_int64(-1)
            assert h.lib.css_stream_push_pcm16(h.h, sid, ptr, n, ss, cs, out.ctypes.data if out is not None else None, cap,
                                               C.byref(n_out)) == want
            assert n_out.value == -1 and [_info(s) for s in streams] == before[len(feeds):]

    def tick():
        for f, got in zip(feeds, group.push_pcm16([f.take(step) for f in feeds])):
            f.check(got)

    fresh = S.CssStream(sep, cfg)
    fid = fresh.id
    # refused before any stream of the call has seen a PCM16 push: no staging is allocated
    refused((fid, q8.ctypes.data, n8, 7, 2, big, big.shape[1]), L.CSS_ERR_INVALID_ARG, streams=(fresh,))
    tick()
    # strides outside the two layouts
    for ss, cs in ((7, 2), (7, 0), (2, 1), (14, 1), (0, 0), (1, 1), (6, 1), (-7, 1), (7, -1), (2, n8)):
        refused((fid, q8.ctypes.data, n8, ss, cs, big, big.shape[1]), L.CSS_ERR_INVALID_ARG, at=ss % 4, streams=(fresh,))
    # planar with planes that overlap
    refused((fid, p8.ctypes.data, n8, 1, n8 - 1, big, big.shape[1]), L.CSS_ERR_INVALID_ARG, streams=(fresh,))
    # no source
    refused((fid, None, n8, 7, 1, big, big.shape[1]), L.CSS_ERR_INVALID_ARG, at=0, streams=(fresh,))
    refused((fid, q8.ctypes.data, -1, 7, 1, big, big.shape[1]), L.CSS_ERR_INVALID_ARG, at=3, streams=(fresh,))
    # an id twice (the second mention is the failing item)
    refused((feeds[0].s.id, q8.ctypes.data, n8, 7, 1, big, big.shape[1]), L.CSS_ERR_INVALID_ARG, at=2)
    # a finished stream
    done = S.CssStream(sep, cfg)
    done.push_pcm16(q8)
    done.finish()
    refused((done.id, q8.ctypes.data, n8, 7, 1, big, big.shape[1]), L.CSS_ERR_STATE, streams=(done,))
    # an output capacity one sample short of what the item finalises, and none at all
    need = fresh.final_samples(n8)
    assert need > 0
    refused((fid, q8.ctypes.data, n8, 7, 1, big, need - 1), L.CSS_ERR_INVALID_ARG, at=3, streams=(fresh,))
    refused((fid, p8.ctypes.data, n8, 1, n8, None, need), L.CSS_ERR_INVALID_ARG, at=3, streams=(fresh,))
    # a push that would finalise frames no segment gives weight to (test_hip_stream_group.py: 3.0 s segments, 2.9 s hop)
    zcfg = CSS.CssCfg(segment_size_sec=3.0, hop_size_sec=2.9)
    zrc = CSS.make_run_cfg(zcfg, 16000, 7)
    assert (zrc.c.segment_frames, zrc.c.hop_frames) == (186, 179)
    zero = S.CssStream(sep, zcfg)
    qz = np.ascontiguousarray(qs[0][:48128])
    refused((zero.id, qz.ctypes.data, 48128, 7, 1, big, big.shape[1]), L.CSS_ERR_ZERO_WEIGHT, at=0, streams=(zero,))
    with pytest.raises(AssertionError, match="zero weights"):
        zero.push_pcm16(qz)
    assert _info(zero)[:2] == (0, 0)
    tick()
    # an exact capacity is enough; n_samples == 0 is accepted (with or without a source) and returns nothing
    exact = np.empty((3, need), np.float32)
    rc, items, _ = _raw_many(h, [(fid, q8.ctypes.data, n8, 7, 1, exact, need), (zero.id, None, 0, 0, 0, None, 0)])
    assert rc == L.CSS_OK and (items[0].n_out, items[1].n_out) == (need, 0)
    assert np.array_equal(exact, feeds[0].ref[:, :need])   # (q8 is the head of the first recording)
    before = _info(fresh)
    n_out = C.c_int64(-1)
    assert h.lib.css_stream_push_pcm16(h.h, fid, q8.ctypes.data, 0, 7, 1, None, 0, C.byref(n_out)) == L.CSS_OK and n_out.value == 0
    assert h.lib.css_stream_push_pcm16(h.h, fid, None, 0, 3, 3, None, 0, C.byref(n_out)) == L.CSS_OK and n_out.value == 0
    assert [np.stack(v).shape for v in (fresh.push_pcm16(q8[:0]),)] == [(3, 0)] and _info(fresh) == before
    assert _raw_many(h, [])[0] == L.CSS_OK
    # Python: other dtypes are not taken for PCM16, and push still takes an int16 array as float sample values
    with pytest.raises(TypeError):
        fresh.push_pcm16(_dequantise(q8))
    with pytest.raises(TypeError):
        group.push_pcm16([f.q[:100].astype(np.int32) for f in feeds])
    assert [_info(f.s)[0] for f in feeds] == [f.n for f in feeds] and _info(fresh) == before
    while feeds[0].n < qs[0].shape[0]:
        tick()
    for f in feeds:
        f.finish()
        f.s.close()
    for s in (done, fresh, zero):
        s.close()
    sep.close()


def test_float_streams_hold_what_they_held(mc_state):
    """device_bytes: a stream that never saw a PCM16 push reports what it reported when it was opened, whatever its siblings on
    the handle do; a stream's first PCM16 push adds its staging (one piece of int16) once."""
    CSS, S = pkg("css"), pkg("stream")
    cfg = CSS.CssCfg()
    sep = _sep(mc_state)
    q = _rec16(8.0, 950)
    x = _dequantise(q)
    f, p = S.CssStream(sep, cfg), S.CssStream(sep, cfg)
    base = f.info().device_bytes
    assert p.info().device_bytes == base
    rc = f._run_cfg.c
    staging = 8 * rc.hop_frames * sep.desc.frame_hop * 7 * 2
    for a in range(0, q.shape[0], 24000):
        f.push(x[a:a + 24000])
        p.push_pcm16(q[a:a + 24000])
        assert f.info().device_bytes == base and p.info().device_bytes == base + staging
    p.push(x[:1000])
    S.CssStreamGroup([f, p]).push([x[:1000], None])
    assert f.info().device_bytes == base and p.info().device_bytes == base + staging
    f.close()
    p.close()
    sep.close()
