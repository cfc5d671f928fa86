"""Grouped stream pushes on the MI355X (css_stream_push_many, notsofar1-challenge_amd/stream.py CssStreamGroup): many streams
pushed in one call share the mask estimator's batches, and every stream's output stays what css_stream_push gives item by
item -- hence css_run's output on the whole recording -- bit for bit.  Every comparison here is np.array_equal."""
import ctypes as C

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

CHUNKS = (0, 1, 255, 256, 257, 4000, 24000, 32000)


def _sep(state, **kw):
    st, _ = state
    return pkg("separator").HipSeparator(st, None, device=0, **kw)


def _rec(seconds, seed):
    x = pkg("synth").synth_meeting(float(seconds), 7, seed=seed)
    return np.ascontiguousarray(x[0] if x.ndim == 3 else x, dtype=np.float32)


def _offline(sep, x, cfg):
    rc = pkg("css").make_run_cfg(cfg, 16000, x.shape[1])
    return sep.handle.run(np.ascontiguousarray(x, np.float32), rc).copy()


def _info(s):
    i = s.info()
    return (i.n_pushed, i.n_emitted, i.finished)


def _done(f):
    """segments of a feed's stream that are complete and not the last one after the samples fed so far (the rule of css_stream_final_samples)"""
    c = f.s._run_cfg.c
    frames = 0 if f.n < 512 else (f.n - 512) // 256 + 1
    return (frames - 1 - c.segment_frames) // c.hop_frames + 1 if frames > c.segment_frames else 0


def _raw_push_many(h, entries):
    """css_stream_push_many with explicit ids / capacities: entries = (id, samples or None, out buffer or None, cap)"""
    L = pkg("_lib")
    items = (L.CssStreamPush * max(len(entries), 1))()
    for it, (sid, x, out, cap) in zip(items, entries):
        it.id, it.pcm_host, it.n_samples = sid, (x.ctypes.data if x is not None else None), (x.shape[0] if x is not None else 0)
        it.out_host, it.cap, it.n_out = (out.ctypes.data if out is not None else None), cap, -1
    stats = L.CssStreamGroupStats()
    rc = h.lib.css_stream_push_many(h.h, items, len(entries), C.byref(stats))
    return rc, items, stats


class _Feed:
    """One stream of a group with its recording and css_run's output: feeds slices, checks every returned piece."""

    def __init__(self, stream, x, ref):
        self.s, self.x, self.ref, self.n, self.em, self.outs = stream, x, ref, 0, 0, []

    def take(self, k):
        k = min(k, self.x.shape[0] - self.n)
        c = self.x[self.n:self.n + k]
        self.n += k
        return c

    def check(self, got):
        got = np.stack(got)
        assert got.shape[1] == self.s.final_samples(self.n) - self.em
        assert np.array_equal(got, self.ref[:, self.em:self.em + got.shape[1]])
        self.em += got.shape[1]
        self.outs.append(got)
        assert _info(self.s)[:2] == (self.n, self.em)

    def finish(self):
        self.outs.append(np.stack(self.s.finish()))
        got = np.concatenate(self.outs, axis=1)
        assert got.shape == self.ref.shape and np.array_equal(got, self.ref)


def test_grouped_equals_single_equals_offline(mc_state):
    """16 streams, 16 recordings of 18 .. 30 s, seeded chunk sizes per stream and round, some rounds without a stream: after
    every round every item returned exactly the newly final slice of css_run's output; one recording streamed alone through
    css_stream_push with the same chunk sequence returns the same pieces."""
    CSS, S = pkg("css"), pkg("stream")
    cfg = CSS.CssCfg()
    sep = _sep(mc_state)
    recs = [_rec(18 + 12 * i / 15, 100 + i) for i in range(16)]
    feeds = [_Feed(S.CssStream(sep, cfg), x, _offline(sep, x, cfg)) for x in recs]
    group = S.CssStreamGroup([f.s for f in feeds])
    rs = np.random.RandomState(11)
    solo_sizes, solo_pieces = [], []
    shared_batches = 0
    while any(f.n < f.x.shape[0] for f in feeds):
        chunks = []
        for i, f in enumerate(feeds):
            size = int(CHUNKS[rs.randint(len(CHUNKS))])
            out_of_round = rs.rand() < 0.15 or f.n >= f.x.shape[0]
            chunks.append(None if out_of_round else f.take(size))
            if i == 3 and chunks[-1] is not None:
                solo_sizes.append(chunks[-1].shape[0])
        res = group.push(chunks)
        shared_batches += group.stats.estimator_batches
        for i, (f, c, got) in enumerate(zip(feeds, chunks, res)):
            if c is None:
                assert all(g.size == 0 for g in got)
                continue
            f.check(got)
            if i == 3:
                solo_pieces.append(np.stack(got))
    for f in feeds:
        f.finish()
    assert shared_batches > 0
    with S.CssStream(sep, cfg) as s:
        n = 0
        for k, piece in zip(solo_sizes, solo_pieces):
            got = np.stack(s.push(recs[3][n:n + k]))
            n += k
            assert got.shape == piece.shape and np.array_equal(got, piece)
        assert n == recs[3].shape[0]
    for f in feeds:
        f.s.close()
    sep.close()


def test_the_estimator_batch_is_shared(mc_state):
    """No clock: 16 streams that each complete exactly one segment per call are ONE estimator batch of 16 segments per call;
    the same pushes as 16 groups of one are one batch of one segment each."""
    CSS, S = pkg("css"), pkg("stream")
    cfg = CSS.CssCfg()
    sep = _sep(mc_state, max_batch_segments=64)
    rc = CSS.make_run_cfg(cfg, 16000, 7).c
    first = sep.desc.frame_len + rc.segment_frames * sep.desc.frame_hop
    step = rc.hop_frames * sep.desc.frame_hop
    assert (first, step) == (48128, 23808)
    calls = 4
    recs = [_rec(8.0, 200 + i)[:first + (calls - 1) * step] for i in range(16)]
    refs = [_offline(sep, x, cfg) for x in recs]
    for grouped in (True, False):
        feeds = [_Feed(S.CssStream(sep, cfg), x, r) for x, r in zip(recs, refs)]
        groups = [S.CssStreamGroup([f.s for f in feeds])] if grouped else [S.CssStreamGroup([f.s]) for f in feeds]
        for call in range(calls):
            k = first if call == 0 else step
            for g in groups:
                mine = [f for f in feeds if f.s in g.streams]
                res = g.push([f.take(k) for f in mine])
                assert g.stats.estimator_batches == 1
                assert g.stats.estimator_segments == (16 if grouped else 1)
                for f, got in zip(mine, res):
                    f.check(got)
        for f in feeds:
            f.finish()
            f.s.close()
    sep.close()


def test_mixed_configurations_in_one_call(mc_state, mix60):
    """Five streams, four configurations of one segmentation and one of another: two estimator batches in a round in which both
    classes complete segments, every stream bit-equal to css_run with its own configuration."""
    CSS, S = pkg("css"), pkg("stream")
    x = np.ascontiguousarray((mix60[0] if mix60.ndim == 3 else mix60)[:16000 * 24])
    cfgs = [CSS.CssCfg() for _ in range(5)]
    cfgs[1].normalize_segment_power = True
    cfgs[2].stitching_input, cfgs[2].stitching_loss = "separation_result", "mse"
    cfgs[3].activity_th = 0.3
    cfgs[4].segment_size_sec, cfgs[4].hop_size_sec = 2.0, 0.5
    sep = _sep(mc_state)
    feeds = [_Feed(S.CssStream(sep, c), x, _offline(sep, x, c)) for c in cfgs]
    group = S.CssStreamGroup([f.s for f in feeds])

    batches = []
    while feeds[0].n < x.shape[0]:
        before = [_done(f) for f in feeds]
        res = group.push({f.s: f.take(24000) for f in feeds})
        new = [_done(f) - b for f, b in zip(feeds, before)]
        # one batch per segmentation that completed segments in this round (all of them fit one batch of 64)
        want = (int(sum(new[:4]) > 0) + int(new[4] > 0), sum(new))
        assert (group.stats.estimator_batches, group.stats.estimator_segments) == want
        batches.append(want)
        for f, got in zip(feeds, res):
            f.check(got)
    assert max(b for b, _ in batches) == 2   # a round in which both segmentations completed segments
    for f in feeds:
        f.finish()
        f.s.close()
    sep.close()


def test_large_pushes_of_several_pieces(mc_state):
    """One call with 40 s for each of four streams (several pieces per item, more than 8 segments) and one sample for a fifth."""
    CSS, S = pkg("css"), pkg("stream")
    cfg = CSS.CssCfg()
    sep = _sep(mc_state)
    recs = [_rec(40.0, 300 + i) for i in range(4)] + [_rec(20.0, 304)]
    feeds = [_Feed(S.CssStream(sep, cfg), x, _offline(sep, x, cfg)) for x in recs]
    group = S.CssStreamGroup([f.s for f in feeds])
    res = group.push([f.take(16000 * 40) for f in feeds[:4]] + [feeds[4].take(1)])
    assert group.stats.estimator_segments == 4 * 25 and group.stats.estimator_batches >= 4
    for f, got in zip(feeds, res):
        f.check(got)
    assert feeds[0].em > 0 and feeds[4].em == 0
    feeds[4].check(feeds[4].s.push(feeds[4].take(16000 * 20)))
    for f in feeds:
        f.finish()
        f.s.close()
    sep.close()


def test_more_than_sixteen_streams(mc_state):
    """24 streams at once cross the 16-entry tables of the stitching kernels and the 8-entry table of the MVDR solve."""
    CSS, S = pkg("css"), pkg("stream")
    cfg = CSS.CssCfg()
    sep = _sep(mc_state)
    recs = [_rec(12.0, 400 + i) for i in range(24)]
    feeds = [_Feed(S.CssStream(sep, cfg), x, _offline(sep, x, cfg)) for x in recs]
    group = S.CssStreamGroup([f.s for f in feeds])
    while feeds[0].n < recs[0].shape[0]:
        before = _done(feeds[0])
        res = group.push([f.take(24000) for f in feeds])
        new = 24 * (_done(feeds[0]) - before)   # (24 000 samples are 93.75 frames and the hop is 93: now and then two segments)
        assert (group.stats.estimator_batches, group.stats.estimator_segments) == (int(new > 0), new)
        for f, got in zip(feeds, res):
            f.check(got)
    for f in feeds:
        f.finish()
        f.s.close()
    sep.close()


def test_sixty_four_streams_open_and_the_next_is_refused(mc_state):
    L, CSS, S = pkg("_lib"), pkg("css"), pkg("stream")
    assert L.MAX_STREAMS == 64
    sep = _sep(mc_state)
    streams = [S.CssStream(sep, CSS.CssCfg()) for _ in range(64)]
    assert sorted(s.id for s in streams) == list(range(64))
    with pytest.raises(L.CssError) as e:
        S.CssStream(sep, CSS.CssCfg())
    assert e.value.code == L.CSS_ERR_STATE
    for s in streams:
        s.close()
    sep.close()


def test_refusals_change_nothing(mc_state):
    """Every refused call returns the failing item's status, leaves css_stream_info of EVERY stream of the call unchanged, and
    the same call without the bad item then returns the right samples."""
    L, CSS, S = pkg("_lib"), pkg("css"), pkg("stream")
    cfg = CSS.CssCfg()
    sep = _sep(mc_state)
    h = sep.handle
    recs = [_rec(20.0, 500 + i) for i in range(3)]
    feeds = [_Feed(S.CssStream(sep, cfg), x, _offline(sep, x, cfg)) for x in recs]
    group = S.CssStreamGroup([f.s for f in feeds])
    step = 32000
    lat = feeds[0].s.latency_samples
    bufs = [np.empty((3, step + lat), np.float32) for _ in feeds]

    def refused(bad_entry, want, at=1, streams=()):
        """the good items with `bad_entry` inserted at position `at`: refused with `want`, nothing moves; then the good items alone"""
        chunks = [f.x[f.n:f.n + step] for f in feeds]
        entries = [(f.s.id, c, b, b.shape[1]) for f, c, b in zip(feeds, chunks, bufs)]
        entries.insert(at, bad_entry)
        before = [_info(f.s) for f in feeds] + [_info(s) for s in streams]
        rc, _, _ = _raw_push_many(h, entries)
        assert rc == want, (rc, want)
        assert f"item {at} (stream {bad_entry[0]})" in h.lib.css_last_error(h.h).decode()
        assert [_info(f.s) for f in feeds] + [_info(s) for s in streams] == before
        res = group.push([f.take(step) for f in feeds])
        for f, got in zip(feeds, res):
            f.check(got)

    for f, got in zip(feeds, group.push([f.take(step) for f in feeds])):
        f.check(got)
    x8 = np.ascontiguousarray(recs[0][:16000 * 8])
    big = np.empty((3, x8.shape[0] + lat), np.float32)
    # an id twice (the second mention is the failing item)
    refused((feeds[0].s.id, x8, big, big.shape[1]), L.CSS_ERR_INVALID_ARG, at=2)
    # a closed id
    gone = S.CssStream(sep, cfg)
    gone_id = gone.id
    gone.close()
    refused((gone_id, x8, big, big.shape[1]), L.CSS_ERR_INVALID_ARG)
    # a finished stream
    done = S.CssStream(sep, cfg)
    done.push(x8)
    done.finish()
    refused((done.id, x8, big, big.shape[1]), L.CSS_ERR_STATE, streams=(done,))
    # a capacity below what the item finalises
    fresh = S.CssStream(sep, cfg)
    refused((fresh.id, x8, big, 10), L.CSS_ERR_INVALID_ARG, at=3, streams=(fresh,))
    # a push that would finalise frames no segment gives weight to: 3.0 s segments, 2.9 s hop, the first segment completed
    zcfg = CSS.CssCfg(segment_size_sec=3.0, hop_size_sec=2.9)
    zrc = CSS.make_run_cfg(zcfg, 16000, 7)
    assert (zrc.c.segment_frames, zrc.c.hop_frames) == (186, 179)
    assert zrc._w[0][177] == 0 and zrc._w[0][178] == 0   # frames below the hop are covered by the first segment alone
    zero = S.CssStream(sep, zcfg)
    xz = np.ascontiguousarray(recs[0][:48128])
    n_out = C.c_int64()
    assert h.lib.css_stream_push(h.h, zero.id, xz.ctypes.data_as(C.c_void_p), xz.shape[0], big.ctypes.data_as(C.c_void_p), big.shape[1],
                                 C.byref(n_out)) == L.CSS_ERR_ZERO_WEIGHT
    refused((zero.id, xz, big, big.shape[1]), L.CSS_ERR_ZERO_WEIGHT, at=0, streams=(zero,))
    # queued sessions outstanding: every item is refused, the first one is named
    out = L.pinned_empty((3, L.plan(sep.desc, CSS.make_run_cfg(cfg, 16000, 7), recs[2].shape[0]).n_out))
    pinned = L.pinned_copy(recs[2])
    h.run_enqueue(pinned, CSS.make_run_cfg(cfg, 16000, 7), out)
    before = [_info(f.s) for f in feeds]
    rc, _, _ = _raw_push_many(h, [(f.s.id, f.x[f.n:f.n + step], b, b.shape[1]) for f, b in zip(feeds, bufs)])
    assert rc == L.CSS_ERR_STATE and [_info(f.s) for f in feeds] == before
    h.wait()
    for f, got in zip(feeds, group.push([f.take(step) for f in feeds])):
        f.check(got)
    # a null handle, no items
    assert h.lib.css_stream_push_many(None, None, 0, None) == L.CSS_ERR_INVALID_ARG
    assert _raw_push_many(h, [])[0] == L.CSS_OK
    while feeds[0].n < recs[0].shape[0]:
        for f, got in zip(feeds, group.push([f.take(step) for f in feeds])):
            f.check(got)
    for f in feeds:
        f.finish()
        f.s.close()
    for s in (done, fresh, zero):
        s.close()
    sep.close()


def test_python_group_argument_errors(mc_state):
    """Shape errors and foreign streams raise ValueError before the library is called."""
    CSS, S = pkg("css"), pkg("stream")
    sep, other = _sep(mc_state), _sep(mc_state)
    a, b, c = S.CssStream(sep, CSS.CssCfg()), S.CssStream(sep, CSS.CssCfg()), S.CssStream(other, CSS.CssCfg())
    with pytest.raises(ValueError):
        S.CssStreamGroup([a, c])
    with pytest.raises(ValueError):
        S.CssStreamGroup([a, a])
    g = S.CssStreamGroup([a, b])
    with pytest.raises(ValueError):
        g.push([np.zeros((100, 7), np.float32), np.zeros((100, 6), np.float32)])
    with pytest.raises(ValueError):
        g.push([np.zeros((100, 7), np.float32)])
    with pytest.raises(ValueError):
        g.push({c: np.zeros((100, 7), np.float32)})
    assert _info(a) == (0, 0, 0) and _info(b) == (0, 0, 0)
    res = g.push({b: np.zeros((100, 7), np.float32)})
    assert [len(r) for r in res] == [3, 3] and _info(a) == (0, 0, 0) and _info(b) == (100, 0, 0)
    for s in (a, b, c):
        s.close()
    sep.close()
    other.close()


def test_isolation_from_the_handles_own_session(mc_state):
    """css_run and a staged pass (css_begin .. css_stage_*) split around a grouped push give the bits they give without the
    streams, and the streams end equal to css_run."""
    L, CSS, S = pkg("_lib"), pkg("css"), pkg("stream")
    cfg = CSS.CssCfg()
    run_cfg = CSS.make_run_cfg(cfg, 16000, 7)
    sep = _sep(mc_state)
    h = sep.handle
    c = _rec(20.0, 8)

    def staged(between=None):
        h.begin(c, c.shape[0], 7, run_cfg)
        p = h.get_plan()
        nseg, TL = p.num_segments, p.mix_frames
        h.stage_stft(); h.stage_masknet(0, nseg)
        if between:
            between()
        h.stage_mvdr(0, nseg); h.stage_pit_costs(0, nseg - 1); h.stage_pit_scan(); h.stage_stitch(0, TL); h.stage_istft(0, TL)
        return h.read(L.BUF_WAV).copy()

    rcc = _offline(sep, c, cfg)
    staged_ref = staged()
    recs = [_rec(24.0, 600 + i) for i in range(3)]
    feeds = [_Feed(S.CssStream(sep, cfg), x, _offline(sep, x, cfg)) for x in recs]
    group = S.CssStreamGroup([f.s for f in feeds])

    def one_round():
        for f, got in zip(feeds, group.push([f.take(24000) for f in feeds])):
            f.check(got)

    while feeds[0].n < recs[0].shape[0]:
        one_round()
        assert np.array_equal(_offline(sep, c, cfg), rcc)
        if feeds[0].n < recs[0].shape[0]:
            assert np.array_equal(staged(one_round), staged_ref)
    for f in feeds:
        f.finish()
        f.s.close()
    sep.close()
