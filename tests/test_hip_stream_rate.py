"""Pushes at the capture rate on the MI355X (include/css_mi355_rate.h; stream.py input_rate, Handle.resample): samples at 48, 44.1,
32 or 8 kHz cross to the device as they were captured and one launch per round filters, decimates and de-interleaves them into
the streams' windows -- scipy.signal.resample_poly's default filter, one float32 fmaf chain per output sample.

css_resample_host is held to the float64 sum of the definition with the library's own float32 taps, within the rounding bound
of the chain; everything a rate stream returns is held, with np.array_equal, to css_run of css_resample_host of the recording:
the stream's kernel and the standalone one share the function that forms a sample, and a sample's bits do not depend on where
pushes, pieces or tiles were cut."""
import ctypes as C

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

HANDOFF = dict(n_mels=80, pad_frames=8, drop_silence=True)
RATIOS = ((1, 3), (1, 2), (2, 1), (2, 3), (160, 441), (1, 6))
PIECES = (1, 7, 8, 9, 63, 1023, 1024, 1025, 2049)


def _sep(state, **kw):
    st, _ = state
    return pkg("separator").HipSeparator(st, None, device=0, **kw)


def _avail(up, down, n_in):
    """model-rate samples computable after n_in inputs of an open stream (the issue's rule, not the library's code)"""
    return max(0, -(-(n_in * up - 10 * max(up, down)) // down))


def _rec(seconds, rate, seed, channels=7):
    """a meeting as a capture device at `rate` delivers it: synth_meeting's 16 kHz samples held for rate / 16000 samples each
    would alias; what the tests need is a signal with speech-like level changes at that rate, so the 16 kHz samples are
    interpolated linearly (float64) -- the device's resampler then sees a band-limited input plus a little imaging"""
    x = pkg("synth").synth_meeting(float(seconds) + 0.1, 7, seed=seed)
    x = np.asarray(x[0] if x.ndim == 3 else x, np.float64)[:, :channels]
    n = int(round(seconds * rate))
    t = np.arange(n) * (16000.0 / rate)
    return np.stack([np.interp(t, np.arange(x.shape[0]), x[:, c]) for c in range(channels)], axis=1)


def _quantise(x, seed=0):
    q = np.clip(np.rint(np.asarray(x, np.float64) * 0.2 * 32768.0), -32768, 32767).astype(np.int16)
    rs = np.random.RandomState(seed)
    for c in range(q.shape[1]):
        at = rs.choice(q.shape[0], 6, replace=False)
        q[at[:3], c] = -32768
        q[at[3:], c] = 32767
    return np.ascontiguousarray(q)


def _run_cfg(cfg, channels=7):
    return pkg("css").make_run_cfg(cfg, 16000, channels)


def _offline(sep, x16, cfg):
    """css_run of model-rate samples [n, C]"""
    x16 = np.ascontiguousarray(x16, np.float32)
    return sep.handle.run(x16, _run_cfg(cfg, x16.shape[1])).copy()


def _info(s):
    i = s.info()
    return (i.n_pushed, i.n_emitted, i.max_lag, i.device_bytes, i.finished)


def _stream(sep, whole, rate, cfg, sizes, ref, push, num_channels=7, **kw):
    """push(stream, whole[a:b] bounds a, b, call index) feeds input samples [a, b) at `rate`.  After every push: the model-rate
    count in the window is avail(inputs), the emitted prefix is the finality rule on it and equals css_run's samples."""
    S, L = pkg("stream"), pkg("_lib")
    up, down = L.rate_ratio(rate)
    outs, em = [], 0
    n_total = whole.shape[0]
    with S.CssStream(sep, cfg, num_channels=num_channels, input_rate=rate, **kw) as s:
        assert s.rate == (up, down) and s.resampler_lag_samples == 10 * max(up, down) // up
        n, i = 0, 0
        while n < n_total:
            k = min(sizes[i % len(sizes)], n_total - n)
            got = np.stack(push(s, n, n + k, i))
            n += k
            i += 1
            m = _avail(up, down, n)
            fin = L.stream_final_samples(sep.desc, _run_cfg(cfg, num_channels), m)
            assert got.shape[1] == fin - em == s.final_samples(n) - em
            assert np.array_equal(got, ref[:, em:em + got.shape[1]])
            em = fin
            inf = s.info()
            assert (inf.n_pushed, inf.n_emitted, inf.finished) == (m, em, 0)
            outs.append(got)
        outs.append(np.stack(s.finish()))
        inf = s.info()
        assert inf.finished == 1 and inf.n_pushed == -(-n_total * up // down) and inf.n_emitted == ref.shape[1]
    return np.concatenate(outs, axis=1)


# ---- css_resample_host against float64 ------------------------------------------------------------------------------------------
def _float64_reference(x, taps, up, down):
    """y[m] = sum_i x[i] h[half + m down - i up] over 0 <= half + m down - i up <= 2 half, x = 0 outside: float64, float32 taps"""
    n, half = x.shape[0], 10 * max(up, down)
    h = taps.astype(np.float64)
    P = -(-h.size // up)
    m = np.arange(-(-n * up // down))[:, None]
    i = (m * down + half) // up - np.arange(P)[None, :]
    k = half + m * down - i * up
    ok = (k <= 2 * half) & (i >= 0) & (i < n)
    w = np.where(ok, h[np.minimum(k, 2 * half)], 0.0)
    return np.einsum("mp,mpc->mc", w, x.astype(np.float64)[np.clip(i, 0, n - 1)])


def _lengths(up, down):
    """the fixed lengths, and per ratio those whose n_out sits at the kernels' tile - 1, tile, tile + 1 (the smallest n_in that
    reaches each count: at 2 / 1 every n_out is even, so 256, 256 and 258)"""
    tile = pkg("_lib").RESAMPLE_TILE
    at = [(t - 1) * down // up + 1 for t in (tile - 1, tile, tile + 1)]
    assert all(-(-n * up // down) >= t and -(-(n - 1) * up // down) < t for n, t in zip(at, (tile - 1, tile, tile + 1)))
    return sorted(set([1, 2, 29, 30, 31, 61, 1000, 4099] + at))


@pytest.mark.parametrize("ratio", RATIOS, ids=lambda r: f"{r[0]}_{r[1]}")
def test_resample_host_against_float64(ratio, mc_state):
    """1 and 7 channels, float32 and int16, interleaved and planar, uniform input in [-1, 1) (int16: the full range).  The bar is
    the rounding bound of a length-P float32 fmaf chain: P * 2^-24 * (max over phases of sum |h|) * max |x|, max |x| = 1."""
    L = pkg("_lib")
    up, down = ratio
    sep = _sep(mc_state)
    h = sep.handle
    taps = L.resample_taps(up, down)
    P = -(-taps.size // up)
    phase_sum = max(float(np.abs(taps[p::up].astype(np.float64)).sum()) for p in range(up))
    bar = P * 2.0 ** -24 * phase_sum * 1.0
    if ratio == (1, 3):
        assert 6.0e-6 < bar < 6.6e-6
    if ratio == (1, 6):
        assert 1.2e-5 < bar < 1.4e-5
    rs = np.random.RandomState(up * 1000 + down)
    worst = 0.0
    for n in _lengths(up, down):
        for ch in (1, 7):
            xf = rs.uniform(-1.0, 1.0, (n, ch)).astype(np.float32)
            xq = rs.randint(-32768, 32768, (n, ch)).astype(np.int16)
            xq[0, 0], xq[-1, -1] = -32768, 32767
            for x in (xf, xq):
                val = x.astype(np.float64) / (32768.0 if x.dtype == np.int16 else 1.0)
                ref = _float64_reference(val, taps, up, down)
                planes = np.ascontiguousarray(x.T)
                for view in (x, planes.T):
                    got = h.resample(view, 16000 * down, 16000 * up)   # (the ratio fs / input_rate in lowest terms is up / down)
                    assert got.dtype == np.float32 and got.shape == ref.shape == (-(-n * up // down), ch)
                    err = float(np.max(np.abs(got.astype(np.float64) - ref)))
                    worst = max(worst, err)
                    assert err <= bar, (ratio, n, ch, x.dtype, err, bar)
                if ch == 1:   # [n] is [n, 1]
                    assert np.array_equal(h.resample(x[:, 0], 16000 * down, 16000 * up)[:, 0], got[:, 0])
    print(f"{up}/{down}: P = {P}, bar {bar:.3g}, worst error {worst:.3g}")
    sep.close()


# ---- streams --------------------------------------------------------------------------------------------------------------------
def test_48k_int16_stream_is_css_run_of_the_resampled_recording(mc_state):
    """4 s of 7 channels at 48 kHz, pieces of 1, 7, 8, 9, 63, 1023, 1024, 1025 and 2049 samples and then the rest, interleaved and
    planar: chunk invariance, the carried history, arbitrary destination columns and the equality of the two kernel forms."""
    sep = _sep(mc_state)
    cfg = pkg("css").CssCfg()
    q = _quantise(_rec(4.0, 48000, 11), 11)
    assert q.shape == (192000, 7)
    planes = np.ascontiguousarray(q.T)
    x16 = sep.handle.resample(q, 48000)
    assert x16.shape == (64000, 7) and np.array_equal(x16, sep.handle.resample(planes.T, 48000))
    ref = _offline(sep, x16, cfg)
    sizes = list(PIECES) + [q.shape[0]]
    got = _stream(sep, q, 48000, cfg, sizes, ref, lambda s, a, b, i: s.push_pcm16(q[a:b]))
    assert got.shape == ref.shape and np.array_equal(got, ref)
    got = _stream(sep, q, 48000, cfg, sizes, ref, lambda s, a, b, i: s.push_pcm16(planes[:, a:b].T))
    assert got.shape == ref.shape and np.array_equal(got, ref)
    sep.close()


@pytest.mark.parametrize("rate", [44100, 8000])
def test_float_pushes(rate, mc_state):
    """4 s of float32 samples at 160 / 441 and at 2 / 1, seeded random piece sizes; every third push is the int16 push of the
    same samples (a rate stream takes both kinds in any order: the carried inputs are kept as float)"""
    sep = _sep(mc_state)
    cfg = pkg("css").CssCfg()
    q = _quantise(_rec(4.0, rate, 12), 12)
    x = np.ascontiguousarray(q.astype(np.float32) / np.float32(32768.0))
    x16 = sep.handle.resample(x, rate)
    assert x16.shape[0] == 64000 and np.array_equal(x16, sep.handle.resample(q, rate))
    ref = _offline(sep, x16, cfg)
    rs = np.random.RandomState(rate)
    sizes = [int(v) for v in rs.choice((1, 2, 255, 441, 1000, 4097, 30000, 70001), 64)]
    got = _stream(sep, x, rate, cfg, sizes, ref, lambda s, a, b, i: s.push_pcm16(q[a:b]) if i % 3 == 2 else s.push(x[a:b]))
    assert got.shape == ref.shape and np.array_equal(got, ref)
    sep.close()


def test_one_push_of_several_pieces_and_a_rebase(mc_state):
    """26 s in ONE push: the call cuts it into three pieces (a piece makes at most 8 hop_frames * 256 = 190 464 window samples
    available: 571 392 inputs at 48 kHz, 95 232 at 8 kHz), the staging and the carried inputs are reused round after round with
    no synchronise between them, and the window (19 s) is rebased on the way.  48 kHz int16 planar and 8 kHz float32."""
    sep = _sep(mc_state)
    cfg = pkg("css").CssCfg()
    for rate, as_float in ((48000, False), (8000, True)):
        q = _quantise(_rec(26.0, rate, 14), 14)
        x = np.ascontiguousarray(q.astype(np.float32) / np.float32(32768.0)) if as_float else np.ascontiguousarray(q.T).T
        ref = _offline(sep, sep.handle.resample(q, rate), cfg)
        got = _stream(sep, x, rate, cfg, [x.shape[0]], ref, lambda s, a, b, i: s.push(x[a:b]) if as_float else s.push_pcm16(x[a:b]))
        assert got.shape == ref.shape and np.array_equal(got, ref)
        # the same in ticks of 1.5 s: pieces end elsewhere, the bits do not move
        got = _stream(sep, x, rate, cfg, [rate * 3 // 2], ref, lambda s, a, b, i: s.push(x[a:b]) if as_float else s.push_pcm16(x[a:b]))
        assert np.array_equal(got, ref)
    sep.close()


def test_single_channel_model(sc_state):
    sep = _sep(sc_state)
    cfg = pkg("css").CssCfg()
    q = _quantise(_rec(4.0, 48000, 13, channels=1), 13)
    ref = _offline(sep, sep.handle.resample(q, 48000), cfg)
    got = _stream(sep, q, 48000, cfg, [1, 31, 4800, 48000, 100001], ref,
                  lambda s, a, b, i: s.push_pcm16(q[a:b] if i % 2 else q[a:b, 0]), num_channels=1)
    assert got.shape == ref.shape and np.array_equal(got, ref)
    sep.close()


def _run_rooms(sep, cfg, rooms, grouped, tick_seconds=None):
    """rooms: (int16 recording, rate or None).  All rooms in one group (grouped) or each in a group of its own, pushed whole
    (or in ticks of tick_seconds) and finished -> (outputs, estimator batches of the calls)"""
    S = pkg("stream")
    streams = [S.CssStream(sep, cfg, input_rate=rate) for _, rate in rooms]
    groups = [S.CssStreamGroup(streams)] if grouped else [S.CssStreamGroup([s]) for s in streams]
    outs = [[] for _ in rooms]
    batches = 0
    seconds = max(q.shape[0] / float(rate or 16000) for q, rate in rooms)
    tick = tick_seconds or seconds
    t = 0.0
    while t < seconds:
        for g in groups:
            idx = [streams.index(s) for s in g.streams]
            chunks = []
            for i in idx:
                q, rate = rooms[i]
                r = rate or 16000
                chunks.append(q[int(round(t * r)):int(round((t + tick) * r))])
            res = g.push_pcm16(chunks)
            batches += g.stats.estimator_batches
            for i, got in zip(idx, res):
                outs[i].append(np.stack(got))
        t += tick
    for i, s in enumerate(streams):
        outs[i].append(np.stack(s.finish()))
        s.close()
    return [np.concatenate(o, axis=1) for o in outs], batches


def test_grouped_call_with_and_without_rates(mc_state):
    """Three rooms of 6 s in one css_stream_push_many_pcm16: 48 kHz, 16 kHz without a rate, 32 kHz.  Each room's output is its
    single-stream run's and css_run's; the call's estimator batches are fewer than the three single runs' together."""
    sep = _sep(mc_state)
    cfg = pkg("css").CssCfg()
    rooms = [(_quantise(_rec(6.0, 48000, 21), 21), 48000), (_quantise(_rec(6.0, 16000, 22), 22), None),
             (_quantise(_rec(6.0, 32000, 23), 23), 32000)]
    refs = []
    for q, rate in rooms:
        x16 = sep.handle.resample(q, rate) if rate else q.astype(np.float32) / np.float32(32768.0)
        assert x16.shape == (96000, 7)
        refs.append(_offline(sep, x16, cfg))
    single, single_batches = _run_rooms(sep, cfg, rooms, grouped=False)
    grouped, grouped_batches = _run_rooms(sep, cfg, rooms, grouped=True)
    for g, s, r in zip(grouped, single, refs):
        assert g.shape == r.shape and np.array_equal(g, r) and np.array_equal(s, r)
    assert 0 < grouped_batches < single_batches, (grouped_batches, single_batches)
    sep.close()


def test_seventeen_rate_streams(mc_state):
    """17 rate streams of 2 s in one call: two tables of the resample launch"""
    sep = _sep(mc_state)
    cfg = pkg("css").CssCfg(seg_weight_m0_sec=0.0)   # (a recording shorter than one segment: test_hip_stream.py test_stream_edges)
    base = _quantise(_rec(4.0, 48000, 31), 31)
    rooms = [(np.ascontiguousarray(base[i * 5003:i * 5003 + 96000]), 48000) for i in range(17)]
    refs = [_offline(sep, sep.handle.resample(q, 48000), cfg) for q, _ in rooms]
    outs, _ = _run_rooms(sep, cfg, rooms, grouped=True, tick_seconds=1.0)
    for o, r in zip(outs, refs):
        assert o.shape == r.shape and np.array_equal(o, r)
    sep.close()


def _merge(ranges):
    out = []
    for a, b in ranges:
        if out and out[-1][1] == a:
            out[-1][1] = b
        else:
            out.append([int(a), int(b)])
    return out


def test_handoff_equals_a_16k_twin_fed_the_resampled_recording():
    """Hand-off on (80 bands, pad 8, drop silence; the 2-block model and the toggling gate of test_hip_stream_handoff.py): a 48 kHz
    int16 stream and a 16 kHz float-pushed twin that is fed Handle.resample of the recording, cut at the model-rate counts the
    first stream's pushes reach.  Frames, ranges, gate bits and raw_max are equal call by call; the rate stream's finish is the
    twin's last push (the samples the resampler flushes) and finish together."""
    w, CSS, S, L = pkg("weights"), pkg("css"), pkg("stream"), pkg("_lib")
    desc = w.ModelDesc(num_blocks=2)
    sep = pkg("separator").HipSeparator(w.apply_golden_recipe(w.portable_state_dict(desc, 21)), None, device=0)
    q = _quantise(_rec(12.0, 48000, 31), 31)
    planes = np.ascontiguousarray(q.T)
    x16 = sep.handle.resample(q, 48000)
    sep.handle.run(x16, CSS.make_run_cfg(CSS.CssCfg(activity_th=0.0, show_progressbar=False), 16000, 7))
    th = float(np.percentile(sep.handle.read(L.BUF_ACTIVITY), 70))
    cfg = CSS.CssCfg(activity_th=th, show_progressbar=False, activity_dilation_sec=0.05, activity_erosion_sec=0.02)
    a, b = S.CssStream(sep, cfg, handoff=HANDOFF, input_rate=48000), S.CssStream(sep, cfg, handoff=HANDOFF)
    rs = np.random.RandomState(3)
    n, m, i, frames, ranges = 0, 0, 0, 0, 0

    def same(ha, mel, rng, act, raw_max, first):
        assert ha.first_activity_frame == first and np.array_equal(ha.raw_max, raw_max)
        for k in range(3):
            assert ha.mel[k].shape == mel[k].shape and np.array_equal(ha.mel[k], mel[k])
            assert _merge(ha.ranges[k]) == _merge(rng[k]) and np.array_equal(ha.activity[k], act[k])
        return sum(v.shape[1] for v in ha.mel), sum(len(r) for r in ha.ranges)

    while n < q.shape[0]:
        k = min(int(rs.choice((1, 767, 768, 12000, 72000, 96000))), q.shape[0] - n)
        ga = a.push_pcm16(q[n:n + k] if i % 2 else planes[:, n:n + k].T)
        n, i = n + k, i + 1
        m1 = _avail(1, 3, n)
        gb = b.push(x16[m:m1])
        m = m1
        assert np.array_equal(np.stack(ga), np.stack(gb))
        hb = b.handoff
        f, r = same(a.handoff, hb.mel, hb.ranges, hb.activity, hb.raw_max, hb.first_activity_frame)
        frames, ranges = frames + f, ranges + r
    assert m == x16.shape[0] - 10   # (30 inputs of lag: the last 10 samples wait for the zeros past the end)
    ga = np.stack(a.finish())
    g1 = np.stack(b.push(x16[m:]))
    h1 = b.handoff
    g2 = np.stack(b.finish())
    h2 = b.handoff
    assert np.array_equal(ga, np.concatenate([g1, g2], axis=1))
    f, r = same(a.handoff, [np.concatenate([h1.mel[k], h2.mel[k]], axis=1) for k in range(3)],
                [list(h1.ranges[k]) + list(h2.ranges[k]) for k in range(3)],
                [np.concatenate([h1.activity[k], h2.activity[k]]) for k in range(3)], h2.raw_max, h1.first_activity_frame)
    assert frames + f > 100 and ranges + r > 3, (frames + f, ranges + r)   # (the gate toggled: there was something to compare)
    a.close()
    b.close()
    sep.close()


def _status(fn):
    L = pkg("_lib")
    try:
        return None, fn()
    except L.CssError as e:
        return L.CssError, e.code
    except AssertionError as e:
        return AssertionError, str(e)


def test_short_recordings(mc_state):
    """finish after 10 input samples at 1 / 3: the status, and where css_run succeeds the output, of css_run on the 4 resampled samples"""
    CSS, S = pkg("css"), pkg("stream")
    sep = _sep(mc_state)
    q = _quantise(_rec(0.01, 48000, 41), 41)[:10]
    x16 = sep.handle.resample(q, 48000)
    assert x16.shape == (4, 7)
    succeeded = 0
    for m0 in (0.15, 0.0):
        cfg = CSS.CssCfg(seg_weight_m0_sec=m0)
        kind, ref = _status(lambda: _offline(sep, x16, cfg))
        with S.CssStream(sep, cfg, input_rate=48000) as s:
            assert all(v.size == 0 for v in s.push_pcm16(q))
            assert _info(s)[:2] == (0, 0)
            got_kind, got = _status(lambda: np.stack(s.finish()))
            assert got_kind == kind
            if kind is None:
                assert got.shape == ref.shape and np.array_equal(got, ref) and _info(s)[0] == 4
                succeeded += 1
            else:
                assert got == ref
    assert succeeded >= 1
    sep.close()


def test_refusals_change_nothing(mc_state):
    """css_stream_set_rate after a push and twice is CSS_ERR_STATE, a bad ratio CSS_ERR_INVALID_ARG, a capacity one below what the
    push returns CSS_ERR_INVALID_ARG; css_stream_info is unchanged by each and the stream goes on to css_run's output."""
    L, CSS, S = pkg("_lib"), pkg("css"), pkg("stream")
    cfg = CSS.CssCfg()
    sep = _sep(mc_state)
    h = sep.handle
    q = _quantise(_rec(4.0, 48000, 51), 51)
    ref = _offline(sep, h.resample(q, 48000), cfg)
    plain = S.CssStream(sep, cfg)
    before = _info(plain)
    for up, down in ((1, 1), (2, 4), (1, 7), (0, 3), (3, 0), (-1, 3), (1, -3)):
        assert h.lib.css_stream_set_rate(h.h, plain.id, up, down) == L.CSS_ERR_INVALID_ARG and _info(plain) == before
    assert h.lib.css_stream_set_rate(h.h, 63, 1, 3) == L.CSS_ERR_INVALID_ARG   # (no such stream)
    with pytest.raises(L.CssError):
        S.CssStream(sep, cfg, input_rate=112000)   # 1 / 7
    pushed = S.CssStream(sep, cfg)
    pushed.push_pcm16(_quantise(_rec(0.1, 16000, 52), 52))
    before_p = _info(pushed)
    assert h.lib.css_stream_set_rate(h.h, pushed.id, 1, 3) == L.CSS_ERR_STATE and _info(pushed) == before_p
    s = S.CssStream(sep, cfg, input_rate=48000)
    before_s = _info(s)
    assert before_s[3] > before[3]
    assert h.lib.css_stream_set_rate(h.h, s.id, 1, 3) == L.CSS_ERR_STATE
    assert h.lib.css_stream_set_rate(h.h, s.id, 1, 2) == L.CSS_ERR_STATE and _info(s) == before_s
    # the first 3.9 s finalise samples: a capacity one below that count is refused, the exact one is enough
    n1 = 187200
    need = L.stream_final_samples(sep.desc, _run_cfg(cfg), _avail(1, 3, n1))
    assert need > 0 and need == s.final_samples(n1)
    out = np.full((3, need), 7.0, np.float32)
    n_out = C.c_int64(-1)
    chunk = np.ascontiguousarray(q[:n1])
    args = (h.h, s.id, C.c_void_p(chunk.ctypes.data), n1, 7, 1, out.ctypes.data_as(C.c_void_p))
    assert h.lib.css_stream_push_pcm16(*args, need - 1, C.byref(n_out)) == L.CSS_ERR_INVALID_ARG
    assert n_out.value == -1 and np.all(out == 7.0) and _info(s) == before_s
    # planar planes that overlap, counted in input samples
    assert h.lib.css_stream_push_pcm16(h.h, s.id, C.c_void_p(chunk.ctypes.data), n1, 1, n1 - 1, out.ctypes.data_as(C.c_void_p), need,
                                       C.byref(n_out)) == L.CSS_ERR_INVALID_ARG and _info(s) == before_s
    assert h.lib.css_stream_push_pcm16(*args, need, C.byref(n_out)) == L.CSS_OK and n_out.value == need
    assert np.array_equal(out, ref[:, :need])
    s._n_in += n1   # (the raw call above went past the Python object's count of inputs)
    assert h.lib.css_stream_set_rate(h.h, s.id, 1, 3) == L.CSS_ERR_STATE
    rest = [np.stack(s.push_pcm16(q[n1:])), np.stack(s.finish())]
    assert np.array_equal(np.concatenate([out] + rest, axis=1), ref)
    assert h.lib.css_stream_set_rate(h.h, s.id, 1, 3) == L.CSS_ERR_STATE
    assert _info(plain) == before
    for v in (plain, pushed, s):
        v.close()
    sep.close()


def test_other_streams_hold_what_they_held(mc_state):
    """device_bytes: a rate stream adds its staging, two generations of carried inputs and its taps at css_stream_set_rate; a
    rate-less stream beside it reports what it reported when it was opened, whatever the rate stream does"""
    CSS, S = pkg("css"), pkg("stream")
    cfg = CSS.CssCfg()
    sep = _sep(mc_state)
    q48 = _quantise(_rec(2.0, 48000, 61), 61)
    q16 = _quantise(_rec(2.0, 16000, 62), 62)
    f = S.CssStream(sep, cfg)
    base = f.info().device_bytes
    r = S.CssStream(sep, cfg, input_rate=48000)
    piece = 8 * f._run_cfg.c.hop_frames * sep.desc.frame_hop
    own = 7 * ((piece * 3 + 30) // 1 + 1) * 4 + 2 * 7 * 61 * 4 + 61 * 4   # staging as float32; H = 2 * 30 + 1; [1][P | 1] taps
    assert r.info().device_bytes == base + own and f.info().device_bytes == base
    for a in range(0, 2):
        r.push_pcm16(q48[a * 48000:(a + 1) * 48000])
        f.push(q16[a * 16000:(a + 1) * 16000].astype(np.float32) / np.float32(32768.0))
        S.CssStreamGroup([f, r]).push_pcm16([None, q48[:100]])
        assert f.info().device_bytes == base and r.info().device_bytes == base + own
    f.close()
    r.close()
    sep.close()
