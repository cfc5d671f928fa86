"""The hand-off of streamed sessions on the MI355X (css_stream_handoff_*, stream.py CssStream(handoff=...)): with every push a
stream returns the Whisper log-mel frames, the kept sample ranges and the gate bits that became final, and what the calls
returned, put together, is what css_handoff_logmel returns after css_run_device on the whole recording -- bit for bit.
Every comparison is np.array_equal unless it says otherwise."""
import ctypes as C
import itertools

import numpy as np
import pytest

import css_oracle as O
from conftest import pkg

pytestmark = pytest.mark.gpu

CHUNKS = (0, 1, 255, 256, 257, 4000, 24000, 32000)     # test_hip_stream_group.py's
CONFIGS = (dict(n_mels=80, pad_frames=8, drop_silence=True), dict(n_mels=128, pad_frames=0, drop_silence=True),
           dict(n_mels=80, pad_frames=8, drop_silence=False))


@pytest.fixture(scope="module")
def model():
    """the 2-block multi-channel model of test_hip_session.py's tiny_models"""
    w = pkg("weights")
    desc = w.ModelDesc(num_blocks=2)
    return w.apply_golden_recipe(w.portable_state_dict(desc, 21)), desc


def _rec(seconds, seed):
    x = pkg("synth").synth_meeting(float(seconds), 7, seed=seed)
    return np.ascontiguousarray(x[0] if x.ndim == 3 else x, dtype=np.float32)


def _sep(model):
    return pkg("separator").HipSeparator(model[0], None, device=0)


def _toggling_cfg(sep, x, percentile=70):
    """test_device_handoff_to_whisper_front_end's recipe: a threshold at the 70th percentile of this model's activity on x,
    dilation 0.05 s, erosion 0.02 s, so that the gate really toggles (a higher percentile: a sparser gate, longer pauses)"""
    css, L = pkg("css"), pkg("_lib")
    h = sep.handle
    h.run(x, css.make_run_cfg(css.CssCfg(activity_th=0.0, show_progressbar=False), 16000, 7))
    th = float(np.percentile(h.read(L.BUF_ACTIVITY), percentile))
    return css.CssCfg(activity_th=th, show_progressbar=False, activity_dilation_sec=0.05, activity_erosion_sec=0.02)


def _offline(sep, x, cfg, configs=CONFIGS):
    """css_run_device on the whole recording -> (waveforms, gate bits, {config index: [(mel, regions) per stream]})"""
    import torch
    css, L = pkg("css"), pkg("_lib")
    h = sep.handle
    rc = css.make_run_cfg(cfg, 16000, 7)
    n_out = int(L.plan(sep.desc, rc, x.shape[0]).n_out)
    pcm = torch.from_numpy(x).cuda()
    wav = torch.empty((3, n_out), dtype=torch.float32, device="cuda")
    h.run_device(pcm.data_ptr(), x.shape[0], 7, rc, wav.data_ptr(), n_out)
    torch.cuda.synchronize()
    act = h.read(L.BUF_ACT_FINAL).copy()
    res = {i: [h.handoff_logmel(wav.data_ptr(), n_out, k, **c) for k in range(3)] for i, c in enumerate(configs)}
    return wav.cpu().numpy(), act, res


def _merged(ranges):
    out = []
    for a, b in ranges:
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], int(b))
        else:
            out.append([int(a), int(b)])
    return np.array(out, np.int64).reshape(-1, 2)


class _Run:
    """one stream with the hand-off on: pushes, keeps every call's Handoff, checks what holds for every call"""

    def __init__(self, sep, cfg, hcfg):
        self.s = pkg("stream").CssStream(sep, cfg, handoff=hcfg)
        self.hcfg, self.calls, self.wav, self.n = hcfg, [], [], 0

    def took(self, wav, n):
        h = self.s.handoff
        self.n += n
        for k in range(3):
            assert h.mel[k].shape[0] == self.hcfg["n_mels"] and h.mel[k].dtype == np.float32
            r = h.ranges[k]
            assert (r[:, 0] < r[:, 1]).all() and (r[1:, 0] > r[:-1, 1]).all()      # ascending, disjoint, touching ones merged
            if h.mel[k].size:
                assert h.raw_max[k] >= h.mel[k].max()
        assert h.first_activity_frame == sum(c.activity[0].shape[0] for c in self.calls)
        if not self.hcfg["drop_silence"] and self.n >= 0:
            assert sum(c.mel[0].shape[1] for c in self.calls) + h.mel[0].shape[1] == self.s.handoff_final_frames(self.n)
        self.calls.append(h)
        self.wav.append(np.stack(wav))

    def push(self, chunk):
        self.took(self.s.push(chunk), chunk.shape[0])

    def finish(self):
        n = self.n
        self.n = -1
        self.took(self.s.finish(), 0)
        self.n = n

    def total(self, k):
        raw = np.concatenate([c.mel[k] for c in self.calls], axis=1)
        ranges = _merged(np.concatenate([c.ranges[k] for c in self.calls]))
        act = np.concatenate([c.activity[k] for c in self.calls])
        return raw, ranges, act


def _same(a, b):
    for k in range(3):
        assert np.array_equal(a.mel[k], b.mel[k]) and np.array_equal(a.ranges[k], b.ranges[k]) and np.array_equal(a.activity[k], b.activity[k])
    assert np.array_equal(a.raw_max, b.raw_max) and a.first_activity_frame == b.first_activity_frame


def _stream_and_compare(sep, x, cfg, configs, wav, act, off):
    """every configuration streamed with the grouped-push test's chunk sizes cycled and with equal 1.5 s ticks: after finish
    the normalised frames, the merged ranges and the gate bits are the offline call's"""
    S = pkg("stream")
    for ci, hcfg in enumerate(configs):
        for sizes in (itertools.cycle(CHUNKS), itertools.repeat(24000)):
            run = _Run(sep, cfg, hcfg)
            n = 0
            for size in sizes:
                if n >= x.shape[0]:
                    break
                run.push(x[n:n + size])
                n += size
            run.finish()
            assert np.array_equal(np.concatenate(run.wav, axis=1), wav)
            for k in range(3):
                raw, ranges, a = run.total(k)
                mel, regions = off[ci][k]
                assert np.array_equal(a, act[k])
                assert np.array_equal(ranges, regions)
                assert raw.shape[1] == int((regions[:, 1] - regions[:, 0]).sum()) // 160 == mel.shape[1]
                assert run.calls[-1].raw_max[k] == raw.max()
                assert np.array_equal(S.whisper_normalize(raw, run.calls[-1].raw_max[k]), mel), (ci, k)
            run.s.close()


def test_streamed_equals_offline(model):
    """20 s, a gate that toggles, three hand-off configurations, the chunk sizes of the grouped-push test cycled and a run of
    equal 1.5 s ticks: after finish the normalised frames, the merged ranges and the gate bits are the offline call's."""
    sep = _sep(model)
    x = _rec(20.0, 12)
    cfg = _toggling_cfg(sep, x)
    wav, act, off = _offline(sep, x, cfg)
    n_out = wav.shape[1]
    # The input exercises the gate: it moves, it cuts at least two speakers into several regions, every speaker loses at
    # least a tenth of its samples.  The three conditions are taken on the gate's own regions -- pad_frames = 0, the second
    # configuration -- because they are about the input, and padding is not: with this recipe the gate is on for about
    # 85 % of the frames in runs a few frames apart, and 8 frames of padding on either side close every gap under 18
    # frames.  The numpy oracle on 24 recordings of this generator (seeds 1 .. 12, 20 s and 40 s) finds none that loses
    # more than 4.3 % of a speaker at pad 8; this recording (seed 12, 20 s) has 36 / 28 / 28 regions at pad 0 and loses
    # 12.2 / 12.9 / 10.8 % there, and has 1 / 2 / 1 regions and loses 0 / 0.1 / 0.2 % at pad 8.  The padded
    # configurations get a recording of their own on which they drop: test_streamed_equals_offline_when_padded_regions_drop.
    assert 0.05 < act.astype(bool).mean() < 0.95
    for ci, hcfg in enumerate(CONFIGS):
        regs = [off[ci][k][1] for k in range(3)]
        print(hcfg, "regions per speaker", [len(r) for r in regs], "kept share", [float((r[:, 1] - r[:, 0]).sum()) / n_out for r in regs])
        if hcfg["drop_silence"]:
            assert all(np.array_equal(r, O.active_regions(act[k].astype(bool), hcfg["pad_frames"], n_out)) for k, r in enumerate(regs))
    gate_regs = [off[1][k][1] for k in range(3)]
    assert CONFIGS[1]["pad_frames"] == 0 and CONFIGS[1]["drop_silence"]
    assert sum(len(r) >= 2 for r in gate_regs) >= 2
    assert all((r[:, 1] - r[:, 0]).sum() <= 0.9 * n_out for r in gate_regs)
    _stream_and_compare(sep, x, cfg, CONFIGS, wav, act, off)
    sep.close()


PADDED = (dict(n_mels=80, pad_frames=8, drop_silence=True), dict(n_mels=128, pad_frames=3, drop_silence=True))


def test_streamed_equals_offline_when_padded_regions_drop(model):
    """The same recording (seed 12, 20 s) with a sparser gate, so that configurations WITH padding really drop: the recipe's
    threshold at the 95th percentile instead of the 70th (dilation and erosion unchanged) turns the gate on for about a
    quarter of the frames, with pauses longer than 2 pad + 2 frames.  The issue's two conditions -- at least two speakers
    with several regions, every speaker loses a tenth of its samples -- are asserted on each configuration's OWN regions
    (numpy oracle: 22 / 18 / 15 regions and 33 / 32 / 35 % dropped at pad 8; 34 / 39 / 30 regions and 55 / 54 / 53 % at
    pad 3).  This is the case that exercises, against the offline call, the membership window t - pad - 1 .. t + pad, the
    carried undecided samples feeding a compaction that skips blocks, and the reach of 2 pad + 1 frames back into the ring."""
    sep = _sep(model)
    x = _rec(20.0, 12)
    cfg = _toggling_cfg(sep, x, percentile=95)
    wav, act, off = _offline(sep, x, cfg, PADDED)
    n_out = wav.shape[1]
    assert 0.05 < act.astype(bool).mean() < 0.95
    for ci, hcfg in enumerate(PADDED):
        regs = [off[ci][k][1] for k in range(3)]
        print(hcfg, "regions per speaker", [len(r) for r in regs], "kept share", [float((r[:, 1] - r[:, 0]).sum()) / n_out for r in regs])
        assert all(np.array_equal(r, O.active_regions(act[k].astype(bool), hcfg["pad_frames"], n_out)) for k, r in enumerate(regs))
        assert sum(len(r) >= 2 for r in regs) >= 2
        assert all((r[:, 1] - r[:, 0]).sum() <= 0.9 * n_out for r in regs)
    _stream_and_compare(sep, x, cfg, PADDED, wav, act, off)
    sep.close()


def test_finality(model):
    """the same 12 s continued by two different recordings: everything returned before they diverge is identical"""
    sep = _sep(model)
    a, b = _rec(24.0, 31), _rec(24.0, 32)
    b[:16000 * 12] = a[:16000 * 12]
    cfg = _toggling_cfg(sep, a, percentile=95)      # (a sparse gate: the pad-8 configuration really drops)
    runs = []
    for x in (a, b):
        run = _Run(sep, cfg, CONFIGS[0])
        for n in range(0, x.shape[0], 24000):
            run.push(x[n:n + 24000])
        run.finish()
        run.s.close()
        runs.append(run)
    before = 16000 * 12 // 24000
    assert sum(c.mel[0].shape[1] + c.mel[1].shape[1] + c.mel[2].shape[1] for c in runs[0].calls[:before]) > 0
    for ca, cb in zip(runs[0].calls[:before], runs[1].calls[:before]):
        _same(ca, cb)
    assert not all(np.array_equal(ca.mel[k], cb.mel[k]) for ca, cb in zip(runs[0].calls[before:], runs[1].calls[before:]) for k in range(3))
    sep.close()


def test_grouped_equals_single(model):
    """16 streams of one separator (drop / no drop, 80 / 128 bands, two pad_frames, two without the hand-off) pushed as a group
    with seeded chunk sizes, and each recording alone with the same chunks: every call returns the same hand-off.  The two
    streams without it return css_run's samples as before."""
    CSS, S = pkg("css"), pkg("stream")
    sep = _sep(model)
    recs = [_rec(12 + 4 * i / 15, 700 + i) for i in range(16)]
    cfg = _toggling_cfg(sep, recs[0])
    variants = [dict(n_mels=80, pad_frames=8, drop_silence=True), dict(n_mels=128, pad_frames=3, drop_silence=True),
                dict(n_mels=80, pad_frames=0, drop_silence=False), dict(n_mels=128, pad_frames=8, drop_silence=False)]
    hcfgs = [None if i in (5, 11) else variants[i % 4] for i in range(16)]
    rc = CSS.make_run_cfg(cfg, 16000, 7)
    refs = {i: sep.handle.run(recs[i], rc).copy() for i in (5, 11)}
    rs = np.random.RandomState(3)
    plan = []                                            # per round: chunk size (or None) per stream
    pos = [0] * 16
    while any(p < x.shape[0] for p, x in zip(pos, recs)):
        row = []
        for i in range(16):
            size = int(CHUNKS[rs.randint(len(CHUNKS))])
            if rs.rand() < 0.15 or pos[i] >= recs[i].shape[0]:
                row.append(None)
            else:
                row.append(min(size, recs[i].shape[0] - pos[i]))
                pos[i] += row[-1]
        plan.append(row)

    def feed(streams, only=None):
        """-> per stream the list of (waveform piece, Handoff or None) of its calls"""
        got = [[] for _ in streams]
        group = S.CssStreamGroup(streams) if only is None else None
        pos = [0] * 16
        for row in plan:
            chunks = []
            for i in range(16):
                chunks.append(None if row[i] is None else recs[i][pos[i]:pos[i] + row[i]])
                pos[i] += row[i] or 0
            if group is not None:
                res = group.push(chunks)
                for i, s in enumerate(streams):
                    if chunks[i] is not None:
                        got[i].append((np.stack(res[i]), s.handoff))
            elif chunks[only] is not None:
                got[0].append((np.stack(streams[0].push(chunks[only])), streams[0].handoff))
        for i, s in enumerate(streams):
            got[i].append((np.stack(s.finish()), s.handoff))
            s.close()
        return got

    grouped = feed([S.CssStream(sep, cfg, handoff=h) for h in hcfgs])
    for i in (5, 11):                                    # hand-off off: the samples of css_run, nothing else
        assert all(h is None for _, h in grouped[i])
        assert np.array_equal(np.concatenate([w for w, _ in grouped[i]], axis=1), refs[i])
    emitted = 0
    for i in range(16):
        single = feed([S.CssStream(sep, cfg, handoff=hcfgs[i])], only=i)[0]
        assert len(single) == len(grouped[i])
        for (wg, hg), (ws, hs) in zip(grouped[i], single):
            assert np.array_equal(wg, ws)
            if hcfgs[i] is not None:
                _same(hg, hs)
                emitted += sum(m.shape[1] for m in hg.mel)
    assert emitted > 0
    sep.close()


def test_launches_do_not_grow_with_the_streams(model):
    """No clock: a grouped tick of 16 streams and one of 4 (one round each) cost the same number of hand-off launches, one of
    them the DFT product."""
    CSS, S = pkg("css"), pkg("stream")
    sep = _sep(model)
    x = _rec(4.0, 40)[:50000]
    stats = []
    for count in (16, 4):
        streams = [S.CssStream(sep, CSS.CssCfg(), handoff=CONFIGS[i % 3]) for i in range(count)]
        S.CssStreamGroup(streams).push([x] * count)
        assert all(s.handoff.activity[0].shape[0] > 0 for s in streams)      # every stream took part in the round's hand-off
        stats.append(sep.handle.stream_handoff_stats())
        for s in streams:
            s.close()
    print("hand-off (launches, products, operand frames) for 16 and 4 streams:", stats)
    assert stats[0][:2] == stats[1][:2] == (3, 1)
    assert stats[0][2] > stats[1][2] > 0
    sep.close()


def test_a_whisper_window(model):
    """One stream, no drop, 35 s: frames [0, 3000) normalised with their own maximum against the oracle's log-mel of the
    first 30 s of css_run's waveform, at the bar the offline hand-off is held to (max 2e-3, rms 2e-4), except the frames
    whose support leaves the window on the right (reflection in the oracle, real samples in the stream)."""
    CSS, S = pkg("css"), pkg("stream")
    sep = _sep(model)
    x = _rec(35.0, 41)
    cfg = CSS.CssCfg()
    wav = sep.handle.run(x, CSS.make_run_cfg(cfg, 16000, 7)).copy()
    run = _Run(sep, cfg, CONFIGS[2])
    for n in range(0, x.shape[0], 24000):
        run.push(x[n:n + 24000])
    run.finish()
    run.s.close()
    edge = [j for j in range(3000) if 160 * j + 200 > 480000]
    assert 1 <= len(edge) <= 2
    inner = np.array([j for j in range(3000) if j not in edge])
    for k in range(3):
        raw = run.total(k)[0]
        assert raw.shape[1] >= 3000
        got = S.whisper_normalize(raw[:, :3000])
        ref = O.whisper_log_mel(wav[k, :480000], 80)
        assert ref.shape == (80, 3000)
        d = (got - ref)[:, inner]
        print("speaker", k, "max", float(np.abs(d).max()), "rms", float(np.sqrt(np.mean(d ** 2))))
        assert np.abs(d).max() < 2e-3 and np.sqrt(np.mean(d ** 2)) < 2e-4
    sep.close()


def _raw_out(S_, n_mels, frames, ranges, activity):
    L = pkg("_lib")
    keep = dict(mel=np.empty((S_, n_mels, max(frames, 1)), np.float32), ranges=np.empty((S_, max(ranges, 1), 2), np.int64),
                act=np.empty((S_, max(activity, 1)), np.uint8), nf=np.zeros(S_, np.int64), nr=np.zeros(S_, np.int32), mx=np.zeros(S_, np.float32))
    o = L.CssStreamHandoffOut()
    o.mel_host, o.cap_frames = keep["mel"].ctypes.data, frames
    o.ranges_host, o.cap_ranges = keep["ranges"].ctypes.data, ranges
    o.activity_host, o.cap_activity = keep["act"].ctypes.data, activity
    o.n_frames, o.n_ranges, o.raw_max = keep["nf"].ctypes.data, keep["nr"].ctypes.data, keep["mx"].ctypes.data
    return o, keep


def test_refusals_leave_the_stream_unchanged(model):
    L, CSS, S = pkg("_lib"), pkg("css"), pkg("stream")
    sep = _sep(model)
    h = sep.handle
    x = _rec(12.0, 50)
    cfg = _toggling_cfg(sep, x, percentile=95)      # (a sparse gate: the pad-8 configuration really drops)
    info = lambda s: (s.info().n_pushed, s.info().n_emitted, s.info().finished, s.info().device_bytes)
    # bad configurations; a stream that has samples; a second open
    plain = S.CssStream(sep, cfg)
    bytes_off = plain.info().device_bytes
    for bad in (L.handoff_cfg(64, 8, True), L.handoff_cfg(80, -1, True)):
        assert h.lib.css_stream_handoff_open(h.h, plain.id, C.byref(bad)) == L.CSS_ERR_INVALID_ARG
    plain.push(x[:1000])
    assert h.lib.css_stream_handoff_open(h.h, plain.id, C.byref(L.handoff_cfg())) == L.CSS_ERR_STATE
    assert h.lib.css_stream_handoff_bind(h.h, plain.id, None) == L.CSS_ERR_STATE
    plain.close()
    s, twin = (S.CssStream(sep, cfg, handoff=CONFIGS[0]) for _ in range(2))
    assert s.info().device_bytes > bytes_off                                  # the hand-off's buffers are counted
    assert h.lib.css_stream_handoff_open(h.h, s.id, C.byref(L.handoff_cfg())) == L.CSS_ERR_STATE
    first = x[:60000]
    assert np.array_equal(np.stack(s.push(first)), np.stack(twin.push(first)))
    _same(s.handoff, twin.handoff)
    # nothing bound: CSS_ERR_STATE, for a push and for finish
    chunk = x[60000:60000 + 40000]
    out = np.empty((3, chunk.shape[0] + s.latency_samples), np.float32)
    n_out = C.c_int64()
    push = lambda: h.lib.css_stream_push(h.h, s.id, chunk.ctypes.data_as(C.c_void_p), chunk.shape[0], out.ctypes.data_as(C.c_void_p),
                                         out.shape[1], C.byref(n_out))
    before = info(s)
    assert h.lib.css_stream_handoff_bind(h.h, s.id, None) == L.CSS_OK
    assert push() == L.CSS_ERR_STATE and info(s) == before
    assert h.lib.css_stream_finish(h.h, s.id, out.ctypes.data_as(C.c_void_p), out.shape[1], C.byref(n_out)) == L.CSS_ERR_STATE and info(s) == before
    # one frame / one range / one gate byte below the bound: CSS_ERR_INVALID_ARG, the stream unchanged
    need = s.handoff_bounds(chunk.shape[0])
    for short in range(3):
        caps = [n - (1 if i == short else 0) for i, n in enumerate(need)]
        o, keep = _raw_out(3, 80, *caps)
        assert h.lib.css_stream_handoff_bind(h.h, s.id, C.byref(o)) == L.CSS_OK
        assert push() == L.CSS_ERR_INVALID_ARG and info(s) == before
    # a refused item of a group leaves the other streams of the call unchanged too
    items = (L.CssStreamPush * 2)()
    out2 = np.empty_like(out)
    twin._handoff_bind(chunk.shape[0])
    for it, st, buf in ((items[0], twin, out2), (items[1], s, out)):
        it.id, it.pcm_host, it.n_samples, it.out_host, it.cap = st.id, chunk.ctypes.data, chunk.shape[0], buf.ctypes.data, buf.shape[1]
    tb = info(twin)
    assert h.lib.css_stream_push_many(h.h, items, 2, None) == L.CSS_ERR_INVALID_ARG and info(twin) == tb and info(s) == before
    assert "item 1" in h.lib.css_last_error(h.h).decode()
    # the same push with enough room returns what the undisturbed twin returns, to the end
    for n in range(60000, x.shape[0], 40000):
        assert np.array_equal(np.stack(s.push(x[n:n + 40000])), np.stack(twin.push(x[n:n + 40000])))
        _same(s.handoff, twin.handoff)
    assert np.array_equal(np.stack(s.finish()), np.stack(twin.finish()))
    _same(s.handoff, twin.handoff)
    s.close()
    twin.close()
    sep.close()


def test_the_handles_own_session_is_untouched(model):
    """css_run and css_run_device + css_handoff_logmel between the pushes of a hand-off stream give the bits they give without
    it (the mel tables of the two paths are separate), and the stream ends equal to an undisturbed one."""
    CSS, S = pkg("css"), pkg("stream")
    sep = _sep(model)
    x, other = _rec(14.0, 60), _rec(9.0, 61)
    cfg = _toggling_cfg(sep, x)
    ocfg = _toggling_cfg(sep, other)
    alone = _Run(sep, cfg, CONFIGS[1])
    for n in range(0, x.shape[0], 24000):
        alone.push(x[n:n + 24000])
    alone.finish()
    alone.s.close()
    w0, a0, off0 = _offline(sep, other, ocfg)
    run = _Run(sep, cfg, CONFIGS[1])
    for n in range(0, x.shape[0], 24000):
        run.push(x[n:n + 24000])
        assert np.array_equal(sep.handle.run(other, CSS.make_run_cfg(ocfg, 16000, 7)), w0)
        if n in (48000, 96000, 192000):
            w1, a1, off1 = _offline(sep, other, ocfg)
            assert np.array_equal(w1, w0) and np.array_equal(a1, a0)
            for ci in off0:
                for k in range(3):
                    assert np.array_equal(off1[ci][k][0], off0[ci][k][0]) and np.array_equal(off1[ci][k][1], off0[ci][k][1])
    run.finish()
    run.s.close()
    assert len(run.calls) == len(alone.calls)
    for ca, cb in zip(run.calls, alone.calls):
        _same(ca, cb)
    sep.close()
