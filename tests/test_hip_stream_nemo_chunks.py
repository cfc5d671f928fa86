"""NeMo chunks out of a stream's frame history on the MI355X (include/css_mi355_nemo_chunk.h; stream.py CssStream(nemo_history=...),
nemo_chunk, CssStreamGroup.nemo_chunks): the ring follows the pushes, raw chunks are the frames the pushes returned and normalised
chunks their numpy statement, bit for bit; the hand-off itself, its launches and a stream without a history stay as they were.  The
2-block model, the recordings and the toggling-gate recipe are tests/test_hip_stream_nemo.py's."""
import ctypes as C

import numpy as np
import pytest

import nemo_chunk_reference as M
from conftest import pkg
from test_hip_stream_nemo import CONFIGS, _main, _rec, _same, model, sep  # noqa: F401  (the fixtures and the shared recording)

pytestmark = pytest.mark.gpu

TICK = 24000


def _bits(t):
    """a torch tensor's words on the host"""
    a = t.detach().cpu().contiguous().numpy()
    return a.view(np.uint16 if a.itemsize == 2 else np.uint32)


def _words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.itemsize == 2 else np.uint32)


class _Tracked:
    """a NeMo stream with a history of H frames: keeps every frame the calls returned and holds the history to them after each call"""

    def __init__(self, sep, cfg, ncfg, H):
        S = pkg("stream")
        self.s = S.CssStream(sep, cfg, nemo=ncfg, nemo_history=H)
        self.group = S.CssStreamGroup([self.s])
        self.H, self.n_mels = H, ncfg["n_mels"]
        self.frames = [np.zeros((self.n_mels, 0), np.float32) for _ in range(3)]
        self.checked = 0

    def took(self):
        S = pkg("stream")
        h = self.s.nemo
        for k in range(3):
            self.frames[k] = np.concatenate([self.frames[k], h.mel[k]], axis=1)
        first, end = self.s.nemo_history_range()
        J = np.array([f.shape[1] for f in self.frames])
        assert np.array_equal(end, J) and np.array_equal(first, np.maximum(J - self.H, 0))
        live = [k for k in range(3) if J[k] > 0]
        if not live:
            return
        width = int((end - first).max())
        held = {k: self.frames[k][:, first[k]:end[k]] for k in live}
        # RAW chunks of the whole range: the last frames the pushes returned
        raw = self.group.nemo_chunks([(self.s, k) for k in live], width, None, "float32", -7.0)
        assert self.group.window_launches == 1 and self.s.chunk_mean is None
        for i, k in enumerate(live):
            want, _, _ = M.chunk(held[k], width, False, np.float32, -7.0)
            assert np.array_equal(_bits(raw[i]), _words(want)), ("raw", k)
        # PER_FEATURE chunks: the numpy statement of those frames, which is the model
        for dtype in ("float32", "float16"):
            got = self.group.nemo_chunks([(self.s, k) for k in live], width, "per_feature", dtype, 0.0)
            for i, k in enumerate(live):
                want, mean, std = M.chunk(held[k], width, True, np.dtype(dtype), 0.0)
                assert np.array_equal(_words(S.nemo_chunk_features(held[k], width, "per_feature", dtype, 0.0)), _words(want))
                assert np.array_equal(_bits(got[i]), _words(want)), (dtype, k)
            assert np.array_equal(M.bits(self.s.chunk_mean), M.bits(mean)) and np.array_equal(M.bits(self.s.chunk_std), M.bits(std))
        self.checked += len(live)


@pytest.mark.parametrize("H,ci", ((32, 2), (256, 0)), ids=("hist32-nodrop", "hist256-drop"))
def test_history_follows_the_pushes(sep, H, ci):
    """after every push and after finish: the range, raw and normalised chunks of the whole range; the twin without a history returns
    the same hand-off outputs with the same launches, and holds exactly the ring less on the device"""
    S = pkg("stream")
    x, cfg, *_ = _main(sep)
    ncfg = CONFIGS[ci]
    run = _Tracked(sep, cfg, ncfg, H)
    twin = S.CssStream(sep, cfg, nemo=ncfg)
    assert run.s.info().device_bytes - twin.info().device_bytes == 3 * ncfg["n_mels"] * H * 4
    most_new = 0
    for n in range(0, x.shape[0], TICK):
        wav = run.s.push(x[n:n + TICK])
        stats = sep.handle.stream_handoff_stats()[:2]
        alone = twin.push(x[n:n + TICK])
        assert sep.handle.stream_handoff_stats()[:2] == stats and stats in ((0, 0), (3, 1))      # three launches per round, history or not
        assert np.array_equal(np.stack(wav), np.stack(alone))
        _same(run.s.nemo, twin.nemo)
        most_new = max(most_new, max(m.shape[1] for m in run.s.nemo.mel))
        run.took()
    wav, alone = run.s.finish(), twin.finish()
    assert np.array_equal(np.stack(wav), np.stack(alone))
    _same(run.s.nemo, twin.nemo)
    run.took()
    at_finish = max(m.shape[1] for m in run.s.nemo.mel)
    print("history", H, "most frames of a push", most_new, "of finish", at_finish, "chunks checked", run.checked)
    assert run.checked >= 6 and most_new > 32
    if H == 32:
        assert at_finish > H        # a round that completes more frames than the ring holds
    assert run.s.info().device_bytes - twin.info().device_bytes == 3 * ncfg["n_mels"] * H * 4
    # spans inside the range, at every alignment of the destination the element size allows
    import torch
    k = int(np.argmax([f.shape[1] for f in run.frames]))
    first, end = run.s.nemo_history_range()
    n = min(int(end[k] - first[k]), 21)
    for dtype, el in (("float32", 4), ("float16", 2)):
        buf = torch.full((ncfg["n_mels"], 64), 3.0, dtype=getattr(torch, dtype), device="cuda")
        for shift in (1, 2, 3):
            view = buf[:, shift:shift + n + 2]
            got = run.s.nemo_chunk(k, int(end[k]) - n - 1, n, n + 2, "per_feature", dtype, 0.5, out=view)
            assert got.data_ptr() == view.data_ptr() and got.data_ptr() % 16 == (buf.data_ptr() + shift * el) % 16
            want, _, _ = M.chunk(run.frames[k][:, end[k] - n - 1:end[k] - 1], n + 2, True, np.dtype(dtype), 0.5)
            assert np.array_equal(_bits(view), _words(want))
            assert (buf[:, :shift] == 3.0).all() and (buf[:, shift + n + 2:] == 3.0).all()
            buf.fill_(3.0)
    run.s.close()
    twin.close()


def test_seventeen_streams_fifty_one_chunks_two_launches(sep):
    S = pkg("stream")
    x = _rec(4.0, 40)
    cfg = pkg("css").CssCfg()
    streams = [S.CssStream(sep, cfg, nemo=CONFIGS[2], nemo_history=(32, 100, 256)[i % 3]) for i in range(17)]
    group = S.CssStreamGroup(streams)
    group.push([x * np.float32(1.0 - 0.03 * i) for i in range(17)])
    assert sep.handle.stream_handoff_stats()[:2] == (5, 1)          # 17 streams: two tables per kernel, one product
    reqs = [(s, k) for s in streams for k in range(3)]
    assert all(s.nemo_history_range()[1].min() > 32 for s in streams)
    got = group.nemo_chunks(reqs, 300, "per_feature", "float16", 0.0)
    assert group.window_launches == 2 and tuple(got.shape) == (51, 80, 300)
    for i, (s, k) in enumerate(reqs):
        alone = s.nemo_chunk(k, width=300, normalize="per_feature", dtype="float16")
        assert np.array_equal(_bits(got[i]), _bits(alone)), i
        first, end = s.nemo_history_range()
        assert end[k] - first[k] == min(s.nemo_history, end[k])
    assert len({_bits(got[3 * i]).tobytes() for i in range(17)}) == 17      # (the streams really differ)
    for s in streams:
        s.close()


def test_a_group_of_both_formats_serves_each_its_own_call(sep):
    L, S = pkg("_lib"), pkg("stream")
    h = sep.handle
    x = _rec(4.0, 40)
    cfg = pkg("css").CssCfg()
    w = S.CssStream(sep, cfg, handoff=dict(n_mels=80, pad_frames=8, drop_silence=False), window_history=256)
    n = S.CssStream(sep, cfg, nemo=CONFIGS[2], nemo_history=256)
    group = S.CssStreamGroup([w, n])
    group.push([x, x])
    win = group.windows([(w, 0)], 300, "float16")
    chunk = group.nemo_chunks([(n, 0)], 300, "per_feature", "float16")
    assert np.array_equal(_bits(win[0]), _bits(w.window(0, width=300))) and np.array_equal(_bits(chunk[0]), _bits(n.nemo_chunk(0, width=300, dtype="float16")))
    assert not np.array_equal(_bits(win[0]), _bits(chunk[0]))
    with pytest.raises(ValueError):
        group.windows([(n, 0)], 300)
    with pytest.raises(ValueError):
        group.nemo_chunks([(w, 0)], 300)
    import torch
    out = torch.full((80, 300), 3.0, dtype=torch.float32, device="cuda")
    first, end = np.zeros(3, np.int64), np.zeros(3, np.int64)
    p64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    err = lambda: h.lib.css_last_error(h.h).decode()
    wi = (L.CssStreamWindow * 1)()
    wi[0].id, wi[0].speaker, wi[0].first_frame, wi[0].n_frames, wi[0].width, wi[0].dtype, wi[0].out_dev, wi[0].ld = n.id, 0, 0, 10, 300, 0, out.data_ptr(), 300
    assert h.lib.css_stream_windows(h.h, wi, 1, None) == L.CSS_ERR_INVALID_ARG and "item 0" in err()
    assert h.lib.css_stream_window_range(h.h, n.id, p64(first), p64(end)) == L.CSS_ERR_STATE
    ci = (L.CssStreamNemoChunk * 1)()
    ci[0].id, ci[0].speaker, ci[0].first_frame, ci[0].n_frames, ci[0].width, ci[0].normalize, ci[0].out_dev, ci[0].ld = w.id, 0, 0, 10, 300, 1, out.data_ptr(), 300
    assert h.lib.css_stream_nemo_chunks(h.h, ci, 1, None) == L.CSS_ERR_INVALID_ARG and "item 0" in err() and f"stream {w.id}" in err()
    assert h.lib.css_stream_nemo_history_range(h.h, w.id, p64(first), p64(end)) == L.CSS_ERR_STATE
    assert h.lib.css_stream_nemo_history_open(h.h, w.id, 256) == L.CSS_ERR_STATE and "Whisper" in err()
    torch.cuda.synchronize()
    assert (out == 3.0).all()
    w.close()
    n.close()


def test_a_plain_preview_never_writes_the_ring(sep):
    S = pkg("stream")
    x, cfg, *_ = _main(sep)
    a, b = (S.CssStream(sep, cfg, nemo=CONFIGS[0], nemo_history=64) for _ in range(2))
    seen = 0
    for i, n in enumerate(range(0, 5 * TICK, TICK)):
        a.push(x[n:n + TICK])
        b.push(x[n:n + TICK])
        live = [k for k in range(3) if a.nemo_history_range()[1][k] > 0]
        before = [_bits(a.nemo_chunk(k, normalize=None)) for k in live]
        if i >= 2:
            assert len(a.preview()) == 3       # (css_run of the prefix needs more than one segment)
        for k, was in zip(live, before):
            assert np.array_equal(_bits(a.nemo_chunk(k, normalize=None)), was)
            assert np.array_equal(_bits(b.nemo_chunk(k, normalize=None)), was)
            assert np.array_equal(_bits(a.nemo_chunk(k, dtype="float16")), _bits(b.nemo_chunk(k, dtype="float16")))
            seen += 1
        assert np.array_equal(a.nemo_history_range()[1], b.nemo_history_range()[1])
    assert seen >= 3
    a.close()
    b.close()


def test_refusals_write_nothing(sep):
    import torch
    L, S = pkg("_lib"), pkg("stream")
    h = sep.handle
    x = _rec(4.0, 40)
    cfg = pkg("css").CssCfg()
    err = lambda: h.lib.css_last_error(h.h).decode()
    # ---- the open call: the size, twice, after the first sample; the stream stays as it was
    s = S.CssStream(sep, cfg, nemo=CONFIGS[2])
    bytes_off = s.info().device_bytes
    for bad in (31, 0, -1, (1 << 20) + 1):
        assert h.lib.css_stream_nemo_history_open(h.h, s.id, bad) == L.CSS_ERR_INVALID_ARG
    assert s.info().device_bytes == bytes_off
    assert h.lib.css_stream_nemo_history_open(h.h, s.id, 64) == L.CSS_OK
    bytes_on = s.info().device_bytes
    assert bytes_on - bytes_off == 3 * 80 * 64 * 4
    assert h.lib.css_stream_nemo_history_open(h.h, s.id, 64) == L.CSS_ERR_STATE and s.info().device_bytes == bytes_on
    s.nemo_history = 64
    late, plain = S.CssStream(sep, cfg, nemo=CONFIGS[2]), S.CssStream(sep, cfg)
    late.push(x[:1000])
    assert h.lib.css_stream_nemo_history_open(h.h, late.id, 64) == L.CSS_ERR_STATE
    assert h.lib.css_stream_nemo_history_open(h.h, plain.id, 64) == L.CSS_ERR_STATE
    with pytest.raises(ValueError):
        S.CssStream(sep, cfg, nemo_history=64)
    with pytest.raises(ValueError):
        S.CssStream(sep, cfg, nemo=CONFIGS[0], window_history=64)
    with pytest.raises(ValueError):
        late.nemo_chunk(0)
    with pytest.raises(L.CssError):
        late.nemo_history_range()
    # ---- the chunks call: before the first frame the defaults have no span to name, which Python says itself
    assert s.nemo_history_range()[1].max() == 0
    for call in (lambda: s.nemo_chunk(0), lambda: s.nemo_chunk(1, width=100, normalize=None), lambda: S.CssStreamGroup([s]).nemo_chunks([(s, 2)], 64)):
        with pytest.raises(ValueError, match="no frames retained yet"):
            call()
    s.push(x)
    first, end = s.nemo_history_range()
    assert end[0] > 64 and first[0] == end[0] - 64
    out = torch.full((80, 80), 3.0, dtype=torch.float32, device="cuda")
    mean, std = np.full(80, 7.0, np.float32), np.full(80, 7.0, np.float32)

    def item(**kw):
        it = dict(id=s.id, speaker=0, first_frame=int(first[0]), n_frames=40, width=64, dtype=0, normalize=1, pad_value=0.0, reserved=0,
                  out_dev=out.data_ptr(), ld=80, mean_host=mean.ctypes.data, std_host=std.ctypes.data)
        it.update(kw)
        return it

    def call(*items):
        tab = (L.CssStreamNemoChunk * len(items))()
        for t, it in zip(tab, items):
            for k, v in it.items():
                setattr(t, k, v)
        launches = C.c_int32(-7)
        return h.lib.css_stream_nemo_chunks(h.h, tab, len(items), C.byref(launches)), launches.value

    bad = [dict(id=late.id), dict(id=plain.id), dict(id=63), dict(id=-1), dict(speaker=3), dict(speaker=-1), dict(first_frame=int(first[0]) - 1),
           dict(first_frame=int(end[0]) - 39), dict(n_frames=0), dict(n_frames=65, width=65), dict(width=39), dict(width=3001, ld=3001), dict(ld=63),
           dict(dtype=2), dict(dtype=-1), dict(normalize=2), dict(normalize=-1), dict(pad_value=float("inf")), dict(pad_value=float("nan")),
           dict(reserved=1), dict(out_dev=None), dict(out_dev=out.data_ptr() + 2), dict(dtype=1, out_dev=out.data_ptr() + 1)]
    for kw in bad:
        rc, launches = call(item(), item(**kw))
        assert rc == L.CSS_ERR_INVALID_ARG and launches == -7, (kw, rc)
        assert "item 1" in err() and f"stream {item(**kw)['id']}" in err(), (kw, err())
        torch.cuda.synchronize()
        assert (out == 3.0).all() and (mean == 7.0).all() and (std == 7.0).all(), kw
    assert call() == (L.CSS_OK, 0)
    # ... and the accepted call writes its columns and the statistics, and nothing else of `out`
    assert call(item()) == (L.CSS_OK, 1)
    torch.cuda.synchronize()
    assert (out[:, 64:] == 3.0).all() and (out[:, 40:64] == 0.0).all() and not (out[:, :40] == 3.0).any() and (mean != 7.0).all()
    assert s.info().device_bytes == bytes_on
    for st in (s, late, plain):
        st.close()
