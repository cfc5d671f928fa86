"""Streaming separation on the MI355X (css_stream_*, notsofar1-challenge_amd/stream.py): whatever the chunking, every push
returns exactly the samples css_stream_final_samples says are final, they equal css_run's output on the whole recording bit
for bit, and a finished stream's output IS css_run's output."""
import ctypes as C

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

CHUNKS = (1, 255, 256, 257, 4000, 24000, 32000)


def _sep(state, **kw):
    st, _ = state
    return pkg("separator").HipSeparator(st, None, device=0, **kw)


def _offline(sep, x, cfg):
    rc = pkg("css").make_run_cfg(cfg, 16000, x.shape[1])
    return sep.handle.run(np.ascontiguousarray(x, np.float32), rc).copy()


def _stream(sep, x, cfg, sizes, ref=None):
    """push x in chunks of `sizes` (cycled); after every push the emitted prefix is checked against `ref`"""
    S = pkg("stream")
    outs = []
    with S.CssStream(sep, cfg, num_channels=x.shape[1]) as s:
        n, i = 0, 0
        while n < x.shape[0]:
            k = min(sizes[i % len(sizes)], x.shape[0] - n)
            got = s.push(x[n:n + k])
            n += k
            i += 1
            outs.append(np.stack(got))
            em = sum(o.shape[1] for o in outs)
            assert em == s.final_samples(n) == s.info().n_emitted
            assert n - em <= s.latency_samples
            if ref is not None and got[0].size:
                assert np.array_equal(outs[-1], ref[:, em - got[0].size:em])
        outs.append(np.stack(s.finish()))
        assert s.info().finished == 1
    return np.concatenate(outs, axis=1)


def _seeded_sizes(seed, n=64):
    rs = np.random.RandomState(seed)
    return [int(CHUNKS[j]) for j in rs.randint(0, len(CHUNKS), n)]


def test_stream_is_bit_identical_to_css_run_multichannel(mc_state, mix60):
    sep = _sep(mc_state)
    cfg = pkg("css").CssCfg()
    x = mix60[0] if mix60.ndim == 3 else mix60
    ref = _offline(sep, x, cfg)
    got = _stream(sep, x, cfg, _seeded_sizes(0), ref)
    assert got.shape == ref.shape and np.array_equal(got, ref)
    one = _stream(sep, x, cfg, [x.shape[0]])
    assert np.array_equal(one, ref)
    sep.close()


@pytest.mark.parametrize("knob", ["sc", "normalize", "sep_mse", "th03", "sqrt_hann", "seg2", "seg10", "dense"])
def test_stream_knobs_and_models(knob, mc_state, sc_state, mix60):
    CSS = pkg("css")
    x = (mix60[0] if mix60.ndim == 3 else mix60)[:16000 * 24]
    cfg = CSS.CssCfg()
    state = mc_state
    if knob == "sc":
        state, x = sc_state, x[:, :1]
    elif knob == "normalize":
        cfg.normalize_segment_power = True
    elif knob == "sep_mse":
        cfg.stitching_input, cfg.stitching_loss = "separation_result", "mse"
    elif knob == "th03":
        cfg.activity_th = 0.3
    elif knob == "seg2":
        cfg.segment_size_sec, cfg.hop_size_sec = 2.0, 0.5
    elif knob == "seg10":
        cfg.segment_size_sec, cfg.hop_size_sec = 10.0, 5.0
        x = (mix60[0] if mix60.ndim == 3 else mix60)[:16000 * 40]
    elif knob == "dense":   # six contributors per frame (186 frames, hop 37): the general overlap-add walk on both sides
        cfg.segment_size_sec, cfg.hop_size_sec = 3.0, 0.6
        x = x[:16000 * 12]
    sep = _sep(state)
    if knob == "sqrt_hann":
        sep.handle.set_analysis_window("sqrt_hann")
    ref = _offline(sep, x, cfg)
    got = _stream(sep, np.ascontiguousarray(x), cfg, _seeded_sizes(1), ref)
    assert np.array_equal(got, ref)
    sep.close()


def _status(fn):
    """(exception type, css_status or None) of a call, (None, None) when it returns"""
    L = pkg("_lib")
    try:
        fn()
    except L.CssError as e:
        return L.CssError, e.code
    except AssertionError as e:   # CSS_ERR_ZERO_WEIGHT / CSS_ERR_MASK_FLOOR raise the reference's assert (_lib.check)
        return AssertionError, str(e)
    return None, None


@pytest.mark.parametrize("m0", [0.15, 0.0])
def test_stream_edges(m0, mc_state, mix60):
    """Streams shorter than one frame, shorter than one segment, one segment plus one frame: css_run's output or css_run's
    status.  With the default windows a one-segment recording fails css.py:297 (w_first is 0 on its right edge); with
    seg_weight_m0_sec = 0 it succeeds and the zero-padded short recording's output is compared."""
    L, CSS, S = pkg("_lib"), pkg("css"), pkg("stream")
    x = mix60[0] if mix60.ndim == 3 else mix60
    cfg = CSS.CssCfg(seg_weight_m0_sec=m0)
    sep = _sep(mc_state)
    T = CSS.make_run_cfg(cfg, 16000, 7).c.segment_frames
    succeeded = 0
    for n in (300, 16000, T * 256 + 512):   # < one frame, < one segment, one segment + one frame
        xs = np.ascontiguousarray(x[:n])
        ref_status = _status(lambda: _offline(sep, xs, cfg))
        if ref_status == (None, None):
            assert np.array_equal(_stream(sep, xs, cfg, [777]), _offline(sep, xs, cfg))
            succeeded += 1
        else:
            with S.CssStream(sep, cfg) as s:
                s.push(xs)
                assert _status(s.finish) == ref_status
    assert succeeded == (1 if m0 else 3)
    sep.close()


def test_stream_empty_push_capacity_and_push_after_finish(mc_state, mix60):
    L, CSS, S = pkg("_lib"), pkg("css"), pkg("stream")
    x = mix60[0] if mix60.ndim == 3 else mix60
    sep = _sep(mc_state)
    with S.CssStream(sep, CSS.CssCfg()) as s:
        assert [a.size for a in s.push(np.zeros((0, 7), np.float32))] == [0, 0, 0]
        h = sep.handle
        # a capacity below what the push finalises: an error, and nothing changes
        out = np.empty((3, 10), np.float32)
        n_out = C.c_int64()
        xs = np.ascontiguousarray(x[:16000 * 8])
        rc_ = h.lib.css_stream_push(h.h, s.id, xs.ctypes.data_as(C.c_void_p), xs.shape[0], out.ctypes.data_as(C.c_void_p), 10,
                                    C.byref(n_out))
        assert rc_ == L.CSS_ERR_INVALID_ARG and s.info().n_pushed == 0
        s.push(xs)
        s.finish()
        with pytest.raises(L.CssError) as e:
            s.push(xs[:10])
        assert e.value.code == L.CSS_ERR_STATE
    sep.close()


def test_stream_isolation_and_refusals(mc_state, mix60):
    L, CSS, S, SYN = pkg("_lib"), pkg("css"), pkg("stream"), pkg("synth")
    cfg = CSS.CssCfg()
    a = mix60[0] if mix60.ndim == 3 else mix60
    a = np.ascontiguousarray(a[:16000 * 30])
    b = SYN.synth_meeting(30.0, 7, seed=7)
    b = np.ascontiguousarray(b[0] if b.ndim == 3 else b)
    c = SYN.synth_meeting(20.0, 7, seed=8)
    c = np.ascontiguousarray(c[0] if c.ndim == 3 else c)
    sep = _sep(mc_state)
    ra, rb, rcc = _offline(sep, a, cfg), _offline(sep, b, cfg), _offline(sep, c, cfg)
    sa, sb = S.CssStream(sep, cfg), S.CssStream(sep, cfg)
    oa, ob = [], []
    step = 24000
    for i in range(0, a.shape[0], step):
        oa.append(np.stack(sa.push(a[i:i + step])))
        assert np.array_equal(_offline(sep, c, cfg), rcc)
        ob.append(np.stack(sb.push(b[i:i + step])))
    oa.append(np.stack(sa.finish()))
    ob.append(np.stack(sb.finish()))
    assert np.array_equal(np.concatenate(oa, 1), ra)
    assert np.array_equal(np.concatenate(ob, 1), rb)
    # split-f16 is refused at open and while a stream is open; queued sessions make pushes CSS_ERR_STATE
    with pytest.raises(L.CssError) as e:
        sep.handle.set_linear_mode("split_f16")
    assert e.value.code == L.CSS_ERR_STATE
    out = L.pinned_empty((3, L.plan(sep.desc, CSS.make_run_cfg(cfg, 16000, 7), c.shape[0]).n_out))
    sep.handle.run_enqueue(L.pinned_copy(c), CSS.make_run_cfg(cfg, 16000, 7), out)
    with pytest.raises(L.CssError) as e:
        S.CssStream(sep, cfg)
    assert e.value.code == L.CSS_ERR_STATE
    n_out = C.c_int64()
    buf = np.empty((3, 100000), np.float32)
    h = sep.handle
    rc_ = h.lib.css_stream_push(h.h, sa.id, a.ctypes.data_as(C.c_void_p), 10, buf.ctypes.data_as(C.c_void_p), 100000, C.byref(n_out))
    assert rc_ == L.CSS_ERR_STATE
    sep.handle.wait()
    # the analysis window and the feature options are the stream's while it is open
    for call in (lambda: sep.handle.set_analysis_window("sqrt_hann"), lambda: sep.handle.set_feature_options()):
        with pytest.raises(L.CssError) as e:
            call()
        assert e.value.code == L.CSS_ERR_STATE
    sa.close(); sb.close()
    sep.handle.set_analysis_window("hann")
    sep.handle.set_linear_mode("split_f16")
    with pytest.raises(L.CssError) as e:
        S.CssStream(sep, cfg)
    assert e.value.code == L.CSS_ERR_STATE
    sep.close()


def test_stream_open_refuses_other_frame_geometries(mc_state):
    """A handle whose model has 400 / 160 frames runs css_run, but css_stream_open refuses it (CSS_ERR_INVALID_ARG)."""
    L, CSS, SEP, S = pkg("_lib"), pkg("css"), pkg("separator"), pkg("stream")
    cfg = SEP.ConformerCssCfg(extractor_conf=SEP.ExtractorCfg(frame_len=400, frame_hop=160),
                              nnet_conf=SEP.NnetCfg(conformer_conf=SEP.ConformerCfg(attention_dim=512, attention_heads=8, num_blocks=18,
                                                                                  dropout_rate=0.0)))
    sep = SEP.HipSeparator(mc_state[0], cfg, device=0, max_batch_segments=16)
    assert (sep.desc.frame_len, sep.desc.frame_hop) == (400, 160)
    with pytest.raises(L.CssError) as e:
        S.CssStream(sep, CSS.CssCfg())
    assert e.value.code == L.CSS_ERR_INVALID_ARG
    sep.close()


def test_stream_memory_is_bounded_on_ten_minutes(mc_state):
    SYN, CSS, S = pkg("synth"), pkg("css"), pkg("stream")
    x = SYN.synth_meeting(600.0, 7, seed=3)
    x = np.ascontiguousarray(x[0] if x.ndim == 3 else x)
    cfg = CSS.CssCfg()
    sep = _sep(mc_state, max_batch_segments=256)
    ref = _offline(sep, x, cfg)
    outs, dev = [], {}
    with S.CssStream(sep, cfg) as s:
        step = 24000
        for i in range(0, x.shape[0], step):
            outs.append(np.stack(s.push(x[i:i + step])))
            if i + step == 16000 * 60:
                dev[1] = s.info().device_bytes
        dev[10] = s.info().device_bytes
        outs.append(np.stack(s.finish()))
    assert dev[1] == dev[10]
    assert np.array_equal(np.concatenate(outs, 1), ref)
    sep.close()


def test_stream_output_written_as_css_inference_writes_it(tmp_path, mc_state, mix60):
    """A finished stream's output, written with the writer css_inference uses (write_wav), is byte for byte the
    sep_stream*.wav files css_inference writes for the same session (7 mono PCM16 files)."""
    import pandas as pd
    CSS, W, S = pkg("css"), pkg("wavio"), pkg("stream")
    mix = (mix60[:, :16000 * 20] * 0.05).astype(np.float32)
    names = []
    for c in range(7):
        p = tmp_path / f"ch{c}.wav"
        W.write_wav(p, mix[0, :, c], 16000, max_norm=False)
        names.append(str(p))
    session = pd.Series({"session_id": "MTG_stream", "is_mc": True, "wav_file_names": names})
    cfg = CSS.CssCfg(activity_th=0.3, show_progressbar=False)
    sep = _sep(mc_state)
    res = CSS.css_inference(str(tmp_path / "out"), "unused", session, cfg, fetch_from_cache=False, separator=sep)
    mixq, sr = W.load_audio(names, is_mc=True)
    got = _stream(sep, np.ascontiguousarray(mixq[0]), cfg, _seeded_sizes(2))
    for i, ref_path in enumerate(res["sep_wav_file_names"]):
        mine = tmp_path / f"stream{i}.wav"
        W.write_wav(mine, samps=got[i], sr=sr)
        assert open(mine, "rb").read() == open(ref_path, "rb").read(), i
    sep.close()


def test_stitching_costs_do_not_depend_on_the_meeting_length(mc_state):
    """A stream cannot know its segment count, so a boundary's stitching cost must be one bit pattern whatever the meeting's
    length: the costs of the boundaries a 60 s recording and a 4-min one (>= 129 segments) share are equal bit for bit."""
    L, CSS, SYN = pkg("_lib"), pkg("css"), pkg("synth")
    x = np.ascontiguousarray(SYN.synth_meeting(240.0, 7, seed=4)[0])
    cfg = CSS.make_run_cfg(CSS.CssCfg(), 16000, 7)
    sep = _sep(mc_state, max_batch_segments=256)
    h = sep.handle
    h.run(x, cfg)
    assert h.get_plan().num_segments >= 129
    long_costs = h.read(L.BUF_PIT_COST).reshape(-1, 9).copy()
    h.run(np.ascontiguousarray(x[:16000 * 60]), cfg)
    nseg = h.get_plan().num_segments
    short_costs = h.read(L.BUF_PIT_COST).reshape(-1, 9)
    shared = nseg - 2   # boundaries between segments that are full and not the last one in both recordings
    assert shared > 30
    assert np.array_equal(long_costs[:shared].view(np.uint64), short_costs[:shared].view(np.uint64))
    sep.close()
