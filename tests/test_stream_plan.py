"""The finality rule of streamed sessions (css_stream_final_samples), on the host: it is exact -- the oracle's
separate_and_stitch gives the same first final(N) samples under two different continuations of x[:N] -- and it is not lax
-- the lag stays under max_lag, final(N) never decreases and never passes css_plan(N).n_out.  No GPU needed."""
import numpy as np
import pytest

import css_oracle as O
from conftest import pkg

FS = 16000
KNOBS = [dict(), dict(segment_size_sec=2.0, hop_size_sec=0.5), dict(activity_dilation_sec=0.6, activity_erosion_sec=0.1)]


def _desc():
    return pkg("weights").ModelDesc.mc_v1()


def _rc(knobs, ch=7):
    CSS = pkg("css")
    return CSS.make_run_cfg(CSS.CssCfg(**knobs), FS, ch)


def _max_lag(rc):
    c = rc.c
    return (c.segment_frames + c.dilation_frames + c.erosion_frames + 2) * 256 + 512


def _segment_stat_separate(i, seg):
    """masks from the segment's own spectrum, with a whole-segment statistic (so the segment's extent matters)"""
    mag = np.abs(seg if seg.ndim == 2 else seg[..., 0]).astype(np.float64)      # [F, T]
    level = mag.mean() + 1e-9
    a = 1.0 / (1.0 + np.exp(-(mag / level - 1.0)))
    b = 1.0 / (1.0 + np.exp(-(mag.mean(axis=0, keepdims=True) / level - 1.0))) * np.ones_like(mag)
    c = np.clip(1.0 - 0.5 * (a + b), 0, 1)
    spk = np.stack([a, b, c], axis=-1).astype(np.float32)
    return spk, (1.0 - a)[..., None].astype(np.float32)


@pytest.mark.parametrize("k", range(len(KNOBS)))
def test_finality_rule_is_exact(k):
    L = pkg("_lib")
    knobs = KNOBS[k]
    rc = _rc(knobs, 1)
    ocfg = O.OracleCssCfg(**knobs)
    rs = np.random.RandomState(10 + k)
    base = rs.randn(FS * 40, 1).astype(np.float32) * np.sin(np.arange(FS * 40) / 3000.0)[:, None].astype(np.float32)
    for N in sorted(rs.randint(FS * 4, FS * 30, 4)):
        fin = L.stream_final_samples(_desc(), rc, int(N))
        tails = [rs.randn(FS * 8, 1).astype(np.float32), np.zeros((FS * 3, 1), np.float32)]
        outs = []
        for t in tails:
            x = np.concatenate([base[:N], t])[None]
            w, _ = O.separate_and_stitch(x, None, FS, ocfg, separate_fn=_segment_stat_separate)
            outs.append(np.stack(w))
        assert fin > 0
        assert np.array_equal(outs[0][:, :fin], outs[1][:, :fin]), (knobs, N, fin)


@pytest.mark.parametrize("k", range(len(KNOBS)))
def test_finality_rule_is_tight_and_monotone(k):
    L = pkg("_lib")
    rc = _rc(KNOBS[k])
    c = rc.c
    desc = _desc()
    lag = _max_lag(rc)
    seg_s, hop_s = c.segment_frames * 256, c.hop_frames * 256
    ns = set(range(0, 4 * seg_s, 97))
    for j in range(1, 60):   # around every segment start / end and its gate horizon
        for edge in (512 + j * hop_s, 512 + j * hop_s + seg_s, 512 + (j * c.hop_frames + c.segment_frames) * 256):
            ns.update(range(max(edge - 300, 0), edge + 300, 7))
    ns.update(np.random.RandomState(k).randint(0, FS * 240, 500).tolist())
    prev = -1
    for n in sorted(ns):
        f = L.stream_final_samples(desc, rc, n)
        assert n - f <= lag, (n, f, lag)
        assert f >= prev
        assert f <= L.plan(desc, rc, n).n_out
        assert f % 256 == 0
        prev = f
    assert lag == (57856 if k == 0 else lag)


def test_stream_entry_points_without_gpu_fail_loudly():
    L = pkg("_lib")
    lib = L.load()
    if lib.css_device_count() > 0:
        pytest.skip("a GPU is present")
    # no handle without a GPU (css_create fails), and the stream entry points refuse the NULL handle
    import ctypes as C
    sid = C.c_int32(-1)
    assert lib.css_stream_open(None, C.byref(_rc({}).c), 7, C.byref(sid)) == L.CSS_ERR_INVALID_ARG
    CSS, SEP, W, S = pkg("css"), pkg("separator"), pkg("weights"), pkg("stream")
    desc = W.ModelDesc(num_blocks=1)
    sep = SEP.HipSeparator(W.portable_state_dict(desc, 0))
    with pytest.raises(L.CssError) as e:
        S.CssStream(sep, CSS.CssCfg())
    assert e.value.code == L.CSS_ERR_NO_DEVICE


def test_other_frame_geometries_are_refused():
    L, CSS, W = pkg("_lib"), pkg("css"), pkg("weights")
    desc = W.ModelDesc(num_blocks=1, frame_len=400, frame_hop=160)
    rc = CSS.make_run_cfg(CSS.CssCfg(), FS, 7, 400, 160)
    with pytest.raises(L.CssError) as e:
        L.stream_final_samples(desc, rc, 100000)
    assert e.value.code == L.CSS_ERR_INVALID_ARG
