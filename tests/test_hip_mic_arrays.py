"""Microphone arrays of 2 to 8 channels, end to end on the MI355X: css_run of a C-microphone model against the oracle, and for C = 4
every path that sits on top of it -- mc_mvdr = False, the PCM16 edges, queued sessions, streams (float and PCM16 pushes, a group,
a preview) -- against css_run.

Model: ModelDesc(num_mics=C, in_features=257 C, num_blocks=1) with portable_state_dict (seed 3); input: synth_meeting(seconds, C,
seed).  The oracle is driven by the library's own masks in complex128, as test_hip_parity.py::test_other_segmentations_vs_oracle
does, so that a winner-take-all flip at float32 rounding level cannot move a waveform; the masks themselves are held against the
oracle's estimator at the survey's 5e-6.

Seeds, chosen on the CPU with the oracle alone among the recordings of seeds 5 .. 14, by the conditioning of the first segment's
IPD features.  A bin's phase carries the float32 transform's error U sum |x w| divided by the bin's magnitude, so two correct
float32 transforms differ there by U a, a = sum |x w| (1 / |X_l| + 1 / |X_r|) per pair, bin and frame (on the 7-microphone model
too: the frame with the largest a is the frame with the largest mask distance).  Rule, per C: of the seeds on which no angle can
cross the atan2 branch cut to first order (min (pi - |IPD|) / (U a) >= 1, bins 1 .. 255 as tests/golden/gen_golden_r5.py screens),
the one with the smallest worst a.  At every boundary the cost of the best and of the second-best permutation differ by far more
than 1e-6 of the best, and no activity value comes near the threshold 0.3 --
  C  seconds  seed  worst a   min (pi - |IPD|) / (U a)  boundaries  (second - best) / best, smallest  |activity - 0.3|, smallest
  2  8        8     1.54e4    2.0                       4           1.46                              0.174
  4  8        8     9.02e3    1.6                       4           1.00                              0.177
  8  8        13    1.53e4    2.5                       4           1.00                              0.176
  3  5        11    8.06e3    2.4                       2           1.00                              0.169
  5  5        5     1.52e4    2.4                       2           1.04                              0.178
  6  5        11    1.63e4    1.2                       2           0.80                              0.173
(On the recording of seed 5, a = 6.0e4 at frame 91, the 6-microphone masks are 5.4e-6 from the oracle's at that frame and within
2.1e-6 elsewhere; the 7-microphone model measures 1.6e-6 .. 8.7e-6 on recordings of this family.)
Needs an MI355X."""
import numpy as np
import pytest

from conftest import pkg, rel_rms
import css_oracle as O

pytestmark = pytest.mark.gpu

S, F, T = 3, 257, 186
WSEED = 3
MSEED = {2: 8, 4: 8, 8: 13, 3: 11, 5: 5, 6: 11}


def _model(C):
    w = pkg("weights")
    desc = w.ModelDesc(num_mics=C, in_features=257 * C, num_blocks=1)
    return desc, w.portable_state_dict(desc, WSEED)


def _cfgs(**kw):
    kw.setdefault("activity_th", 0.3)
    return pkg("css").CssCfg(show_progressbar=False, **kw), O.OracleCssCfg(**kw)


_MIX = {}


def _mix(C, seconds):
    if (C, seconds) not in _MIX:
        _MIX[(C, seconds)] = pkg("synth").synth_meeting(seconds, C, seed=MSEED[C])
    return _MIX[(C, seconds)]


def _against_oracle(C, seconds, mode="exact_f32", **kw):
    """css_run of the C-microphone model; the oracle on the library's masks: permutations and gate exact, waveforms rel-RMS < 2e-5"""
    L, CSS = pkg("_lib"), pkg("css")
    desc, st = _model(C)
    sep = pkg("separator").HipSeparator(st, None, device=0, num_mics=C, linear_mode=mode)
    try:
        assert sep.desc == desc
        cfg, ocfg = _cfgs(**kw)
        mix = _mix(C, seconds)
        assert mix.shape[2] == C
        wavs, side = CSS.separate_and_stitch(mix, sep, 16000, "cuda:0", cfg)
        h = sep.handle
        plan, oplan = h.get_plan(), O.make_plan(mix.shape[1], 16000, ocfg)
        nseg = int(plan.num_segments)
        assert (plan.mix_frames, nseg, oplan.segment_frames) == (oplan.mix_frames, oplan.num_segments, T)
        m = h.read(L.BUF_MASKS).reshape(S + 1, F, nseg, T)
        params = O.ConformerParams(st)
        if mode == "exact_f32":
            om = O.conformer_forward(params, O.features(O.stft(mix[0])[:, :T]))
            err = float(np.abs(m[:, :, 0, :] - om).max())
            print(f"C = {C}: masks of segment 0 against the oracle's estimator, max-abs error {err:.2e}")
            assert err < 5e-6, err
        if cfg.mc_mvdr:
            assert h.read(L.BUF_SCM).shape == (nseg, S + 1, F, C * C) and h.read(L.BUF_BFW).shape == (nseg, S, F, 2 * C)
        per_seg = [(np.ascontiguousarray(np.moveaxis(m[:S, :, i], 0, 2)), np.ascontiguousarray(np.moveaxis(m[S:, :, i], 0, 2)))
                   for i in range(nseg)]
        ow, oside = O.separate_and_stitch(mix, params, 16000, ocfg, separate_fn=lambda i, seg: per_seg[i], mvdr_cplx=np.complex128)
        assert [tuple(p) for p in h.read(L.BUF_PERMS)] == [tuple(p) for p in oside["perms"]]
        assert np.array_equal(side["activity_final"].numpy()[0], oside["activity_final"][0])
        worst = max(rel_rms(wavs[k], ow[k]) for k in range(S))
        print(f"C = {C} ({seconds} s, {mode}, {kw}): waveforms against the oracle, worst rel-RMS {worst:.2e}")
        if mode == "exact_f32":
            assert all(len(wavs[k]) == len(ow[k]) for k in range(S)) and worst < 2e-5, worst
        return wavs, ow
    finally:
        sep.close()


@pytest.mark.parametrize("C", (2, 4, 8))
def test_css_run_against_the_oracle(C):
    _against_oracle(C, 8.0)


@pytest.mark.parametrize("C", (3, 5, 6))
def test_css_run_against_the_oracle_short(C):
    _against_oracle(C, 5.0)


def test_without_mvdr_masks_channel_zero():
    wavs, ow = _against_oracle(4, 8.0, mc_mvdr=False)
    # and it is not the beamformer's output
    with_mvdr, _ = _against_oracle(4, 8.0)
    assert max(rel_rms(wavs[k], with_mvdr[k]) for k in range(S)) > 1e-3


def test_split_f16_decisions_are_exact():
    _against_oracle(4, 8.0, mode="split_f16")


# ---- C = 4: the paths on top of css_run -------------------------------------------------------------------------------------------

def _quantise(x):
    return np.ascontiguousarray(np.clip(np.rint(np.asarray(x, np.float64) * 0.2 * 32768.0), -32768, 32767).astype(np.int16))


def _dequantise(q):
    return np.ascontiguousarray(q.astype(np.float32) / np.float32(32768.0))


@pytest.fixture(scope="module")
def four():
    """the 4-microphone model, its run configuration, the quantised 8 s recording [n, 4] and css_run of it"""
    desc, st = _model(4)
    sep = pkg("separator").HipSeparator(st, None, device=0, num_mics=4)
    cfg, _ = _cfgs()
    rc = pkg("css").make_run_cfg(cfg, 16000, 4)
    q = _quantise(_mix(4, 8.0)[0])
    x = _dequantise(q)
    ref = sep.handle.run(x, rc).copy()
    assert ref.shape[0] == S and np.isfinite(ref).all() and np.abs(ref).max() > 0
    yield dict(sep=sep, h=sep.handle, cfg=cfg, rc=rc, q=q, x=x, ref=ref)
    sep.close()


def test_run_pcm16_is_the_float_path(four):
    h, q, ref = four["h"], four["q"], four["ref"]
    pcm16, peaks = h.run_pcm16([np.ascontiguousarray(q[:, c]) for c in range(4)], four["rc"])
    assert pcm16.dtype == np.int16 and pcm16.shape == ref.shape
    for i in range(S):
        assert peaks[i] == np.max(np.abs(ref[i]))
        y = ref[i] * 0.99 / (np.max(np.abs(ref[i])) + 1e-7)                     # utils/audio_utils.py:44-45
        assert np.array_equal(pcm16[i], np.clip(np.rint(y.astype(np.float64) * 32767.0), -32768, 32767).astype(np.int16))


def test_three_queued_sessions_share_a_batch(four):
    """page-locked sessions queued back to back (two float, one as PCM16 planes) are one estimator batch of the queue group;
    each is css_run of its own recording, bit for bit"""
    L, h, rc, x, q = pkg("_lib"), four["h"], four["rc"], four["x"], four["q"]
    cuts = (x.shape[0], x.shape[0] - 16000 - 37, x.shape[0] - 24001)
    refs = [h.run(x[:n], rc).copy() for n in cuts[:2]]
    assert np.array_equal(refs[0], four["ref"])
    ref16, refpk = h.run_pcm16([np.ascontiguousarray(q[:cuts[2], c]) for c in range(4)], rc)
    ref16, refpk = ref16.copy(), refpk.copy()
    ins = [L.pinned_copy(np.ascontiguousarray(x[:n])) for n in cuts[:2]]
    block = L.pinned_empty((4, cuts[2]), np.int16)
    block[:] = q[:cuts[2]].T
    outs = [L.pinned_empty(r.shape, np.float32) for r in refs[:2]]
    o16, pk = L.pinned_empty(ref16.shape, np.int16), L.pinned_empty((S,), np.float32)
    got = [h.run_enqueue(ins[0], rc, outs[0]), h.run_enqueue(ins[1], rc, outs[1])]
    got16 = h.run_enqueue_pcm16([block[c] for c in range(4)], rc, o16, pk)
    h.wait()
    for k in range(2):
        assert np.array_equal(got[k], refs[k]), k
    assert np.array_equal(got16, ref16) and np.array_equal(pk, refpk)


def test_streams_are_css_run(four):
    """a stream pushed in chunks of 1 000, 24 001 and 7 samples in turn: what it returns, put together, is css_run"""
    ST = pkg("stream")
    sep, cfg, x, ref = four["sep"], four["cfg"], four["x"], four["ref"]
    n = x.shape[0]
    with ST.CssStream(sep, cfg) as s:
        assert s.num_channels == 4
        outs, at, i = [], 0, 0
        while at < n:
            step = min((1000, 24001, 7)[i % 3], n - at)
            outs.append(np.stack(s.push(x[at:at + step])))
            at, i = at + step, i + 1
        outs.append(np.stack(s.finish()))
    assert np.array_equal(np.concatenate(outs, axis=1), ref)


def test_grouped_pcm16_pushes_share_the_round(four):
    """two streams pushed in ONE grouped PCM16 call per round"""
    ST = pkg("stream")
    sep, cfg, q, ref = four["sep"], four["cfg"], four["q"], four["ref"]
    n = q.shape[0]
    with ST.CssStream(sep, cfg) as a, ST.CssStream(sep, cfg) as b:
        group = ST.CssStreamGroup([a, b])
        got, at = ([], []), 0
        while at < n:
            step = min(24001, n - at)
            for k, r in enumerate(group.push_pcm16([q[at:at + step], q[at:at + step]])):
                got[k].append(np.stack(r))
            at += step
        for k, s in enumerate((a, b)):
            got[k].append(np.stack(s.finish()))
    for k in range(2):
        assert np.array_equal(np.concatenate(got[k], axis=1), ref), k


def test_preview_is_css_run_of_the_prefix(four):
    ST = pkg("stream")
    sep, cfg, rc, x = four["sep"], four["cfg"], four["rc"], four["x"]
    n = 5 * 16000 + 123
    with ST.CssStream(sep, cfg) as s:
        emitted = np.stack(s.push(x[:n]))
        tail = np.stack(s.preview())
        want = sep.handle.run(x[:n], rc)
        assert emitted.shape[1] + tail.shape[1] == want.shape[1] and tail.shape[1] > 0
        assert np.array_equal(emitted, want[:, :emitted.shape[1]]) and np.array_equal(tail, want[:, emitted.shape[1]:])
        rest = [np.stack(s.push(x[n:])), np.stack(s.finish())]
    assert np.array_equal(np.concatenate([emitted] + rest, axis=1), four["ref"])


def test_eight_channels_into_the_four_channel_stream(four):
    """an 8-channel stream on the 4-microphone model is CSS_ERR_SHAPE at css_stream_open, 8-channel samples at css_run"""
    L, ST = pkg("_lib"), pkg("stream")
    sep, cfg, h = four["sep"], four["cfg"], four["h"]
    with ST.CssStream(sep, cfg) as s:
        bad = np.zeros((4000, 8), np.float32)
        with pytest.raises(ValueError):
            s.push(bad)           # (css_stream_push takes no channel count: the wrapper holds the stream's)
    with pytest.raises(L.CssError) as e:
        ST.CssStream(sep, cfg, num_channels=8)      # css_stream_open: the model has 4 microphones
    assert e.value.code == L.CSS_ERR_SHAPE
    with pytest.raises(L.CssError) as e:
        h.run(np.zeros((64000, 8), np.float32), four["rc"])
    assert e.value.code == L.CSS_ERR_SHAPE
