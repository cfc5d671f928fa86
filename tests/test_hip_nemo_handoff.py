"""The hand-off to NeMo hosts on the MI355X (include/css_mi355_nemo_handoff.h; Handle.handoff_nemo_all, run_enqueue_nemo,
run_enqueue_pcm16_nemo): kept ranges and NeMo log-mel features of all three separated streams, found and computed on the device --
synchronously after a pass, and behind the waveforms of queued sessions that share queue groups with every other kind of session.
The queued form, the synchronous form and the kernel entries applied to the same waveforms and ranges agree bit for bit; the values
are held to the float64 definition of tests/nemo_reference.py within its counted bound, every element."""
import numpy as np
import pytest

import nemo_reference as N
from conftest import pkg
from test_hip_stream_handoff import _rec, _sep, _toggling_cfg

pytestmark = pytest.mark.gpu

SENT = -7
LENGTHS = (4.0, 6.0, 8.0)
NCFG = dict(n_mels=80, pad_frames=8, drop_silence=True, preemphasis=0.97, normalize=True)
WCFG = dict(n_mels=80, pad_frames=8, drop_silence=True)


@pytest.fixture(scope="module")
def model():
    """the 2-block multi-channel model of test_hip_session_handoff.py"""
    w = pkg("weights")
    desc = w.ModelDesc(num_blocks=2)
    return w.apply_golden_recipe(w.portable_state_dict(desc, 21)), desc


@pytest.fixture(scope="module")
def world(model):
    """one handle, the recordings, a configuration under which the gate toggles, and the solo results -- each computed once"""
    import torch
    css, L = pkg("css"), pkg("_lib")
    sep = _sep(model)
    recs = {s: L.pinned_copy(_rec(s, 60 + i)) for i, s in enumerate(LENGTHS)}
    cfg = _toggling_cfg(sep, recs[8.0])
    rc = css.make_run_cfg(cfg, 16000, 7)
    w = dict(sep=sep, h=sep.handle, recs=recs, cfg=cfg, rc=rc, solo={})

    def device_pass(x):
        n_out = int(L.plan(sep.desc, rc, x.shape[0]).n_out)
        pcm = torch.from_numpy(np.asarray(x)).cuda()
        wav = torch.empty((3, n_out), dtype=torch.float32, device="cuda")
        w["h"].run_device(pcm.data_ptr(), x.shape[0], 7, rc, wav.data_ptr(), n_out)
        torch.cuda.synchronize()
        return wav, n_out

    def solo(sec, **ncfg):
        """(run()'s waveforms, the synchronous NeMo hand-off after run_device) of recording `sec`, copied"""
        key = (sec, tuple(sorted(ncfg.items())))
        if key not in w["solo"]:
            want = w["h"].run(recs[sec], rc).copy()
            wav, n_out = device_pass(recs[sec])
            assert np.array_equal(wav.cpu().numpy(), want)
            ho = w["h"].handoff_nemo_all(wav.data_ptr(), n_out, **ncfg)
            w["solo"][key] = (want, _snapshot(ho))
        return w["solo"][key]

    w["device_pass"], w["solo_of"] = device_pass, solo
    yield w
    sep.close()


def _snapshot(ho):
    return dict(mel=[m.copy() for m in ho.mel], ranges=[r.copy() for r in ho.ranges], n_frames=ho.n_frames.copy(), n_ranges=ho.n_ranges.copy(),
                mean=ho.mean.copy(), std=ho.std.copy())


def _same(ho, want):
    """bit for bit: counts, ranges, features, statistics (the statistics of speakers with a frame)"""
    got = _snapshot(ho)
    assert np.array_equal(got["n_frames"], want["n_frames"]) and np.array_equal(got["n_ranges"], want["n_ranges"])
    for k in range(3):
        assert np.array_equal(got["ranges"][k], want["ranges"][k]), k
        assert got["mel"][k].dtype == np.float32 and np.array_equal(N.bits(got["mel"][k]), N.bits(want["mel"][k])), k
        if want["n_frames"][k] > 0:
            assert np.array_equal(N.bits(got["mean"][k]), N.bits(want["mean"][k])) and np.array_equal(N.bits(got["std"][k]), N.bits(want["std"][k])), k


def _nemo_out(world, sec, ncfg=NCFG, fill=SENT):
    L = pkg("_lib")
    frames, ranges = L.nemo_handoff_bounds(world["sep"].desc, world["rc"], L.nemo_cfg(**ncfg), world["recs"][sec].shape[0])
    return L.NemoHandoff(3, ncfg["n_mels"], frames, ranges, pinned=True, fill=fill)


def _untouched_beyond_counts(ho):
    """nothing but the stated parts of the caller's arrays is written"""
    for k in range(3):
        nf, nr = int(ho.n_frames[k]), int(ho.n_ranges[k])
        assert (ho.mel_all[k, :, nf:] == SENT).all() and (ho.ranges_all[k, nr:] == SENT).all(), k
        if nf == 0:
            assert (ho.mean[k] == SENT).all() and (ho.std[k] == SENT).all()


@pytest.mark.parametrize("ncfg", (NCFG, dict(NCFG, n_mels=128, pad_frames=0), dict(NCFG, normalize=False, drop_silence=False),
                                  dict(NCFG, preemphasis=0.0)), ids=("80", "128_pad0", "raw_whole_stream", "no_preemphasis"))
def test_queued_synchronous_and_kernel_entry_agree_and_match_the_definition(world, ncfg):
    L, h, rc = pkg("_lib"), world["h"], world["rc"]
    sec = 6.0
    x = world["recs"][sec]
    want_wav, want = world["solo_of"](sec, **ncfg)
    n_out = want_wav.shape[1]
    assert any(int(r) >= 2 for r in want["n_ranges"]) or not ncfg["drop_silence"]     # the gate toggles
    # the queued form: waveforms run_enqueue's bits, hand-off the synchronous form's bits, nothing else written
    out = L.pinned_empty((3, n_out), np.float32)
    ho = _nemo_out(world, sec, ncfg)
    view, ho = h.run_enqueue_nemo(x, rc, out, handoff=ho, **ncfg)
    h.wait()
    assert np.array_equal(view, want_wav)
    _same(ho, want)
    _untouched_beyond_counts(ho)
    # the synchronous form into page-locked arrays: the kernels' own stores
    wav, _ = world["device_pass"](x)
    _same(h.handoff_nemo_all(wav.data_ptr(), n_out, out=_nemo_out(world, sec, ncfg), **ncfg), want)
    # the kernel entries on that run's waveforms and ranges
    nm = ncfg["n_mels"]
    cap = max(int(want["n_ranges"].max()), 1)
    regs, offs = np.zeros((3, cap, 2), np.int64), np.zeros((3, cap), np.int64)
    st = np.zeros(3, L.HANDOFF_STATE)
    for k in range(3):
        regs[k], offs[k], A, _ = N.run_table(want["ranges"][k], cap)
        st[k]["A"], st[k]["J"] = A, A // 160
        assert A // 160 == int(want["n_frames"][k])
    rows = n_out // 160 + 4
    got = h.nemo_kernels(dict(S=3, n_mels=nm, normalize=int(ncfg["normalize"]), cap_ranges=cap, wav_off=0, preemphasis=ncfg["preemphasis"],
                              wav_ld=n_out, rows=rows, raw_ld=rows, out_ld=rows - 4, wav=want_wav, regs=regs, offs=offs, st=st,
                              n_ranges=want["n_ranges"].astype(np.int32), operand=N.canary(3 * rows * 160 + 512), raw=N.canary(3 * nm * rows),
                              mean=N.canary(3 * nm), stdv=N.canary(3 * nm), out=N.canary(3 * nm * (rows - 4))))
    k_out, k_mean, k_std = got["out"].reshape(3, nm, rows - 4), got["mean"].reshape(3, nm), got["stdv"].reshape(3, nm)
    for k in range(3):
        J = int(want["n_frames"][k])
        assert np.array_equal(N.bits(k_out[k, :, :J]), N.bits(want["mel"][k])), k
        if J:
            assert np.array_equal(N.bits(k_mean[k]), N.bits(want["mean"][k])) and np.array_equal(N.bits(k_std[k]), N.bits(want["std"][k])), k
            # and the definition, every element
            ref = N.reference(want_wav[k], want["ranges"][k], nm, ncfg["preemphasis"], ncfg["normalize"])
            d = np.abs(want["mel"][k].astype(np.float64) - ref.out)
            assert ref.out.shape == want["mel"][k].shape and (d <= ref.bound).all(), (k, float((d / ref.bound).max()))


def test_ranges_and_counts_are_the_whisper_hand_offs(world):
    L, h, rc = pkg("_lib"), world["h"], world["rc"]
    x = world["recs"][6.0]
    _, want = world["solo_of"](6.0, **NCFG)
    _, wh = h.run_enqueue_handoff(x, rc, None, **WCFG)
    h.wait()
    assert np.array_equal(wh.n_frames, want["n_frames"]) and np.array_equal(wh.n_ranges, want["n_ranges"])
    for k in range(3):
        assert np.array_equal(wh.ranges[k], want["ranges"][k])
    assert L.nemo_handoff_bounds(world["sep"].desc, rc, L.nemo_cfg(**NCFG), x.shape[0]) == \
        L.session_handoff_bounds(world["sep"].desc, rc, L.handoff_cfg(**WCFG), x.shape[0])


def test_features_only(world):
    """out=None: no waveform leaves the GPU, the hand-off is the same"""
    h, rc = world["h"], world["rc"]
    _, want = world["solo_of"](4.0, **NCFG)
    view, ho = h.run_enqueue_nemo(world["recs"][4.0], rc, None, **NCFG)
    h.wait()
    assert view is None
    _same(ho, want)


def test_pcm16_twin(world):
    """PCM16 planes in, peak-normalised PCM16 streams out as run_pcm16 gives them, and the features of the float waveforms before
    that normalisation: run_device on the same samples as float (q / 32768, the ingest's own scaling) + handoff_nemo_all.  And
    with no PCM16 output at all."""
    L, h, rc = pkg("_lib"), world["h"], world["rc"]
    x = world["recs"][4.0]
    q = np.clip(np.round(np.asarray(x) * 32768.0), -32768, 32767).astype(np.int16)
    planes = [L.pinned_copy(np.ascontiguousarray(q[:, c])) for c in range(7)]
    want16, want_peaks = h.run_pcm16(planes, rc)
    xf = np.ascontiguousarray(q.astype(np.float32) / np.float32(32768.0))
    wav, n_out = world["device_pass"](xf)
    want = _snapshot(h.handoff_nemo_all(wav.data_ptr(), n_out, **NCFG))
    out16 = L.pinned_empty((3, n_out), np.int16)
    peaks = L.pinned_empty((3,), np.float32)
    out16[:] = 0
    peaks[:] = 0
    view, ho = h.run_enqueue_pcm16_nemo(planes, rc, out16, peaks, **NCFG)
    none_view, ho_only = h.run_enqueue_pcm16_nemo(planes, rc, None, None, **NCFG)
    h.wait()
    assert np.array_equal(view, want16) and np.array_equal(peaks, want_peaks) and none_view is None
    _same(ho, want)
    _same(ho_only, want)


def test_one_queue_of_nemo_whisper_and_plain_sessions_twice(world):
    """NeMo, Whisper hand-off and plain sessions in one queue (they share groups), queued twice, everything page-locked: every
    session has the bits it has alone"""
    L, h, rc = pkg("_lib"), world["h"], world["rc"]
    solo = {sec: world["solo_of"](sec, **NCFG) for sec in LENGTHS}
    raw_cfg = dict(NCFG, normalize=False, n_mels=128)
    solo_raw = world["solo_of"](6.0, **raw_cfg)
    whisper = {}
    for sec in (4.0, 8.0):
        _, wh = h.run_enqueue_handoff(world["recs"][sec], rc, None, **WCFG)
        h.wait()
        whisper[sec] = (wh.n_frames.copy(), [m.copy() for m in wh.mel])
    for _ in range(2):
        got = []
        for kind, sec in (("nemo", 4.0), ("whisper", 8.0), ("plain", 6.0), ("nemo", 8.0), ("nemo_raw", 6.0), ("whisper", 4.0), ("nemo", 6.0)):
            x = world["recs"][sec]
            n_out = solo[sec][0].shape[1]
            out = L.pinned_empty((3, n_out), np.float32)
            out[:] = np.nan
            if kind == "plain":
                got.append((kind, sec, h.run_enqueue(x, rc, out), None))
            elif kind == "whisper":
                got.append((kind, sec) + h.run_enqueue_handoff(x, rc, out, **WCFG))
            elif kind == "nemo_raw":
                got.append((kind, sec) + h.run_enqueue_nemo(x, rc, out, handoff=_nemo_out(world, sec, raw_cfg), **raw_cfg))
            else:
                got.append((kind, sec) + h.run_enqueue_nemo(x, rc, out, handoff=_nemo_out(world, sec), **NCFG))
        h.wait()
        for kind, sec, view, ho in got:
            assert np.array_equal(view, solo[sec][0]), (kind, sec)
            if kind == "nemo":
                _same(ho, solo[sec][1])
                _untouched_beyond_counts(ho)
            elif kind == "nemo_raw":
                _same(ho, solo_raw[1])
            elif kind == "whisper":
                assert np.array_equal(ho.n_frames, whisper[sec][0])
                assert all(np.array_equal(a, b) for a, b in zip(ho.mel, whisper[sec][1]))


def _refused(L, call, code):
    with pytest.raises(L.CssError) as e:
        call()
    assert e.value.code == code, (e.value.code, code)


def test_refusals_leave_the_queue_and_the_arrays_alone(world):
    L, h, rc, desc = pkg("_lib"), world["h"], world["rc"], world["sep"].desc
    x = world["recs"][4.0]
    n_out = int(L.plan(desc, rc, x.shape[0]).n_out)
    frames, ranges = L.nemo_handoff_bounds(desc, rc, L.nemo_cfg(**NCFG), x.shape[0])
    assert ranges >= 2
    wav = L.pinned_empty((3, n_out), np.float32)
    wav[:] = SENT

    def untouched(ho):
        assert (ho.mel_all == SENT).all() and (ho.ranges_all == SENT).all() and (ho.n_frames == SENT).all() and (ho.n_ranges == SENT).all()
        assert (ho.mean == SENT).all() and (ho.std == SENT).all() and (wav == SENT).all()
        h.wait()                                             # nothing was queued, and waiting for nothing is fine
        assert (wav == SENT).all()

    good = lambda **kw: L.NemoHandoff(3, kw.get("n_mels", 80), kw.get("frames", frames), kw.get("ranges", ranges),
                                      pinned=kw.get("pinned", True), fill=SENT)
    ho = good()
    h.set_linear_mode("split_f16")
    try:
        _refused(L, lambda: h.run_enqueue_nemo(x, rc, wav, handoff=ho, **NCFG), L.CSS_ERR_STATE)
    finally:
        h.set_linear_mode("exact_f32")
    untouched(ho)
    n = 0
    for kw, ncfg in ((dict(frames=frames - 1), NCFG), (dict(ranges=ranges - 1), NCFG), (dict(pinned=False), NCFG),
                     (dict(n_mels=64), dict(NCFG, n_mels=64)), (dict(), dict(NCFG, pad_frames=4097)), (dict(), dict(NCFG, pad_frames=-1)),
                     (dict(), dict(NCFG, preemphasis=1.0)), (dict(), dict(NCFG, preemphasis=-0.5)), (dict(), dict(NCFG, preemphasis=float("nan"))),
                     (dict(), dict(NCFG, preemphasis=float("inf")))):
        ho = good(**kw)
        _refused(L, lambda: h.run_enqueue_nemo(x, rc, wav, handoff=ho, **ncfg), L.CSS_ERR_INVALID_ARG)
        untouched(ho)
        _refused(L, lambda: h.run_enqueue_nemo(x, rc, None, handoff=ho, **ncfg), L.CSS_ERR_INVALID_ARG)
        untouched(ho)
        n += 1
    assert n == 10
    # the synchronous form refuses short capacities and bad configurations too (it accepts pageable arrays)
    dwav, _ = world["device_pass"](x)
    for kw, ncfg in ((dict(frames=frames - 1), NCFG), (dict(ranges=ranges - 1), NCFG), (dict(), dict(NCFG, preemphasis=1.5))):
        ho = good(**kw)
        _refused(L, lambda: h.handoff_nemo_all(dwav.data_ptr(), n_out, out=ho, **ncfg), L.CSS_ERR_INVALID_ARG)
        assert (ho.mel_all == SENT).all() and (ho.n_frames == SENT).all()
    with pytest.raises(L.CssError):
        L.nemo_handoff_bounds(desc, rc, L.nemo_cfg(64), x.shape[0])
    # and the handle still runs a session correctly
    ho = good()
    view, _ = h.run_enqueue_nemo(x, rc, wav, handoff=ho, **NCFG)
    h.wait()
    want_wav, want = world["solo_of"](4.0, **NCFG)
    assert np.array_equal(view, want_wav)
    _same(ho, want)


def test_other_frame_geometry_is_refused(mc_state):
    L, CSS, SEP = pkg("_lib"), pkg("css"), pkg("separator")
    cfg = SEP.ConformerCssCfg(extractor_conf=SEP.ExtractorCfg(frame_len=400, frame_hop=160),
                              nnet_conf=SEP.NnetCfg(conformer_conf=SEP.ConformerCfg(attention_dim=512, attention_heads=8, num_blocks=18,
                                                                                  dropout_rate=0.0)))
    sep = SEP.HipSeparator(mc_state[0], cfg, device=0, max_batch_segments=16)
    try:
        rc = CSS.make_run_cfg(CSS.CssCfg(show_progressbar=False), 16000, 7, 400, 160)
        x = L.pinned_copy(_rec(4.0, 3))
        n_out = int(L.plan(sep.desc, rc, x.shape[0]).n_out)
        wav = L.pinned_empty((3, n_out), np.float32)
        wav[:] = SENT
        ho = L.NemoHandoff(3, 80, n_out // 160 + 8, 64, pinned=True, fill=SENT)
        _refused(L, lambda: sep.handle.run_enqueue_nemo(x, rc, wav, handoff=ho), L.CSS_ERR_INVALID_ARG)
        sep.handle.wait()
        assert (wav == SENT).all() and (ho.mel_all == SENT).all() and (ho.n_ranges == SENT).all()
    finally:
        sep.close()
