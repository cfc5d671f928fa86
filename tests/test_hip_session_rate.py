"""Whole sessions at the capture rate on the MI355X (include/css_mi355_session_rate.h; DESIGN.md 7 "N1 / N2 at the capture rate").

The oracle is the definition, composed of calls that existed before: x16 = handle.resample(input) (css_resample_host; int16 enters
as q * 2^-15), w = handle.run(x16, cfg), y = w at 1 / 1 or handle.resample(w.T, 16000, rate).T, and for PCM16 output
write_wav's two lines per stream on y.  Every comparison is np.array_equal.  Recordings and definitions are made once per module
and shared, read-only."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

FS = 16000
PAIRS = ((48000, 16000), (48000, 48000), (44100, 44100), (8000, 16000), (16000, 48000), (16000, 8000))


def _encode(y):
    """write_wav's two lines per stream (utils/audio_utils.py:37-49) -> (int16 [S, n], float32 [S] peaks)"""
    y = np.asarray(y, np.float32)
    peaks = np.max(np.abs(y), axis=1).astype(np.float32)
    z = (y * np.float32(0.99)) / (peaks + np.float32(1e-7))[:, None]
    assert z.dtype == np.float32
    q = np.clip(np.rint(z.astype(np.float64) * 32767.0), -32768.0, 32767.0).astype(np.int16)
    return q, peaks


def _quantise(x):
    return np.clip(np.rint(np.asarray(x, np.float64) * 32768.0), -32768, 32767).astype(np.int16)


def _as_rate(L, in_rate, out_rate):
    return L.session_rate(None if in_rate == FS else in_rate, None if out_rate == FS else out_rate, FS)


def _definition(h, x, cfg, in_rate, out_rate, pcm16):
    """x: float32 [n, C] or int16 [n, C] at in_rate -> float32 [S, n_out], or (int16 [S, n_out], peaks)"""
    if in_rate != FS:
        x16 = h.resample(x, in_rate, FS)
    else:
        x16 = x.astype(np.float32) / np.float32(32768.0) if x.dtype == np.int16 else np.ascontiguousarray(x, np.float32)
    w = h.run(x16, cfg).copy()
    y = w if out_rate == FS else np.ascontiguousarray(h.resample(w.T, FS, out_rate).T)
    return _encode(y) if pcm16 else y


class _Env:
    """one separator per model, recordings per capture rate, and the definitions, made on first use"""

    def __init__(self, state, **kw):
        st, self.desc = state
        self.sep = pkg("separator").HipSeparator(st, None, device=0, **kw)
        self.h = self.sep.handle
        self.C = int(self.desc.num_mics)
        CSS = pkg("css")
        self.cfg = CSS.make_run_cfg(CSS.CssCfg(segment_size_sec=2.0, hop_size_sec=0.5, activity_th=0.3), FS, self.C,
                                    self.desc.frame_len, self.desc.frame_hop)
        self._rec, self._def = {}, {}

    def rec(self, rate, seconds=6.5, seed=31):
        """float32 [n, C] of `seconds` at `rate`, inside [-1, 1]"""
        key = (rate, seconds, seed)
        if key not in self._rec:
            x = (pkg("synth").synth_meeting(seconds, self.C, seed=seed, fs=rate)[0] * 0.05).astype(np.float32)
            x.setflags(write=False)
            self._rec[key] = x
        return self._rec[key]

    def definition(self, x, in_rate, out_rate, pcm16, key=None):
        if key is None or key not in self._def:
            d = _definition(self.h, x, self.cfg, in_rate, out_rate, pcm16)
            if key is None:
                return d
            self._def[key] = d
        return self._def[key]

    def run_rate(self, x, in_rate, out_rate):
        L = pkg("_lib")
        rate = _as_rate(L, in_rate, out_rate)
        if x.dtype == np.int16:
            return self.h.run_pcm16_rate([np.ascontiguousarray(x[:, c]) for c in range(x.shape[1])], self.cfg, rate)
        return self.h.run_rate(x, self.cfg, rate)


@pytest.fixture(scope="module")
def tiny():
    w = pkg("weights")
    desc = w.ModelDesc(num_blocks=2)
    env = _Env((w.apply_golden_recipe(w.portable_state_dict(desc, 21)), desc))
    yield env
    env.sep.close()


def _check(got, want, pcm16):
    if pcm16:
        (q, pk), (wq, wpk) = got, want
        assert q.dtype == np.int16 and q.shape == wq.shape and np.array_equal(q, wq)
        assert pk.dtype == np.float32 and np.array_equal(pk, wpk)
        for k in range(q.shape[0]):
            if wq[k].any():
                assert int(np.abs(q[k].astype(np.int32)).max()) == 32439, k
    else:
        assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got, want)


# ---- 1. synchronous, every edge -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pcm16", (False, True), ids=("float", "pcm16"))
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}_{p[1]}")
def test_synchronous_every_edge(pair, pcm16, tiny):
    L = pkg("_lib")
    in_rate, out_rate = pair
    x = tiny.rec(in_rate)
    if pcm16:
        x = _quantise(x)
    want = tiny.definition(x, in_rate, out_rate, pcm16, key=("sync", pair, pcm16))
    n_model, n_out_model, n_out = tiny.h.session_rate_samples(tiny.cfg, _as_rate(L, in_rate, out_rate), x.shape[0])
    assert n_model == -(-x.shape[0] * FS // in_rate) and n_out == -(-n_out_model * out_rate // FS)
    assert (want[0] if pcm16 else want).shape == (3, n_out)
    before = tiny.h.session_rate_stats()
    _check(tiny.run_rate(x, in_rate, out_rate), want, pcm16)
    after = tiny.h.session_rate_stats()
    assert after[0] - before[0] == int(in_rate != FS) and after[1] - before[1] == int(out_rate != FS) and after[2] - before[2] == 1


# ---- 2. lengths where tiles and phases end ---------------------------------------------------------------------------------------
def _shortest_k(tiny):
    """the smallest k for which k * 256 model-rate samples make a session css_run accepts (two segments: no zero weight)"""
    L = pkg("_lib")
    k = 2
    while True:
        p = L.plan(tiny.desc, tiny.cfg, k * 256)
        if p.num_segments >= 2 and not p.zero_weight:
            return k
        k += 1


def _n_in_for(n_model, up, down):
    """capture-rate samples with ceil(n_in up / down) == n_model, not a multiple of `down`"""
    n_in = n_model * down // up
    while -(-n_in * up // down) != n_model or n_in % down == 0:
        n_in -= 1
    return n_in


@pytest.mark.parametrize("residue", (0, 1, 255))
@pytest.mark.parametrize("pair", ((48000, 16000), (44100, 44100)), ids=lambda p: f"{p[0]}_{p[1]}")
def test_lengths_at_the_input_side(pair, residue, tiny):
    """n_model = k 256 + {0, 1, 255} just above the shortest accepted session, n_in no multiple of in_down; the last outputs' taps
    always run past the end of the input (i_hi = floor((m down + half) / up) > n_in - 1 for m = n_model - 1): the zero tail"""
    L = pkg("_lib")
    in_rate, out_rate = pair
    up, down = L.rate_ratio(in_rate, FS)
    n_model = (_shortest_k(tiny) + 3) * 256 + residue
    n_in = _n_in_for(n_model, up, down)
    assert n_in % down and ((n_model - 1) * down + 10 * max(up, down)) // up > n_in - 1
    for pcm16 in (False, True):
        x = tiny.rec(in_rate)[:n_in]
        assert x.shape[0] == n_in
        x = _quantise(x) if pcm16 else x
        assert tiny.h.session_rate_samples(tiny.cfg, _as_rate(L, in_rate, out_rate), n_in)[0] == n_model
        _check(tiny.run_rate(x, in_rate, out_rate), tiny.definition(x, in_rate, out_rate, pcm16), pcm16)


@pytest.mark.parametrize("frames", (439, 480, 498, 640, 759))
def test_lengths_at_the_output_side(frames, tiny):
    """44.1 kHz -> 44.1 kHz.  n_out_model is always a multiple of 256 ((mix_frames + 1) 256), so n_out = ceil(705.6 (mix_frames + 1))
    takes few residues: mix_frames + 1 = 480 and 439 give n_out = 0 and 255 mod 256 (no count between 5 and 13 s gives 1), 640 and
    759 give 0 and 1023 mod 1024, the output kernel's tile, and 498 gives 1 mod 4, its 16-byte store"""
    L = pkg("_lib")
    n_out_model = frames * 256
    n_out = -(-n_out_model * 441 // 160)
    assert {439: n_out % 256 == 255, 480: n_out % 256 == 0, 498: n_out % 4 == 1, 640: n_out % 1024 == 0, 759: n_out % 1024 == 1023}[frames]
    n_model = (frames - 2) * 256 + 512 + 77        # stft_frames = frames - 1 = mix_frames
    n_in = _n_in_for(n_model, 160, 441)
    x = _quantise(tiny.rec(44100, 13.0)[:n_in])
    assert x.shape[0] == n_in
    assert tiny.h.session_rate_samples(tiny.cfg, _as_rate(L, 44100, 44100), n_in) == (n_model, n_out_model, n_out)
    _check(tiny.run_rate(x, 44100, 44100), tiny.definition(x, 44100, 44100, True), True)


# ---- 3. alignment ----------------------------------------------------------------------------------------------------------------
def test_unaligned_inputs(tiny):
    """int16 planes at an odd sample offset inside a page-locked block (run_to_lds's head and tail); the float input a C-contiguous
    [n, 7] view 4 bytes off a 16-byte boundary"""
    L = pkg("_lib")
    x = tiny.rec(48000)
    n, c = x.shape
    xq = _quantise(x)
    block = L.pinned_empty((c * (n + 8) + 16,), np.int16)
    assert block.ctypes.data % 16 == 0
    planes = []
    for k in range(c):
        at = 1 + k * (n + 8) + 2 * k            # odd offsets: 1, n + 11, 2 n + 21, ...
        at += 1 - at % 2
        block[at:at + n] = xq[:, k]
        planes.append(block[at:at + n])
        assert (planes[-1].ctypes.data // 2) % 2 == 1
    rate = _as_rate(L, 48000, 48000)
    want = tiny.definition(xq, 48000, 48000, True, key=("sync", (48000, 48000), True))
    _check(tiny.h.run_pcm16_rate(planes, tiny.cfg, rate), want, True)
    raw = np.zeros(n * c + 8, np.float32)
    off = (4 - (raw.ctypes.data % 16) // 4 + 1) % 4
    view = raw[off:off + n * c].reshape(n, c)
    assert view.ctypes.data % 16 == 4 and view.flags.c_contiguous
    view[...] = x
    want = tiny.definition(x, 48000, 48000, False, key=("sync", (48000, 48000), False))
    _check(tiny.h.run_rate(view, tiny.cfg, rate), want, False)


# ---- 4. channel counts -----------------------------------------------------------------------------------------------------------
def test_single_channel_model(sc_state):
    env = _Env(sc_state)
    try:
        x = _quantise(env.rec(48000, 6.0, seed=32))
        assert x.shape[1] == 1
        _check(env.run_rate(x, 48000, 48000), env.definition(x, 48000, 48000, True), True)
        xf = env.rec(8000, 6.0, seed=33)
        _check(env.run_rate(xf, 8000, 16000), env.definition(xf, 8000, 16000, False), False)
    finally:
        env.sep.close()


def test_four_microphones():
    w = pkg("weights")
    desc = w.ModelDesc(num_mics=4, in_features=257 * 4, num_blocks=1)     # (the model of test_hip_mic_arrays.py)
    env = _Env((w.portable_state_dict(desc, 3), desc), num_mics=4)
    try:
        assert env.C == 4
        x = _quantise(env.rec(44100, 6.0, seed=34))
        _check(env.run_rate(x, 44100, 44100), env.definition(x, 44100, 44100, True), True)
    finally:
        env.sep.close()


# ---- 5. the queue ----------------------------------------------------------------------------------------------------------------
SENT16, SENTF = np.int16(-12345), np.float32(-77.5)


def _queue_group(env, pinned):
    """the five sessions of the group: (kind, input, rate pair) -> the arguments and output buffers of one queueing"""
    L = pkg("_lib")
    alloc = L.pinned_empty if pinned else (lambda shape, dt: np.empty(shape, dt))
    hold = L.pinned_copy if pinned else (lambda a: a.copy())
    specs = (("pcm16_rate", 48000, 16000, 14.0, 41), ("pcm16_rate", 44100, 44100, 12.0, 42), ("float_rate", 8000, 16000, 16.0, 43),
             ("pcm16", 16000, 16000, 13.0, 44), ("float", 16000, 16000, 15.0, 45))
    group = []
    for kind, in_rate, out_rate, seconds, seed in specs:
        x = env.rec(in_rate, seconds, seed)
        rate = _as_rate(L, in_rate, out_rate)
        n_out = env.h.session_rate_samples(env.cfg, rate, x.shape[0])[2]
        s = dict(kind=kind, pair=(in_rate, out_rate), rate=rate, n_out=n_out, key=("queue", kind, in_rate, out_rate, seed))
        if kind.startswith("pcm16"):
            xq = _quantise(x)
            s["x"] = xq
            block = hold(np.ascontiguousarray(xq.T))
            s["planes"] = [block[c] for c in range(block.shape[0])]
            s["out"] = alloc((3, n_out + 37), np.int16)
            s["out"][...] = SENT16
            s["peaks"] = alloc((3,), np.float32)
            s["peaks"][...] = SENTF
        else:
            s["x"] = x
            s["in"] = hold(np.ascontiguousarray(x))
            s["out"] = alloc((3, n_out + 37), np.float32)
            s["out"][...] = SENTF
        group.append(s)
    return group


def _enqueue(env, s):
    h = env.h
    if s["kind"] == "pcm16_rate":
        return h.run_enqueue_pcm16_rate(s["planes"], env.cfg, s["rate"], s["out"], s["peaks"])
    if s["kind"] == "float_rate":
        return h.run_enqueue_rate(s["in"], env.cfg, s["rate"], s["out"])
    if s["kind"] == "pcm16":
        return h.run_enqueue_pcm16(s["planes"], env.cfg, s["out"], s["peaks"])
    return h.run_enqueue(s["in"], env.cfg, s["out"])


def _sync_result(env, s):
    """the session's own synchronous result (held to the definition by the tests above): run_pcm16_rate / run_rate / run_pcm16 / run"""
    if s["key"] not in env._def:
        h = env.h
        if s["kind"] == "pcm16_rate":
            r = h.run_pcm16_rate(s["planes"], env.cfg, s["rate"])
        elif s["kind"] == "float_rate":
            r = h.run_rate(s["x"], env.cfg, s["rate"]).copy()
        elif s["kind"] == "pcm16":
            r = h.run_pcm16(s["planes"], env.cfg)
        else:
            r = h.run(s["x"], env.cfg).copy()
        env._def[s["key"]] = r
    return env._def[s["key"]]


def _check_queued(env, s):
    want = _sync_result(env, s)
    n = s["n_out"]
    if s["kind"].startswith("pcm16"):
        assert np.array_equal(s["out"][:, :n], want[0]) and np.array_equal(s["peaks"], want[1]), s["key"]
        assert np.all(s["out"][:, n:] == SENT16), s["key"]
    else:
        assert np.array_equal(s["out"][:, :n], want), s["key"]
        assert np.all(s["out"][:, n:] == SENTF), s["key"]


def test_queue_of_rate_and_plain_sessions(mc_state):
    env = _Env(mc_state, max_batch_segments=128)
    try:
        h = env.h
        for s in _queue_group(env, True):      # every session's synchronous result first (and one of them against the definition)
            _sync_result(env, s)
            if s["pair"] == (44100, 44100):
                _check(_sync_result(env, s), env.definition(s["x"], 44100, 44100, True), True)
        # twice over with page-locked buffers: the sessions share estimator batches
        first, second = _queue_group(env, True), _queue_group(env, True)
        before = h.session_rate_stats()
        for s in first + second:
            _enqueue(env, s)
        h.wait_sessions(2)
        for s in first[:2]:
            _check_queued(env, s)               # released with their outputs complete
        h.wait()
        after = h.session_rate_stats()
        for s in first + second:
            _check_queued(env, s)
        n_rate = sum(1 for s in first + second if s["kind"].endswith("_rate"))
        assert after[2] - before[2] == n_rate == 6
        # one ingest launch per shared group, not one per session: the queue cut these ten sessions into fewer groups than it has
        # rate sessions, and every group with a rate session launched once
        assert 1 <= after[0] - before[0] < n_rate, (before, after)
        assert after[1] - before[1] == 2        # the two 44.1 kHz -> 44.1 kHz sessions
        # once with pageable outputs: the sessions run one by one
        third = _queue_group(env, False)
        before = h.session_rate_stats()
        for s in third:
            _enqueue(env, s)
        h.wait()
        for s in third:
            _check_queued(env, s)
        after = h.session_rate_stats()
        assert after[0] - before[0] == 3 and after[1] - before[1] == 1 and after[2] - before[2] == 3
    finally:
        env.sep.close()


# ---- 6. refusals on a live handle --------------------------------------------------------------------------------------------------
def test_refusals_on_a_live_handle(tiny):
    L = pkg("_lib")
    h, lib, cfg = tiny.h, tiny.h.lib, tiny.cfg
    xq = _quantise(tiny.rec(48000))
    n, c = xq.shape
    planes = [np.ascontiguousarray(xq[:, k]) for k in range(c)]
    ptrs = (C.c_void_p * c)(*[p.ctypes.data for p in planes])
    ok = _as_rate(L, 48000, 48000)
    n_out = h.session_rate_samples(cfg, ok, n)[2]
    out16 = L.pinned_empty((3, n_out), np.int16)
    out16[...] = SENT16
    peaks = L.pinned_empty((3,), np.float32)
    peaks[...] = SENTF
    xf = L.pinned_copy(np.ascontiguousarray(tiny.rec(48000)))
    outf = L.pinned_empty((3, n_out), np.float32)
    outf[...] = SENTF
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    before = h.session_rate_stats()

    def pcm16_calls(ptrs_, n_, rate, cap):
        return [fn(h.h, ptrs_, n_, c, C.byref(cfg.c), C.byref(rate), P(out16), cap, P(peaks))
                for fn in (lib.css_run_enqueue_pcm16_rate, lib.css_run_pcm16_rate)]

    def float_calls(n_, rate, cap):
        return [fn(h.h, P(xf), n_, c, C.byref(cfg.c), C.byref(rate), P(outf), cap) for fn in (lib.css_run_enqueue_rate, lib.css_run_rate)]

    E = L.CSS_ERR_INVALID_ARG
    for bad in (L.CssSessionRate(1, 7, 1, 1), L.CssSessionRate(1, 3, 1, 7), L.CssSessionRate(2, 2, 1, 1)):
        assert pcm16_calls(ptrs, n, bad, n_out) + float_calls(n, bad, n_out) == [E] * 4
    assert pcm16_calls(ptrs, n, ok, n_out - 1) + float_calls(n, ok, n_out - 1) == [E] * 4
    assert pcm16_calls(ptrs, 0, ok, n_out) + float_calls(0, ok, n_out) == [E] * 4
    holed = (C.c_void_p * c)(*[p.ctypes.data if k != 3 else None for k, p in enumerate(planes)])
    assert pcm16_calls(holed, n, ok, n_out) == [E] * 2
    # too short for css_run after the conversion: one segment, css_run's own status for the converted recording
    short = 48000
    x16 = h.resample(xq[:short], 48000, FS)
    with pytest.raises(AssertionError) as e_run:
        h.run(x16, cfg)
    assert pcm16_calls(ptrs, short, ok, n_out) + float_calls(short, ok, n_out) == [L.CSS_ERR_ZERO_WEIGHT] * 4
    with pytest.raises(AssertionError) as e_rate:
        h.run_pcm16_rate([p[:short] for p in planes], cfg, ok)
    assert str(e_rate.value) == str(e_run.value)
    # nothing was queued, written or counted: wait() returns at once, and a following valid session is bit-exact
    h.wait()
    assert np.all(out16 == SENT16) and np.all(peaks == SENTF) and np.all(outf == SENTF)
    assert h.session_rate_stats() == before
    want = tiny.definition(xq, 48000, 48000, True, key=("sync", (48000, 48000), True))
    got = h.run_enqueue_pcm16_rate(planes, cfg, ok, out16, peaks)
    h.wait()
    _check((got, peaks), want, True)
    # split_f16: css_wait may repeat a session from its input buffers
    h.set_linear_mode("split_f16")
    try:
        assert pcm16_calls(ptrs, n, ok, n_out) + float_calls(n, ok, n_out) == [L.CSS_ERR_STATE] * 4
        h.wait()
    finally:
        h.set_linear_mode("exact_f32")
    _check(h.run_pcm16_rate(planes, cfg, ok), want, True)


# ---- 7. files --------------------------------------------------------------------------------------------------------------------
def test_sessions_from_48k_files(tmp_path, tiny):
    import pandas as pd
    import torch
    import yaml
    css, wavio, pipe, sep_mod, L = pkg("css"), pkg("wavio"), pkg("pipeline"), pkg("separator"), pkg("_lib")
    # the tiny model's checkpoint directory, as test_hip_session.py::tiny_models writes it
    d = tmp_path / "models" / "notsofar" / "conformer1.0" / "mc"
    d.mkdir(parents=True)
    st = pkg("weights").apply_golden_recipe(pkg("weights").portable_state_dict(tiny.desc, 21))
    torch.save({"model": {"module." + k: torch.from_numpy(np.asarray(v)) for k, v in st.items()}}, d / "model.pt")
    with open(d / "train_cfg.yaml", "w") as f:
        yaml.safe_dump({"train_dir": "x", "val_dir": "x", "out_dir": "x",
                        "conformer_css_cfg": {"nnet_conf": {"conformer_conf": {"attention_dim": 512, "attention_heads": 8, "num_blocks": 2,
                                                                               "dropout_rate": 0.0}}}}, f)
    models_dir = str(tmp_path / "models")
    rows, payload = [], {}
    for i in range(2):
        xq = _quantise(tiny.rec(48000, 6.0 + 0.5 * i, seed=51 + i))
        names = []
        for c in range(7):
            p = tmp_path / f"S{i}_ch{c}.wav"
            wavio.write_pcm16_samples(p, xq[:, c], 48000)
            names.append(str(p))
        rows.append({"wav_file_names": names, "session_id": f"S{i}", "is_mc": True})
        payload[f"S{i}"] = xq
    df = pd.DataFrame(rows)
    cfg = css.CssCfg(activity_th=0.3, show_progressbar=False)
    run_cfg = css.make_run_cfg(cfg, FS, 7, tiny.desc.frame_len, tiny.desc.frame_hop)
    for out_rate, out_sr, sub in ((None, 16000, "a"), ("input", 48000, "b")):
        res = pipe.css_sessions(str(tmp_path / sub), models_dir, df, cfg, device="cuda:0", model_rate=16000, output_rate=out_rate)
        for _, row in res.iterrows():
            want, _ = _definition(tiny.h, payload[row.session_id], run_cfg, 48000, out_sr, True)
            assert [os.path.basename(f) for f in row.sep_wav_file_names] == [f"sep_stream{k}.wav" for k in range(3)]
            for k, f in enumerate(row.sep_wav_file_names):
                got, sr = wavio.read_wav_pcm16(f)
                assert sr == out_sr and np.array_equal(got, want[k]), (row.session_id, out_rate, k)
            mixq, sr = wavio.read_wav_pcm16(os.path.join(os.path.dirname(row.sep_wav_file_names[0]), "input_mixture.wav"))
            assert sr == 48000 and len(mixq) == payload[row.session_id].shape[0]      # channel 0 as read, at the files' rate
    # css_inference alone takes the same calls
    one = css.css_inference(str(tmp_path / "c"), models_dir, df.iloc[0], cfg, False, model_rate=16000, output_rate="input")
    want, _ = _definition(tiny.h, payload["S0"], run_cfg, 48000, 48000, True)
    for k, f in enumerate(one["sep_wav_file_names"]):
        got, sr = wavio.read_wav_pcm16(f)
        assert sr == 48000 and np.array_equal(got, want[k])
    # model_rate=None: byte for byte what css_inference writes the old way (the files' rate is taken as the model's)
    res = pipe.css_sessions(str(tmp_path / "new"), models_dir, df, cfg, device="cuda:0", model_rate=None)
    for _, row in res.iterrows():
        old = css.css_inference(str(tmp_path / "old"), models_dir, df[df.session_id == row.session_id].iloc[0], cfg, False)
        for f_new, f_old in zip(row.sep_wav_file_names, old["sep_wav_file_names"]):
            assert open(f_new, "rb").read() == open(f_old, "rb").read()
        mix_new = os.path.join(os.path.dirname(row.sep_wav_file_names[0]), "input_mixture.wav")
        mix_old = os.path.join(os.path.dirname(old["sep_wav_file_names"][0]), "input_mixture.wav")
        assert open(mix_new, "rb").read() == open(mix_old, "rb").read()
