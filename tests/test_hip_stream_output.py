"""Final samples at the playback rate on the MI355X (include/css_mi355_stream_out.h; stream.py output=).

The oracle is the definition: with w = css_run's waveforms of the whole recording, a float32 stream wrote
y = handle.resample(w.T, 16000, rate) -- css_resample_host of the S waveforms as S planar channels -- and an int16 stream
_lib.pcm16_encode(y, gain), the numpy statement of the two PCM16 lines, however the pushes were cut.  Every comparison is
np.array_equal.  Where the issue speaks of "the float twin's output" or "its single-stream result", the tests compare with this
definition instead of a second stream: test_float_output and test_int16_output hold the single streams to it, so the
comparison is the same and one stream fewer runs.  References are computed once per module and shared."""
import ctypes as C

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

CHUNKS = (1, 255, 256, 257, 4000, 24000, 32000)
HANDOFF = dict(n_mels=80, pad_frames=8, drop_silence=True)


def _seeded_sizes(seed, n=64):
    rs = np.random.RandomState(seed)
    return [int(CHUNKS[j]) for j in rs.randint(0, len(CHUNKS), n)]


class _Env:
    """one separator, the recordings and their references (css_run, the definition at each rate), made on first use"""

    def __init__(self, state, mix60):
        st, _ = state
        self.sep = pkg("separator").HipSeparator(st, None, device=0)
        CSS = pkg("css")
        self.x = np.ascontiguousarray((mix60[0] if mix60.ndim == 3 else mix60)[:12 * 16000], np.float32)
        self.cfgs = {"short": CSS.CssCfg(segment_size_sec=2.0, hop_size_sec=0.5), "default": CSS.CssCfg()}
        self._w, self._y = {}, {}

    def rec(self, key):
        return {"short": self.x, "default": self.x[:10 * 16000], "six": self.x[:6 * 16000]}[key]

    def cfg(self, key):
        return self.cfgs["default" if key == "default" else "short"]

    def w(self, key):
        """css_run of recording `key`: float32 [S, n_out]"""
        if key not in self._w:
            x = self.rec(key)
            self._w[key] = self.sep.handle.run(x, pkg("css").make_run_cfg(self.cfg(key), 16000, x.shape[1])).copy()
            self._w[key].setflags(write=False)
        return self._w[key]

    def y(self, key, rate):
        """the definition's float output of recording `key` at `rate`: float32 [S, ceil(n_out up / down)]"""
        if (key, rate) not in self._y:
            w = self.w(key)
            y = w if rate == 16000 else np.ascontiguousarray(self.sep.handle.resample(w.T, 16000, rate).T)
            y.setflags(write=False)
            self._y[(key, rate)] = y
        return self._y[(key, rate)]


@pytest.fixture(scope="module")
def env(mc_state, mix60):
    return _Env(mc_state, mix60)


def _play(env, key, sizes, output, between=None, **kw):
    """one stream over recording `key` cut by `sizes`; after every push the count rule -> (outputs [S, m], the stream's last
    counts, the model-rate samples if asked for)"""
    S = pkg("stream")
    x, outs, model = env.rec(key), [], []
    with S.CssStream(env.sep, env.cfg(key), num_channels=x.shape[1], output=output, **kw) as s:
        n, i, total = 0, 0, 0
        while n < x.shape[0]:
            k = min(sizes[i % len(sizes)], x.shape[0] - n)
            got = np.stack(s.push(x[n:n + k]))
            n += k
            i += 1
            total += got.shape[1]
            assert total == s.output_samples(s.final_samples(n)) == s.output_total, (n, total)
            assert got.dtype == s._odtype
            outs.append(got)
            if s.model_rate is not None:
                model.append(np.stack(s.model_rate))
            if between is not None:
                between(s)
        outs.append(np.stack(s.finish()))
        if s.model_rate is not None:
            model.append(np.stack(s.model_rate))
        total += outs[-1].shape[1]
        assert total == s.output_samples(s.info().n_emitted, True) == s.output_total
        res = dict(clipped=s.output_clipped, peaks=s.output_peaks)
    return np.concatenate(outs, axis=1), res, (np.concatenate(model, axis=1) if model else None)


def _clipping_gain(y):
    """a gain under which about 5 % of the samples leave the int16 range: chosen from the float output, asserted 1 .. 20 %"""
    L = pkg("_lib")
    gain = float(np.float32(1.0 / np.quantile(np.abs(y), 0.95)))
    _, n = L.pcm16_encode(y, gain)
    assert 0.01 * y.size <= n <= 0.20 * y.size, (gain, n, y.size)
    return gain


# ---- 1. float output -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", (48000, 44100, 8000))
def test_float_output(rate, env):
    y = env.y("short", rate)
    assert y.shape[1] == -(-env.w("short").shape[1] * rate // 16000)
    got, res, _ = _play(env, "short", _seeded_sizes(rate), dict(rate=rate))
    assert got.dtype == np.float32 and got.shape == y.shape and np.array_equal(got, y)
    assert not res["clipped"].any()
    one, _, _ = _play(env, "short", [env.rec("short").shape[0]], dict(rate=rate, dtype="float32"))
    assert np.array_equal(one, y)


def test_float_output_default_segments(env):
    """3 s / 1.5 s segments on 10 s: other round sizes, other window rebases"""
    y = env.y("default", 48000)
    got, _, _ = _play(env, "default", _seeded_sizes(7), dict(rate=48000))
    assert got.shape == y.shape and np.array_equal(got, y)


# ---- 2. int16 output -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", (48000, 16000))
def test_int16_output(rate, env):
    L = pkg("_lib")
    y = env.y("short", rate)
    gain = _clipping_gain(y)
    want = [L.pcm16_encode(y[k], gain) for k in range(y.shape[0])]
    got, res, _ = _play(env, "short", _seeded_sizes(rate + 1), dict(rate=rate, dtype="int16", gain=gain))
    assert got.dtype == np.int16 and got.shape == y.shape
    assert np.array_equal(got, np.stack([q for q, _ in want]))
    assert res["clipped"].tolist() == [n for _, n in want] and min(n for _, n in want) > 0
    # a gain that clips nothing: the same lines, a count of zero
    low = float(np.float32(0.5 / np.abs(y).max()))
    got, res, _ = _play(env, "short", [24000], dict(rate=rate, dtype="int16", gain=low))
    assert np.array_equal(got, np.stack([L.pcm16_encode(y[k], low)[0] for k in range(y.shape[0])])) and not res["clipped"].any()


# ---- 3. the whole live path ----------------------------------------------------------------------------------------------------
def test_pcm16_in_at_48k_pcm16_out_at_48k(env):
    S, L = pkg("stream"), pkg("_lib")
    x = env.rec("short")
    q16 = np.clip(np.rint(x.astype(np.float64) * 0.5 * 32768.0), -32768, 32767).astype(np.int16)
    rec48 = np.ascontiguousarray(np.repeat(q16, 3, axis=0))   # (a capture at 48 kHz; its spectrum is of no interest here)
    h = env.sep.handle
    x16 = h.resample(rec48, 48000)
    w = h.run(x16, pkg("css").make_run_cfg(env.cfg("short"), 16000, x16.shape[1])).copy()
    y = h.resample(w.T, 16000, 48000).T
    gain = 0.7
    want = np.stack([L.pcm16_encode(y[k], gain)[0] for k in range(y.shape[0])])
    sizes = [3 * k for k in _seeded_sizes(3)]
    outs = []
    with S.CssStream(env.sep, env.cfg("short"), input_rate=48000, output=dict(rate=48000, dtype="int16", gain=gain)) as s:
        n, i = 0, 0
        while n < rec48.shape[0]:
            k = min(sizes[i % len(sizes)], rec48.shape[0] - n)
            outs.append(np.stack(s.push_pcm16(rec48[n:n + k])))
            n += k
            i += 1
            assert sum(o.shape[1] for o in outs) == s.output_samples(s.final_samples(n))
        outs.append(np.stack(s.finish()))
    got = np.concatenate(outs, axis=1)
    assert got.shape == want.shape and np.array_equal(got, want)


# ---- 4. groups -----------------------------------------------------------------------------------------------------------------
def _group(env, key, outputs, sizes_of):
    """streams with `outputs` (None: no output format) in one group over recording `key`, stream j cut by sizes_of(j)"""
    S = pkg("stream")
    x = env.rec(key)
    streams = [S.CssStream(env.sep, env.cfg(key), output=o) for o in outputs]
    stats = []
    try:
        g = S.CssStreamGroup(streams)
        pos, outs = [0] * len(streams), [[] for _ in streams]
        sizes = [sizes_of(j) for j in range(len(streams))]
        i = 0
        while any(p < x.shape[0] for p in pos):
            chunks = []
            for j in range(len(streams)):
                k = min(sizes[j][i % len(sizes[j])], x.shape[0] - pos[j])
                chunks.append(x[pos[j]:pos[j] + k] if k > 0 else None)
                pos[j] += k
            for j, got in enumerate(g.push(chunks)):
                outs[j].append(np.stack(got))
            stats.append((env.sep.handle.stream_output_stats(), sum(c is not None for c in chunks)))
            i += 1
        for j, s in enumerate(streams):
            outs[j].append(np.stack(s.finish()))
        peaks = [s.output_peaks for s in streams]
    finally:
        for s in streams:
            s.close()
    return [np.concatenate(o, axis=1) for o in outs], stats, peaks


def test_group_of_mixed_formats(env):
    L = pkg("_lib")
    y48, y44, w = env.y("short", 48000), env.y("short", 44100), env.w("short")
    outs, stats, _ = _group(env, "short", [dict(rate=48000, dtype="int16", gain=0.5), dict(rate=44100), None],
                            lambda j: _seeded_sizes(40 + j))
    assert outs[0].dtype == np.int16 and np.array_equal(outs[0], np.stack([L.pcm16_encode(y48[k], 0.5)[0] for k in range(3)]))
    assert outs[1].dtype == np.float32 and np.array_equal(outs[1], y44)
    assert outs[2].dtype == np.float32 and np.array_equal(outs[2], w)
    assert all(launches == rounds for (launches, rounds), _ in stats) and any(rounds > 0 for (_, rounds), _ in stats)


def test_group_of_eighteen_crosses_the_table(env):
    L = pkg("_lib")
    kinds = [dict(rate=48000, dtype="int16", gain=0.5), dict(rate=44100), dict(rate=8000), dict(rate=16000, dtype="int16", gain=2.0)]
    outputs = [kinds[j % 4] for j in range(18)]
    assert len(outputs) > L.STREAM_OUTPUT_TABLE
    # every stream takes the same cuts, so every round that makes samples final holds all 18
    outs, stats, _ = _group(env, "six", outputs, lambda j: [16000, 4000, 257, 24000])
    for j, o in enumerate(outputs):
        y = env.y("six", o["rate"])
        want = np.stack([L.pcm16_encode(y[k], o["gain"])[0] for k in range(y.shape[0])]) if o.get("dtype") == "int16" else y
        assert outs[j].dtype == want.dtype and np.array_equal(outs[j], want), j
    per_table = -(-18 // L.STREAM_OUTPUT_TABLE)
    assert all(launches == per_table * rounds for (launches, rounds), _ in stats), stats
    assert sum(rounds for (_, rounds), _ in stats) >= 3


# ---- 5. twins ------------------------------------------------------------------------------------------------------------------
def test_handoff_preview_and_model_rate_twins(env):
    """a stream with the hand-off, an output format, the model-rate floats asked for as well and a preview() between the pushes,
    beside a twin with the hand-off alone: the same hand-off and the same floats, and the outputs of the definition"""
    S, L = pkg("stream"), pkg("_lib")
    x, w, y = env.rec("short"), env.w("short"), env.y("short", 48000)
    sizes = _seeded_sizes(11)
    seen = {"a": [], "b": []}

    def run(tag, output, preview):
        outs, floats = [], []
        with S.CssStream(env.sep, env.cfg("short"), handoff=HANDOFF, output=output) as s:
            n, i = 0, 0
            while n <= x.shape[0]:
                last = n == x.shape[0]
                if last:
                    got = s.finish()
                else:
                    k = min(sizes[i % len(sizes)], x.shape[0] - n)
                    got = s.push(x[n:n + k])
                    n += k
                    i += 1
                outs.append(np.stack(got))
                floats.append(np.stack(s.model_rate) if output else outs[-1])
                ho = s.handoff
                seen[tag].append((ho.mel, ho.ranges, ho.activity, ho.raw_max.copy(), ho.first_activity_frame))
                if last:
                    break
                if preview:
                    try:
                        pv = s.preview()
                        assert pv[0].dtype == np.float32 and s.preview_first_sample == s.info().n_emitted
                    except AssertionError as e:   # (css_run refuses a prefix of less than two segments)
                        assert "zero weights" in str(e)
        return np.concatenate(outs, axis=1), np.concatenate(floats, axis=1)

    out_a, fl_a = run("a", dict(rate=48000, dtype="int16", gain=0.5, model_rate=True), True)
    out_b, fl_b = run("b", None, False)
    assert np.array_equal(out_a, np.stack([L.pcm16_encode(y[k], 0.5)[0] for k in range(3)]))
    assert np.array_equal(fl_a, w) and np.array_equal(fl_b, w) and np.array_equal(out_b, w)
    assert len(seen["a"]) == len(seen["b"])
    for a, b in zip(seen["a"], seen["b"]):
        for k in range(3):
            assert np.array_equal(a[0][k], b[0][k]) and np.array_equal(a[1][k], b[1][k]) and np.array_equal(a[2][k], b[2][k])
        assert np.array_equal(a[3], b[3]) and a[4] == b[4]


def test_preview_with_handoff_on_a_stream_with_an_output_format(env):
    """preview(handoff=True) after every push of a stream with the hand-off and an output format, beside a twin with the hand-off
    alone (6 s, 2.0 s / 0.5 s segments): the same provisional samples and the same provisional hand-off; a preview writes nothing
    at the playback rate, so the stream's outputs are the definition's"""
    S, L = pkg("stream"), pkg("_lib")
    x, w, y = env.rec("six"), env.w("six"), env.y("six", 48000)
    sizes = [16000, 4000, 257, 24000]

    def run(output):
        outs, pvs = [], []
        with S.CssStream(env.sep, env.cfg("six"), handoff=HANDOFF, output=output) as s:
            n, i = 0, 0
            while n < x.shape[0]:
                k = min(sizes[i % len(sizes)], x.shape[0] - n)
                outs.append(np.stack(s.push(x[n:n + k])))
                n += k
                i += 1
                total = s.output_total if output else 0
                try:
                    pv = np.stack(s.preview(handoff=True))
                    ho = s.preview_handoff
                    pvs.append((s.preview_first_sample, pv, ho.mel, ho.ranges, ho.activity, ho.raw_max.copy(), ho.first_activity_frame,
                                ho.first_frame.copy()))
                except AssertionError as e:   # (css_run refuses a prefix of less than two segments)
                    assert "zero weights" in str(e)
                    pvs.append(None)
                assert not output or s.output_total == total
            outs.append(np.stack(s.finish()))
        return np.concatenate(outs, axis=1), pvs

    out_a, pv_a = run(dict(rate=48000, dtype="int16", gain=0.5))
    out_b, pv_b = run(None)
    assert np.array_equal(out_a, np.stack([L.pcm16_encode(y[k], 0.5)[0] for k in range(3)])) and np.array_equal(out_b, w)
    assert len(pv_a) == len(pv_b) and any(p is not None for p in pv_a)
    for a, b in zip(pv_a, pv_b):
        assert (a is None) == (b is None)
        if a is None:
            continue
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[5], b[5]) and a[6] == b[6] and np.array_equal(a[7], b[7])
        for k in range(3):
            assert np.array_equal(a[2][k], b[2][k]) and np.array_equal(a[3][k], b[3][k]) and np.array_equal(a[4][k], b[4][k])


# ---- 6. peaks ------------------------------------------------------------------------------------------------------------------
def test_peaks_are_run_pcm16s(env):
    S = pkg("stream")
    x = env.rec("short")
    q16 = np.clip(np.rint(x.astype(np.float64) * 0.5 * 32768.0), -32768, 32767).astype(np.int16)
    planes = [np.ascontiguousarray(q16[:, c]) for c in range(q16.shape[1])]
    _, peaks = env.sep.handle.run_pcm16(planes, pkg("css").make_run_cfg(env.cfg("short"), 16000, len(planes)))
    assert peaks.dtype == np.float32 and (peaks > 0).all()
    sizes = _seeded_sizes(21)
    for output in (dict(rate=48000, dtype="int16", gain=0.5), dict(rate=16000), None):
        with S.CssStream(env.sep, env.cfg("short"), output=output) as s:
            assert not s.output_peaks.any()
            n, i, running = 0, 0, np.zeros(3, np.float32)
            while n < q16.shape[0]:
                k = min(sizes[i % len(sizes)], q16.shape[0] - n)
                got = s.push_pcm16(q16[n:n + k])
                n += k
                i += 1
                if output is None and got[0].size:   # (the running peak, not only the final one)
                    running = np.maximum(running, np.abs(np.stack(got)).max(axis=1))
                    assert np.array_equal(s.output_peaks.view(np.uint32), running.view(np.uint32))
            s.finish()
            assert np.array_equal(s.output_peaks.view(np.uint32), peaks.view(np.uint32)), output


# ---- 7. refusals change nothing ------------------------------------------------------------------------------------------------
def _state(s):
    i = s.info()
    return (i.n_pushed, i.n_emitted, i.device_bytes, i.finished)


def test_refusals_change_nothing(env):
    S, L = pkg("stream"), pkg("_lib")
    lib, h = env.sep.handle.lib, env.sep.handle.h
    x, w, y = env.rec("short"), env.w("short"), env.y("short", 48000)
    gain = 0.5
    want = np.stack([L.pcm16_encode(y[k], gain)[0] for k in range(3)])
    ok = L.CssStreamOutputCfg(3, 1, 1, gain)
    with S.CssStream(env.sep, env.cfg("short"), output=dict(rate=48000, dtype="int16", gain=gain)) as s, \
            S.CssStream(env.sep, env.cfg("short")) as t:
        before, with_format = _state(t), _state(s)
        assert with_format[2] > before[2] and with_format[:2] == (0, 0)
        # what is no output format is refused, and t stays the plain stream it was
        for up, down, g in ((2, 2, 1.0), (0, 1, 1.0), (1, 7, 1.0), (6, 2, 1.0), (3, 1, 0.0), (3, 1, -1.0), (3, 1, float("nan")),
                            (3, 1, float("inf")), (1, 1, 0.0)):
            bad = L.CssStreamOutputCfg(up, down, 1, g)
            assert lib.css_stream_set_output(h, t.id, C.byref(bad)) == L.CSS_ERR_INVALID_ARG, (up, down, g)
        assert lib.css_stream_set_output(h, t.id, None) == L.CSS_ERR_INVALID_ARG
        buf = L.pinned_empty((3, 8), np.int16)
        clip, bits = np.zeros(3, np.int64), np.zeros(3, np.uint32)
        counts = L.CssStreamOutputCounts(-5, -5, clip.ctypes.data, bits.ctypes.data)
        # no output format: nothing to bind to
        assert lib.css_stream_output_bind(h, t.id, C.c_void_p(buf.ctypes.data), 8, C.byref(counts)) == L.CSS_ERR_STATE
        assert _state(t) == before
        assert lib.css_stream_set_output(h, s.id, C.byref(ok)) == L.CSS_ERR_STATE          # a second time
        assert lib.css_stream_output_bind(h, s.id, C.c_void_p(buf.ctypes.data), 8, None) == L.CSS_ERR_INVALID_ARG
        assert _state(s) == with_format
        # a push with nothing bound, then with a capacity one sample short: nothing moves
        first = np.ascontiguousarray(x[:48000])
        need = L.stream_output_samples(ok, s.final_samples(48000))
        assert need > 0
        n_out = C.c_int64(-1)
        push = lambda: lib.css_stream_push(h, s.id, first.ctypes.data_as(C.c_void_p), first.shape[0], None, 0, C.byref(n_out))
        assert push() == L.CSS_ERR_STATE and _state(s) == with_format
        short = L.pinned_empty((3, need), np.int16)
        short[...] = 77
        assert lib.css_stream_output_bind(h, s.id, C.c_void_p(short.ctypes.data), need - 1, C.byref(counts)) == L.CSS_OK
        assert push() == L.CSS_ERR_INVALID_ARG and _state(s) == with_format
        assert (short == 77).all() and (counts.n_written, counts.n_total) == (-5, -5) and n_out.value == -1
        assert lib.css_stream_output_bind(h, s.id, None, 0, None) == L.CSS_OK             # unbound again
        assert push() == L.CSS_ERR_STATE and _state(s) == with_format
        # the stream takes the recording as if nothing had happened
        outs, n = [], 0
        for k in [48000] + _seeded_sizes(31):
            k = min(k, x.shape[0] - n)
            if k == 0:
                break
            outs.append(np.stack(s.push(x[n:n + k])))
            n += k
            if n == 48000:   # a stream that has samples takes no output format, and is what it was
                tb = _state(t)
                got_t = np.stack(t.push(first))
                assert lib.css_stream_set_output(h, t.id, C.byref(ok)) == L.CSS_ERR_STATE
                assert lib.css_stream_set_output(h, s.id, C.byref(ok)) == L.CSS_ERR_STATE
                assert _state(t)[2] == tb[2] and np.array_equal(got_t, w[:, :got_t.shape[1]])
                more = np.stack(t.push(x[48000:56000]))
                assert np.array_equal(more, w[:, got_t.shape[1]:got_t.shape[1] + more.shape[1]])
        outs.append(np.stack(s.finish()))
        assert np.array_equal(np.concatenate(outs, axis=1), want)


# ---- 8. streams without an output format hold what they held -------------------------------------------------------------------
def test_plain_streams_hold_what_they_held(mc_state, mix60):
    """on a fresh handle: a plain stream opened before any stream had an output format, and one opened after"""
    S, CSS = pkg("stream"), pkg("css")
    st, _ = mc_state
    sep = pkg("separator").HipSeparator(st, None, device=0)
    x = np.ascontiguousarray((mix60[0] if mix60.ndim == 3 else mix60)[:6 * 16000], np.float32)
    cfg = CSS.CssCfg(segment_size_sec=2.0, hop_size_sec=0.5)

    def plain():
        outs = []
        with S.CssStream(sep, cfg) as s:
            bytes_ = [s.info().device_bytes]
            for a in range(0, x.shape[0], 20000):
                outs.append(np.stack(s.push(x[a:a + 20000])))
                bytes_.append(s.info().device_bytes)
            outs.append(np.stack(s.finish()))
            bytes_.append(s.info().device_bytes)
        return np.concatenate(outs, axis=1), bytes_

    first, bytes_first = plain()
    with S.CssStream(sep, cfg, output=dict(rate=48000, dtype="int16")) as o:
        o.push(x[:40000])
        second, bytes_second = plain()
        assert o.info().device_bytes > bytes_first[0]
    assert bytes_first == bytes_second and np.array_equal(first, second)
    sep.close()
