"""Streaming separation: a meeting separated while it happens (css_stream_* of include/css_mi355.h).

Samples arrive in chunks of any size; every ``push`` returns the output samples of the S separated streams that have become
final -- equal, bit for bit, to what ``css_run`` (this package's ``separate_and_stitch``) gives on the whole recording,
whatever follows -- and ``finish`` returns the rest.  The lag between input and final output is bounded by the
segmentation (``latency_samples``: 3.6 s with the default 3 s / 1.5 s segments).  Exact float32 arithmetic and 512 / 256 frames only.

``CssStreamGroup`` pushes into many streams of one separator in one call (css_stream_push_many): the segments the streams
complete in that call share the mask estimator's batches, so N live meetings cost about one estimator pass per tick instead
of N.  Every stream's output is what its own ``push`` would have returned, bit for bit.

``push_pcm16`` on both takes 16-bit PCM as a capture device or a decoder delivers it -- int16 [n, C] interleaved, or the planar
view ``planes.T`` of C mono recordings -- moves it to the device as int16 and scales and de-interleaves it there
(css_stream_push_pcm16, css_stream_push_many_pcm16): the result is that of ``push(chunk.astype(float32) / 32768)``, bit for bit.

``CssStream(..., handoff=dict(n_mels=80, pad_frames=8, drop_silence=True))`` switches the hand-off to the ASR front end on
(css_stream_handoff_*): after every ``push`` / ``finish`` / grouped push, ``stream.handoff`` holds what became final in that
call -- raw Whisper log-mel frames, the kept sample ranges and the gate bits per separated stream (``Handoff``).  All calls'
frames of a finished stream, through ``whisper_normalize``, are ``Handle.handoff_logmel`` of the whole recording, bit for bit.

``CssStream(..., nemo=dict(n_mels=80, pad_frames=8, drop_silence=True, preemphasis=0.97))`` switches the NeMo hand-off on instead
(css_stream_nemo_open, include/css_mi355_stream_nemo.h): after every ``push`` / ``push_pcm16`` / ``finish`` / grouped push,
``stream.nemo`` holds what became final in that call -- the raw NeMo frames ``ln(mel + 2^-24)`` that became complete (frame j once
160 j + 256 kept samples are appended; ``finish`` emits the rest), the kept ranges and the gate bits by the Whisper hand-off's
rules (``Handoff``; ``raw_max`` is None).  All calls' frames of a finished stream are
``Handle.handoff_nemo_all(..., normalize=False).mel[k]`` of the whole recording, bit for bit.  A stream has one format:
``nemo=`` with ``handoff=`` or ``window_history=`` raises ValueError.

``CssStream(..., nemo={...}, nemo_history=1024)`` (css_stream_nemo_history_open, include/css_mi355_nemo_chunk.h) also keeps the last
``nemo_history`` raw NeMo frames of every separated stream on the device.  ``nemo_chunk(k)`` and
``CssStreamGroup.nemo_chunks(requests)`` (css_stream_nemo_chunks) return a NeMo consumer's chunks as torch tensors on the handle's
device -- a span of those frames, raw (cache-aware streaming FastConformer, ``normalize: NA``) or normalised per band over the span
(buffered inference: ``(x - mean) / (std + 1e-5)`` with the span's own mean and unbiased std), padded to ``width`` columns with
``pad_value``, float32 or float16 -- without the frames crossing PCIe again: ``nemo_chunk_features`` of the frames the pushes
returned, bit for bit.

``CssStream(..., input_rate=48000)`` takes its pushes at the capture rate (css_stream_set_rate): ``push`` and ``push_pcm16`` move the
samples to the device as they were captured and the rate conversion to the model's ``fs`` -- ``scipy.signal.resample_poly``'s
default filter, in float32 -- is part of the ingest kernel.  A finished stream returned ``css_run`` of
``handle.resample(recording, input_rate)``, bit for bit; ``final_samples``, ``handoff_bounds`` and ``handoff_final_frames`` then
count input samples, everything a stream returns stays at the model rate.

``preview()`` on both (css_stream_preview, css_stream_preview_many; include/css_mi355_preview.h) returns the unfinished tail: the
samples between the final ones and the present, equal to ``css_run`` of what was pushed so far, bit for bit, while the stream
stays as it was.  One pending segment per stream passes the estimator; a grouped preview is one batch for all its streams.

``preview(handoff=True)`` on a stream opened with ``handoff=`` (css_stream_preview_handoff, css_stream_preview_handoff_many;
include/css_mi355_preview_handoff.h) also sets ``stream.preview_handoff``: the hand-off outputs ``finish`` would return at this
moment -- provisional raw log-mel frames from frame ``first_frame[k]`` of stream k's concatenation on, the kept ranges of the
undecided samples, the gate bits up to the present and the maximum over all of it -- while ``stream.handoff``, the last push's,
and the stream stay as they were.  With what the pushes returned this is ``Handle.handoff_logmel`` of the prefix, bit for bit.

``CssStream(..., handoff={...}, window_history=3000)`` (css_stream_window_open, include/css_mi355_window.h) also keeps the last
``window_history`` raw frames of every separated stream on the device.  ``window(k)`` and ``CssStreamGroup.windows(requests)``
(css_stream_windows) return Whisper encoder inputs as torch tensors on the handle's device -- a span of those frames clamped at
its own maximum - 8, (x + 4) / 4, padded to ``width`` columns, float16 or float32 -- without the frames crossing PCIe again:
``whisper_window`` of the frames the pushes returned, bit for bit.

``present_window(k)`` and ``CssStreamGroup.present_windows(requests)`` (css_stream_present_windows,
include/css_mi355_present_window.h) are ``preview(handoff=True)`` and windows in one call and under one synchronise: the span
ends at the present frame -- the history's final frames, then the preview's provisional ones, which never leave the device for
this -- and ``present_span`` tells (first_frame, n_used, n_provisional).  ``whisper_window`` of the frames the pushes returned
followed by ``preview_handoff.mel[k]``, bit for bit.

``CssStream(..., output=dict(rate=48000, dtype="int16", gain=1 / 16))`` (css_stream_set_output, include/css_mi355_stream_out.h)
gives the stream an output format: ``push`` / ``push_pcm16`` / ``finish`` and the grouped pushes then return the final samples at
the playback rate -- ``handle.resample(css_run(x).T, fs, rate)`` of the whole recording, bit for bit, however the pushes were cut
-- as float32, or as int16 through ``_lib.pcm16_encode``'s two lines (``gain``, round half to even, clamp; no peak
normalisation), converted on the device into page-locked buffers; nothing crosses PCIe at the model rate unless
``model_rate=True`` is among the options (``stream.model_rate`` then holds the call's float32 samples).  ``rate`` defaults to
``fs`` (no rate change), ``dtype`` to float32, ``gain`` to 1.  ``output_clipped`` counts the samples the clamp changed,
``output_peaks`` is max |w_k| over the final samples so far -- on every stream, with or without an output format; after ``finish``
it is ``Handle.run_pcm16``'s peaks.  ``preview()`` stays float32 at the model rate.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Mapping, Optional, Sequence, Union

import numpy as np

from . import _lib
from .css import CssCfg, make_run_cfg
from .separator import HipSeparator


def whisper_normalize(raw: np.ndarray, raw_max: Optional[float] = None) -> np.ndarray:
    """Whisper's clamp and scaling of raw log-mel frames: (max(raw, raw_max - 8) + 4) / 4 in float32.  ``raw_max`` defaults to
    the maximum of ``raw`` itself -- what Whisper does with one (30 s) window; pass a stream's running maximum to reproduce
    ``Handle.handoff_logmel`` over everything the stream returned."""
    raw = np.asarray(raw, dtype=np.float32)
    if raw.size == 0:
        return raw.copy()
    mx = np.float32(raw.max() if raw_max is None else raw_max)
    return (np.maximum(raw, mx - np.float32(8.0)) + np.float32(4.0)) * np.float32(0.25)


_NEMO_TABLES: dict = {}


def nemo_tables(n_mels: int):
    """The two float32 tables of the NeMo hand-off (csrc/nemo.hip): the analysis matrix [514, 512] -- rows f: cos, 257 + f: -sin of
    2 pi f n / 512, times the symmetric 400-point Hann window (a float32 value) at offset 56 -- and the slaney mel bank
    [n_mels, 257] over 0 .. 8 kHz, both from float64 formulas rounded once."""
    if n_mels not in _NEMO_TABLES:
        f, n = np.arange(257)[:, None], np.arange(512)[None, :]
        w = np.zeros(512)
        w[56:456] = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(400) / 399.0)).astype(np.float32)
        a = 2.0 * np.pi * ((f * n) % 512) / 512.0
        A = (np.concatenate([np.cos(a), -np.sin(a)]) * w[None, :]).astype(np.float32)
        f_sp, min_log_hz, logstep = 200.0 / 3.0, 1000.0, np.log(6.4) / 27.0
        min_log_mel = min_log_hz / f_sp
        mel2hz = lambda m: np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)
        mel_f = mel2hz(np.linspace(0.0, min_log_mel + np.log(8000.0 / min_log_hz) / logstep, n_mels + 2))
        fft_f = np.linspace(0.0, 8000.0, 257)
        W = np.zeros((n_mels, 257))
        for i in range(n_mels):
            lower = (fft_f - mel_f[i]) / (mel_f[i + 1] - mel_f[i])
            upper = (mel_f[i + 2] - fft_f) / (mel_f[i + 2] - mel_f[i + 1])
            W[i] = np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (mel_f[i + 2] - mel_f[i]))
        _NEMO_TABLES[n_mels] = (A, W.astype(np.float32))
    return _NEMO_TABLES[n_mels]


def nemo_features(x: np.ndarray, n_mels: int = 80, preemphasis: float = 0.97, normalize: bool = True) -> np.ndarray:
    """The numpy statement, in float32, of what ``Handle.run_enqueue_nemo`` hands to a NeMo host for one stream: ``x`` is the
    concatenation of the stream's kept ranges -> float32 [n_mels, len(x) // 160].  NeMo's AudioToMelSpectrogramPreprocessor
    (published as transformers' ParakeetFeatureExtractor): pre-emphasis ``y[c] = x[c] - p x[c - 1]``, 256 zeros on both sides,
    frames of 512 at hop 160 under a symmetric 400-point Hann window at offset 56, power spectrum, slaney mel bank at 257 bins,
    ``ln(mel + 2^-24)``, and with ``normalize`` per band ``(v - mean) / (std + 1e-5)`` with the unbiased std over the frames (0
    for a single frame).  The device sums in another order: its values agree within the bound of tests/nemo_reference.py, not
    bit for bit."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    L = len(x) // 160
    if L == 0:
        return np.zeros((n_mels, 0), np.float32)
    y = x.copy()
    if preemphasis:
        y[1:] = x[1:] - np.float32(preemphasis) * x[:-1]
    A, W = nemo_tables(n_mels)
    padded = np.concatenate([np.zeros(256, np.float32), y, np.zeros(256, np.float32)])
    frames = np.lib.stride_tricks.sliding_window_view(padded, 512)[::160][:L].T              # [512, L]
    spec = A @ frames
    power = spec[:257] * spec[:257] + spec[257:] * spec[257:]
    raw = np.log((W @ power).astype(np.float32) + np.float32(2.0 ** -24)).astype(np.float32)
    if not normalize:
        return raw
    mean = raw.astype(np.float64).mean(axis=1)
    std = np.sqrt(((raw - mean[:, None]) ** 2).sum(axis=1) / (L - 1)) if L > 1 else np.zeros(n_mels)
    return (raw - mean.astype(np.float32)[:, None]) / (std.astype(np.float32)[:, None] + np.float32(1e-5))


def nemo_chunk_stats(raw: np.ndarray):
    """Per band mean and unbiased std (0 for one frame) of raw NeMo frames [n_mels, n], as css_stream_nemo_chunks computes them:
    float64 sums in one fixed order -- lane l of 64 adds frames l, l + 64, ... in increasing order, then ``x[l] += x[l + s]`` for
    s = 32 .. 1 -- with ``d = raw - mean`` squared and added in two roundings, each result rounded to float32 once
    -> (mean, std) float32 [n_mels]."""
    raw = np.asarray(raw, dtype=np.float32)
    if raw.ndim != 2 or raw.shape[1] < 1:
        raise ValueError(f"expected [n_mels, n >= 1] frames, got {raw.shape}")
    n_mels, n = raw.shape
    rounds = -(-n // 64)
    valid = (np.arange(rounds * 64) < n).reshape(rounds, 64)

    def ordered_sum(x):   # x [n_mels, n] float64
        lanes = np.zeros((n_mels, rounds * 64))
        lanes[:, :n] = x
        lanes = lanes.reshape(n_mels, rounds, 64)
        acc = np.zeros((n_mels, 64))
        for r in range(rounds):
            acc = np.where(valid[r], acc + lanes[:, r], acc)
        s = 32
        while s:
            acc[:, :s] = acc[:, :s] + acc[:, s:2 * s]
            s //= 2
        return acc[:, 0]

    x = raw.astype(np.float64)
    mean = ordered_sum(x) / np.float64(n)
    d = x - mean[:, None]
    std = np.sqrt(ordered_sum(d * d) / np.float64(n - 1)) if n > 1 else np.zeros(n_mels)
    return mean.astype(np.float32), std.astype(np.float32)


def nemo_chunk_features(raw: np.ndarray, width: Optional[int] = None, normalize: Optional[str] = "per_feature", dtype="float32",
                        pad_value: float = 0.0) -> np.ndarray:
    """The numpy statement of css_stream_nemo_chunks: raw NeMo frames [n_mels, n] of one span -> [n_mels, width] (default n).
    Columns < n are the raw frames (``normalize=None``) or ``(raw - mean) / (std + 1e-5)`` in float32 with ``nemo_chunk_stats``
    of the span (``"per_feature"``); the columns behind them hold ``pad_value`` and are never normalised; float16 is ``astype`` of
    the float32 values.  Bit for bit what the device writes."""
    raw = np.asarray(raw, dtype=np.float32)
    dt = np.dtype(dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.float16)):
        raise ValueError(f"chunks are float32 or float16, got {dt}")
    if normalize not in _lib.NEMO_CHUNK_NORMALIZE:
        raise ValueError(f"normalize is None or 'per_feature', got {normalize!r}")
    width = raw.shape[1] if width is None and raw.ndim == 2 else width
    if raw.ndim != 2 or not 1 <= raw.shape[1] <= int(width) <= _lib.NEMO_CHUNK_MAX_WIDTH:
        raise ValueError(f"expected [n_mels, 1 .. width <= {_lib.NEMO_CHUNK_MAX_WIDTH}] frames, got {raw.shape} for width {width}")
    if not np.isfinite(pad_value):
        raise ValueError("pad_value is finite")
    out = np.full((raw.shape[0], int(width)), np.float32(pad_value), np.float32)
    if normalize is None:
        out[:, :raw.shape[1]] = raw
    else:
        mean, std = nemo_chunk_stats(raw)
        out[:, :raw.shape[1]] = (raw - mean[:, None]) / (std + np.float32(1e-5))[:, None]
    return out.astype(dt)


def whisper_window(raw: np.ndarray, width: int = 3000, dtype="float16") -> np.ndarray:
    """The numpy statement of css_stream_windows: raw log-mel frames [n_mels, n] of one span -> [n_mels, width].  Columns < n are
    ``whisper_normalize(raw)``, clamped at the span's own maximum M; the columns behind them hold what a frame of digital zeros
    (log10(1e-10) = -10) takes under the same clamp, (max(-10, M - 8) + 4) / 4 in float32; float16 is ``astype`` of that."""
    raw = np.asarray(raw, dtype=np.float32)
    dt = np.dtype(dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.float16)):
        raise ValueError(f"windows are float32 or float16, got {dt}")
    if raw.ndim != 2 or not 1 <= raw.shape[1] <= width:
        raise ValueError(f"expected [n_mels, 1 .. {width}] frames, got {raw.shape}")
    fill = (np.maximum(np.float32(-10.0), np.float32(raw.max()) - np.float32(8.0)) + np.float32(4.0)) * np.float32(0.25)
    out = np.full((raw.shape[0], int(width)), fill, np.float32)
    out[:, :raw.shape[1]] = whisper_normalize(raw)
    return out.astype(dt)


def session_window_fill(M) -> np.float32:
    """what a frame of digital zeros (log10(1e-10) = -10) takes under a clamp at the maximum M: (max(-10, M - 8) + 4) / 4 in float32"""
    return (np.maximum(np.float32(-10.0), np.float32(M) - np.float32(8.0)) + np.float32(4.0)) * np.float32(0.25)


def session_windows(mel: np.ndarray, M, width: int = 3000, stride: int = 3000, dtype="float16") -> np.ndarray:
    """The numpy statement of css_run_enqueue_windows for one speaker: ``mel`` [n_mels, J] is the session hand-off's normalised
    log-mel and ``M`` the maximum its clamp used -> [ceil(J / stride), n_mels, width].  Window w holds columns
    ``mel[:, w * stride : w * stride + width]``; the columns behind them hold ``session_window_fill(M)``; float16 is ``astype`` of
    the float32 values.  (One window over raw frames: ``session_windows(whisper_normalize(raw), raw.max(), width, width)[0]`` is
    ``whisper_window(raw, width)``.)"""
    mel = np.asarray(mel, dtype=np.float32)
    dt = np.dtype(dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.float16)):
        raise ValueError(f"windows are float32 or float16, got {dt}")
    if mel.ndim != 2 or not 1 <= width <= 3000 or not 1 <= stride <= width:
        raise ValueError(f"expected [n_mels, J] frames, width in 1 .. 3000 and stride in 1 .. width, got {mel.shape}, {width}, {stride}")
    J = mel.shape[1]
    n = -(-J // int(stride))
    out = np.full((n, mel.shape[0], int(width)), session_window_fill(M), np.float32)
    for w in range(n):
        part = mel[:, w * stride:w * stride + width]
        out[w, :, :part.shape[1]] = part
    return out.astype(dt)


def _torch():
    import torch
    return torch


def _window_out(h, n, n_mels, width, dtype, out):
    """the tensor [n, n_mels, width] a windows call writes (a new one, or the caller's: any view whose last stride is 1 and whose
    rows of one window are a constant pitch apart, windows that do not overlap) -> (tensor, ld)"""
    torch = _torch()
    if dtype not in _lib.WINDOW_DTYPES:
        raise ValueError(f"windows are float32 or float16, got {dtype!r}")
    dt = getattr(torch, dtype)
    if out is None:
        out = torch.empty((n, n_mels, width), dtype=dt, device=f"cuda:{h.device}")
    if (out.dtype != dt or tuple(out.shape) != (n, n_mels, width) or not out.is_cuda or (out.device.index or 0) != h.device or
            (width > 1 and out.stride(2) != 1) or (n_mels > 1 and out.stride(1) < width)):
        raise ValueError(f"out: a {dtype} tensor {(n, n_mels, width)} on cuda:{h.device} with unit stride along the columns")
    ld = out.stride(1) if n_mels > 1 else width
    if n > 1 and out.stride(0) < n_mels * ld:
        raise ValueError("out: the windows overlap (an expanded or overlapping view)")
    return out, ld


def pcm16_layout(chunk, num_channels: int):
    """int16 samples [n, C] (or [n] for one channel) -> (array, sample_stride, channel_stride) as css_stream_push_pcm16 takes
    them (strides in elements): a C-contiguous [n, C] array is interleaved (C, 1); the transposed view of a [C, n] array --
    ``planes.T``, or a slice of it, ``planes[:, a:b].T`` -- is planar (1, row pitch of ``planes``).  Both are passed on as
    they are; any other layout is copied to C-contiguous once.  Other dtypes raise TypeError: there is no silent conversion."""
    a = np.asarray(chunk)
    if a.dtype != np.int16:
        raise TypeError(f"push_pcm16 takes int16 samples, got {a.dtype} (push takes float sample values)")
    if a.ndim == 1:
        a = a[:, None]
    C_ = int(num_channels)
    if a.ndim != 2 or a.shape[1] != C_:
        raise ValueError(f"expected [n, {C_}] samples, got {a.shape}")
    n = a.shape[0]
    if a.flags.c_contiguous and a.flags.aligned:
        return a, C_, 1
    cs = a.strides[1] // 2   # (a planar view: consecutive samples of a channel, channels a row pitch apart)
    if n >= 1 and a.flags.aligned and (n == 1 or a.strides[0] == 2) and a.strides[1] == 2 * cs and cs >= n:
        return a, 1, cs
    return np.ascontiguousarray(a), C_, 1


class Handoff:
    """What one call made final for the ASR front end, per separated stream k: ``mel[k]`` raw log-mel frames [n_mels, n],
    ``ranges[k]`` the sample ranges [r, 2] (int64) appended to k's concatenation, ``activity[k]`` the gate bits of frames
    ``first_activity_frame`` .. and ``raw_max[k]`` the maximum of every raw value returned for k so far."""

    def __init__(self, mel, ranges, activity, raw_max, first_activity_frame, first_frame=None):
        self.mel, self.ranges, self.activity, self.raw_max = mel, ranges, activity, raw_max
        self.first_activity_frame = first_activity_frame
        # a preview's hand-off only (``preview_handoff``): ``mel[k]`` starts at frame ``first_frame[k]`` of k's concatenation
        self.first_frame = first_frame


class CssStream:
    """One stream on a ``HipSeparator``'s handle.  ``push(chunk)`` -> list of S float32 arrays (the newly final samples),
    ``finish()`` -> the rest; use as a context manager (closes the stream).  ``handoff``, ``output``: see the module text."""

    def __init__(self, separator: HipSeparator, cfg: Optional[CssCfg] = None, fs: int = 16000, num_channels: Optional[int] = None,
                 handoff: Optional[Mapping[str, object]] = None, input_rate: Optional[int] = None,
                 window_history: Optional[int] = None, output: Optional[Mapping[str, object]] = None,
                 nemo: Optional[Mapping[str, object]] = None, nemo_history: Optional[int] = None):
        if nemo is not None and (handoff is not None or window_history is not None):
            raise ValueError("nemo= is a hand-off format of its own: not together with handoff= or window_history=")
        if nemo_history is not None and nemo is None:
            raise ValueError("nemo_history needs a stream opened with nemo=")
        self.separator = separator
        self.cfg = cfg if cfg is not None else CssCfg()
        desc = separator.desc
        self.num_channels = int(desc.num_mics if num_channels is None else num_channels)   # (another count: CSS_ERR_SHAPE at css_stream_open)
        self.num_spks = int(desc.num_spks)
        self._run_cfg = make_run_cfg(self.cfg, fs, self.num_channels, desc.frame_len, desc.frame_hop)
        self._h = separator.handle
        sid = C.c_int32(-1)
        _lib.check(self._h.h, self._h.lib.css_stream_open(self._h.h, C.byref(self._run_cfg.c), self.num_channels, C.byref(sid)))
        self.id = int(sid.value)
        self.latency_samples = self.info().max_lag
        # the rate ratio (up, down) of a stream pushed at another rate than the model's, the inputs pushed so far and the
        # resampler's own lag in input samples (half / up: 30 samples at 48 kHz) on top of latency_samples (model rate)
        self.rate = None
        self._n_in = 0
        self.resampler_lag_samples = 0
        if input_rate is not None and int(input_rate) != int(fs):
            up, down = _lib.rate_ratio(input_rate, fs)
            try:
                _lib.check(self._h.h, self._h.lib.css_stream_set_rate(self._h.h, self.id, up, down))
            except Exception:
                self.close()
                raise
            self.rate = (up, down)
            self.resampler_lag_samples = 10 * max(up, down) // up
        # the output format (css_stream_set_output): what push / finish return then, and the counts bound with the buffer
        self._ocfg = None
        self.output_total = 0
        self.model_rate: Optional[List[np.ndarray]] = None
        if output is not None:
            opts = dict(output)
            self._o_model_rate = bool(opts.pop("model_rate", False))
            try:
                ocfg = _lib.stream_output_cfg(fs=fs, **opts)
                _lib.check(self._h.h, self._h.lib.css_stream_set_output(self._h.h, self.id, C.byref(ocfg)))
            except Exception:
                self.close()
                raise
            self._ocfg = ocfg
            self.output_rate = int(opts.get("rate", fs))
            self._odtype = np.dtype(np.int16 if ocfg.pcm16 else np.float32)
            self._oclip, self._opeak = np.zeros(self.num_spks, np.int64), np.zeros(self.num_spks, np.uint32)
            self._ocounts = _lib.CssStreamOutputCounts(0, 0, self._oclip.ctypes.data, self._opeak.ctypes.data)
            self._obuf = None
        self._out = np.empty((self.num_spks, 0), np.float32)
        self.handoff: Optional[Handoff] = None
        self.preview_handoff: Optional[Handoff] = None
        self._pv = None
        self.preview_first_sample = 0
        self._hcfg = None
        self.nemo: Optional[Handoff] = None
        self._ncfg = None
        if handoff is not None or nemo is not None:
            try:
                if nemo is not None:
                    self._ncfg = _lib.stream_nemo_cfg(**dict(nemo))
                    self._hcfg = _lib.handoff_cfg(self._ncfg.n_mels, self._ncfg.pad_frames, self._ncfg.drop_silence)
                    _lib.check(self._h.h, self._h.lib.css_stream_nemo_open(self._h.h, self.id, C.byref(self._ncfg)))
                else:
                    self._hcfg = _lib.handoff_cfg(**dict(handoff))
                    _lib.check(self._h.h, self._h.lib.css_stream_handoff_open(self._h.h, self.id, C.byref(self._hcfg)))
            except Exception:
                self.close()
                raise
            self._ho = _lib.CssStreamHandoffOut()
            self._ho_caps = (0, 0, 0)
            S = self.num_spks
            self._ho_n = (np.zeros(S, np.int64), np.zeros(S, np.int32), np.zeros(S, np.float32))
            self._nemo_frames = np.zeros(S, np.int64)   # (frames returned so far: Handoff.first_frame of the next call)
        self.window_history = None
        self.window_max = None
        self.present_span = None
        if window_history is not None:
            try:
                if handoff is None:
                    raise ValueError("window_history needs a stream opened with handoff=")
                _lib.check(self._h.h, self._h.lib.css_stream_window_open(self._h.h, self.id, int(window_history)))
            except Exception:
                self.close()
                raise
            self.window_history = int(window_history)
        self.nemo_history = None
        self.chunk_mean = None
        self.chunk_std = None
        if nemo_history is not None:
            try:
                _lib.check(self._h.h, self._h.lib.css_stream_nemo_history_open(self._h.h, self.id, int(nemo_history)))
            except Exception:
                self.close()
                raise
            self.nemo_history = int(nemo_history)

    def _model_samples(self, n_in: int, finished: bool = False) -> int:
        """model-rate samples after ``n_in`` samples as they are pushed (css_stream_rate_samples; without a rate: ``n_in``)"""
        return n_in if self.rate is None else _lib.stream_rate_samples(self.rate[0], self.rate[1], n_in, finished)

    def _model_new(self, n: int) -> int:
        """model-rate samples that the next push of ``n`` samples adds to the window"""
        return self._model_samples(self._n_in + n) - self._model_samples(self._n_in)

    def handoff_bounds(self, n_samples: int):
        """(frames, ranges, gate frames) the next push of ``n_samples`` (-1: finish) needs room for"""
        n = self._model_new(n_samples) if n_samples >= 0 else n_samples
        if self._ncfg is not None:
            return _lib.stream_nemo_bounds(self.separator.desc, self._run_cfg, self._ncfg, n)
        return _lib.stream_handoff_bounds(self.separator.desc, self._run_cfg, self._hcfg, n)

    def handoff_final_frames(self, n_pushed: int) -> int:
        return _lib.stream_handoff_final_frames(self.separator.desc, self._run_cfg, self._hcfg, self._model_samples(n_pushed))

    def nemo_bounds(self, n_samples: int):
        """(frames, ranges, gate frames) the next push of ``n_samples`` (-1: finish) of a stream opened with ``nemo=`` needs room for"""
        if self._ncfg is None:
            raise ValueError("nemo_bounds() needs a stream opened with nemo=")
        return self.handoff_bounds(n_samples)

    def nemo_final_frames(self, n_pushed: int) -> int:
        """NeMo frames that are final after ``n_pushed`` pushed samples (``drop_silence=False`` only)"""
        if self._ncfg is None:
            raise ValueError("nemo_final_frames() needs a stream opened with nemo=")
        return _lib.stream_nemo_final_frames(self.separator.desc, self._run_cfg, self._ncfg, self._model_samples(n_pushed))

    def _handoff_bind(self, n_samples: int):
        """binds buffers that suffice for a call with ``n_samples`` (kept while they are large enough)"""
        if self._hcfg is None:
            return
        need = self.handoff_bounds(n_samples)
        if any(n > c for n, c in zip(need, self._ho_caps)) or not self._ho.mel_host:
            S, nm = self.num_spks, int(self._hcfg.n_mels)
            caps = tuple(max(n, c) for n, c in zip(need, self._ho_caps))
            self._ho_mel = np.empty((S, nm, caps[0]), np.float32)
            self._ho_ranges = np.empty((S, caps[1], 2), np.int64)
            self._ho_act = np.empty((S, caps[2]), np.uint8)
            self._ho_caps = caps
            o = self._ho
            o.mel_host, o.cap_frames = self._ho_mel.ctypes.data, caps[0]
            o.ranges_host, o.cap_ranges = self._ho_ranges.ctypes.data, caps[1]
            o.activity_host, o.cap_activity = self._ho_act.ctypes.data, caps[2]
            o.n_frames, o.n_ranges, o.raw_max = (a.ctypes.data for a in self._ho_n)
        _lib.check(self._h.h, self._h.lib.css_stream_handoff_bind(self._h.h, self.id, C.byref(self._ho)))

    def _handoff_take(self):
        if self._hcfg is None:
            return
        nf, nr, mx = self._ho_n
        na = int(self._ho.n_activity)
        S = range(self.num_spks)
        got = Handoff([self._ho_mel[k, :, :nf[k]].copy() for k in S], [self._ho_ranges[k, :nr[k]].copy() for k in S],
                      [self._ho_act[k, :na].copy() for k in S], mx.copy(), int(self._ho.first_activity_frame))
        if self._ncfg is None:
            self.handoff = got
            return
        # (a NeMo stream: no running maximum; mel[k] starts at frame first_frame[k] of k's concatenation)
        got.raw_max, got.first_frame = None, self._nemo_frames.copy()
        self._nemo_frames += nf
        self.nemo = got

    def info(self) -> _lib.CssStreamInfo:
        inf = _lib.CssStreamInfo()
        _lib.check(self._h.h, self._h.lib.css_stream_info(self._h.h, self.id, C.byref(inf)))
        return inf

    def final_samples(self, n_pushed: int) -> int:
        """output samples per separated stream that are final after ``n_pushed`` pushed samples (input samples with ``input_rate``)"""
        return _lib.stream_final_samples(self.separator.desc, self._run_cfg, self._model_samples(n_pushed))

    def output_samples(self, n_final: int, finished: bool = False) -> int:
        """output-rate samples written once ``n_final`` model-rate samples are final -- ``final_samples(n_pushed)`` while the
        stream is open -- or, ``finished``, by a finished stream that returned ``n_final`` (css_stream_output_samples)"""
        if self._ocfg is None:
            raise ValueError("output_samples() needs a stream opened with output=")
        return _lib.stream_output_samples(self._ocfg, n_final, finished)

    @property
    def output_peaks(self) -> np.ndarray:
        """float32 [S]: max |w_k| over the final model-rate samples so far (css_stream_output_peaks; any stream)"""
        bits = np.zeros(self.num_spks, np.uint32)
        _lib.check(self._h.h, self._h.lib.css_stream_output_peaks(self._h.h, self.id, bits.ctypes.data_as(C.c_void_p)))
        return bits.view(np.float32)

    @property
    def output_clipped(self) -> np.ndarray:
        """int64 [S]: output samples so far that the PCM16 clamp changed"""
        if self._ocfg is None:
            raise ValueError("output_clipped needs a stream opened with output=")
        return self._oclip.copy()

    def _output_bind(self, n_pushed: int, n_final: Optional[int] = None, finished: bool = False):
        """binds a page-locked buffer that holds what a call writes after which ``n_pushed`` samples are pushed (``n_final`` final)"""
        if self._ocfg is None:
            return
        if n_final is None:
            n_final = self.final_samples(n_pushed)
        need = _lib.stream_output_samples(self._ocfg, n_final, finished) - self.output_total
        if self._obuf is None or self._obuf.shape[1] < need:
            self._obuf = _lib.pinned_empty((self.num_spks, max(need, 1)), self._odtype)
        _lib.check(self._h.h, self._h.lib.css_stream_output_bind(self._h.h, self.id, C.c_void_p(self._obuf.ctypes.data),
                                                                 self._obuf.shape[1], C.byref(self._ocounts)))

    def _model_out(self, cap: int):
        """(array or None, pointer, capacity) for the model-rate samples of a call: nothing with an output format, unless asked for"""
        if self._ocfg is not None and not self._o_model_rate:
            return None, None, 0
        out = self._buffer(cap)
        return out, out.ctypes.data_as(C.c_void_p), out.shape[1]

    def _returned(self, out, n_out: int) -> List[np.ndarray]:
        """what a call returns: the model-rate samples, or with an output format those it wrote at the playback rate"""
        got = None if out is None else [out[s, :n_out].copy() for s in range(self.num_spks)]
        if self._ocfg is None:
            return got
        self.model_rate = got
        self.output_total = int(self._ocounts.n_total)
        return [self._obuf[s, :int(self._ocounts.n_written)].copy() for s in range(self.num_spks)]

    def _cap(self, n: int) -> int:
        """an output capacity that suffices for the next push of ``n`` samples"""
        return self._model_new(n) + self.latency_samples

    def _buffer(self, cap: int) -> np.ndarray:
        if self._out.shape[1] < cap:
            self._out = np.empty((self.num_spks, max(cap, 1)), np.float32)
        return self._out

    def _samples(self, chunk) -> np.ndarray:
        x = np.asarray(chunk, dtype=np.float32)
        if x.ndim == 1:
            x = x[:, None]
        if x.ndim != 2 or x.shape[1] != self.num_channels:
            raise ValueError(f"expected [n, {self.num_channels}] samples, got {x.shape}")
        return np.ascontiguousarray(x)

    def push(self, chunk) -> List[np.ndarray]:
        x = self._samples(chunk)
        n = x.shape[0]
        out, ptr, cap = self._model_out(self._cap(n))
        n_out = C.c_int64(0)
        self._handoff_bind(n)
        self._output_bind(self._n_in + n)
        _lib.check(self._h.h, self._h.lib.css_stream_push(self._h.h, self.id, x.ctypes.data_as(C.c_void_p), n, ptr, cap, C.byref(n_out)))
        self._n_in += n
        self._handoff_take()
        return self._returned(out, n_out.value)

    def push_pcm16(self, chunk) -> List[np.ndarray]:
        """``push`` for int16 samples [n, C] (interleaved, or the planar view ``planes.T``: ``pcm16_layout``): what ``push`` of
        ``chunk.astype(float32) / 32768`` returns, bit for bit; the samples are scaled and de-interleaved on the device."""
        x, ss, cs = pcm16_layout(chunk, self.num_channels)
        n = x.shape[0]
        out, ptr, cap = self._model_out(self._cap(n))
        n_out = C.c_int64(0)
        self._handoff_bind(n)
        self._output_bind(self._n_in + n)
        _lib.check(self._h.h, self._h.lib.css_stream_push_pcm16(self._h.h, self.id, C.c_void_p(x.ctypes.data), n, ss, cs, ptr, cap,
                                                                C.byref(n_out)))
        self._n_in += n
        self._handoff_take()
        return self._returned(out, n_out.value)

    def finish(self) -> List[np.ndarray]:
        inf = self.info()
        n_total = inf.n_pushed if self.rate is None else self._model_samples(self._n_in, True)
        rest = _lib.plan(self.separator.desc, self._run_cfg, n_total).n_out - inf.n_emitted
        out, ptr, cap = self._model_out(max(rest, 1))
        n_out = C.c_int64(0)
        self._handoff_bind(-1)
        self._output_bind(0, inf.n_emitted + rest, True)
        _lib.check(self._h.h, self._h.lib.css_stream_finish(self._h.h, self.id, ptr, cap, C.byref(n_out)))
        self._handoff_take()
        return self._returned(out, n_out.value)

    def preview_samples(self, n_pushed: int):
        """(first, count): a preview after ``n_pushed`` pushed samples (input samples with ``input_rate``) returns samples
        [first, first + count) per separated stream; ``first`` is ``final_samples(n_pushed)``"""
        desc = self.separator.desc
        first = _lib.stream_final_samples(desc, self._run_cfg, self._model_samples(n_pushed))
        f, c, _ = _lib.stream_preview_samples(desc, self._run_cfg, self._model_samples(n_pushed, True))
        return first, f + c - first

    def _preview_handoff_out(self):
        """the outputs of a preview with hand-off (kept): (CssStreamHandoffOut, first_frame); sized for finish, which suffices"""
        if self._pv is None:
            S, nm = self.num_spks, int(self._hcfg.n_mels)
            caps = _lib.stream_handoff_bounds(self.separator.desc, self._run_cfg, self._hcfg, -1)
            arrays = (np.empty((S, nm, caps[0]), np.float32), np.empty((S, caps[1], 2), np.int64), np.empty((S, caps[2]), np.uint8),
                      np.zeros(S, np.int64), np.zeros(S, np.int32), np.zeros(S, np.float32), np.zeros(S, np.int64))
            o = _lib.CssStreamHandoffOut()
            o.mel_host, o.cap_frames = arrays[0].ctypes.data, caps[0]
            o.ranges_host, o.cap_ranges = arrays[1].ctypes.data, caps[1]
            o.activity_host, o.cap_activity = arrays[2].ctypes.data, caps[2]
            o.n_frames, o.n_ranges, o.raw_max = (a.ctypes.data for a in arrays[3:6])
            self._pv = (o, arrays)
        return self._pv[0], self._pv[1][6]

    def _preview_handoff_take(self):
        o, (mel, ranges, act, nf, nr, mx, first) = self._pv
        na = int(o.n_activity)
        S = range(self.num_spks)
        self.preview_handoff = Handoff([mel[k, :, :nf[k]].copy() for k in S], [ranges[k, :nr[k]].copy() for k in S],
                                       [act[k, :na].copy() for k in S], mx.copy(), int(o.first_activity_frame), first.copy())

    def preview(self, handoff: bool = False) -> List[np.ndarray]:
        """The unfinished tail (css_stream_preview): samples [n_emitted, n_out) of ``css_run`` on what was pushed so far --
        what ``finish`` would return now -- while the stream stays as it was.  The samples are provisional: later pushes
        return other values for them once they are final.  ``preview_first_sample`` holds the first one's index.  Raises
        what ``css_run`` of the prefix raises (with the default windows: the reference's assert until more than one segment
        was pushed).  ``handoff=True`` (css_stream_preview_handoff; a stream opened with ``handoff=``, else ValueError) also
        sets ``preview_handoff`` to the hand-off outputs ``finish`` would return now; ``handoff`` stays the last push's."""
        if handoff and (self._hcfg is None or self._ncfg is not None):
            raise ValueError("preview(handoff=True) needs a stream opened with handoff=")
        out = np.empty((self.num_spks, max(self.latency_samples, 1)), np.float32)
        n_out, first = C.c_int64(0), C.c_int64(0)
        if handoff:
            ho, first_frame = self._preview_handoff_out()
            _lib.check(self._h.h, self._h.lib.css_stream_preview_handoff(
                self._h.h, self.id, out.ctypes.data_as(C.c_void_p), out.shape[1], C.byref(n_out), C.byref(first), C.byref(ho),
                first_frame.ctypes.data_as(C.c_void_p)))
            self._preview_handoff_take()
        else:
            _lib.check(self._h.h, self._h.lib.css_stream_preview(self._h.h, self.id, out.ctypes.data_as(C.c_void_p), out.shape[1],
                                                                 C.byref(n_out), C.byref(first)))
        self.preview_first_sample = int(first.value)
        return [out[s, :n_out.value].copy() for s in range(self.num_spks)]

    def window_range(self):
        """(first, end): the frames [first[k], end[k]) of separated stream k's concatenation the history holds (css_stream_window_range)"""
        first, end = np.zeros(self.num_spks, np.int64), np.zeros(self.num_spks, np.int64)
        _lib.check(self._h.h, self._h.lib.css_stream_window_range(self._h.h, self.id, first.ctypes.data_as(C.POINTER(C.c_int64)),
                                                                  end.ctypes.data_as(C.POINTER(C.c_int64))))
        return first, end

    def _window_span(self, k: int, first_frame, n_frames, width: int):
        """the defaults of a window request: the last min(end - first, width) retained frames"""
        if first_frame is None or n_frames is None:
            first, end = self.window_range()
            if first_frame is None:
                n = min(int(end[k] - first[k]), width) if n_frames is None else int(n_frames)
                first_frame = int(end[k]) - n
            if n_frames is None:
                n_frames = min(int(end[k]) - int(first_frame), width)
        return int(first_frame), int(n_frames)

    def window(self, k: int, first_frame: Optional[int] = None, n_frames: Optional[int] = None, width: int = 3000,
               dtype: str = "float16", out=None):
        """One Whisper encoder input of separated stream k as a torch tensor [n_mels, width] on the handle's device
        (css_stream_windows): frames [first_frame, first_frame + n_frames) of the history -- by default the last
        min(end - first, width) retained ones -- normalised over the span, padded, in ``dtype``.  ``out``: a tensor (or a slice
        of one) to write into.  ``window_max`` holds the maximum the clamp used."""
        if self._hcfg is None or self.window_history is None:
            raise ValueError("window() needs a stream opened with handoff= and window_history=")
        got = CssStreamGroup([self]).windows([(self, k, first_frame, n_frames)], width, dtype, None if out is None else out[None])
        return got[0]

    def present_window(self, k: int, n_frames: Optional[int] = None, width: int = 3000, dtype: str = "float16", out=None):
        """One Whisper encoder input of separated stream k that ends at the present (css_stream_present_windows): at most
        ``n_frames`` (default ``width``) frames counted back from the last provisional frame of a preview made in the same call
        -- the history's final frames, then the provisional ones -- normalised over the span and padded, as a torch tensor
        [n_mels, width] on the handle's device (``out``, if given); None when there is no frame yet and no ``out`` was given.
        Sets ``present_span`` = (first_frame, n_used, n_provisional) and ``window_max``, and ``preview_handoff`` /
        ``preview_first_sample`` as ``preview(handoff=True)`` does; raises what that raises.  The stream stays as it was."""
        if self._hcfg is None or self.window_history is None:
            raise ValueError("present_window() needs a stream opened with handoff= and window_history=")
        got, spans, _ = CssStreamGroup([self]).present_windows([(self, k, n_frames)], width, dtype, None if out is None else out[None],
                                                               _raise_refused=True)
        return got[0] if out is not None or spans[0, 1] > 0 else None

    def nemo_history_range(self):
        """(first, end): the frames [first[k], end[k]) of separated stream k's concatenation the NeMo history holds
        (css_stream_nemo_history_range)"""
        first, end = np.zeros(self.num_spks, np.int64), np.zeros(self.num_spks, np.int64)
        _lib.check(self._h.h, self._h.lib.css_stream_nemo_history_range(self._h.h, self.id, first.ctypes.data_as(C.POINTER(C.c_int64)),
                                                                        end.ctypes.data_as(C.POINTER(C.c_int64))))
        return first, end

    def nemo_chunk(self, k: int, first_frame: Optional[int] = None, n_frames: Optional[int] = None, width: Optional[int] = None,
                   normalize: Optional[str] = "per_feature", dtype: str = "float32", pad_value: float = 0.0, out=None):
        """One chunk of separated stream k for a NeMo consumer as a torch tensor [n_mels, width] on the handle's device
        (css_stream_nemo_chunks): frames [first_frame, first_frame + n_frames) of the history -- by default the last
        min(end - first, width) retained ones; ``width`` defaults to ``n_frames``, or to everything retained (at most 3000) --
        raw (``normalize=None``) or normalised per band over the span, padded with ``pad_value``, in ``dtype``.  ``out``: a tensor
        (or a slice of one) to write into.  ``chunk_mean`` / ``chunk_std`` hold the statistics a normalised chunk used."""
        if self.nemo_history is None:
            raise ValueError("nemo_chunk() needs a stream opened with nemo= and nemo_history=")
        if width is None:
            if n_frames is not None:
                width = int(n_frames)
            elif out is not None:
                width = int(out.shape[-1])
            else:
                first, end = self.nemo_history_range()
                width = max(min(int(end[k] - first[k]), _lib.NEMO_CHUNK_MAX_WIDTH), 1)
        got = CssStreamGroup([self]).nemo_chunks([(self, k, first_frame, n_frames)], width, normalize, dtype, pad_value,
                                                 None if out is None else out[None])
        return got[0]

    def close(self):
        if self.id >= 0 and self._h.h:
            self._h.lib.css_stream_close(self._h.h, self.id)
        self.id = -1

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class CssStreamGroup:
    """Streams of ONE ``HipSeparator`` pushed together.  ``push(chunks)`` takes a mapping stream -> chunk, or a sequence with
    one chunk (or None) per stream of the group, and returns per stream of the group what ``CssStream.push`` returns (empty
    arrays for a stream that took no part).  ``stats`` holds the estimator batches and segments of the last push.
    ``windows(requests)`` writes Whisper encoder inputs of any of its streams in one call (``CssStream.window`` for many)."""

    def __init__(self, streams: Sequence[CssStream]):
        self.streams = list(streams)
        if not self.streams:
            raise ValueError("a group needs at least one stream")
        if any(s.separator is not self.streams[0].separator for s in self.streams):
            raise ValueError("the streams of a group live on one HipSeparator")
        if len(set(id(s) for s in self.streams)) != len(self.streams):
            raise ValueError("a stream appears twice in the group")
        self._h = self.streams[0]._h
        self.stats = _lib.CssStreamGroupStats()
        self.window_launches = 0

    def _per_stream(self, chunks) -> list:
        if isinstance(chunks, Mapping):
            if any(s not in self.streams for s in chunks):
                raise ValueError("a chunk for a stream that is not in this group")
            return [chunks.get(s) for s in self.streams]
        per = list(chunks)
        if len(per) != len(self.streams):
            raise ValueError(f"expected {len(self.streams)} chunks (None: the stream takes no part), got {len(per)}")
        return per

    def _call(self, fn, items, part, outs) -> List[List[np.ndarray]]:
        stats = _lib.CssStreamGroupStats()
        _lib.check(self._h.h, fn(self._h.h, items, len(part), C.byref(stats)))
        self.stats = stats
        for it, (s, _) in zip(items, part):
            s._n_in += int(it.n_samples)
            s._handoff_take()
        got = {id(s): s._returned(out, it.n_out) for it, (s, _), out in zip(items, part, outs)}
        return [got.get(id(s), [np.empty(0, np.float32 if s._ocfg is None else s._odtype) for _ in range(s.num_spks)]) for s in self.streams]

    def push(self, chunks: Union[Mapping[CssStream, object], Sequence[object]]) -> List[List[np.ndarray]]:
        part = [(s, s._samples(c)) for s, c in zip(self.streams, self._per_stream(chunks)) if c is not None]
        items = (_lib.CssStreamPush * max(len(part), 1))()
        outs = []
        for it, (s, x) in zip(items, part):
            out, _, cap = s._model_out(s._cap(x.shape[0]))
            outs.append(out)
            s._output_bind(s._n_in + x.shape[0])
            it.id, it.pcm_host, it.n_samples = s.id, x.ctypes.data, x.shape[0]
            it.out_host, it.cap, it.n_out = None if out is None else out.ctypes.data, cap, 0
            s._handoff_bind(x.shape[0])
        return self._call(self._h.lib.css_stream_push_many, items, part, outs)

    def push_pcm16(self, chunks: Union[Mapping[CssStream, object], Sequence[object]]) -> List[List[np.ndarray]]:
        """``push`` for int16 chunks (``CssStream.push_pcm16``): one css_stream_push_many_pcm16 for the group."""
        part = [(s, pcm16_layout(c, s.num_channels)) for s, c in zip(self.streams, self._per_stream(chunks)) if c is not None]
        items = (_lib.CssStreamPushPcm16 * max(len(part), 1))()
        outs = []
        for it, (s, (x, ss, cs)) in zip(items, part):
            out, _, cap = s._model_out(s._cap(x.shape[0]))
            outs.append(out)
            s._output_bind(s._n_in + x.shape[0])
            it.id, it.pcm16_host, it.n_samples, it.sample_stride, it.channel_stride = s.id, x.ctypes.data, x.shape[0], ss, cs
            it.out_host, it.cap, it.n_out = None if out is None else out.ctypes.data, cap, 0
            s._handoff_bind(x.shape[0])
        return self._call(self._h.lib.css_stream_push_many_pcm16, items, part, outs)

    def preview(self, streams: Optional[Sequence[CssStream]] = None, handoff: bool = False) -> List[Optional[List[np.ndarray]]]:
        """``CssStream.preview`` of ``streams`` (default: every stream of the group) in ONE css_stream_preview_many: the pending
        segments of all of them share one estimator batch (``stats``).  Per stream of the group: its S arrays, or None for a
        stream that took no part or whose prefix ``css_run`` refuses (a meeting that began less than a segment ago).
        ``handoff=True``: ONE css_stream_preview_handoff_many; every previewed stream opened with ``handoff=`` gets its
        ``preview_handoff``, the others (and a refused prefix) ``preview_handoff = None``."""
        part = self.streams if streams is None else list(streams)
        if any(s not in self.streams for s in part):
            raise ValueError("a stream that is not in this group")
        items = ((_lib.CssStreamPreviewHandoff if handoff else _lib.CssStreamPreview) * max(len(part), 1))()
        outs = []
        for it, s in zip(items, part):
            out = np.empty((s.num_spks, max(s.latency_samples, 1)), np.float32)
            outs.append(out)
            p = it.p if handoff else it
            p.id, p.out_host, p.cap = s.id, out.ctypes.data, out.shape[1]
            if handoff and s._hcfg is not None and s._ncfg is None:
                ho, first_frame = s._preview_handoff_out()
                it.ho, it.first_frame = C.pointer(ho), first_frame.ctypes.data
        stats = _lib.CssStreamGroupStats()
        fn = self._h.lib.css_stream_preview_handoff_many if handoff else self._h.lib.css_stream_preview_many
        _lib.check(self._h.h, fn(self._h.h, items, len(part), C.byref(stats)))
        self.stats = stats
        got = {}
        for it, s, out in zip(items, part, outs):
            p = it.p if handoff else it
            if handoff:
                s.preview_handoff = None
            if p.status == _lib.CSS_OK:
                s.preview_first_sample = int(p.first_sample)
                got[id(s)] = [out[k, :p.n_out].copy() for k in range(s.num_spks)]
                if handoff and s._hcfg is not None and s._ncfg is None:
                    s._preview_handoff_take()
        return [got.get(id(s)) for s in self.streams]

    def _window_requests(self, method, requests, fields, width, dtype, out):
        """what ``windows`` and ``present_windows`` (``method``) do first: the request tuples padded with None to ``fields``,
        checked, and the tensor the call writes -> (reqs, width, out, ld)"""
        reqs = [tuple(r) + (None,) * (fields - len(r)) for r in requests]
        if not reqs:
            raise ValueError("no window requests")
        for s, *_ in reqs:
            if s not in self.streams:
                raise ValueError("a stream that is not in this group")
            if s._hcfg is None or s.window_history is None:
                raise ValueError(f"{method}() needs streams opened with handoff= and window_history=")
        n_mels = int(reqs[0][0]._hcfg.n_mels)
        if any(int(s._hcfg.n_mels) != n_mels for s, *_ in reqs):
            raise ValueError(f"the streams of one {method}() call hand off the same n_mels")
        width = int(width)
        return (reqs, width) + _window_out(self._h, len(reqs), n_mels, width, dtype, out)

    def windows(self, requests, width: int = 3000, dtype: str = "float16", out=None):
        """Many encoder inputs in ONE css_stream_windows: ``requests`` are (stream, k) or (stream, k, first_frame, n_frames) with
        the defaults of ``CssStream.window`` -> a torch tensor [B, n_mels, width] on the handle's device (``out``, or a slice of a
        caller's tensor, if given).  All streams of the requests hand off the same n_mels.  ``window_launches`` holds the
        kernel launches of the call, and every named stream's ``window_max`` the maximum of its last request."""
        reqs, width, out, ld = self._window_requests("windows", requests, 4, width, dtype, out)
        items = (_lib.CssStreamWindow * len(reqs))()
        el = out.element_size()
        for i, (it, (s, k, first_frame, n_frames)) in enumerate(zip(items, reqs)):
            first_frame, n_frames = s._window_span(int(k), first_frame, n_frames, width)
            it.id, it.speaker, it.first_frame, it.n_frames, it.width = s.id, int(k), first_frame, n_frames, width
            it.dtype, it.out_dev, it.ld = _lib.WINDOW_DTYPES[dtype], out.data_ptr() + i * out.stride(0) * el, ld
        # (the library works on the handle's stream and returns after a synchronise of it: what torch has queued for `out` on its
        # own stream is finished first)
        _torch().cuda.current_stream(out.device).synchronize()
        launches = C.c_int32(0)
        _lib.check(self._h.h, self._h.lib.css_stream_windows(self._h.h, items, len(reqs), C.byref(launches)))
        self.window_launches = int(launches.value)
        for it, (s, *_) in zip(items, reqs):
            s.window_max = float(it.window_max)
        return out

    def nemo_chunks(self, requests, width: int, normalize: Optional[str] = "per_feature", dtype: str = "float32", pad_value: float = 0.0,
                    out=None):
        """Many chunks for a NeMo consumer in ONE css_stream_nemo_chunks: ``requests`` are (stream, k) or (stream, k, first_frame,
        n_frames) with the defaults of ``CssStream.nemo_chunk`` -> a torch tensor [W, n_mels, width] on the handle's device
        (``out``, or a slice of a caller's tensor, if given: ``windows``' rules).  All streams of the requests hand off the same
        n_mels.  ``window_launches`` holds the kernel launches of the call, and every named stream's ``chunk_mean`` /
        ``chunk_std`` (float32 [n_mels]; None for a raw chunk) the statistics of its last request."""
        reqs = [tuple(r) + (None,) * (4 - len(r)) for r in requests]
        if not reqs:
            raise ValueError("no chunk requests")
        for s, *_ in reqs:
            if s not in self.streams:
                raise ValueError("a stream that is not in this group")
            if s.nemo_history is None:
                raise ValueError("nemo_chunks() needs streams opened with nemo= and nemo_history=")
        if normalize not in _lib.NEMO_CHUNK_NORMALIZE:
            raise ValueError(f"normalize is None or 'per_feature', got {normalize!r}")
        n_mels = int(reqs[0][0]._hcfg.n_mels)
        if any(int(s._hcfg.n_mels) != n_mels for s, *_ in reqs):
            raise ValueError("the streams of one nemo_chunks() call hand off the same n_mels")
        width = int(width)
        out, ld = _window_out(self._h, len(reqs), n_mels, width, dtype, out)
        items = (_lib.CssStreamNemoChunk * len(reqs))()
        stats = np.zeros((len(reqs), 2, n_mels), np.float32)
        el = out.element_size()
        for i, (it, (s, k, first_frame, n_frames)) in enumerate(zip(items, reqs)):
            if first_frame is None or n_frames is None:
                first, end = s.nemo_history_range()
                if first_frame is None:
                    n = min(int(end[k] - first[k]), width) if n_frames is None else int(n_frames)
                    first_frame = int(end[k]) - n
                if n_frames is None:
                    n_frames = min(int(end[k]) - int(first_frame), width)
                if end[k] == 0:   # (a live caller's first ticks: said here, not as the library's refusal of a span of no frames)
                    raise ValueError(f"request {i}: no frames retained yet for separated stream {int(k)} (nemo_history_range())")
            it.id, it.speaker, it.first_frame, it.n_frames, it.width = s.id, int(k), int(first_frame), int(n_frames), width
            it.dtype, it.normalize, it.pad_value = _lib.WINDOW_DTYPES[dtype], _lib.NEMO_CHUNK_NORMALIZE[normalize], float(pad_value)
            it.out_dev, it.ld = out.data_ptr() + i * out.stride(0) * el, ld
            it.mean_host, it.std_host = stats[i, 0].ctypes.data, stats[i, 1].ctypes.data
        # (as in windows(): what torch has queued for `out` on its own stream is finished first)
        _torch().cuda.current_stream(out.device).synchronize()
        launches = C.c_int32(0)
        _lib.check(self._h.h, self._h.lib.css_stream_nemo_chunks(self._h.h, items, len(reqs), C.byref(launches)))
        self.window_launches = int(launches.value)
        for i, (s, *_) in enumerate(reqs):
            s.chunk_mean, s.chunk_std = (None, None) if normalize is None else (stats[i, 0].copy(), stats[i, 1].copy())
        return out

    def present_windows(self, requests, width: int = 3000, dtype: str = "float16", out=None, _raise_refused: bool = False):
        """Encoder inputs that end at the present, in ONE css_stream_present_windows: ``requests`` are (stream, k) or
        (stream, k, n_frames) (default ``width``); every stream that is named becomes one preview item of the call, so the
        pending segments share one estimator batch (``stats``) and all windows one synchronise (``window_launches``: their kernel
        launches).  -> (torch tensor [n, n_mels, width] on the handle's device -- ``out``, by ``windows``' rules, if given --,
        spans int64 [n, 3] of (first_frame, n_used, n_provisional), maxima float32 [n]).  A window without a frame (n_used 0), and
        every window of a stream whose prefix ``css_run`` refuses (spans row (-1, 0, 0), ``preview_handoff`` None), is left
        unwritten with a NaN maximum.  Every named stream gets ``preview_handoff`` / ``preview_first_sample`` as
        ``preview(handoff=True)`` sets them, and ``present_span`` / ``window_max`` of its last request."""
        reqs, width, out, ld = self._window_requests("present_windows", requests, 3, width, dtype, out)
        el = out.element_size()
        part = [s for s in self.streams if any(r[0] is s for r in reqs)]
        items = (_lib.CssStreamPresentItem * len(part))()
        outs, tables, where = [], [], {}
        for it, s in zip(items, part):
            mine = [i for i, r in enumerate(reqs) if r[0] is s]
            wav = np.empty((s.num_spks, max(s.latency_samples, 1)), np.float32)
            outs.append(wav)
            it.ph.p.id, it.ph.p.out_host, it.ph.p.cap = s.id, wav.ctypes.data, wav.shape[1]
            ho, first_frame = s._preview_handoff_out()
            it.ph.ho, it.ph.first_frame = C.pointer(ho), first_frame.ctypes.data
            tab = (_lib.CssStreamPresentWindow * len(mine))()
            tables.append(tab)
            for w, i in zip(tab, mine):
                _, k, n_frames = reqs[i]
                w.speaker, w.n_frames, w.width = int(k), width if n_frames is None else int(n_frames), width
                w.dtype, w.out_dev, w.ld = _lib.WINDOW_DTYPES[dtype], out.data_ptr() + i * out.stride(0) * el, ld
                w.first_frame, w.window_max = -1, float("nan")
                where[i] = w
            it.windows, it.n_windows = tab, len(mine)
        # (as in windows(): what torch has queued for `out` on its own stream is finished first)
        _torch().cuda.current_stream(out.device).synchronize()
        stats, launches = _lib.CssStreamGroupStats(), C.c_int32(0)
        _lib.check(self._h.h, self._h.lib.css_stream_present_windows(self._h.h, items, len(part), C.byref(stats), C.byref(launches)))
        self.stats = stats
        self.window_launches = int(launches.value)
        for it, s, wav in zip(items, part, outs):
            s.preview_handoff = None
            if it.ph.p.status == _lib.CSS_OK:
                s.preview_first_sample = int(it.ph.p.first_sample)
                s._preview_handoff_take()
            elif _raise_refused:
                _lib.check(self._h.h, it.ph.p.status)
        spans = np.array([[where[i].first_frame, where[i].n_used, where[i].n_provisional] for i in range(len(reqs))], np.int64)
        maxima = np.array([where[i].window_max for i in range(len(reqs))], np.float32)
        for i, (s, *_) in enumerate(reqs):
            s.present_span = tuple(int(v) for v in spans[i])
            if spans[i, 1] > 0:
                s.window_max = float(maxima[i])
        return out, spans, maxima
