"""Streaming separation: a meeting separated while it happens (css_stream_* of include/css_mi355.h).

Samples arrive in chunks of any size; every ``push`` returns the output samples of the S separated streams that have become
final -- equal, bit for bit, to what ``css_run`` (this package's ``separate_and_stitch``) gives on the whole recording,
whatever follows -- and ``finish`` returns the rest.  The lag between input and final output is bounded by the
segmentation (``latency_samples``: 3.6 s with the default 3 s / 1.5 s segments).  Exact float32 arithmetic and 512 / 256 frames only.

``CssStreamGroup`` pushes into many streams of one separator in one call (css_stream_push_many): the segments the streams
complete in that call share the mask estimator's batches, so N live meetings cost about one estimator pass per tick instead
of N.  Every stream's output is what its own ``push`` would have returned, bit for bit.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Mapping, Optional, Sequence, Union

import numpy as np

from . import _lib
from .css import CssCfg, make_run_cfg
from .separator import HipSeparator


class CssStream:
    """One stream on a ``HipSeparator``'s handle.  ``push(chunk)`` -> list of S float32 arrays (the newly final samples),
    ``finish()`` -> the rest; use as a context manager (closes the stream)."""

    def __init__(self, separator: HipSeparator, cfg: Optional[CssCfg] = None, fs: int = 16000, num_channels: int = 7):
        self.separator = separator
        self.cfg = cfg if cfg is not None else CssCfg()
        desc = separator.desc
        self.num_channels = int(num_channels)
        self.num_spks = int(desc.num_spks)
        self._run_cfg = make_run_cfg(self.cfg, fs, self.num_channels, desc.frame_len, desc.frame_hop)
        self._h = separator.handle
        sid = C.c_int32(-1)
        _lib.check(self._h.h, self._h.lib.css_stream_open(self._h.h, C.byref(self._run_cfg.c), self.num_channels, C.byref(sid)))
        self.id = int(sid.value)
        self.latency_samples = self.info().max_lag
        self._out = np.empty((self.num_spks, 0), np.float32)

    def info(self) -> _lib.CssStreamInfo:
        inf = _lib.CssStreamInfo()
        _lib.check(self._h.h, self._h.lib.css_stream_info(self._h.h, self.id, C.byref(inf)))
        return inf

    def final_samples(self, n_pushed: int) -> int:
        return _lib.stream_final_samples(self.separator.desc, self._run_cfg, n_pushed)

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
        cap = n + self.latency_samples
        out = self._buffer(cap)
        n_out = C.c_int64(0)
        _lib.check(self._h.h, self._h.lib.css_stream_push(self._h.h, self.id, x.ctypes.data_as(C.c_void_p), n,
                                                          out.ctypes.data_as(C.c_void_p), out.shape[1], C.byref(n_out)))
        return [out[s, :n_out.value].copy() for s in range(self.num_spks)]

    def finish(self) -> List[np.ndarray]:
        inf = self.info()
        rest = _lib.plan(self.separator.desc, self._run_cfg, inf.n_pushed).n_out - inf.n_emitted
        out = self._buffer(max(rest, 1))
        n_out = C.c_int64(0)
        _lib.check(self._h.h, self._h.lib.css_stream_finish(self._h.h, self.id, out.ctypes.data_as(C.c_void_p), out.shape[1],
                                                            C.byref(n_out)))
        return [out[s, :n_out.value].copy() for s in range(self.num_spks)]

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
    arrays for a stream that took no part).  ``stats`` holds the estimator batches and segments of the last push."""

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

    def push(self, chunks: Union[Mapping[CssStream, object], Sequence[object]]) -> List[List[np.ndarray]]:
        if isinstance(chunks, Mapping):
            if any(s not in self.streams for s in chunks):
                raise ValueError("a chunk for a stream that is not in this group")
            per = [chunks.get(s) for s in self.streams]
        else:
            per = list(chunks)
            if len(per) != len(self.streams):
                raise ValueError(f"expected {len(self.streams)} chunks (None: the stream takes no part), got {len(per)}")
        part = [(s, s._samples(c)) for s, c in zip(self.streams, per) if c is not None]
        items = (_lib.CssStreamPush * max(len(part), 1))()
        outs = []
        for it, (s, x) in zip(items, part):
            out = s._buffer(x.shape[0] + s.latency_samples)
            outs.append(out)
            it.id, it.pcm_host, it.n_samples = s.id, x.ctypes.data, x.shape[0]
            it.out_host, it.cap, it.n_out = out.ctypes.data, out.shape[1], 0
        stats = _lib.CssStreamGroupStats()
        _lib.check(self._h.h, self._h.lib.css_stream_push_many(self._h.h, items, len(part), C.byref(stats)))
        self.stats = stats
        got = {id(s): [out[k, :it.n_out].copy() for k in range(s.num_spks)] for it, (s, _), out in zip(items, part, outs)}
        return [got.get(id(s), [np.empty(0, np.float32) for _ in range(s.num_spks)]) for s in self.streams]
