"""Streaming separation: a meeting separated while it happens (css_stream_* of include/css_mi355.h).

Samples arrive in chunks of any size; every ``push`` returns the output samples of the S separated streams that have become
final -- equal, bit for bit, to what ``css_run`` (this package's ``separate_and_stitch``) gives on the whole recording,
whatever follows -- and ``finish`` returns the rest.  The lag between input and final output is bounded by the
segmentation (``latency_samples``: 3.6 s with the default 3 s / 1.5 s segments).  Exact float32 arithmetic and 512 / 256 frames only.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

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

    def push(self, chunk) -> List[np.ndarray]:
        x = np.asarray(chunk, dtype=np.float32)
        if x.ndim == 1:
            x = x[:, None]
        if x.ndim != 2 or x.shape[1] != self.num_channels:
            raise ValueError(f"expected [n, {self.num_channels}] samples, got {x.shape}")
        x = np.ascontiguousarray(x)
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
