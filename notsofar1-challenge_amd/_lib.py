"""ctypes binding of libcss_mi355.so (the C ABI declared in include/css_mi355.h).

The product path has NO CPU fallback: if the shared library is missing or cannot be loaded, every
compute entry point raises ``CssLibraryError`` (build it with ``python __graft_entry__.py`` or
``make -C notsofar1-challenge_amd/csrc``).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (CSS_MI355_LIBRARY: another build of the SAME library -- the AddressSanitizer build of tools/asan_tests.sh; nothing else)
LIB_PATH = os.environ.get("CSS_MI355_LIBRARY") or os.path.join(_HERE, "libcss_mi355.so")


class CssLibraryError(RuntimeError):
    pass


class CssError(RuntimeError):
    def __init__(self, code: int, text: str):
        super().__init__(f"css_mi355 error {code}: {text}")
        self.code = code
        self.text = text


# status codes (include/css_mi355.h: css_status)
CSS_OK, CSS_ERR_INVALID_ARG, CSS_ERR_HIP, CSS_ERR_ZERO_WEIGHT, CSS_ERR_MASK_FLOOR = 0, -1, -2, -3, -4
CSS_ERR_SHAPE, CSS_ERR_STATE, CSS_ERR_NO_DEVICE, CSS_ERR_WEIGHT_WINDOW, CSS_ERR_RANGE = -5, -6, -7, -8, -9
ANALYSIS_WINDOWS = {"hann": 0, "sqrt_hann": 1}   # CSS_WINDOW_* (css_set_analysis_window)
MAX_SEGMENT_FRAMES = 16384                       # CSS_MAX_SEGMENT_FRAMES

# buffer ids (css_buffer)
(BUF_X, BUF_FEATURES, BUF_MASKS, BUF_SCM, BUF_BFW, BUF_SEP, BUF_PIT_COST, BUF_PERMS, BUF_MASK_ST, BUF_ACTIVITY,
 BUF_ACT_B, BUF_ACT_FINAL, BUF_Y, BUF_WAV, BUF_HIDDEN, BUF_WTA_OVERRIDE, BUF_LEVEL) = range(17)
_BUF_DTYPES = {BUF_SCM: np.float64, BUF_BFW: np.float64, BUF_PIT_COST: np.float64, BUF_PERMS: np.int32,
               BUF_ACT_B: np.uint8, BUF_ACT_FINAL: np.uint8, BUF_WTA_OVERRIDE: np.uint8}


class CssModelDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "num_mics", "num_bins", "in_features", "attention_dim", "attention_heads", "linear_units", "num_blocks",
        "kernel_size", "num_spks", "num_nois", "frame_len", "frame_hop", "maxlen")]


class CssFeatureCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("log_spectrogram", "mvn_spectrogram", "ipd_mean_normalize",
                                         "ipd_mean_normalize_version", "ipd_cos", "num_pairs")] + \
               [("pair_l", C.c_int32 * 16), ("pair_r", C.c_int32 * 16)]


class CssRunCfg(C.Structure):
    _fields_ = [("segment_frames", C.c_int32), ("hop_frames", C.c_int32), ("dilation_frames", C.c_int32),
                ("erosion_frames", C.c_int32), ("mc_mvdr", C.c_int32), ("stitching_loss", C.c_int32),
                ("stitching_input", C.c_int32), ("normalize_segment_power", C.c_int32),
                ("mask_floor", C.c_float), ("activity_th", C.c_float),
                ("w_first", C.POINTER(C.c_float)), ("w_mid", C.POINTER(C.c_float)), ("w_last", C.POINTER(C.c_float))]


class CssPlan(C.Structure):
    _fields_ = [("n_samples", C.c_int64), ("stft_frames", C.c_int64), ("mix_frames", C.c_int64),
                ("num_segments", C.c_int64), ("n_out", C.c_int64), ("last_valid", C.c_int32),
                ("zero_weight", C.c_int32)]


class CssCfgSeconds(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("segment_size_sec", "hop_size_sec", "seg_weight_m0_sec", "seg_weight_m1_sec",
                                           "activity_dilation_sec", "activity_erosion_sec", "activity_th", "mask_floor_db")] + \
               [(n, C.c_int32) for n in ("mc_mvdr", "stitching_loss", "stitching_input", "normalize_segment_power")]


class CssStreamInfo(C.Structure):
    _fields_ = [("n_pushed", C.c_int64), ("n_emitted", C.c_int64), ("max_lag", C.c_int64), ("device_bytes", C.c_int64),
                ("finished", C.c_int32)]


MAX_STREAMS = 64                                 # CSS_MAX_STREAMS


class CssStreamPush(C.Structure):
    _fields_ = [("id", C.c_int32), ("pcm_host", C.c_void_p), ("n_samples", C.c_int64), ("out_host", C.c_void_p),
                ("cap", C.c_int64), ("n_out", C.c_int64)]


class CssStreamPushPcm16(C.Structure):
    _fields_ = [("id", C.c_int32), ("pcm16_host", C.c_void_p), ("n_samples", C.c_int64), ("sample_stride", C.c_int64),
                ("channel_stride", C.c_int64), ("out_host", C.c_void_p), ("cap", C.c_int64), ("n_out", C.c_int64)]


class CssStreamGroupStats(C.Structure):
    _fields_ = [("estimator_batches", C.c_int32), ("estimator_segments", C.c_int64)]


class CssStreamPreview(C.Structure):
    _fields_ = [("id", C.c_int32), ("out_host", C.c_void_p), ("cap", C.c_int64), ("n_out", C.c_int64), ("first_sample", C.c_int64),
                ("status", C.c_int32)]


class CssStreamHandoffCfg(C.Structure):
    _fields_ = [("n_mels", C.c_int32), ("pad_frames", C.c_int32), ("drop_silence", C.c_int32)]


class CssStreamHandoffOut(C.Structure):
    _fields_ = [("mel_host", C.c_void_p), ("cap_frames", C.c_int64), ("ranges_host", C.c_void_p), ("cap_ranges", C.c_int32),
                ("activity_host", C.c_void_p), ("cap_activity", C.c_int64), ("n_frames", C.c_void_p), ("n_ranges", C.c_void_p),
                ("raw_max", C.c_void_p), ("n_activity", C.c_int64), ("first_activity_frame", C.c_int64)]


class CssSessionHandoffOut(C.Structure):
    """include/css_mi355_session_handoff.h: the caller's arrays of a session's hand-off (all S streams)"""
    _fields_ = [("mel_host", C.c_void_p), ("cap_frames", C.c_int64), ("ranges_host", C.c_void_p), ("cap_ranges", C.c_int32),
                ("n_frames", C.c_void_p), ("n_ranges", C.c_void_p)]


class CssSessionWindows(C.Structure):
    """include/css_mi355_session_window.h: the encoder windows of a session, in the caller's device memory"""
    _fields_ = [("width", C.c_int32), ("stride", C.c_int32), ("dtype", C.c_int32), ("reserved", C.c_int32),
                ("windows_dev", C.c_void_p), ("ld", C.c_int64), ("cap_windows", C.c_int64), ("mel_dev", C.c_void_p),
                ("mel_ld", C.c_int64), ("n_windows", C.c_void_p), ("window_max", C.c_void_p)]


class CssStreamPreviewHandoff(C.Structure):
    _fields_ = [("p", CssStreamPreview), ("ho", C.POINTER(CssStreamHandoffOut)), ("first_frame", C.c_void_p)]


class CssStreamOutputCfg(C.Structure):
    """include/css_mi355_stream_out.h: the output format of a stream"""
    _fields_ = [("up", C.c_int32), ("down", C.c_int32), ("pcm16", C.c_int32), ("gain", C.c_float)]


class CssStreamOutputCounts(C.Structure):
    _fields_ = [("n_written", C.c_int64), ("n_total", C.c_int64), ("n_clipped", C.c_void_p), ("peak_bits", C.c_void_p)]


class CssSessionRate(C.Structure):              # include/css_mi355_session_rate.h
    _fields_ = [("in_up", C.c_int32), ("in_down", C.c_int32), ("out_up", C.c_int32), ("out_down", C.c_int32)]


STREAM_OUTPUT_TABLE = 16                         # CSS_STREAM_OUTPUT_TABLE: streams per launch of the output kernel
STREAM_OUTPUT_TILE = 1024                        # output samples per block of the output kernel (kernels.hpp SO_TILE)
WINDOW_DTYPES = {"float32": 0, "float16": 1}     # CSS_WINDOW_F32, CSS_WINDOW_F16 (include/css_mi355_window.h)
WINDOW_MAX_WIDTH = 3000                          # CSS_WINDOW_MAX_WIDTH
WINDOW_TABLE = 32                                # CSS_WINDOW_TABLE: windows per launch of css_stream_windows


class CssStreamWindow(C.Structure):
    _fields_ = [("id", C.c_int32), ("speaker", C.c_int32), ("first_frame", C.c_int64), ("n_frames", C.c_int32), ("width", C.c_int32),
                ("dtype", C.c_int32), ("out_dev", C.c_void_p), ("ld", C.c_int64), ("window_max", C.c_float)]


class CssStreamPresentWindow(C.Structure):      # include/css_mi355_present_window.h
    _fields_ = [("speaker", C.c_int32), ("n_frames", C.c_int32), ("width", C.c_int32), ("dtype", C.c_int32), ("out_dev", C.c_void_p),
                ("ld", C.c_int64), ("first_frame", C.c_int64), ("n_used", C.c_int32), ("n_provisional", C.c_int32),
                ("window_max", C.c_float)]


class CssStreamPresentItem(C.Structure):
    _fields_ = [("ph", CssStreamPreviewHandoff), ("windows", C.POINTER(CssStreamPresentWindow)), ("n_windows", C.c_int32)]


class CssGemmDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("kernel", "layout", "tile_rows", "batch", "M", "N", "K", "act")] + \
               [(n, C.c_int64) for n in ("lda", "ldb", "ldc", "ldr", "strideA", "strideB", "strideC", "a_off", "c_off", "r_off",
                                         "a_floats", "b_floats", "c_floats", "r_floats")] + \
               [("bias", C.c_int32), ("residual", C.c_int32), ("alpha", C.c_float)] + \
               [(n, C.c_int32) for n in ("b_frag32", "split_out", "c_transposed", "m_fastest", "nt_store", "concurrent")]


class CssLayerNormDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("form", "rows", "D", "inplace")] + [(n, C.c_int64) for n in ("x_floats", "out_floats")]


class CssConvModuleDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("form", "nseg", "T", "D", "taps", "reserved")] + \
               [(n, C.c_int64) for n in ("x_floats", "out_floats")]


class CssAttentionDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("mode", "nseg", "T", "D", "H", "maxlen", "K", "split_out")] + \
               [("canary", C.c_uint32), ("reserved", C.c_int32)] + \
               [(n, C.c_int64) for n in ("x_floats", "w_floats", "pe_floats", "qkv_floats", "ctx_floats")]


class CssAnalysisDesc(C.Structure):             # include/css_mi355_frontend.h
    _fields_ = [(n, C.c_int32) for n in ("C", "t_lo", "t_hi", "offset", "window", "want_phase")] + \
               [(n, C.c_int64) for n in ("x_stride", "row_ld", "x_floats", "out_floats", "phase_floats")]


class CssFeaturesDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("C", "F", "nseg", "T", "hop", "Kp", "split_out", "reserved")] + \
               [(n, C.c_int64) for n in ("T_ld", "stft_frames", "seg_lo", "x_floats", "ph_floats", "feat_floats")] + \
               [("cfg", CssFeatureCfg)]


class CssSynthesisTailDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("form", "B", "hop", "L", "world", "S", "F2", "KIp", "has_level")] + \
               [("level", C.c_uint32)] + \
               [(n, C.c_int64) for n in ("T_frames", "q_lo", "q_hi", "f_lo", "f_hi", "out_ld", "out_q0", "ld", "n_out", "in_floats",
                                         "out_floats")] + \
               [("t_lo", C.c_int64 * 64), ("t_hi", C.c_int64 * 64)]


class CssPcmEdgesDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("form", "C", "split_out", "S", "src_offset")] + [("peak_before", C.c_uint32)] + \
               [(n, C.c_int64) for n in ("n", "n_pad", "i_lo", "i_hi", "count", "out_ld", "in_elems", "out_elems")]


class CssRateIngestJob(C.Structure):            # include/css_mi355_rate_kernels.h
    _fields_ = [(n, C.c_int32) for n in ("up", "down", "C", "is_int16", "src_offset", "H", "dst_col", "has_hist_out")] + \
               [("level_before", C.c_uint32), ("level_after", C.c_uint32)] + \
               [(n, C.c_int64) for n in ("plane_ld", "n", "N0", "m0", "n_m", "dst_ld", "n_peak", "src_elems", "hist_elems", "dst_floats")] + \
               [(n, C.c_void_p) for n in ("src", "hist_in", "hist_out", "dst")]


class CssRateOutputJob(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("up", "down", "H", "pcm16", "has_hist_out", "reserved")] + \
               [("gain", C.c_float), ("reserved_f", C.c_float)] + \
               [(n, C.c_int64) for n in ("src_ld", "n", "N0", "m0", "n_m", "dst_ld", "src_floats", "hist_elems", "dst_elems")] + \
               [(n, C.c_void_p) for n in ("src", "hist_in", "hist_out", "dst", "peak", "clipped")]


class CssKArray(C.Structure):                   # include/css_mi355_stream_kernels.h
    _fields_ = [("p", C.c_void_p), ("elems", C.c_int64)]


class CssStreamTailJob(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("S", "F", "T", "hop", "KIp", "dilation", "erosion", "has_ring")] + \
               [("activity_th", C.c_float), ("reserved_f", C.c_float)] + \
               [(n, C.c_int64) for n in ("num_slots", "seg_base", "frame_base", "num_segments_global", "T_long_global", "mask_ld",
                                         "ld_frames", "gate_ld", "t_lo", "t_hi")] + \
               [(n, CssKArray) for n in ("masks", "sep", "perms", "w_first", "w_mid", "w_last", "act_b", "Y", "ring")]


class CssStreamScatterJob(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("dst_off", "dst_ld", "src_col", "n_cols")] + [("dst", CssKArray)]


class CssStreamIngestJob(C.Structure):
    _fields_ = [("C", C.c_int32), ("dst_col", C.c_int32)] + [(n, C.c_int64) for n in ("plane_ld", "n", "dst_ld")] + \
               [("src", CssKArray), ("dst", CssKArray)]


class CssStreamAppendJob(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("pad", "drop", "closing", "S", "preview", "reserved")] + \
               [(n, C.c_int64) for n in ("gate_ld", "out_ld", "out_base", "carry_ld", "t_g0", "t_g1", "D0", "D1", "row0", "rows")] + \
               [(n, CssKArray) for n in ("gate", "out", "carry_in", "carry_out", "tail_in", "tail_out", "st", "st_out", "act_out", "n_new")]


class CssStreamMelJob(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_mels", "has_ring", "has_pvmax", "reserved")] + \
               [(n, C.c_int64) for n in ("row0", "rows", "hist", "mel_ld")] + \
               [(n, CssKArray) for n in ("n_new", "st", "mel", "ring", "fmax", "pvmax")]


class CssStreamNemoCfg(C.Structure):            # include/css_mi355_stream_nemo.h
    _fields_ = [("n_mels", C.c_int32), ("pad_frames", C.c_int32), ("drop_silence", C.c_int32), ("preemphasis", C.c_float)]


class CssStreamNemoArray(C.Structure):
    _fields_ = [("p", C.c_void_p), ("elems", C.c_int64)]


class CssStreamNemoAppendJob(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("pad", "drop", "closing", "S")] + [("preemphasis", C.c_float), ("reserved", C.c_int32)] + \
               [(n, C.c_int64) for n in ("gate_ld", "out_ld", "out_base", "carry_ld", "t_g0", "t_g1", "D0", "D1", "row0", "rows")] + \
               [(n, CssStreamNemoArray) for n in ("gate", "out", "carry_in", "carry_out", "tail_in", "tail_out", "st", "act_out", "n_new",
                                                  "xlast_in", "xlast_out")]


class CssStreamNemoMelJob(C.Structure):
    _fields_ = [("n_mels", C.c_int32), ("reserved", C.c_int32)] + [(n, C.c_int64) for n in ("row0", "rows", "mel_ld")] + \
               [("n_new", CssStreamNemoArray), ("mel", CssStreamNemoArray)]


# a state row of the streamed hand-off (csrc/kernels.hpp HandoffState)
HANDOFF_STATE = np.dtype([("A", "<i8"), ("J", "<i8"), ("gmax", "<i4"), ("pad", "<i4")])
# per descriptor: the arrays a launch only reads, and the arrays it may write (copied first, returned as the launch left them)
STREAM_KERNEL_ARRAYS = {
    "CssStreamTailJob": ((("masks", np.float32), ("sep", np.float32), ("perms", np.int32), ("w_first", np.float32), ("w_mid", np.float32),
                          ("w_last", np.float32)), (("act_b", np.uint8), ("Y", np.float32), ("ring", np.uint8))),
    "CssStreamScatterJob": ((), (("dst", np.float32),)),
    "CssStreamIngestJob": ((("src", np.int16),), (("dst", np.float32),)),
    "CssStreamAppendJob": ((("gate", np.uint8), ("out", np.float32), ("carry_in", np.float32), ("tail_in", np.float32)),
                           (("carry_out", np.float32), ("tail_out", np.float32), ("st", HANDOFF_STATE), ("st_out", HANDOFF_STATE),
                            ("act_out", np.uint8), ("n_new", np.int32))),
    "CssStreamMelJob": ((("n_new", np.int32),), (("st", HANDOFF_STATE), ("mel", np.float32), ("ring", np.float32), ("fmax", np.float32),
                                                  ("pvmax", np.float32))),
}
# the same for the two kernel entries of include/css_mi355_stream_nemo.h
STREAM_NEMO_ARRAYS = {
    "CssStreamNemoAppendJob": ((("gate", np.uint8), ("out", np.float32), ("carry_in", np.float32), ("tail_in", np.float32),
                                ("xlast_in", np.float32)),
                               (("carry_out", np.float32), ("tail_out", np.float32), ("st", HANDOFF_STATE), ("act_out", np.uint8),
                                ("n_new", np.int32), ("xlast_out", np.float32))),
    "CssStreamNemoMelJob": ((("n_new", np.int32),), (("mel", np.float32),)),
}


# include/css_mi355_nemo_chunk.h: chunks out of a NeMo stream's frame history
NEMO_CHUNK_NORMALIZE = {None: 0, "per_feature": 1}   # CSS_NEMO_CHUNK_RAW, CSS_NEMO_CHUNK_PER_FEATURE
NEMO_CHUNK_MAX_WIDTH = 3000                      # CSS_NEMO_CHUNK_MAX_WIDTH
NEMO_CHUNK_TABLE = 32                            # CSS_NEMO_CHUNK_TABLE: chunks per launch of css_stream_nemo_chunks


class CssStreamNemoChunk(C.Structure):
    _fields_ = [("id", C.c_int32), ("speaker", C.c_int32), ("first_frame", C.c_int64), ("n_frames", C.c_int32), ("width", C.c_int32),
                ("dtype", C.c_int32), ("normalize", C.c_int32), ("pad_value", C.c_float), ("reserved", C.c_int32),
                ("out_dev", C.c_void_p), ("ld", C.c_int64), ("mean_host", C.c_void_p), ("std_host", C.c_void_p)]


class CssNemoChunkArray(C.Structure):
    _fields_ = [("p", C.c_void_p), ("elems", C.c_int64)]


class CssNemoChunkJob(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_mels", "n_frames", "width", "dtype", "normalize")] + [("pad_value", C.c_float)] + \
               [(n, C.c_int64) for n in ("hist", "end_frame", "first_frame", "ld", "out_offset")] + \
               [(n, CssNemoChunkArray) for n in ("ring", "out", "mean", "std")]


class CssStreamNemoMelHistoryJob(C.Structure):
    _fields_ = [("n_mels", C.c_int32), ("reserved", C.c_int32)] + [(n, C.c_int64) for n in ("row0", "rows", "mel_ld", "hist")] + \
               [(n, CssNemoChunkArray) for n in ("n_new", "mel", "ring", "frames_after")]


# the arrays of the two kernel entries, as STREAM_NEMO_ARRAYS (out: float32, or float16 words where the job's dtype is 1)
NEMO_CHUNK_ARRAYS = {
    "CssNemoChunkJob": ((("ring", np.float32),), (("out", None), ("mean", np.float32), ("std", np.float32))),
    "CssStreamNemoMelHistoryJob": ((("n_new", np.int32), ("frames_after", np.int64)), (("mel", np.float32), ("ring", np.float32))),
}


class CssSessionScanJob(C.Structure):           # include/css_mi355_handoff_kernels.h
    _fields_ = [(n, C.c_int32) for n in ("S", "pad", "drop", "cap_ranges", "gate_off", "reserved")] + [("TL", C.c_int64)] + \
               [(n, CssKArray) for n in ("gate", "psum", "regs", "offs", "st", "n_new", "n_ranges", "ranges_out", "n_frames_out",
                                         "n_ranges_out")]


class CssSessionGatherJob(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("S", "cap_ranges", "wav_off", "reserved")] + [(n, C.c_int64) for n in ("wav_ld", "rows")] + \
               [(n, CssKArray) for n in ("regs", "offs", "st", "n_ranges", "wav", "operand")]


class CssSessionNormJob(C.Structure):
    _fields_ = [("S", C.c_int32), ("n_mels", C.c_int32)] + [(n, C.c_int64) for n in ("mel_ld", "out_ld", "rows")] + \
               [(n, CssKArray) for n in ("st", "mel", "out")]


class CssSessionWindowsJob(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("S", "n_mels", "width", "stride", "f16", "has_win", "has_whole", "win_off", "whole_off",
                                         "mel_off")] + \
               [(n, C.c_int64) for n in ("mel_ld", "max_frames", "ld", "cap_windows", "whole_ld", "n_win_jobs", "n_whole_jobs")] + \
               [(n, CssKArray) for n in ("st", "mel", "win", "whole", "n_windows_out", "window_max_out")]


class CssStreamWindowJob(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_frames", "width", "n_mels", "f16", "has_pv", "ring_off", "pv_off", "out_off")] + \
               [(n, C.c_int64) for n in ("hist", "ld", "J", "pv_ld")] + \
               [(n, CssKArray) for n in ("ring", "fmax", "pv", "pvmax", "n_new", "out")]


# a result row of the window kernel (csrc/kernels.hpp WindowOut)
WINDOW_OUT = np.dtype([("first_frame", "<i8"), ("n_used", "<i4"), ("n_provisional", "<i4"), ("window_max", "<f4"), ("pad", "<i4")])
# per descriptor, as STREAM_KERNEL_ARRAYS: the arrays a launch only reads, and those it may write.  None: float32, or float16 (as
# uint16 words) where the descriptor's f16 is set
HANDOFF_KERNEL_ARRAYS = {
    "CssSessionScanJob": ((("gate", np.uint8),), (("psum", np.int32), ("regs", np.int64), ("offs", np.int64), ("st", HANDOFF_STATE),
                                                  ("n_new", np.int32), ("n_ranges", np.int32), ("ranges_out", np.int64),
                                                  ("n_frames_out", np.int64), ("n_ranges_out", np.int32))),
    "CssSessionGatherJob": ((("regs", np.int64), ("offs", np.int64), ("st", HANDOFF_STATE), ("n_ranges", np.int32), ("wav", np.float32)),
                            (("operand", np.float32),)),
    "CssSessionNormJob": ((("st", HANDOFF_STATE), ("mel", np.float32)), (("out", np.float32),)),
    "CssSessionWindowsJob": ((("st", HANDOFF_STATE), ("mel", np.float32)),
                             (("win", None), ("whole", None), ("n_windows_out", np.int32), ("window_max_out", np.float32))),
    "CssStreamWindowJob": ((("ring", np.float32), ("fmax", np.float32), ("pv", np.float32), ("pvmax", np.float32), ("n_new", np.int32)),
                           (("out", None),)),
}


class CssNemoCfg(C.Structure):                  # include/css_mi355_nemo_handoff.h
    _fields_ = [("n_mels", C.c_int32), ("pad_frames", C.c_int32), ("drop_silence", C.c_int32), ("preemphasis", C.c_float),
                ("normalize", C.c_int32)]


class CssNemoOut(C.Structure):
    _fields_ = [("mel_host", C.c_void_p), ("cap_frames", C.c_int64), ("ranges_host", C.c_void_p), ("cap_ranges", C.c_int32),
                ("n_frames", C.c_void_p), ("n_ranges", C.c_void_p), ("mean_host", C.c_void_p), ("std_host", C.c_void_p)]


class CssNemoArray(C.Structure):
    _fields_ = [("p", C.c_void_p), ("elems", C.c_int64)]


class CssNemoKernelsJob(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("S", "n_mels", "normalize", "cap_ranges", "wav_off")] + [("preemphasis", C.c_float)] + \
               [(n, C.c_int64) for n in ("wav_ld", "rows", "raw_ld", "out_ld")] + \
               [(n, CssNemoArray) for n in ("wav", "regs", "offs", "st", "n_ranges", "operand", "raw", "mean", "stdv", "out")]


# the arrays of CssNemoKernelsJob: those the launches only read, and those they write (returned as the launches left them)
NEMO_KERNEL_ARRAYS = ((("wav", np.float32), ("regs", np.int64), ("offs", np.int64), ("st", HANDOFF_STATE), ("n_ranges", np.int32)),
                      (("operand", np.float32), ("raw", np.float32), ("mean", np.float32), ("stdv", np.float32), ("out", np.float32)))


class CssMvdrSet(C.Structure):                  # include/css_mi355_backend.h
    _fields_ = [(n, C.c_int64) for n in ("seg_lo", "nseg", "scm_off", "bfw_off")]


class CssMvdrDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("form", "C", "F", "S", "T", "hop", "nseg", "use_mvdr", "n_sets", "reserved")] + \
               [(n, C.c_float) for n in ("mask_floor", "reserved_f")] + \
               [(n, C.c_int64) for n in ("seg_lo", "stft_frames", "T_ld", "mask_ld", "x_floats", "mask_floats", "override_bytes",
                                         "scm_doubles", "bfw_doubles", "sep_floats")] + \
               [("sets", CssMvdrSet * 16)]


class CssMvdrArraySet(C.Structure):             # include/css_mi355_array.h (the members of CssMvdrSet / CssMvdrDesc)
    _fields_ = list(CssMvdrSet._fields_)


class CssMvdrArrayDesc(C.Structure):
    _fields_ = list(CssMvdrDesc._fields_[:-1]) + [("sets", CssMvdrArraySet * 16)]


class CssStitchSet(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("num_segments", "mask_off", "sep_off", "costs_off")]


class CssStitchDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("form", "S", "F", "T", "hop", "loss", "input", "KIp", "y_split", "has_level", "dilation",
                                         "erosion", "n_sets")] + \
               [("level", C.c_uint32)] + \
               [(n, C.c_float) for n in ("activity_th", "reserved_f")] + \
               [(n, C.c_int64) for n in ("num_segments", "T_long", "mask_ld", "lo", "hi", "mask_floats", "sep_floats", "costs_doubles",
                                         "perms_ints", "mask_st_floats", "activity_floats", "act_bytes", "y_floats")] + \
               [("sets", CssStitchSet * 16)]


class CssKernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("ms", C.c_float), ("launches", C.c_int32)]


class CssTimings(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("upload", "stft", "features", "masknet", "mvdr", "stitch", "istft",
                                          "download", "total", "gemm_ms")] + \
               [("gemm_launches", C.c_int64), ("gemm_flops", C.c_double), ("host_enqueue", C.c_float), ("host_total", C.c_float)]


# name -> (restype, argtypes); exactly the symbols include/css_mi355.h declares
_P = C.c_void_p
_FP = C.POINTER(C.c_float)
SIGNATURES = {
    "css_version": (C.c_char_p, []),
    "css_last_error": (C.c_char_p, [_P]),
    "css_device_count": (C.c_int, []),
    "css_blob_num_floats": (C.c_int64, [C.POINTER(CssModelDesc)]),
    "css_create": (C.c_int, [C.POINTER(CssModelDesc), _P, C.c_int64, C.c_int, _P, C.c_int32, C.POINTER(_P)]),
    "css_destroy": (C.c_int, [_P]),
    "css_get_stream": (C.c_int, [_P, C.POINTER(_P)]),
    "css_set_lanes": (C.c_int, [_P, C.c_int]),
    "css_get_lanes": (C.c_int, [_P]),
    "css_set_tuning": (C.c_int, [_P, C.c_int, C.c_int]),
    "css_set_queue_group": (C.c_int, [_P, C.c_int]),
    "css_host_alloc": (C.c_int, [C.c_size_t, C.POINTER(_P)]),
    "css_host_free": (C.c_int, [_P]),
    "css_plan": (C.c_int, [C.POINTER(CssModelDesc), C.POINTER(CssRunCfg), C.c_int64, C.POINTER(CssPlan)]),
    "css_make_run_cfg": (C.c_int, [C.POINTER(CssModelDesc), C.POINTER(CssCfgSeconds), C.c_int32, C.POINTER(CssRunCfg), _FP, C.c_int64]),
    "css_pit_scan": (C.c_int, [_P, C.c_int64, C.c_int32, _P]),
    "css_run": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.POINTER(CssRunCfg), _P, C.c_int64]),
    "css_run_enqueue": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.POINTER(CssRunCfg), _P, C.c_int64]),
    "css_wait": (C.c_int, [_P]),
    "css_wait_sessions": (C.c_int, [_P, C.c_int64]),
    "css_run_device": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.POINTER(CssRunCfg), _P, C.c_int64]),
    "css_run_pcm16": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.POINTER(CssRunCfg), _P, C.c_int64, _P]),
    "css_run_enqueue_pcm16": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.POINTER(CssRunCfg), _P, C.c_int64, _P]),
    "css_get_timings": (C.c_int, [_P, C.POINTER(CssTimings)]),
    "css_set_profile": (C.c_int, [_P, C.c_int]),
    "css_get_kernel_stats": (C.c_int, [_P, _P, C.c_int32, C.POINTER(C.c_int32)]),
    "css_set_linear_mode": (C.c_int, [_P, C.c_int]),
    "css_get_linear_mode": (C.c_int, [_P]),
    "css_set_range_fallback": (C.c_int, [_P, C.c_int]),
    "css_range_status": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "css_check_range": (C.c_int, [_P]),
    "css_linear_host": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P]),
    "css_gemm_host": (C.c_int, [_P, C.POINTER(CssGemmDesc), _P, _P, _P, _P, _P]),
    "css_get_plan": (C.c_int, [_P, C.POINTER(CssPlan)]),
    "css_begin": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.POINTER(CssRunCfg), C.c_int]),
    "css_begin_range": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.POINTER(CssRunCfg), C.c_int64, C.c_int64]),
    "css_upload_range": (C.c_int, [_P, _P, C.c_int64, C.c_int64]),
    "css_stage_stft": (C.c_int, [_P]),
    "css_stage_stft_range": (C.c_int, [_P, C.c_int64, C.c_int64]),
    "css_stage_stitch_masks": (C.c_int, [_P, C.c_int64, C.c_int64]),
    "css_stage_stitch_gate": (C.c_int, [_P, C.c_int64, C.c_int64]),
    "css_stage_istft_partial": (C.c_int, [_P, C.c_int64, C.c_int64, _P, C.c_int64]),
    "css_stage_masknet": (C.c_int, [_P, C.c_int64, C.c_int64]),
    "css_stage_mvdr": (C.c_int, [_P, C.c_int64, C.c_int64]),
    "css_stage_pit_costs": (C.c_int, [_P, C.c_int64, C.c_int64]),
    "css_stage_pit_scan": (C.c_int, [_P]),
    "css_stage_stitch": (C.c_int, [_P, C.c_int64, C.c_int64]),
    "css_stage_istft": (C.c_int, [_P, C.c_int64, C.c_int64]),
    "css_stage_join_shards": (C.c_int, [_P, _P, C.c_int32, C.c_int64, _P, _P, _P, C.c_int64]),
    "css_stage_synthesis": (C.c_int, [_P, C.c_int64, C.c_int64]),
    "css_stage_seam_rows": (C.c_int, [_P, C.c_int64, C.c_int64, _P, C.c_int32]),
    "css_stage_overlap_add": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _P, C.c_int64, C.c_int64]),
    "css_sync": (C.c_int, [_P]),
    "css_stft_host": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, C.c_int64]),
    "css_separate_host": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P]),
    "css_set_feature_options": (C.c_int, [_P, C.POINTER(CssFeatureCfg)]),
    "css_set_analysis_window": (C.c_int, [_P, C.c_int32]),
    "css_forward_host": (C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int32, _P]),
    "css_istft_host": (C.c_int, [_P, _P, C.c_int32, C.c_int64, _P]),
    "css_handoff_logmel": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int64,
                                     C.POINTER(C.c_int64), _P, C.c_int32, C.POINTER(C.c_int32)]),
    "css_validation_loss_host": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                           C.c_float, _P, _P, _P, C.POINTER(C.c_float)]),
    "css_comm_unique_id": (C.c_int, [_P]),
    "css_comm_init": (C.c_int, [_P, _P, C.c_int32, C.c_int32]),
    "css_comm_destroy": (C.c_int, [_P]),
    "css_comm_info": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "css_comm_all_gather": (C.c_int, [_P, _P, _P, C.c_int64]),
    "css_stream_open": (C.c_int, [_P, C.POINTER(CssRunCfg), C.c_int32, C.POINTER(C.c_int32)]),
    "css_stream_push": (C.c_int, [_P, C.c_int32, _P, C.c_int64, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "css_stream_push_many": (C.c_int, [_P, C.POINTER(CssStreamPush), C.c_int32, C.POINTER(CssStreamGroupStats)]),
    "css_stream_push_pcm16": (C.c_int, [_P, C.c_int32, _P, C.c_int64, C.c_int64, C.c_int64, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "css_stream_push_many_pcm16": (C.c_int, [_P, C.POINTER(CssStreamPushPcm16), C.c_int32, C.POINTER(CssStreamGroupStats)]),
    "css_stream_finish": (C.c_int, [_P, C.c_int32, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "css_stream_close": (C.c_int, [_P, C.c_int32]),
    "css_stream_info": (C.c_int, [_P, C.c_int32, C.POINTER(CssStreamInfo)]),
    "css_stream_final_samples": (C.c_int, [C.POINTER(CssModelDesc), C.POINTER(CssRunCfg), C.c_int64, C.POINTER(C.c_int64)]),
    "css_stream_handoff_open": (C.c_int, [_P, C.c_int32, C.POINTER(CssStreamHandoffCfg)]),
    "css_stream_handoff_bind": (C.c_int, [_P, C.c_int32, C.POINTER(CssStreamHandoffOut)]),
    "css_stream_handoff_bounds": (C.c_int, [C.POINTER(CssModelDesc), C.POINTER(CssRunCfg), C.POINTER(CssStreamHandoffCfg), C.c_int64,
                                            C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "css_stream_handoff_final_frames": (C.c_int, [C.POINTER(CssModelDesc), C.POINTER(CssRunCfg), C.POINTER(CssStreamHandoffCfg), C.c_int64,
                                                  C.POINTER(C.c_int64)]),
    "css_handoff_kept_ranges": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64, _P, C.c_int32, C.c_int32,
                                          C.POINTER(C.c_int32)]),
    "css_stream_handoff_stats": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "css_buffer_dims": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "css_read_buffer": (C.c_int, [_P, C.c_int, _P, C.c_int64]),
    "css_write_buffer": (C.c_int, [_P, C.c_int, _P, C.c_int64]),
    "css_buffer_devptr": (C.c_int, [_P, C.c_int, C.POINTER(_P)]),
}

# the entry points include/css_mi355_rate.h declares (pushes at the capture rate), bound next to the table above
SIGNATURES_RATE = {
    "css_stream_set_rate": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32]),
    "css_stream_rate_samples": (C.c_int, [C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]),
    "css_resample_taps": (C.c_int, [C.c_int32, C.c_int32, _P, C.c_int32, C.POINTER(C.c_int32)]),
    "css_resample_host": (C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int32, _P, C.c_int64,
                                    C.POINTER(C.c_int64)]),
}
# the entry points include/css_mi355_preview.h declares (the unfinished tail of a stream), the third table load() applies
SIGNATURES_PREVIEW = {
    "css_stream_preview_samples": (C.c_int, [C.POINTER(CssModelDesc), C.POINTER(CssRunCfg), C.c_int64, C.POINTER(C.c_int64),
                                             C.POINTER(C.c_int64)]),
    "css_stream_preview": (C.c_int, [_P, C.c_int32, _P, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "css_stream_preview_many": (C.c_int, [_P, C.POINTER(CssStreamPreview), C.c_int32, C.POINTER(CssStreamGroupStats)]),
}
# the entry points include/css_mi355_preview_handoff.h declares (a preview that also hands off), the fourth table load() applies
SIGNATURES_PREVIEW_HANDOFF = {
    "css_stream_preview_handoff": (C.c_int, [_P, C.c_int32, _P, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                             C.POINTER(CssStreamHandoffOut), _P]),
    "css_stream_preview_handoff_many": (C.c_int, [_P, C.POINTER(CssStreamPreviewHandoff), C.c_int32, C.POINTER(CssStreamGroupStats)]),
}
# the entry points include/css_mi355_encoder.h declares (the kernels of csrc/encoder.hip on caller data), the fifth table load() applies
SIGNATURES_ENCODER = {
    "css_layernorm_host": (C.c_int, [_P, C.POINTER(CssLayerNormDesc), _P, _P, _P, _P, _P, _P, _P, _P]),
    "css_conv_module_host": (C.c_int, [_P, C.POINTER(CssConvModuleDesc), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                       C.POINTER(C.c_int32)]),
    "css_attention_host": (C.c_int, [_P, C.POINTER(CssAttentionDesc), _P, _P, _P, _P, _P, _P]),
}
# the entry points include/css_mi355_window.h declares (encoder windows out of a stream's frame history), the sixth table load() applies
SIGNATURES_WINDOW = {
    "css_stream_window_open": (C.c_int, [_P, C.c_int32, C.c_int32]),
    "css_stream_window_range": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "css_stream_windows": (C.c_int, [_P, C.POINTER(CssStreamWindow), C.c_int32, C.POINTER(C.c_int32)]),
}
# the entry point include/css_mi355_present_window.h declares (a preview that also writes encoder windows up to the present), the
# seventh table load() applies
SIGNATURES_PRESENT = {
    "css_stream_present_windows": (C.c_int, [_P, C.POINTER(CssStreamPresentItem), C.c_int32, C.POINTER(CssStreamGroupStats),
                                             C.POINTER(C.c_int32)]),
}
# the entry points include/css_mi355_frontend.h declares (the kernels of csrc/stft.hip and csrc/frontend.hip on caller data), the
# eighth table load() applies
SIGNATURES_FRONTEND = {
    "css_analysis_host": (C.c_int, [_P, C.POINTER(CssAnalysisDesc), _P, _P, _P]),
    "css_features_host": (C.c_int, [_P, C.POINTER(CssFeaturesDesc), _P, _P, _P, _P, _P]),
    "css_synthesis_tail_host": (C.c_int, [_P, C.POINTER(CssSynthesisTailDesc), _P, _P]),
    "css_pcm_edges_host": (C.c_int, [_P, C.POINTER(CssPcmEdgesDesc), _P, _P, _P]),
}
# the entry points include/css_mi355_session_handoff.h declares (kept ranges and log-mel of all streams of a session, found and
# computed on the device; queued sessions that hand off), the ninth table load() applies
SIGNATURES_SESSION_HANDOFF = {
    "css_session_handoff_bounds": (C.c_int, [C.POINTER(CssModelDesc), C.POINTER(CssRunCfg), C.POINTER(CssStreamHandoffCfg), C.c_int64,
                                             C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "css_handoff_logmel_all": (C.c_int, [_P, _P, C.c_int64, C.POINTER(CssStreamHandoffCfg), C.POINTER(CssSessionHandoffOut)]),
    "css_run_enqueue_handoff": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.POINTER(CssRunCfg), _P, C.c_int64,
                                          C.POINTER(CssStreamHandoffCfg), C.POINTER(CssSessionHandoffOut)]),
    "css_run_enqueue_pcm16_handoff": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.POINTER(CssRunCfg), _P, C.c_int64, _P,
                                                C.POINTER(CssStreamHandoffCfg), C.POINTER(CssSessionHandoffOut)]),
}
# the entry points include/css_mi355_stream_out.h declares (final samples at the playback rate, float32 or PCM16), the tenth table
# load() applies
SIGNATURES_STREAM_OUT = {
    "css_stream_set_output": (C.c_int, [_P, C.c_int32, C.POINTER(CssStreamOutputCfg)]),
    "css_stream_output_bind": (C.c_int, [_P, C.c_int32, _P, C.c_int64, C.POINTER(CssStreamOutputCounts)]),
    "css_stream_output_samples": (C.c_int, [C.POINTER(CssStreamOutputCfg), C.c_int64, C.c_int32, C.POINTER(C.c_int64)]),
    "css_stream_output_peaks": (C.c_int, [_P, C.c_int32, _P]),
    "css_stream_output_stats": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
}
# the entry points include/css_mi355_backend.h declares (the kernels of csrc/mvdr.hip and csrc/stitch.hip on caller data), the
# eleventh table load() applies
SIGNATURES_BACKEND = {
    "css_mvdr_host": (C.c_int, [_P, C.POINTER(CssMvdrDesc), _P, _P, _P, _P, _P, _P]),
    "css_stitch_host": (C.c_int, [_P, C.POINTER(CssStitchDesc), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
}
# the entry point include/css_mi355_array.h declares (the MVDR kernels of 2 .. 8 microphones on caller data), the twelfth table
# load() applies (named ARRAY_...: tests/test_backend_reference.py counts the module's SIGNATURES... tables)
ARRAY_SIGNATURES = {
    "css_mvdr_array_host": (C.c_int, [_P, C.POINTER(CssMvdrArrayDesc), _P, _P, _P, _P, _P, _P]),
}
# the entry points include/css_mi355_session_rate.h declares (whole sessions at the capture rate, both wav edges resampled on the
# device), the thirteenth table load() applies (named SESSION_RATE_...: the same count in tests/test_backend_reference.py)
SESSION_RATE_SIGNATURES = {
    "css_session_rate_samples": (C.c_int, [C.POINTER(CssModelDesc), C.POINTER(CssRunCfg), C.POINTER(CssSessionRate), C.c_int64,
                                           C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "css_run_rate": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.POINTER(CssRunCfg), C.POINTER(CssSessionRate), _P, C.c_int64]),
    "css_run_pcm16_rate": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.POINTER(CssRunCfg), C.POINTER(CssSessionRate), _P, C.c_int64, _P]),
    "css_run_enqueue_rate": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.POINTER(CssRunCfg), C.POINTER(CssSessionRate), _P, C.c_int64]),
    "css_run_enqueue_pcm16_rate": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.POINTER(CssRunCfg), C.POINTER(CssSessionRate), _P, C.c_int64,
                                             _P]),
    "css_session_rate_stats": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
}
# the entry points include/css_mi355_session_window.h declares (encoder windows of whole sessions, written on the device), the
# fourteenth table load() applies (named ..._BINDINGS: tests count the module's SIGNATURES... and ..._SIGNATURES tables)
_SW_TAIL = [C.POINTER(CssStreamHandoffCfg), C.POINTER(CssSessionHandoffOut), C.POINTER(CssSessionWindows)]
SESSION_WINDOW_BINDINGS = {
    "css_session_window_bounds": (C.c_int, [C.POINTER(CssModelDesc), C.POINTER(CssRunCfg), C.POINTER(CssStreamHandoffCfg), C.c_int32,
                                            C.c_int32, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "css_handoff_windows_all": (C.c_int, [_P, _P, C.c_int64] + _SW_TAIL),
    "css_run_enqueue_windows": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.POINTER(CssRunCfg), _P, C.c_int64] + _SW_TAIL),
    "css_run_enqueue_pcm16_windows": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.POINTER(CssRunCfg), _P, C.c_int64, _P] + _SW_TAIL),
    "css_session_window_stats": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
}
# the entry points include/css_mi355_rate_kernels.h declares (the table and session kernels of csrc/resample.hip on caller data), the
# fifteenth table load() applies (a ..._BINDINGS table, as the one above)
RATE_KERNEL_BINDINGS = {
    "css_rate_ingest_host": (C.c_int, [_P, C.c_int32, C.POINTER(CssRateIngestJob), C.c_int32]),
    "css_rate_output_host": (C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(CssRateOutputJob), C.c_int32]),
}
RATE_KERNEL_JOBS = 64                            # CSS_RATE_KERNEL_JOBS
# the entry points include/css_mi355_stream_kernels.h declares (the kernels of csrc/stream.hip and the streamed part of
# csrc/handoff.hip on caller data), the sixteenth table load() applies (a ..._BINDINGS table, as the two above)
STREAM_KERNEL_BINDINGS = {
    "css_stream_tail_host": (C.c_int, [_P, C.c_int32, C.POINTER(CssStreamTailJob), C.c_int32]),
    "css_stream_scatter_host": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_int32, C.POINTER(CssStreamScatterJob), C.c_int32]),
    "css_stream_ingest_host": (C.c_int, [_P, C.POINTER(CssStreamIngestJob), C.c_int32]),
    "css_stream_append_host": (C.c_int, [_P, C.POINTER(CssStreamAppendJob), C.c_int32, _P, C.c_int64]),
    "css_stream_mel_host": (C.c_int, [_P, C.c_int32, _P, C.c_int64, C.c_int64, C.POINTER(CssStreamMelJob), C.c_int32]),
}
STREAM_KERNEL_JOBS = 64                          # CSS_STREAM_KERNEL_JOBS
# the entry points include/css_mi355_handoff_kernels.h declares (the window kernels and the queued sessions' hand-off kernels of
# csrc/handoff.hip on caller data), the seventeenth table load() applies (a ..._BINDINGS table, as the three above)
HANDOFF_KERNEL_BINDINGS = {
    "css_session_scan_host": (C.c_int, [_P, C.POINTER(CssSessionScanJob)]),
    "css_session_gather_host": (C.c_int, [_P, C.POINTER(CssSessionGatherJob)]),
    "css_session_norm_host": (C.c_int, [_P, C.POINTER(CssSessionNormJob)]),
    "css_session_windows_host": (C.c_int, [_P, C.POINTER(CssSessionWindowsJob)]),
    "css_stream_windows_host": (C.c_int, [_P, C.POINTER(CssStreamWindowJob), C.c_int32, _P, C.c_int64]),
}
# the entry points include/css_mi355_nemo_handoff.h declares (kept ranges and NeMo log-mel features of all streams of a session,
# on the device; queued sessions that hand off to NeMo hosts; the kernels of csrc/nemo.hip on caller data), the eighteenth table
# load() applies (named ..._ABI: tests count the module's SIGNATURES..., ..._SIGNATURES and ..._BINDINGS tables)
NEMO_HANDOFF_ABI = {
    "css_nemo_handoff_bounds": (C.c_int, [C.POINTER(CssModelDesc), C.POINTER(CssRunCfg), C.POINTER(CssNemoCfg), C.c_int64,
                                          C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "css_handoff_nemo_all": (C.c_int, [_P, _P, C.c_int64, C.POINTER(CssNemoCfg), C.POINTER(CssNemoOut)]),
    "css_run_enqueue_nemo": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.POINTER(CssRunCfg), _P, C.c_int64, C.POINTER(CssNemoCfg),
                                       C.POINTER(CssNemoOut)]),
    "css_run_enqueue_pcm16_nemo": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.POINTER(CssRunCfg), _P, C.c_int64, _P,
                                             C.POINTER(CssNemoCfg), C.POINTER(CssNemoOut)]),
    "css_nemo_kernels_host": (C.c_int, [_P, C.POINTER(CssNemoKernelsJob)]),
}
# include/css_mi355_stream_nemo.h (a table of its own, as NEMO_HANDOFF_ABI)
STREAM_NEMO_ABI = {
    "css_stream_nemo_open": (C.c_int, [_P, C.c_int32, C.POINTER(CssStreamNemoCfg)]),
    "css_stream_nemo_bounds": (C.c_int, [C.POINTER(CssModelDesc), C.POINTER(CssRunCfg), C.POINTER(CssStreamNemoCfg), C.c_int64,
                                         C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "css_stream_nemo_final_frames": (C.c_int, [C.POINTER(CssModelDesc), C.POINTER(CssRunCfg), C.POINTER(CssStreamNemoCfg), C.c_int64,
                                               C.POINTER(C.c_int64)]),
    "css_stream_nemo_append_host": (C.c_int, [_P, C.POINTER(CssStreamNemoAppendJob), C.c_int32, _P, C.c_int64]),
    "css_stream_nemo_mel_host": (C.c_int, [_P, C.c_int32, _P, C.c_int64, C.c_int64, C.POINTER(CssStreamNemoMelJob), C.c_int32]),
}
# include/css_mi355_nemo_chunk.h (a table of its own, as STREAM_NEMO_ABI)
NEMO_CHUNK_ABI = {
    "css_stream_nemo_history_open": (C.c_int, [_P, C.c_int32, C.c_int32]),
    "css_stream_nemo_history_range": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "css_stream_nemo_chunks": (C.c_int, [_P, C.POINTER(CssStreamNemoChunk), C.c_int32, C.POINTER(C.c_int32)]),
    "css_nemo_chunk_host": (C.c_int, [_P, C.POINTER(CssNemoChunkJob), C.c_int32]),
    "css_stream_nemo_mel_history_host": (C.c_int, [_P, C.c_int32, _P, C.c_int64, C.c_int64, C.POINTER(CssStreamNemoMelHistoryJob), C.c_int32]),
}
WINDOW_KERNEL_ITEMS = 64                         # CSS_WINDOW_KERNEL_ITEMS
ARRAY_MIN_MICS, ARRAY_MAX_MICS = 2, 8            # CSS_ARRAY_MIN_MICS, CSS_ARRAY_MAX_MICS
SESSION_SCAN_CHUNK = 1024                        # CSS_SESSION_SCAN_CHUNK: the keep-scan kernel's step, in gate frames / sample blocks
RESAMPLE_TILE = 256                              # output samples per block of the two resampling kernels (resample.hip RS_TILE)

_lib: Optional[C.CDLL] = None


def _share_hip_runtime_with_torch() -> None:
    """One process must hold ONE HIP runtime.  The PyTorch-ROCm wheel bundles its own libamdhip64.so
    (SONAME libamdhip64.so.7, found through torch's RPATH under the name "libamdhip64.so"), while
    libcss_mi355.so asks the loader for "libamdhip64.so.7".  If our library is loaded first, the system
    runtime gets in, torch later adds its bundled one, and torch then sees no GPU.  Loading torch's copy
    first (without importing torch) makes the loader resolve our dependency to that same object by
    SONAME, whichever side is imported first.  Without torch installed the system runtime is used."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):  # pragma: no cover
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(path):
        try:
            C.CDLL(path, mode=C.RTLD_GLOBAL)
        except OSError:  # pragma: no cover
            pass


def load() -> C.CDLL:
    """Load the library once; raise loudly (no fallback) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CssLibraryError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run `python __graft_entry__.py` "
            f"(or `make -C notsofar1-challenge_amd/csrc`). There is no CPU fallback.")
    _share_hip_runtime_with_torch()
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise CssLibraryError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in (list(SIGNATURES.items()) + list(SIGNATURES_RATE.items()) + list(SIGNATURES_PREVIEW.items()) +
                              list(SIGNATURES_PREVIEW_HANDOFF.items()) + list(SIGNATURES_ENCODER.items()) +
                              list(SIGNATURES_WINDOW.items()) + list(SIGNATURES_PRESENT.items()) +
                              list(SIGNATURES_FRONTEND.items()) + list(SIGNATURES_SESSION_HANDOFF.items()) +
                              list(SIGNATURES_STREAM_OUT.items()) + list(SIGNATURES_BACKEND.items()) +
                              list(ARRAY_SIGNATURES.items()) + list(SESSION_RATE_SIGNATURES.items()) +
                              list(SESSION_WINDOW_BINDINGS.items()) + list(RATE_KERNEL_BINDINGS.items()) +
                              list(STREAM_KERNEL_BINDINGS.items()) + list(HANDOFF_KERNEL_BINDINGS.items()) +
                              list(NEMO_HANDOFF_ABI.items()) + list(STREAM_NEMO_ABI.items()) + list(NEMO_CHUNK_ABI.items())):
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _np_ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def _flat(a, dtype=np.float32, copy=False):
    """`a` as a flat contiguous array of `dtype` (with `copy`: one of its own, which a launch may write); None stays None."""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=dtype).reshape(-1)
    return a.copy() if copy else a


def _ptr(a):
    return None if a is None else _np_ptr(a)


def _size(a) -> int:
    return 0 if a is None else a.size


def check(handle, rc: int):
    if rc != CSS_OK:
        text = load().css_last_error(handle).decode("utf-8", "replace")
        if rc == CSS_ERR_ZERO_WEIGHT:
            # same exception type and text as the reference's assert (css/css.py:297)
            raise AssertionError(text or "zero weights found. check hop_size, segment_size or m0, m1")
        if rc == CSS_ERR_MASK_FLOOR:
            raise AssertionError(text)  # css/css.py:224
        raise CssError(rc, text)


def make_desc(d) -> CssModelDesc:
    return CssModelDesc(*[int(getattr(d, n)) for n, _ in CssModelDesc._fields_])


class RunCfg:
    """Owns the CssRunCfg struct together with the numpy weight windows it points to."""

    def __init__(self, segment_frames, hop_frames, dilation_frames, erosion_frames, mc_mvdr, stitching_loss,
                 stitching_input, normalize_segment_power, mask_floor, activity_th, w_first, w_mid, w_last):
        self._w = [np.ascontiguousarray(w, dtype=np.float32) for w in (w_first, w_mid, w_last)]
        for w in self._w:
            assert w.shape == (segment_frames,)
        self.c = CssRunCfg(int(segment_frames), int(hop_frames), int(dilation_frames), int(erosion_frames),
                           int(bool(mc_mvdr)), int(stitching_loss), int(stitching_input),
                           int(bool(normalize_segment_power)), float(mask_floor), float(activity_th),
                           self._w[0].ctypes.data_as(_FP), self._w[1].ctypes.data_as(_FP),
                           self._w[2].ctypes.data_as(_FP))


COMM_ID_BYTES = 128


def comm_unique_id() -> bytes:
    """ncclGetUniqueId through the C ABI: rank 0 calls it and hands the 128 bytes to every rank (over its own channel)"""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    rc = load().css_comm_unique_id(buf)
    if rc != 0:
        raise CssError(rc, "css_comm_unique_id failed (is librccl.so loadable?)")
    return buf.raw


def plan(desc, run_cfg: RunCfg, n_samples: int) -> CssPlan:
    p = CssPlan()
    rc = load().css_plan(C.byref(make_desc(desc)), C.byref(run_cfg.c), int(n_samples), C.byref(p))
    if rc != CSS_OK:
        raise CssError(rc, "css_plan: bad configuration")
    return p


def stream_final_samples(desc, run_cfg: RunCfg, n_pushed: int) -> int:
    """css_stream_final_samples: output samples per stream that are final after `n_pushed` input samples of a stream"""
    n = C.c_int64()
    rc = load().css_stream_final_samples(C.byref(make_desc(desc)), C.byref(run_cfg.c), int(n_pushed), C.byref(n))
    if rc != CSS_OK:
        raise CssError(rc, "css_stream_final_samples: unsupported frame geometry or bad configuration")
    return int(n.value)


def stream_preview_samples(desc, run_cfg: RunCfg, n_pushed: int):
    """css_stream_preview_samples: (first, count, status) -- a preview after `n_pushed` model-rate samples returns samples
    [first, first + count) per separated stream; status is CSS_OK or what css_run gives for this prefix (CSS_ERR_ZERO_WEIGHT)"""
    first, count = C.c_int64(), C.c_int64()
    rc = load().css_stream_preview_samples(C.byref(make_desc(desc)), C.byref(run_cfg.c), int(n_pushed), C.byref(first), C.byref(count))
    if rc not in (CSS_OK, CSS_ERR_ZERO_WEIGHT):
        raise CssError(rc, "css_stream_preview_samples: unsupported frame geometry or bad configuration")
    return int(first.value), int(count.value), int(rc)


def rate_ratio(input_rate: int, fs: int = 16000):
    """(up, down) = fs / input_rate in lowest terms: 48000 -> (1, 3), 44100 -> (160, 441), 8000 -> (2, 1)"""
    import math
    input_rate, fs = int(input_rate), int(fs)
    if input_rate <= 0 or fs <= 0:
        raise ValueError("sample rates are positive")
    g = math.gcd(input_rate, fs)
    return fs // g, input_rate // g


def stream_rate_samples(up: int, down: int, n_in: int, finished: bool = False) -> int:
    """css_stream_rate_samples: model-rate samples after `n_in` input samples at the ratio up / down (finished: of the whole recording)"""
    n = C.c_int64()
    rc = load().css_stream_rate_samples(int(up), int(down), int(n_in), int(bool(finished)), C.byref(n))
    if rc != CSS_OK:
        raise CssError(rc, f"css_stream_rate_samples: the ratio {up} / {down} is not supported, or a negative count")
    return int(n.value)


def resample_taps(up: int, down: int) -> np.ndarray:
    """css_resample_taps: the float32 taps the device uses for the ratio up / down (scipy.signal.resample_poly's default filter)"""
    n = C.c_int32()
    load().css_resample_taps(int(up), int(down), None, 0, C.byref(n))
    taps = np.empty(max(n.value, 1), np.float32)
    rc = load().css_resample_taps(int(up), int(down), _np_ptr(taps), taps.size, C.byref(n))
    if rc != CSS_OK:
        raise CssError(rc, f"css_resample_taps: the ratio {up} / {down} is not supported")
    return taps[:n.value]


def session_rate(input_rate: Optional[int] = None, output_rate: Optional[int] = None, fs: int = 16000) -> CssSessionRate:
    """The two ratios of a session whose files are at `input_rate` and whose streams are wanted at `output_rate` (None: the
    model's rate `fs` on that side): 48000 in, 16000 out -> 1 / 3 and 1 / 1; 48000 in and out -> 1 / 3 and 3 / 1"""
    in_up, in_down = (1, 1) if input_rate is None else rate_ratio(input_rate, fs)
    out_down, out_up = (1, 1) if output_rate is None else rate_ratio(output_rate, fs)   # (rate_ratio gives fs / rate)
    return CssSessionRate(in_up, in_down, out_up, out_down)


def session_rate_samples(desc, run_cfg: RunCfg, rate: CssSessionRate, n_in: int):
    """css_session_rate_samples: (n_model, n_out_model, n_out) of a recording of `n_in` capture-rate samples"""
    a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
    rc = load().css_session_rate_samples(C.byref(make_desc(desc)), C.byref(run_cfg.c), C.byref(rate), int(n_in), C.byref(a), C.byref(b), C.byref(c))
    if rc != CSS_OK:
        raise CssError(rc, f"css_session_rate_samples: the ratios {rate.in_up} / {rate.in_down}, {rate.out_up} / {rate.out_down} are not "
                           f"supported, or {n_in} samples are outside [1, 2^40] or too few for this configuration")
    return int(a.value), int(b.value), int(c.value)


def stream_output_cfg(rate: int = 16000, dtype="float32", gain: float = 1.0, fs: int = 16000) -> CssStreamOutputCfg:
    """The output format of a stream playing at `rate`: up / down = rate / fs in lowest terms, float32 or int16 samples"""
    dt = np.dtype(dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.int16)):
        raise ValueError(f"output samples are float32 or int16, got {dt}")
    down, up = rate_ratio(rate, fs)   # (rate_ratio gives fs / rate)
    return CssStreamOutputCfg(up, down, int(dt == np.dtype(np.int16)), float(gain))


def stream_output_samples(cfg: CssStreamOutputCfg, n_final_model: int, finished: bool = False) -> int:
    """css_stream_output_samples: output samples written after `n_final_model` final model-rate samples"""
    n = C.c_int64()
    rc = load().css_stream_output_samples(C.byref(cfg), int(n_final_model), int(bool(finished)), C.byref(n))
    if rc != CSS_OK:
        raise CssError(rc, f"css_stream_output_samples: the ratio {cfg.up} / {cfg.down} is not supported, or a negative count")
    return int(n.value)


def pcm16_encode(y: np.ndarray, gain: float = 1.0):
    """The numpy statement of the PCM16 output: float32 samples -> (int16 samples, the number of them the clamp changed)"""
    v = np.asarray(y, np.float32) * np.float32(gain)
    r = np.rint(v.astype(np.float64) * 32767.0)
    return np.clip(r, -32768.0, 32767.0).astype(np.int16), int(np.count_nonzero((r < -32768.0) | (r > 32767.0)))


def handoff_cfg(n_mels: int = 80, pad_frames: int = 8, drop_silence: bool = True) -> CssStreamHandoffCfg:
    return CssStreamHandoffCfg(int(n_mels), int(pad_frames), int(bool(drop_silence)))


def stream_handoff_bounds(desc, run_cfg: RunCfg, hcfg: CssStreamHandoffCfg, n_samples: int):
    """css_stream_handoff_bounds: (frames, ranges, gate frames) that suffice for a push of `n_samples` (-1: finish)"""
    f, r, a = C.c_int64(), C.c_int32(), C.c_int64()
    rc = load().css_stream_handoff_bounds(C.byref(make_desc(desc)), C.byref(run_cfg.c), C.byref(hcfg), int(n_samples),
                                          C.byref(f), C.byref(r), C.byref(a))
    if rc != CSS_OK:
        raise CssError(rc, "css_stream_handoff_bounds: bad configuration")
    return int(f.value), int(r.value), int(a.value)


def session_handoff_bounds(desc, run_cfg: RunCfg, hcfg: CssStreamHandoffCfg, n_samples: int):
    """css_session_handoff_bounds: (frames, ranges) per stream that suffice for the hand-off of a session of `n_samples`"""
    f, r = C.c_int64(), C.c_int32()
    rc = load().css_session_handoff_bounds(C.byref(make_desc(desc)), C.byref(run_cfg.c), C.byref(hcfg), int(n_samples), C.byref(f), C.byref(r))
    if rc != CSS_OK:
        raise CssError(rc, "css_session_handoff_bounds: bad configuration, or frames other than 512 / 256")
    return int(f.value), int(r.value)


class SessionHandoff:
    """The arrays of one session's hand-off (css_mi355_session_handoff.h) and, once they are valid -- after wait() /
    wait_sessions() for a queued session --, their trimmed views: ``mel[k]`` float32 [n_mels, n_frames[k]], ``ranges[k]`` int64
    [n_ranges[k], 2] (the time map back to the meeting), ``n_frames``, ``n_ranges``.  pinned: page-locked arrays (what the queued
    forms need).  cap_frames / cap_ranges: capacities beyond the bounds (tests)."""

    def __init__(self, S: int, n_mels: int, frames: int, ranges: int, pinned: bool = True, fill=None):
        make = pinned_empty if pinned else (lambda shape, dtype: np.empty(shape, dtype))
        self.S, self.n_mels = int(S), int(n_mels)
        self.mel_all = make((self.S, self.n_mels, max(int(frames), 1)), np.float32)
        self.ranges_all = make((self.S, max(int(ranges), 1), 2), np.int64)
        self.n_frames = make((self.S,), np.int64)
        self.n_ranges = make((self.S,), np.int32)
        if fill is not None:
            self.mel_all[...] = fill
            self.ranges_all[...] = int(fill)
            self.n_frames[...] = int(fill)
            self.n_ranges[...] = int(fill)
        self.c = CssSessionHandoffOut(self.mel_all.ctypes.data, int(frames), self.ranges_all.ctypes.data, int(ranges),
                                      self.n_frames.ctypes.data, self.n_ranges.ctypes.data)

    @property
    def mel(self):
        return [self.mel_all[k, :, :int(self.n_frames[k])] for k in range(self.S)]

    @property
    def ranges(self):
        return [self.ranges_all[k, :int(self.n_ranges[k])] for k in range(self.S)]


def nemo_cfg(n_mels: int = 80, pad_frames: int = 8, drop_silence: bool = True, preemphasis: float = 0.97,
             normalize: bool = True) -> CssNemoCfg:
    return CssNemoCfg(int(n_mels), int(pad_frames), int(bool(drop_silence)), float(preemphasis), int(bool(normalize)))


def nemo_handoff_bounds(desc, run_cfg: RunCfg, ncfg: CssNemoCfg, n_samples: int):
    """css_nemo_handoff_bounds: (frames, ranges) per stream that suffice for the NeMo hand-off of a session of `n_samples`"""
    f, r = C.c_int64(), C.c_int32()
    rc = load().css_nemo_handoff_bounds(C.byref(make_desc(desc)), C.byref(run_cfg.c), C.byref(ncfg), int(n_samples), C.byref(f), C.byref(r))
    if rc != CSS_OK:
        raise CssError(rc, "css_nemo_handoff_bounds: bad configuration, or frames other than 512 / 256")
    return int(f.value), int(r.value)


class NemoHandoff:
    """The arrays of one session's hand-off to a NeMo host (css_mi355_nemo_handoff.h) and, once they are valid -- after wait() /
    wait_sessions() for a queued session --, their trimmed views: ``mel[k]`` float32 [n_mels, n_frames[k]] (normalised per band,
    or the raw ln values with normalize off), ``ranges[k]`` int64 [n_ranges[k], 2] (the time map back to the meeting),
    ``n_frames``, ``n_ranges``, and with ``stats`` ``mean`` / ``std`` float32 [S, n_mels] of the raw values (rows of speakers
    with a frame).  pinned: page-locked arrays (what the queued forms need)."""

    def __init__(self, S: int, n_mels: int, frames: int, ranges: int, pinned: bool = True, fill=None, stats: bool = True):
        make = pinned_empty if pinned else (lambda shape, dtype: np.empty(shape, dtype))
        self.S, self.n_mels = int(S), int(n_mels)
        self.mel_all = make((self.S, self.n_mels, max(int(frames), 1)), np.float32)
        self.ranges_all = make((self.S, max(int(ranges), 1), 2), np.int64)
        self.n_frames = make((self.S,), np.int64)
        self.n_ranges = make((self.S,), np.int32)
        self.mean = make((self.S, self.n_mels), np.float32) if stats else None
        self.std = make((self.S, self.n_mels), np.float32) if stats else None
        if fill is not None:
            self.mel_all[...] = fill
            self.ranges_all[...] = int(fill)
            self.n_frames[...] = int(fill)
            self.n_ranges[...] = int(fill)
            if stats:
                self.mean[...] = fill
                self.std[...] = fill
        self.c = CssNemoOut(self.mel_all.ctypes.data, int(frames), self.ranges_all.ctypes.data, int(ranges), self.n_frames.ctypes.data,
                            self.n_ranges.ctypes.data, self.mean.ctypes.data if stats else None, self.std.ctypes.data if stats else None)

    @property
    def mel(self):
        return [self.mel_all[k, :, :int(self.n_frames[k])] for k in range(self.S)]

    @property
    def ranges(self):
        return [self.ranges_all[k, :int(self.n_ranges[k])] for k in range(self.S)]


def session_window_bounds(desc, run_cfg: RunCfg, hcfg: CssStreamHandoffCfg, width: int, stride: int, n_samples: int):
    """css_session_window_bounds: (frames, ranges, windows) per stream that suffice for a window session of `n_samples`"""
    f, r, w = C.c_int64(), C.c_int32(), C.c_int64()
    rc = load().css_session_window_bounds(C.byref(make_desc(desc)), C.byref(run_cfg.c), C.byref(hcfg), int(width), int(stride),
                                          int(n_samples), C.byref(f), C.byref(r), C.byref(w))
    if rc != CSS_OK:
        raise CssError(rc, "css_session_window_bounds: bad configuration, width outside 1 .. 3000 or stride outside 1 .. width")
    return int(f.value), int(r.value), int(w.value)


class SessionWindows:
    """The encoder windows of one session (css_mi355_session_window.h): the struct, the two page-locked count arrays and the
    torch tensors the kernel writes.  ``windows``: the caller's CUDA tensor [S, W, n_mels, >= width] of the dtype (dense but for
    the row pitch) or, with None, a new one of W = cap_windows; False: no windows.  ``mel``: likewise [S, n_mels, mel_ld] for the
    whole padded log-mel, True for a new one of mel_ld columns, None / False for none.  After wait() / wait_sessions():
    ``n_windows[k]``, ``window_max[k]``, and window w of speaker k is ``windows[k, w, :, :width]``."""

    def __init__(self, device: int, S: int, n_mels: int, width: int, stride: int, dtype="float16", cap_windows: int = 0, windows=None,
                 mel=None, mel_ld: int = 0, pinned: bool = True, fill=None):
        import torch
        from .stream import _window_out
        if dtype not in WINDOW_DTYPES:
            raise ValueError(f"windows are float32 or float16, got {dtype!r}")
        dt = getattr(torch, dtype)
        self.S, self.n_mels, self.width, self.stride, self.dtype = int(S), int(n_mels), int(width), int(stride), dtype
        make = pinned_empty if pinned else (lambda shape, d: np.empty(shape, d))
        self.n_windows = make((self.S,), np.int32)
        self.window_max = make((self.S,), np.float32)
        if fill is not None:
            self.n_windows[...] = int(fill)
            self.window_max[...] = fill

        class _Dev:   # (what _window_out asks of a handle)
            pass
        dev = _Dev()
        dev.device = int(device)
        ld = 0
        if windows is None:
            W = max(int(cap_windows), 1)
            windows = _window_out(dev, self.S * W, self.n_mels, self.width, dtype, None)[0].view(self.S, W, self.n_mels, self.width)
        if windows is False:
            windows = None
        if windows is not None:
            W = int(windows.shape[1]) if windows.dim() == 4 else 0
            ld = windows.stride(2) if windows.dim() == 4 else 0
            if (windows.dtype != dt or not windows.is_cuda or (windows.device.index or 0) != dev.device or windows.dim() != 4 or
                    windows.shape[0] != self.S or windows.shape[2] != self.n_mels or windows.shape[3] < self.width or
                    windows.stride(3) != 1 or ld < self.width or windows.stride(1) != self.n_mels * ld or
                    windows.stride(0) != W * self.n_mels * ld):
                raise ValueError(f"windows: a {dtype} tensor [{self.S}, W, {self.n_mels}, >= {self.width}] on cuda:{dev.device}, dense "
                                 f"but for the row pitch")
            cap_windows = W
        if mel is True:
            mel = torch.empty((self.S, self.n_mels, max(int(mel_ld), 1)), dtype=dt, device=f"cuda:{dev.device}")
        if mel is False:
            mel = None
        if mel is not None:
            if (mel.dtype != dt or not mel.is_cuda or (mel.device.index or 0) != dev.device or mel.dim() != 3 or
                    mel.shape[0] != self.S or mel.shape[1] != self.n_mels or not mel.is_contiguous()):
                raise ValueError(f"mel: a contiguous {dtype} tensor [{self.S}, {self.n_mels}, mel_ld] on cuda:{dev.device}")
            mel_ld = int(mel.shape[2])
        self.windows, self.mel = windows, mel
        self.c = CssSessionWindows(self.width, self.stride, WINDOW_DTYPES[dtype], 0, windows.data_ptr() if windows is not None else None,
                                   int(ld), int(cap_windows) if windows is not None else 0, mel.data_ptr() if mel is not None else None,
                                   int(mel_ld) if mel is not None else 0, self.n_windows.ctypes.data, self.window_max.ctypes.data)


def handoff_kept_ranges(act: np.ndarray, first_frame: int, n_known: int, pad_frames: int, a: int, b: int, n_out: int,
                        ranges: Optional[np.ndarray] = None, cap: int = 4096) -> np.ndarray:
    """css_handoff_kept_ranges: `ranges` [n, 2] (or None) extended by the sample ranges of [a, b) the gate bits keep"""
    act = np.ascontiguousarray(act, dtype=np.uint8)
    buf = np.zeros((cap, 2), np.int64)
    n_in = 0 if ranges is None else int(len(ranges))
    if n_in:
        buf[:n_in] = ranges
    n = C.c_int32()
    rc = load().css_handoff_kept_ranges(_np_ptr(act), int(first_frame), int(n_known), int(pad_frames), int(a), int(b), int(n_out),
                                        _np_ptr(buf), n_in, cap, C.byref(n))
    if rc != CSS_OK:
        raise CssError(rc, "css_handoff_kept_ranges: bad argument, a missing frame or too little room")
    return buf[:n.value].copy()


def stream_nemo_cfg(n_mels: int = 80, pad_frames: int = 8, drop_silence: bool = True, preemphasis: float = 0.97) -> CssStreamNemoCfg:
    return CssStreamNemoCfg(int(n_mels), int(pad_frames), int(bool(drop_silence)), float(preemphasis))


def stream_nemo_bounds(desc, run_cfg: RunCfg, ncfg: CssStreamNemoCfg, n_samples: int):
    """css_stream_nemo_bounds: (frames, ranges, gate frames) that suffice for a push of `n_samples` (-1: finish)"""
    f, r, a = C.c_int64(), C.c_int32(), C.c_int64()
    rc = load().css_stream_nemo_bounds(C.byref(make_desc(desc)), C.byref(run_cfg.c), C.byref(ncfg), int(n_samples),
                                       C.byref(f), C.byref(r), C.byref(a))
    if rc != CSS_OK:
        raise CssError(rc, "css_stream_nemo_bounds: bad configuration")
    return int(f.value), int(r.value), int(a.value)


def stream_nemo_final_frames(desc, run_cfg: RunCfg, ncfg: CssStreamNemoCfg, n_pushed: int) -> int:
    """css_stream_nemo_final_frames (drop_silence = 0 only): NeMo frames that are final after `n_pushed` samples"""
    n = C.c_int64()
    rc = load().css_stream_nemo_final_frames(C.byref(make_desc(desc)), C.byref(run_cfg.c), C.byref(ncfg), int(n_pushed), C.byref(n))
    if rc != CSS_OK:
        raise CssError(rc, "css_stream_nemo_final_frames: bad configuration, or drop_silence is on")
    return int(n.value)


def stream_handoff_final_frames(desc, run_cfg: RunCfg, hcfg: CssStreamHandoffCfg, n_pushed: int) -> int:
    """css_stream_handoff_final_frames (drop_silence = 0 only): log-mel frames that are final after `n_pushed` samples"""
    n = C.c_int64()
    rc = load().css_stream_handoff_final_frames(C.byref(make_desc(desc)), C.byref(run_cfg.c), C.byref(hcfg), int(n_pushed), C.byref(n))
    if rc != CSS_OK:
        raise CssError(rc, "css_stream_handoff_final_frames: bad configuration, or drop_silence is on")
    return int(n.value)


def pit_scan(costs: np.ndarray, num_spks: int) -> np.ndarray:
    costs = np.ascontiguousarray(costs, dtype=np.float64).reshape(-1, num_spks * num_spks)
    perms = np.zeros((costs.shape[0] + 1, num_spks), dtype=np.int32)
    rc = load().css_pit_scan(_np_ptr(costs), costs.shape[0], num_spks, _np_ptr(perms))
    if rc != CSS_OK:
        raise CssError(rc, "css_pit_scan")
    return perms


class _PinnedBlock:
    """Owner of one css_host_alloc block (page-locked host memory), freed when the last array over it dies."""

    def __init__(self, nbytes: int):
        self.lib = load()
        p = C.c_void_p()
        rc = self.lib.css_host_alloc(max(int(nbytes), 1), C.byref(p))
        if rc != CSS_OK or not p.value:
            raise CssError(rc, "css_host_alloc failed")
        self.ptr, self.nbytes = p.value, int(nbytes)
        self.__array_interface__ = {"shape": (max(int(nbytes), 1),), "typestr": "|u1", "data": (self.ptr, False), "version": 3}

    def __del__(self):  # pragma: no cover
        try:
            self.lib.css_host_free(C.c_void_p(self.ptr))
        except Exception:
            pass


def pinned_empty(shape, dtype=np.float32) -> np.ndarray:
    """numpy array in page-locked host memory (css_host_alloc): css_run* on such buffers moves the samples by DMA,
    asynchronously, overlapped with the first and last kernels of the pass."""
    dt = np.dtype(dtype)
    n = int(np.prod(shape)) * dt.itemsize
    block = _PinnedBlock(n)
    return np.asarray(block)[:n].view(dt).reshape(shape)   # the view chain keeps `block` alive


def pinned_copy(a: np.ndarray) -> np.ndarray:
    out = pinned_empty(a.shape, a.dtype)
    out[...] = a
    return out


class Handle:
    """One model resident on one GPU (css_create .. css_destroy)."""

    def __init__(self, desc, blob: np.ndarray, device: int = 0, stream: int = 0, max_batch_segments: int = 64):
        lib = load()
        self.lib = lib
        self.desc = desc
        self._cdesc = make_desc(desc)
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        need = lib.css_blob_num_floats(C.byref(self._cdesc))
        if need != blob.size:
            raise CssError(CSS_ERR_INVALID_ARG, f"weight blob has {blob.size} floats, library expects {need}")
        h = C.c_void_p()
        rc = lib.css_create(C.byref(self._cdesc), _np_ptr(blob), blob.size, int(device),
                            C.c_void_p(stream) if stream else None, int(max_batch_segments), C.byref(h))
        if rc != CSS_OK:
            raise CssError(rc, lib.css_last_error(None).decode("utf-8", "replace"))
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self.lib.css_destroy(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def stream_ptr(self) -> int:
        """hipStream_t of the handle (wrap with torch.cuda.ExternalStream to order torch work with its kernels)."""
        p = C.c_void_p()
        check(self.h, self.lib.css_get_stream(self.h, C.byref(p)))
        return int(p.value or 0)

    def set_lanes(self, lanes: int):
        check(self.h, self.lib.css_set_lanes(self.h, int(lanes)))

    def set_tuning(self, which, value: int):
        """which: "tail_pieces" | "out_mapped" | "tail_per_unit" | "mvdr_on_lanes" | "pipeline_device" (include/css_mi355.h css_tuning)"""
        idx = {"tail_pieces": 0, "out_mapped": 1, "tail_per_unit": 2, "mvdr_on_lanes": 3, "pipeline_device": 4,
               "group_lanes": 5, "group_transform_on_main": 6, "group_mvdr_on_lanes": 7, "group_out_dma": 8, "f32_gemm": 9, "split_batch_rows": 10, "f32_lane_rows": 11}[which] if isinstance(which, str) else int(which)
        check(self.h, self.lib.css_set_tuning(self.h, idx, int(value)))

    def set_queue_group(self, max_sessions: int):
        """queued sessions (run_enqueue) merged into one mask-estimator batch: at most `max_sessions` (1 = none)"""
        check(self.h, self.lib.css_set_queue_group(self.h, int(max_sessions)))

    def lanes(self) -> int:
        return int(self.lib.css_get_lanes(self.h))

    # ---- fused path
    def run(self, pcm: np.ndarray, cfg: RunCfg, out: Optional[np.ndarray] = None) -> np.ndarray:
        """pcm [n, C] float32 host -> wav [S, n_out] float32 host (css/css.py:110).  `out`: an existing [S, >= n_out]
        float32 array to fill (page-locked buffers from pinned_empty make both PCIe legs asynchronous DMA)."""
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        n, c = pcm.shape
        p = plan(self.desc, cfg, n)
        if out is None:
            out = np.empty((self.desc.num_spks, p.n_out), dtype=np.float32)
        assert out.dtype == np.float32 and out.ndim == 2 and out.shape[0] == self.desc.num_spks and out.shape[1] >= p.n_out \
            and out.strides[1] == 4
        check(self.h, self.lib.css_run(self.h, _np_ptr(pcm), n, c, C.byref(cfg.c), _np_ptr(out), out.strides[0] // 4))
        return out[:, :p.n_out]

    def run_enqueue(self, pcm: np.ndarray, cfg: RunCfg, out: np.ndarray) -> np.ndarray:
        """css_run without the closing synchronisation (a queue of sessions): `pcm` (float32 [n, C], C-contiguous) must
        stay alive and `out` untouched until wait().  With page-locked buffers (pinned_empty / pinned_copy) consecutive
        queued passes overlap: a session's PCIe legs hide under its neighbours' kernels.  Returns the view of `out` that
        wait() makes valid."""
        assert pcm.dtype == np.float32 and pcm.flags.c_contiguous and pcm.ndim == 2
        n, c = pcm.shape
        p = plan(self.desc, cfg, n)
        assert out.dtype == np.float32 and out.ndim == 2 and out.shape[0] == self.desc.num_spks and out.shape[1] >= p.n_out \
            and out.strides[1] == 4
        self._queued_keep = getattr(self, "_queued_keep", []) + [(pcm, out, cfg)]
        check(self.h, self.lib.css_run_enqueue(self.h, _np_ptr(pcm), n, c, C.byref(cfg.c), _np_ptr(out), out.strides[0] // 4))
        return out[:, :p.n_out]

    def wait(self):
        """Blocks until every pass queued with run_enqueue has finished (CssError CSS_ERR_RANGE if one left the split-f16
        range: repeat those sessions with run())."""
        try:
            check(self.h, self.lib.css_wait(self.h))
        finally:
            self._queued_keep = []

    def wait_sessions(self, n: int):
        """Blocks until the first `n` sessions queued since the last wait() have finished (outputs in host memory); the later
        ones keep running.  Not a wait(): call that eventually (it releases the references this object keeps, and in
        "split_f16" mode it is where a session that left the operand range is repeated -- from its input buffers)."""
        check(self.h, self.lib.css_wait_sessions(self.h, int(n)))

    def run_device(self, pcm_ptr: int, n: int, c: int, cfg: RunCfg, wav_ptr: int, cap: int):
        check(self.h, self.lib.css_run_device(self.h, C.c_void_p(pcm_ptr), n, c, C.byref(cfg.c),
                                              C.c_void_p(wav_ptr), cap))

    def run_pcm16(self, planes, cfg: RunCfg):
        """planes: sequence of C mono int16 arrays of equal length (the session's wav payloads).
        -> (int16 [S, n_out] peak-normalised PCM16 samples of the separated streams, float32 [S] peaks)."""
        planes = [np.ascontiguousarray(p, dtype=np.int16) for p in planes]
        n = planes[0].shape[0]
        if any(p.ndim != 1 or p.shape[0] != n for p in planes):
            raise ValueError("all channel planes must be one-dimensional and of equal length")
        c = len(planes)
        pl = plan(self.desc, cfg, n)
        S = int(self.desc.num_spks)
        out = np.empty((S, pl.n_out), dtype=np.int16)
        peaks = np.empty((S,), dtype=np.float32)
        ptrs = (C.c_void_p * c)(*[p.ctypes.data for p in planes])
        check(self.h, self.lib.css_run_pcm16(self.h, ptrs, n, c, C.byref(cfg.c), out.ctypes.data_as(C.c_void_p), pl.n_out,
                                             peaks.ctypes.data_as(C.c_void_p)))
        return out, peaks

    def run_enqueue_pcm16(self, planes, cfg: RunCfg, out16: np.ndarray, peaks: Optional[np.ndarray] = None) -> np.ndarray:
        """run_pcm16 as a queued session (css_run_enqueue_pcm16): `planes` = C mono int16 arrays of equal length, `out16` an
        int16 [S, >= n_out] array, `peaks` None or a float32 [S] array -- all of them must stay alive and untouched until
        wait(); page-locked buffers (pinned_empty / pinned_copy) let the session share an estimator batch with its neighbours
        in the queue and hide its PCIe legs.  Returns the view of `out16` that wait() makes valid."""
        n = planes[0].shape[0]
        for p in planes:
            assert p.dtype == np.int16 and p.ndim == 1 and p.shape[0] == n and p.flags.c_contiguous
        c = len(planes)
        pl = plan(self.desc, cfg, n)
        S = int(self.desc.num_spks)
        assert out16.dtype == np.int16 and out16.ndim == 2 and out16.shape[0] == S and out16.shape[1] >= pl.n_out and out16.strides[1] == 2
        assert peaks is None or (peaks.dtype == np.float32 and peaks.shape == (S,) and peaks.flags.c_contiguous)
        ptrs = (C.c_void_p * c)(*[p.ctypes.data for p in planes])
        self._queued_keep = getattr(self, "_queued_keep", []) + [(planes, out16, peaks, cfg)]
        check(self.h, self.lib.css_run_enqueue_pcm16(self.h, ptrs, n, c, C.byref(cfg.c), out16.ctypes.data_as(C.c_void_p), out16.strides[0] // 2,
                                                     peaks.ctypes.data_as(C.c_void_p) if peaks is not None else None))
        return out16[:, :pl.n_out]

    # ---- whole sessions at the capture rate (include/css_mi355_session_rate.h)
    def session_rate_samples(self, cfg: RunCfg, rate: CssSessionRate, n_in: int):
        """(n_model, n_out_model, n_out) of a recording of `n_in` capture-rate samples on this handle's model"""
        return session_rate_samples(self.desc, cfg, rate, n_in)

    def _rate_float_args(self, pcm, cfg, rate, out):
        assert pcm.dtype == np.float32 and pcm.flags.c_contiguous and pcm.ndim == 2
        n, c = pcm.shape
        n_out = self.session_rate_samples(cfg, rate, n)[2]
        S = int(self.desc.num_spks)
        if out is None:
            out = np.empty((S, n_out), dtype=np.float32)
        assert out.dtype == np.float32 and out.ndim == 2 and out.shape[0] == S and out.shape[1] >= n_out and out.strides[1] == 4
        return n, c, n_out, out

    def _rate_pcm16_args(self, planes, cfg, rate, out16, peaks):
        n = planes[0].shape[0]
        for p in planes:
            assert p.dtype == np.int16 and p.ndim == 1 and p.shape[0] == n and p.flags.c_contiguous
        n_out = self.session_rate_samples(cfg, rate, n)[2]
        S = int(self.desc.num_spks)
        if out16 is None:
            out16 = np.empty((S, n_out), dtype=np.int16)
        if peaks is None:
            peaks = np.empty((S,), dtype=np.float32)
        assert out16.dtype == np.int16 and out16.ndim == 2 and out16.shape[0] == S and out16.shape[1] >= n_out and out16.strides[1] == 2
        assert peaks.dtype == np.float32 and peaks.shape == (S,) and peaks.flags.c_contiguous
        ptrs = (C.c_void_p * len(planes))(*[p.ctypes.data for p in planes])
        return n, len(planes), n_out, out16, peaks, ptrs

    def run_rate(self, pcm: np.ndarray, cfg: RunCfg, rate: CssSessionRate, out: Optional[np.ndarray] = None) -> np.ndarray:
        """css_run_rate: pcm [n_in, C] float32 at the capture rate -> wav [S, n_out] float32 at the output rate.  `cfg` is the
        configuration at the MODEL's rate (make_run_cfg(cfg, 16000, ...))."""
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        n, c, n_out, out = self._rate_float_args(pcm, cfg, rate, out)
        check(self.h, self.lib.css_run_rate(self.h, _np_ptr(pcm), n, c, C.byref(cfg.c), C.byref(rate), _np_ptr(out), out.strides[0] // 4))
        return out[:, :n_out]

    def run_pcm16_rate(self, planes, cfg: RunCfg, rate: CssSessionRate):
        """css_run_pcm16_rate: C mono int16 planes at the capture rate -> (int16 [S, n_out] peak-normalised at the output rate,
        float32 [S] peaks of the streams at that rate)."""
        planes = [np.ascontiguousarray(p, dtype=np.int16) for p in planes]
        n, c, n_out, out16, peaks, ptrs = self._rate_pcm16_args(planes, cfg, rate, None, None)
        check(self.h, self.lib.css_run_pcm16_rate(self.h, ptrs, n, c, C.byref(cfg.c), C.byref(rate), out16.ctypes.data_as(C.c_void_p),
                                                  out16.strides[0] // 2, peaks.ctypes.data_as(C.c_void_p)))
        return out16[:, :n_out], peaks

    def run_enqueue_rate(self, pcm: np.ndarray, cfg: RunCfg, rate: CssSessionRate, out: np.ndarray) -> np.ndarray:
        """run_rate as a queued session (css_run_enqueue_rate): run_enqueue's lifetime rules; returns the view of `out` that
        wait() makes valid."""
        n, c, n_out, out = self._rate_float_args(pcm, cfg, rate, out)
        self._queued_keep = getattr(self, "_queued_keep", []) + [(pcm, out, cfg, rate)]
        check(self.h, self.lib.css_run_enqueue_rate(self.h, _np_ptr(pcm), n, c, C.byref(cfg.c), C.byref(rate), _np_ptr(out),
                                                    out.strides[0] // 4))
        return out[:, :n_out]

    def run_enqueue_pcm16_rate(self, planes, cfg: RunCfg, rate: CssSessionRate, out16: np.ndarray,
                               peaks: Optional[np.ndarray] = None) -> np.ndarray:
        """run_pcm16_rate as a queued session (css_run_enqueue_pcm16_rate): run_enqueue_pcm16's lifetime rules; returns the view
        of `out16` that wait() makes valid."""
        assert out16 is not None
        keep_peaks = peaks
        n, c, n_out, out16, peaks, ptrs = self._rate_pcm16_args(planes, cfg, rate, out16, peaks)
        self._queued_keep = getattr(self, "_queued_keep", []) + [(planes, out16, peaks, cfg, rate)]
        check(self.h, self.lib.css_run_enqueue_pcm16_rate(self.h, ptrs, n, c, C.byref(cfg.c), C.byref(rate), out16.ctypes.data_as(C.c_void_p),
                                                          out16.strides[0] // 2,
                                                          peaks.ctypes.data_as(C.c_void_p) if keep_peaks is not None else None))
        return out16[:, :n_out]

    def session_rate_stats(self):
        """(launches of the ingest kernel, launches of the output kernel, rate sessions) on this handle since it was created"""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        check(self.h, self.lib.css_session_rate_stats(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def timings(self) -> dict:
        t = CssTimings()
        check(self.h, self.lib.css_get_timings(self.h, C.byref(t)))
        return {n: getattr(t, n) for n, _ in CssTimings._fields_}

    def kernel_stats(self) -> dict:
        """{family: (ms, launches)} of the last pass run with set_profile(True)"""
        arr = (CssKernelStat * 32)()
        cnt = C.c_int32()
        check(self.h, self.lib.css_get_kernel_stats(self.h, C.cast(arr, C.c_void_p), 32, C.byref(cnt)))
        return {arr[i].name.decode(): (float(arr[i].ms), int(arr[i].launches)) for i in range(min(cnt.value, 32))}

    def set_profile(self, enable: bool):
        check(self.h, self.lib.css_set_profile(self.h, int(enable)))

    def set_linear_mode(self, mode):
        """"exact_f32" (the default of a new handle: float32 operands, the reference's own precision) or "split_f16" (opt-in:
        22-bit operands as float16 pairs on the f16 matrix cores, ~2x the throughput)."""
        check(self.h, self.lib.css_set_linear_mode(self.h, {"split_f16": 0, "exact_f32": 1}[mode]))

    def set_feature_options(self, log_spectrogram=False, mvn_spectrogram=True, ipd_mean_normalize=True,
                            ipd_mean_normalize_version=1, ipd_cos=False, pairs=None):
        """ExtractorCfg options beyond the shipped configuration (css_set_feature_options); pairs: [(l, r), ...]"""
        c = CssFeatureCfg(int(log_spectrogram), int(mvn_spectrogram), int(ipd_mean_normalize), int(ipd_mean_normalize_version),
                          int(ipd_cos), 0)
        pairs = list(pairs) if pairs is not None else [(m, 0) for m in range(1, int(self.desc.num_mics))]
        c.num_pairs = len(pairs)
        for i, (l, r) in enumerate(pairs[:16]):
            c.pair_l[i], c.pair_r[i] = int(l), int(r)
        check(self.h, self.lib.css_set_feature_options(self.h, C.byref(c)))

    def set_analysis_window(self, window: str):
        """ExtractorCfg.window: 'hann' (default) or 'sqrt_hann' (css_set_analysis_window; feature.py:19-45)"""
        if window not in ANALYSIS_WINDOWS:
            raise RuntimeError("Now only support sqrt hanning window or hann window")   # feature.py:24-25
        check(self.h, self.lib.css_set_analysis_window(self.h, ANALYSIS_WINDOWS[window]))

    def set_range_fallback(self, enable: bool):
        check(self.h, self.lib.css_set_range_fallback(self.h, int(enable)))

    def range_status(self):
        """(passes repeated on the exact float32 kernels so far, whether the last pass was one)"""
        n, last = C.c_int64(), C.c_int32()
        check(self.h, self.lib.css_range_status(self.h, C.byref(n), C.byref(last)))
        return int(n.value), bool(last.value)

    def check_range(self):
        check(self.h, self.lib.css_check_range(self.h))

    def linear(self, x: np.ndarray, w: np.ndarray, bias=None, kernel: int = 0, layout: int = 0) -> np.ndarray:
        """y = x @ w.T + bias through one of the path's GEMM kernels (css_linear_host)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        w = np.ascontiguousarray(w, dtype=np.float32)
        m, k = x.shape
        n = w.shape[0]
        assert w.shape[1] == k
        b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
        y = np.empty((m, n), dtype=np.float32)
        check(self.h, self.lib.css_linear_host(self.h, _np_ptr(x), _np_ptr(w), _np_ptr(b) if b is not None else None,
                                               m, n, k, int(kernel), int(layout), _np_ptr(y)))
        return y

    def gemm(self, a: np.ndarray, b: np.ndarray, c: np.ndarray, M: int, N: int, K: int, *, kernel: int = 2, layout: int = 0,
             tile_rows: int = 0, batch: int = 1, lda=None, ldb=None, ldc=None, ldr=None, strideA: int = 0, strideB: int = 0,
             strideC: int = 0, a_off: int = 0, c_off: int = 0, r_off: int = 0, act: int = 0, bias=None, bias_along_m: bool = False,
             residual=None, alpha: float = 1.0, b_frag32: bool = False, split_out: int = 0, c_transposed: bool = False,
             m_fastest: bool = False, nt_store: bool = False, concurrent: bool = False) -> np.ndarray:
        """One GEMM launch of the path in any of its forms (css_gemm_host; the header describes every field).  a, b, c and a
        separate residual are the WHOLE flat float32 allocations, the matrices a_off / c_off / r_off floats into them;
        residual = "inplace" is the form C = C + alpha * (...).  Returns c as the launch left it, every float of it."""
        flat = lambda x: np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
        a, b, out = flat(a), flat(b), flat(c).copy()
        inplace = isinstance(residual, str)
        if inplace and residual != "inplace":
            raise ValueError("residual: None, an array, or 'inplace'")
        r = None if residual is None or inplace else flat(residual)
        bv = None if bias is None else flat(bias)
        d = CssGemmDesc(kernel=int(kernel), layout=int(layout), tile_rows=int(tile_rows), batch=int(batch), M=int(M), N=int(N), K=int(K),
                        act=int(act), lda=int(K if lda is None else lda), ldb=int(K if ldb is None else ldb),
                        ldc=int((M if c_transposed else N) if ldc is None else ldc), ldr=int(N if ldr is None else ldr),
                        strideA=int(strideA), strideB=int(strideB), strideC=int(strideC), a_off=int(a_off), c_off=int(c_off),
                        r_off=int(r_off), a_floats=a.size, b_floats=b.size, c_floats=out.size, r_floats=0 if r is None else r.size,
                        bias=0 if bv is None else (2 if bias_along_m else 1), residual=2 if inplace else (0 if r is None else 1),
                        alpha=float(alpha), b_frag32=int(bool(b_frag32)), split_out=int(split_out), c_transposed=int(bool(c_transposed)),
                        m_fastest=int(bool(m_fastest)), nt_store=int(bool(nt_store)), concurrent=int(bool(concurrent)))
        if bv is not None and bv.size != (M if bias_along_m else N):
            raise ValueError("bias: one value per output column (or per row with bias_along_m)")
        check(self.h, self.lib.css_gemm_host(self.h, C.byref(d), _np_ptr(a), _np_ptr(b), _np_ptr(bv) if bv is not None else None,
                                             _np_ptr(r) if r is not None else None, _np_ptr(out)))
        return out

    # ---- the kernels of csrc/encoder.hip on caller data (include/css_mi355_encoder.h; tests/test_hip_encoder_kernels.py)
    def layernorm(self, form: int, x: np.ndarray, rows: int, D: int, w, b, w2=None, b2=None, *, inplace: bool = False, y=None,
                  z=None, ys=None):
        """One LayerNorm launch (css_layernorm_host; the header describes the forms).  x, y, z, ys are the WHOLE flat float32
        allocations (None: the launch does not get that pointer).  Returns (x, y, z, ys) as the launch left them."""
        x, y, z, ys = (_flat(a, copy=True) for a in (x, y, z, ys))
        w, b, w2, b2 = _flat(w), _flat(b), _flat(w2), _flat(b2)
        outs = [a.size for a in (y, z, ys) if a is not None]
        if len(set(outs)) > 1:
            raise ValueError("y, z and ys are allocations of one length")
        d = CssLayerNormDesc(form=int(form), rows=int(rows), D=int(D), inplace=int(bool(inplace)), x_floats=x.size,
                             out_floats=outs[0] if outs else 0)
        check(self.h, self.lib.css_layernorm_host(self.h, C.byref(d), _ptr(x), _ptr(w), _ptr(b), _ptr(w2), _ptr(b2), _ptr(y), _ptr(z),
                                                  _ptr(ys)))
        return x, y, z, ys

    def conv_module(self, form: int, x: np.ndarray, nseg: int, T: int, D: int, taps: int, ln_w, ln_b, pw, dw_wt, dw_b, bn_alpha,
                    bn_beta, ln2_w=None, ln2_b=None, *, x_out=None, z=None, zs=None):
        """The conv module, fused (form 0) or as its two-kernel fallback in place (form 1) (css_conv_module_host).  Returns
        (launched, x, x_out, z, zs): whole allocations as the launches left them; launched is False when the fused kernel does
        not cover (D, taps) or the device refused its LDS."""
        x, x_out, z, zs = (_flat(a, copy=True) for a in (x, x_out, z, zs))
        ops = [_flat(a) for a in (ln_w, ln_b, pw, dw_wt, dw_b, bn_alpha, bn_beta, ln2_w, ln2_b)]
        outs = [a.size for a in (x_out, z, zs) if a is not None]
        if len(set(outs)) > 1:
            raise ValueError("x_out, z and zs are allocations of one length")
        if ops[2].size != 6 or ops[3].size != taps * D or any(a is not None and a.size != D for a in ops[:2] + ops[4:]):
            raise ValueError("pw [6], dw_wt [taps][D], every other operand [D]")
        d = CssConvModuleDesc(form=int(form), nseg=int(nseg), T=int(T), D=int(D), taps=int(taps), x_floats=x.size,
                              out_floats=outs[0] if outs else 0)
        launched = C.c_int32(-1)
        check(self.h, self.lib.css_conv_module_host(self.h, C.byref(d), _ptr(x), *[_ptr(a) for a in ops], _ptr(x_out), _ptr(z), _ptr(zs),
                                                    C.byref(launched)))
        return bool(launched.value), x, x_out, z, zs

    def attention(self, mode: int, x: np.ndarray, w: np.ndarray, bias: np.ndarray, pe: np.ndarray, nseg: int, T: int, D: int, H: int,
                  maxlen: int, *, split_out: int = 0, canary: int = 0x7FC0BEEF, slack_rows: int = 0):
        """QKV product + relative-position attention (css_attention_host; mode 0 exact float32, 1 split-f16, 2 any length).
        Returns (qkv, ctx): the allocations of nseg * T + slack_rows rows of 3 D / D floats as the launches left them; every
        float they did not write holds `canary`."""
        x, w, bias, pe = _flat(x), _flat(w), _flat(bias), _flat(pe)
        K = w.size // (3 * D)
        rows = nseg * T + int(slack_rows)
        qkv = np.empty(rows * 3 * D, np.float32)
        ctx = np.empty(rows * D, np.float32)
        if bias.size != 3 * D:
            raise ValueError("bias [3 D]")
        d = CssAttentionDesc(mode=int(mode), nseg=int(nseg), T=int(T), D=int(D), H=int(H), maxlen=int(maxlen), K=int(K),
                             split_out=int(split_out), canary=int(canary), x_floats=x.size, w_floats=w.size, pe_floats=pe.size,
                             qkv_floats=qkv.size, ctx_floats=ctx.size)
        check(self.h, self.lib.css_attention_host(self.h, C.byref(d), _np_ptr(x), _np_ptr(w), _np_ptr(bias), _np_ptr(pe), _np_ptr(qkv),
                                                  _np_ptr(ctx)))
        return qkv, ctx

    # ---- the kernels of csrc/stft.hip and csrc/frontend.hip on caller data (include/css_mi355_frontend.h;
    #      tests/test_hip_frontend_kernels.py).  Arrays are the WHOLE allocations; outputs are returned as the launch left them.
    def analysis(self, x: np.ndarray, C_: int, x_stride: int, t_lo: int, t_hi: int, row_ld: int, out: np.ndarray, *, offset: int = 0,
                 window: int = 0, phase=None):
        """launch_stft_fft (css_analysis_host).  Returns (out, phase)."""
        x, out, phase = _flat(x), _flat(out, copy=True), _flat(phase, copy=True)
        d = CssAnalysisDesc(C=int(C_), t_lo=int(t_lo), t_hi=int(t_hi), offset=int(offset), window=int(window),
                            want_phase=int(phase is not None), x_stride=int(x_stride), row_ld=int(row_ld), x_floats=x.size,
                            out_floats=out.size, phase_floats=_size(phase))
        check(self.h, self.lib.css_analysis_host(self.h, C.byref(d), _np_ptr(x), _np_ptr(out), _ptr(phase)))
        return out, phase

    def features_host(self, X: np.ndarray, C_: int, F: int, T_ld: int, stft_frames: int, seg_lo: int, nseg: int, T: int, hop: int,
                      Kp: int, cfg: "CssFeatureCfg", in_bias, in_scale, feat: np.ndarray, *, split_out: int = 0, PH=None):
        """launch_features (css_features_host).  Returns feat."""
        X, in_bias, in_scale, feat, PH = _flat(X), _flat(in_bias), _flat(in_scale), _flat(feat, copy=True), _flat(PH)
        d = CssFeaturesDesc(C=int(C_), F=int(F), nseg=int(nseg), T=int(T), hop=int(hop), Kp=int(Kp), split_out=int(split_out),
                            T_ld=int(T_ld), stft_frames=int(stft_frames), seg_lo=int(seg_lo), x_floats=X.size,
                            ph_floats=_size(PH), feat_floats=feat.size, cfg=cfg)
        if in_bias.size != F * (1 + cfg.num_pairs) or in_scale.size != in_bias.size:
            raise ValueError("in_bias, in_scale [F (1 + pairs)]")
        check(self.h, self.lib.css_features_host(self.h, C.byref(d), _np_ptr(X), _ptr(PH), _np_ptr(in_bias),
                                                 _np_ptr(in_scale), _np_ptr(feat)))
        return feat

    def synthesis_tail(self, form: int, src: np.ndarray, out: np.ndarray, *, t_lo=(), t_hi=(), level=None, **fields):
        """launch_wave_ola (0), launch_join_shards (1), launch_planes_to_rows (2) (css_synthesis_tail_host); fields are the
        descriptor's.  level: None (absent) or the word.  Returns out."""
        src, out = _flat(src), _flat(out, copy=True)
        d = CssSynthesisTailDesc(form=int(form), has_level=int(level is not None), level=int(level or 0), in_floats=src.size,
                                 out_floats=out.size, **{k: int(v) for k, v in fields.items()})
        for k, (lo, hi) in enumerate(zip(t_lo, t_hi)):
            d.t_lo[k], d.t_hi[k] = int(lo), int(hi)
        check(self.h, self.lib.css_synthesis_tail_host(self.h, C.byref(d), _np_ptr(src), _np_ptr(out)))
        return out

    def pcm_edges(self, form: int, src: np.ndarray, out=None, **fields):
        """The PCM edges (css_pcm_edges_host; the header lists the forms); fields are the descriptor's.  Returns (out, peak):
        the output allocation (None for the peak forms) and the peak words (None for forms 0 .. 2)."""
        src = np.ascontiguousarray(src).reshape(-1)
        out = None if out is None else np.ascontiguousarray(out).reshape(-1).copy()
        want = {0: (np.float32, np.float32), 1: (np.int16, np.float32), 2: (np.int16, np.float32), 3: (np.float32, None),
                4: (np.int16, None), 5: (np.float32, np.int16)}[int(form)]
        if src.dtype != want[0] or (out is not None and out.dtype != want[1]):
            raise ValueError("array types do not match the form")
        peak = np.zeros(max(1, int(fields.get("S", 1))), np.uint32) if form >= 3 else None
        d = CssPcmEdgesDesc(form=int(form), in_elems=src.size, out_elems=0 if out is None else out.size,
                            **{k: int(v) for k, v in fields.items()})
        check(self.h, self.lib.css_pcm_edges_host(self.h, C.byref(d), _np_ptr(src), None if out is None else _np_ptr(out),
                                                  None if peak is None else _np_ptr(peak)))
        return out, peak

    # ---- the table and session kernels of csrc/resample.hip on caller data (include/css_mi355_rate_kernels.h;
    #      tests/test_hip_rate_kernels.py).  A job is a dict of the descriptor's fields; its arrays are the WHOLE allocations and
    #      the ones a launch writes are copied first and returned as the launch left them.
    def rate_ingest(self, form: int, jobs):
        """launch_stream_ingest_resample_multi (0) / launch_session_ingest_multi (1) (css_rate_ingest_host).  Per job: src (int16 or
        float32), hist_in, dst, hist_out (None: not passed) and the scalar fields.  Returns [(dst, hist_out, level_after)]."""
        tab = (CssRateIngestJob * len(jobs))()
        keep = []
        for d, j in zip(tab, jobs):
            j = dict(j)
            src = np.ascontiguousarray(j.pop("src")).reshape(-1)
            if src.dtype not in (np.int16, np.float32):
                raise ValueError("src is int16 or float32")
            hin = j.pop("hist_in", None)
            hin = np.zeros(0, np.float32) if hin is None else np.ascontiguousarray(hin, dtype=np.float32).reshape(-1)
            hout = j.pop("hist_out", None)
            hout = None if hout is None else np.ascontiguousarray(hout, dtype=np.float32).reshape(-1).copy()
            dst = np.ascontiguousarray(j.pop("dst"), dtype=np.float32).reshape(-1).copy()
            if hout is not None and hout.size != hin.size:
                raise ValueError("hist_out has hist_in's size")
            for k, v in j.items():
                setattr(d, k, int(v))
            d.is_int16, d.has_hist_out = int(src.dtype == np.int16), int(hout is not None)
            d.src_elems, d.hist_elems, d.dst_floats = src.size, hin.size, dst.size
            d.src, d.hist_in, d.dst = src.ctypes.data, hin.ctypes.data, dst.ctypes.data
            d.hist_out = None if hout is None else hout.ctypes.data
            keep.append((src, hin, hout, dst))
        rc = self.lib.css_rate_ingest_host(self.h, int(form), tab, len(jobs))
        return self._rate_left(rc, [(k[3], k[2], int(d.level_after)) for d, k in zip(tab, keep)])

    def rate_output(self, form: int, S: int, jobs):
        """launch_stream_output_multi (0) / launch_session_output (1) (css_rate_output_host).  Per job: src, hist_in, dst (float32, or
        int16 with pcm16), hist_out (None: not passed), peak [S] uint32, clipped [S] uint64 and the scalar fields.
        Returns [(dst, hist_out, peak, clipped)]."""
        tab = (CssRateOutputJob * len(jobs))()
        keep = []
        for d, j in zip(tab, jobs):
            j = dict(j)
            src = np.ascontiguousarray(j.pop("src"), dtype=np.float32).reshape(-1)
            hin = j.pop("hist_in", None)
            hin = np.zeros(0, np.float32) if hin is None else np.ascontiguousarray(hin, dtype=np.float32).reshape(-1)
            hout = j.pop("hist_out", None)
            hout = None if hout is None else np.ascontiguousarray(hout, dtype=np.float32).reshape(-1).copy()
            dst = np.ascontiguousarray(j.pop("dst")).reshape(-1).copy()
            peak = np.ascontiguousarray(j.pop("peak", np.zeros(S, np.uint32)), dtype=np.uint32).reshape(-1).copy()
            clipped = np.ascontiguousarray(j.pop("clipped", np.zeros(S, np.uint64)), dtype=np.uint64).reshape(-1).copy()
            pcm16 = int(j.get("pcm16", 0))
            if dst.dtype != (np.int16 if pcm16 else np.float32) or peak.size != S or clipped.size != S:
                raise ValueError("dst is int16 with pcm16, float32 without; peak and clipped [S]")
            if hout is not None and hout.size != hin.size:
                raise ValueError("hist_out has hist_in's size")
            d.gain = float(j.pop("gain", 1.0))
            for k, v in j.items():
                setattr(d, k, int(v))
            d.has_hist_out = int(hout is not None)
            d.src_floats, d.hist_elems, d.dst_elems = src.size, hin.size, dst.size
            d.src, d.hist_in, d.dst, d.peak, d.clipped = src.ctypes.data, hin.ctypes.data, dst.ctypes.data, peak.ctypes.data, clipped.ctypes.data
            d.hist_out = None if hout is None else hout.ctypes.data
            keep.append((src, hin, hout, dst, peak, clipped))
        rc = self.lib.css_rate_output_host(self.h, int(form), int(S), tab, len(jobs))
        return self._rate_left(rc, [(k[3], k[2], k[4], k[5]) for k in keep])

    def _rate_left(self, rc, left):
        """`left` after a call that succeeded; a refused call raises CssError with `left` (the arrays as the call left them) on it"""
        try:
            check(self.h, rc)
        except CssError as e:
            e.left = left
            raise
        return left

    # ---- the kernels of csrc/stream.hip and the streamed part of csrc/handoff.hip on caller data
    #      (include/css_mi355_stream_kernels.h; tests/test_hip_stream_kernels.py).  A job is a dict of the descriptor's scalar fields
    #      and its arrays (the WHOLE allocations; None or absent: not passed); the arrays a launch may write are copied first, and
    #      every call returns one dict per job with them as the launch left them.
    def _stream_kernel_table(self, kind, jobs, arrays=None, skip=()):
        """(``skip``: keys of a job that only say how its arrays are read -- ``f16`` -- and are no field of ``kind``)"""
        ins, outs = (arrays or STREAM_KERNEL_ARRAYS)[kind.__name__]
        tab = (kind * len(jobs))()
        keep, left = [], []
        for d, j in zip(tab, jobs):
            j = dict(j)
            got = {}
            for (name, dtype), out in [(f, False) for f in ins] + [(f, True) for f in outs]:
                a = j.pop(name, None)
                if a is None:
                    continue
                if dtype is None:   # (float32, or float16 words: the job's f16 says which)
                    dtype = np.uint16 if int(j.get("f16", 0)) else np.float32
                a = np.ascontiguousarray(a, dtype=dtype).reshape(-1)
                a = a.copy() if out else a
                getattr(d, name).p, getattr(d, name).elems = a.ctypes.data, a.size
                keep.append(a)
                if out:
                    got[name] = a
            for k, v in j.items():
                if k not in skip:
                    setattr(d, k, float(v) if k == "activity_th" else int(v))
            left.append(got)
        return tab, keep, left

    def stream_tail(self, form: int, jobs):
        """launch_stream_activity_multi (0) / launch_stream_gate_ola_multi (1) (css_stream_tail_host) -> [{act_b, Y, ring}]"""
        tab, keep, left = self._stream_kernel_table(CssStreamTailJob, jobs)
        for d in tab:
            d.has_ring = int(bool(d.ring.p))
        return self._rate_left(self.lib.css_stream_tail_host(self.h, int(form), tab, len(jobs)), left)

    def stream_scatter(self, src, src_ld: int, rows: int, jobs):
        """launch_stream_scatter_masks (css_stream_scatter_host) of src [rows][src_ld] -> [{dst}]"""
        src = np.ascontiguousarray(src, dtype=np.float32).reshape(-1)
        tab, keep, left = self._stream_kernel_table(CssStreamScatterJob, jobs)
        return self._rate_left(self.lib.css_stream_scatter_host(self.h, _np_ptr(src), src.size, int(src_ld), int(rows), tab, len(jobs)), left)

    def stream_ingest(self, jobs):
        """launch_stream_ingest_pcm16_multi (css_stream_ingest_host) -> [{dst}]"""
        tab, keep, left = self._stream_kernel_table(CssStreamIngestJob, jobs)
        return self._rate_left(self.lib.css_stream_ingest_host(self.h, tab, len(jobs)), left)

    def stream_append(self, jobs, operand):
        """launch_handoff_append_multi (css_stream_append_host); a job with st_out is a preview's.  -> ([{carry_out, tail_out, st,
        st_out, act_out, n_new, rows, row0}], operand as the launch left it)"""
        operand = np.ascontiguousarray(operand, dtype=np.float32).reshape(-1).copy()
        tab, keep, left = self._stream_kernel_table(CssStreamAppendJob, jobs)
        for d in tab:
            d.preview = int(bool(d.st_out.p))
        rc = self.lib.css_stream_append_host(self.h, tab, len(jobs), _np_ptr(operand), operand.size)
        for d, got in zip(tab, left):
            got["rows"], got["row0"] = int(d.rows), int(d.row0)
        return self._rate_left(rc, (left, operand))

    def stream_mel(self, S: int, spec, ld: int, jobs):
        """launch_handoff_mel_multi (css_stream_mel_host) on spec [402][ld] -> [{st, mel, ring, fmax, pvmax}]"""
        spec = np.ascontiguousarray(spec, dtype=np.float32).reshape(-1)
        tab, keep, left = self._stream_kernel_table(CssStreamMelJob, jobs)
        for d in tab:
            d.has_ring, d.has_pvmax = int(bool(d.ring.p)), int(bool(d.pvmax.p))
        return self._rate_left(self.lib.css_stream_mel_host(self.h, int(S), _np_ptr(spec), spec.size, int(ld), tab, len(jobs)), left)

    def stream_nemo_append(self, jobs, operand):
        """launch_nemo_append_multi (css_stream_nemo_append_host): ``stream_append``'s jobs with ``preemphasis``, ``xlast_in`` and
        ``xlast_out``, tails of y[160 J - 256, A).  -> ([{carry_out, tail_out, st, act_out, n_new, xlast_out, rows, row0}], operand)"""
        operand = np.ascontiguousarray(operand, dtype=np.float32).reshape(-1).copy()
        jobs = [dict(j) for j in jobs]
        pre = [float(j.pop("preemphasis", 0.0)) for j in jobs]
        tab, keep, left = self._stream_kernel_table(CssStreamNemoAppendJob, jobs, STREAM_NEMO_ARRAYS)
        for d, p in zip(tab, pre):
            d.preemphasis = p
        rc = self.lib.css_stream_nemo_append_host(self.h, tab, len(jobs), _np_ptr(operand), operand.size)
        for d, got in zip(tab, left):
            got["rows"], got["row0"] = int(d.rows), int(d.row0)
        return self._rate_left(rc, (left, operand))

    def stream_nemo_mel(self, S: int, spec, ld: int, jobs):
        """launch_nemo_mel_multi (css_stream_nemo_mel_host) on spec [514][ld] -> [{mel}]"""
        spec = np.ascontiguousarray(spec, dtype=np.float32).reshape(-1)
        tab, keep, left = self._stream_kernel_table(CssStreamNemoMelJob, jobs, STREAM_NEMO_ARRAYS)
        return self._rate_left(self.lib.css_stream_nemo_mel_host(self.h, int(S), _np_ptr(spec), spec.size, int(ld), tab, len(jobs)), left)

    # ---- the two kernel entries of include/css_mi355_nemo_chunk.h (tests/test_hip_nemo_chunk_kernels.py); jobs are dicts as above
    def stream_nemo_mel_history(self, S: int, spec, ld: int, jobs):
        """launch_nemo_mel_multi with a frame history (css_stream_nemo_mel_history_host): ``stream_nemo_mel``'s jobs with ``hist``,
        ``ring`` [S, n_mels, hist] and ``frames_after`` [S] (int64: the frame counts after the round) -> [{mel, ring}]"""
        spec = np.ascontiguousarray(spec, dtype=np.float32).reshape(-1)
        tab, keep, left = self._stream_kernel_table(CssStreamNemoMelHistoryJob, jobs, NEMO_CHUNK_ARRAYS)
        return self._rate_left(self.lib.css_stream_nemo_mel_history_host(self.h, int(S), _np_ptr(spec), spec.size, int(ld), tab, len(jobs)), left)

    def nemo_chunk_kernel(self, jobs):
        """launch_nemo_chunks per 32 jobs (css_nemo_chunk_host) on caller rings [n_mels, hist]: the descriptor's fields, with
        ``normalize`` and ``dtype`` as numbers; ``out`` is float32, or uint16 words of float16 with ``dtype`` 1 -> [{out, mean, std}]"""
        jobs = [dict(j) for j in jobs]
        pads = [float(j.pop("pad_value", 0.0)) for j in jobs]
        tab, keep, left = self._stream_kernel_table(CssNemoChunkJob, [dict(j, f16=int(int(j["dtype"]) == 1)) for j in jobs], NEMO_CHUNK_ARRAYS, skip=("f16",))
        for d, p in zip(tab, pads):
            d.pad_value = p
        return self._rate_left(self.lib.css_nemo_chunk_host(self.h, tab, len(jobs)), left)

    # ---- the window kernels and the queued sessions' hand-off kernels of csrc/handoff.hip on caller data
    #      (include/css_mi355_handoff_kernels.h; tests/test_hip_window_kernels.py).  A job is a dict as above; an array with an
    #      element offset field is the WHOLE allocation, the offset's elements in front included.
    def _handoff_kernel(self, entry, kind, job):
        tab, keep, left = self._stream_kernel_table(kind, [job], HANDOFF_KERNEL_ARRAYS)
        return tab, self._rate_left(entry(self.h, tab), left)[0]

    def session_scan(self, job):
        """launch_session_keep_scan (css_session_scan_host) -> {psum, regs, offs, st, n_new, n_ranges, ranges_out, n_frames_out,
        n_ranges_out}"""
        return self._handoff_kernel(self.lib.css_session_scan_host, CssSessionScanJob, job)[1]

    def session_gather(self, job):
        """launch_session_gather (css_session_gather_host) -> {operand}"""
        return self._handoff_kernel(self.lib.css_session_gather_host, CssSessionGatherJob, job)[1]

    def session_norm(self, job):
        """launch_session_norm (css_session_norm_host) -> {out}"""
        return self._handoff_kernel(self.lib.css_session_norm_host, CssSessionNormJob, job)[1]

    def session_windows(self, job):
        """launch_session_windows (css_session_windows_host); win / whole are float32, or uint16 words of float16 with f16
        -> {win, whole, n_windows_out, window_max_out, n_win_jobs, n_whole_jobs}"""
        job = dict(job, has_win=int(job.get("win") is not None), has_whole=int(job.get("whole") is not None))
        tab, keep, left = self._stream_kernel_table(CssSessionWindowsJob, [job], HANDOFF_KERNEL_ARRAYS)
        rc = self.lib.css_session_windows_host(self.h, tab)
        left[0]["n_win_jobs"], left[0]["n_whole_jobs"] = int(tab[0].n_win_jobs), int(tab[0].n_whole_jobs)
        return self._rate_left(rc, left)[0]

    def stream_windows(self, items, res):
        """launch_stream_windows per 32 items (css_stream_windows_host); res: WINDOW_OUT rows, item i takes row i
        -> ([{out}], res as the launches left it)"""
        res = np.array(res, dtype=WINDOW_OUT).reshape(-1)
        items = [dict(j, has_pv=int(j.get("pv") is not None)) for j in items]
        tab, keep, left = self._stream_kernel_table(CssStreamWindowJob, items, HANDOFF_KERNEL_ARRAYS)
        return self._rate_left(self.lib.css_stream_windows_host(self.h, tab, len(items), _np_ptr(res), res.size), (left, res))

    # ---- the kernels of csrc/mvdr.hip and csrc/stitch.hip on caller data (include/css_mi355_backend.h;
    #      tests/test_hip_backend_kernels.py).  Arrays are the WHOLE allocations (None where a form takes none); the arrays a form
    #      writes are copied first and returned as the launch left them.
    def mvdr_host(self, form: int, **kw):
        """launch_scm (0), launch_mvdr_solve (1), launch_mvdr_solve_multi (2; sets = (seg_lo, nseg, scm_off, bfw_off) each),
        launch_beamform (3), launch_segment_power_norm (4) (css_mvdr_host); fields are the descriptor's.  Returns the array the
        form writes: scm, bfw, sep, sep."""
        return self._mvdr_host(self.lib.css_mvdr_host, CssMvdrDesc, CssMvdrSet, form, **kw)

    def mvdr_array_host(self, form: int, **kw):
        """css_mvdr_array_host (include/css_mi355_array.h): forms 0 .. 3 of mvdr_host for C = 2 .. 8 microphones; scm is
        [segments][S + 1][F][C C], bfw [segments][S][F][C][2]."""
        if not 0 <= int(form) <= 3:
            raise ValueError("css_mvdr_array_host has the forms 0 .. 3")
        return self._mvdr_host(self.lib.css_mvdr_array_host, CssMvdrArrayDesc, CssMvdrArraySet, form, **kw)

    def _mvdr_host(self, entry, Desc, Set, form: int, *, X=None, masks=None, override=None, scm=None, bfw=None, sep=None, sets=(), **fields):
        X, masks, override = _flat(X), _flat(masks), _flat(override, np.uint8)
        scm, bfw, sep = _flat(scm, np.float64, form == 0), _flat(bfw, np.float64, form in (1, 2)), _flat(sep, np.float32, form >= 3)
        d = Desc(form=int(form), n_sets=len(sets), x_floats=_size(X), mask_floats=_size(masks), override_bytes=_size(override),
                 scm_doubles=_size(scm), bfw_doubles=_size(bfw), sep_floats=_size(sep),
                 **{k: (float(v) if k == "mask_floor" else int(v)) for k, v in fields.items()})
        for i, e in enumerate(sets):
            d.sets[i] = Set(*(int(v) for v in e))
        check(self.h, entry(self.h, C.byref(d), _ptr(X), _ptr(masks), _ptr(override), _ptr(scm), _ptr(bfw), _ptr(sep)))
        return (scm, bfw, bfw, sep, sep)[int(form)]

    def stitch_host(self, form: int, *, masks=None, sep=None, windows=None, costs=None, perms=None, mask_st=None, activity=None,
                    act_b=None, act_tmp=None, act_final=None, Y=None, sets=(), level=None, **fields):
        """launch_pit_costs (0), launch_pit_costs_multi (1; sets = (num_segments, mask_off, sep_off, costs_off) each),
        launch_pit_scan (2), launch_ola_masks (3), launch_morphology (4), launch_ola_stft (5) (css_stitch_host); fields are the
        descriptor's; level: None (absent) or the word.  Returns what the form writes: costs; costs; perms; (mask_st, activity,
        act_b); (act_tmp, act_final); Y."""
        masks, sep, windows = _flat(masks), _flat(sep), _flat(windows)
        costs, perms = _flat(costs, np.float64, form <= 1), _flat(perms, np.int32, form == 2)
        mask_st, activity, act_b = _flat(mask_st, copy=True), _flat(activity, copy=True), _flat(act_b, np.uint8, form == 3)
        act_tmp, act_final, Y = _flat(act_tmp, np.uint8, True), _flat(act_final, np.uint8, form == 4), _flat(Y, copy=True)
        acts = [a.size for a in (act_b, act_tmp, act_final) if a is not None]
        if len(set(acts)) > 1:
            raise ValueError("act_b, act_tmp and act_final have one length")
        if windows is not None and windows.size != 3 * int(fields["T"]):
            raise ValueError("windows [3][T]")
        d = CssStitchDesc(form=int(form), n_sets=len(sets), has_level=int(level is not None), level=int(level or 0),
                          mask_floats=_size(masks), sep_floats=_size(sep), costs_doubles=_size(costs), perms_ints=_size(perms),
                          mask_st_floats=_size(mask_st), activity_floats=_size(activity), act_bytes=acts[0] if acts else 0,
                          y_floats=_size(Y),
                          **{k: (float(v) if k == "activity_th" else int(v)) for k, v in fields.items()})
        for i, e in enumerate(sets):
            d.sets[i] = CssStitchSet(*(int(v) for v in e))
        check(self.h, self.lib.css_stitch_host(self.h, C.byref(d), _ptr(masks), _ptr(sep), _ptr(windows), _ptr(costs), _ptr(perms),
                                               _ptr(mask_st), _ptr(activity), _ptr(act_b), _ptr(act_tmp), _ptr(act_final), _ptr(Y)))
        return (costs, costs, perms, (mask_st, activity, act_b), (act_tmp, act_final), Y)[int(form)]

    # ---- RCCL through the C ABI (css_comm_*): what a host in another language would call
    def comm_init(self, unique_id: bytes, nranks: int, rank: int):
        assert len(unique_id) == COMM_ID_BYTES
        buf = C.create_string_buffer(bytes(unique_id), COMM_ID_BYTES)
        check(self.h, self.lib.css_comm_init(self.h, buf, int(nranks), int(rank)))

    def comm_destroy(self):
        check(self.h, self.lib.css_comm_destroy(self.h))

    def comm_info(self):
        n, r, d, v = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        check(self.h, self.lib.css_comm_info(self.h, C.byref(n), C.byref(r), C.byref(d), C.byref(v)))
        return {"nranks": n.value, "rank": r.value, "device": d.value, "rccl_version_code": v.value}

    def comm_all_gather(self, send_ptr: int, recv_ptr: int, bytes_per_rank: int):
        """device pointers; enqueued on the handle's stream"""
        check(self.h, self.lib.css_comm_all_gather(self.h, C.c_void_p(int(send_ptr)), C.c_void_p(int(recv_ptr)), int(bytes_per_rank)))

    def linear_mode(self):
        m = self.lib.css_get_linear_mode(self.h)
        if m < 0:
            check(self.h, m)
        return ("split_f16", "exact_f32")[m]

    def get_plan(self) -> CssPlan:
        p = CssPlan()
        check(self.h, self.lib.css_get_plan(self.h, C.byref(p)))
        return p

    # ---- stages
    def begin(self, pcm, n: int, c: int, cfg: RunCfg, device: bool = False):
        if device:
            ptr = C.c_void_p(int(pcm))
        else:
            self._pcm_keep = np.ascontiguousarray(pcm, dtype=np.float32)
            ptr = _np_ptr(self._pcm_keep)
        check(self.h, self.lib.css_begin(self.h, ptr, n, c, C.byref(cfg.c), int(device)))

    def begin_range(self, pcm: np.ndarray, n: int, c: int, cfg: RunCfg, s_lo: int, s_hi: int, slice_only: bool = False,
                    base_sample: Optional[int] = None):
        """Session over a host recording of n samples of which only samples [s_lo, s_hi) are uploaded (a rank's slice).
        slice_only: `pcm` holds just a slice starting at sample `base_sample` (default s_lo) of the recording (the library
        is handed the address sample 0 would have and never reads outside [s_lo, s_hi))."""
        assert pcm.dtype == np.float32 and pcm.flags.c_contiguous
        self._pcm_keep = pcm
        base = pcm.ctypes.data
        if slice_only:
            b0 = int(s_lo) if base_sample is None else int(base_sample)
            assert b0 <= s_lo and s_hi - b0 <= pcm.shape[0]
            base -= b0 * c * 4
        else:
            assert pcm.shape[0] == n
        check(self.h, self.lib.css_begin_range(self.h, C.c_void_p(base), n, c, C.byref(cfg.c), int(s_lo), int(s_hi)))

    def upload_range(self, pcm: np.ndarray, c: int, s_lo: int, s_hi: int, base_sample: int = 0):
        """Further samples [s_lo, s_hi) of the recording begin_range opened, asynchronously on the copy stream;
        `pcm[0]` is sample `base_sample` of the recording."""
        assert pcm.dtype == np.float32 and pcm.flags.c_contiguous and base_sample <= s_lo and s_hi - base_sample <= pcm.shape[0]
        base = pcm.ctypes.data - int(base_sample) * c * 4
        check(self.h, self.lib.css_upload_range(self.h, C.c_void_p(base), int(s_lo), int(s_hi)))

    def stage_stft(self):
        check(self.h, self.lib.css_stage_stft(self.h))

    def stage_stft_range(self, lo, hi):
        check(self.h, self.lib.css_stage_stft_range(self.h, lo, hi))

    def stage_stitch_masks(self, lo, hi):
        check(self.h, self.lib.css_stage_stitch_masks(self.h, lo, hi))

    def stage_stitch_gate(self, lo, hi):
        check(self.h, self.lib.css_stage_stitch_gate(self.h, lo, hi))

    def stage_istft_partial(self, lo, hi, shard_ptr: int, shard_ld: int):
        check(self.h, self.lib.css_stage_istft_partial(self.h, lo, hi, C.c_void_p(shard_ptr), shard_ld))

    def stage_synthesis(self, lo, hi):
        check(self.h, self.lib.css_stage_synthesis(self.h, lo, hi))

    def stage_seam_rows(self, lo, hi, rows_ptr: int, write: bool):
        check(self.h, self.lib.css_stage_seam_rows(self.h, lo, hi, C.c_void_p(rows_ptr), int(bool(write))))

    def stage_overlap_add(self, f_lo, f_hi, q_lo, q_hi, out_ptr: int, out_ld: int, out_q0: int):
        check(self.h, self.lib.css_stage_overlap_add(self.h, f_lo, f_hi, q_lo, q_hi, C.c_void_p(out_ptr), int(out_ld), int(out_q0)))

    def stage_join_shards(self, gathered_ptr: int, world: int, shard_ld: int, t_lo, t_hi, out_ptr: int, out_ld: int):
        lo = np.ascontiguousarray(t_lo, dtype=np.int64)
        hi = np.ascontiguousarray(t_hi, dtype=np.int64)
        check(self.h, self.lib.css_stage_join_shards(self.h, C.c_void_p(gathered_ptr), int(world), int(shard_ld), _np_ptr(lo), _np_ptr(hi),
                                                     C.c_void_p(out_ptr), int(out_ld)))

    def stage_masknet(self, lo, hi):
        check(self.h, self.lib.css_stage_masknet(self.h, lo, hi))

    def stage_mvdr(self, lo, hi):
        check(self.h, self.lib.css_stage_mvdr(self.h, lo, hi))

    def stage_pit_costs(self, lo, hi):
        check(self.h, self.lib.css_stage_pit_costs(self.h, lo, hi))

    def stage_pit_scan(self):
        check(self.h, self.lib.css_stage_pit_scan(self.h))

    def stage_stitch(self, lo, hi):
        check(self.h, self.lib.css_stage_stitch(self.h, lo, hi))

    def stage_istft(self, lo, hi):
        check(self.h, self.lib.css_stage_istft(self.h, lo, hi))

    def sync(self):
        check(self.h, self.lib.css_sync(self.h))

    # ---- separator protocol helpers
    def stft_host(self, pcm: np.ndarray) -> np.ndarray:
        """pcm [n, C] -> planes [C, 2F, T]."""
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        n, c = pcm.shape
        t = 0 if n < self.desc.frame_len else (n - self.desc.frame_len) // self.desc.frame_hop + 1
        out = np.zeros((c, 2 * self.desc.num_bins, t), dtype=np.float32)
        check(self.h, self.lib.css_stft_host(self.h, _np_ptr(pcm), n, c, _np_ptr(out), t))
        return out

    def separate_host(self, planes: np.ndarray, batch: int) -> np.ndarray:
        """planes [C, 2F, B*T] (B segments back to back) -> masks [(S+1)F, B*T]."""
        planes = np.ascontiguousarray(planes, dtype=np.float32)
        c, f2, tt = planes.shape
        assert c == self.desc.num_mics and f2 == 2 * self.desc.num_bins and tt % batch == 0
        out = np.empty(((self.desc.num_spks + self.desc.num_nois) * self.desc.num_bins, tt), dtype=np.float32)
        check(self.h, self.lib.css_separate_host(self.h, _np_ptr(planes), batch, tt // batch, _np_ptr(out)))
        return out

    def forward_host(self, pcm: np.ndarray) -> np.ndarray:
        """pcm [B, n, C] (equally long clips) -> masks [(S+1)F, B*T'], clip b in columns [b T', (b+1) T')."""
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        b, n, c = pcm.shape
        t = (n - self.desc.frame_len) // self.desc.frame_hop + 1
        out = np.empty(((self.desc.num_spks + self.desc.num_nois) * self.desc.num_bins, b * max(t, 0)), dtype=np.float32)
        check(self.h, self.lib.css_forward_host(self.h, _np_ptr(pcm), b, n, c, _np_ptr(out)))
        return out

    def handoff_logmel(self, wav_ptr: int, wav_ld: int, stream: int, n_mels: int = 80, pad_frames: int = 8,
                       drop_silence: bool = True, max_regions: int = 4096):
        """After run_device: (log-mel [n_mels, frames] of the stream's active regions, regions [n, 2] sample ranges)."""
        p = self.get_plan()
        cap = int(p.n_out) // 160 + 1
        mel = np.empty((n_mels, cap), dtype=np.float32)
        regions = np.zeros((max_regions, 2), dtype=np.int64)
        nfr, nreg = C.c_int64(), C.c_int32()
        flat = np.empty(n_mels * cap, dtype=np.float32)
        check(self.h, self.lib.css_handoff_logmel(self.h, C.c_void_p(wav_ptr), int(wav_ld), int(stream), int(n_mels), int(pad_frames),
                                                  int(bool(drop_silence)), _np_ptr(flat), cap, C.byref(nfr), _np_ptr(regions),
                                                  max_regions, C.byref(nreg)))
        del mel
        return flat[:n_mels * nfr.value].reshape(n_mels, nfr.value).copy(), regions[:nreg.value].copy()

    def _session_handoff(self, cfg: RunCfg, n: int, n_mels, pad_frames, drop_silence, pinned=True):
        hcfg = handoff_cfg(n_mels, pad_frames, drop_silence)
        frames, ranges = session_handoff_bounds(self.desc, cfg, hcfg, n)
        return hcfg, SessionHandoff(int(self.desc.num_spks), n_mels, frames, ranges, pinned=pinned)

    def handoff_logmel_all(self, wav_ptr: int, wav_ld: int, n_mels: int = 80, pad_frames: int = 8, drop_silence: bool = True,
                           out: Optional[SessionHandoff] = None) -> SessionHandoff:
        """After run_device: kept ranges and log-mel of ALL streams (css_handoff_logmel_all) -- per stream, bit for bit,
        what handoff_logmel returns, with the ranges found on the device.  `out`: a SessionHandoff to fill (any memory)."""
        hcfg = handoff_cfg(n_mels, pad_frames, drop_silence)
        if out is None:
            p = self.get_plan()
            TL = int(p.mix_frames)
            out = SessionHandoff(int(self.desc.num_spks), n_mels, int(p.n_out) // 160,
                                 (TL - 1) // (2 * int(pad_frames) + 3) + 1 if drop_silence else 1, pinned=False)
        check(self.h, self.lib.css_handoff_logmel_all(self.h, C.c_void_p(wav_ptr), int(wav_ld), C.byref(hcfg), C.byref(out.c)))
        return out

    def run_enqueue_handoff(self, pcm: np.ndarray, cfg: RunCfg, out: Optional[np.ndarray], n_mels: int = 80, pad_frames: int = 8,
                            drop_silence: bool = True, handoff: Optional[SessionHandoff] = None):
        """run_enqueue plus the hand-off to Whisper (css_run_enqueue_handoff): behind the session's waveforms, on the device,
        the kept ranges and the normalised log-mel of all streams.  `out` None: log-mel only, no waveform leaves the GPU.
        Returns (view of `out` or None, SessionHandoff); both are valid after wait() / wait_sessions().  Not in "split_f16"."""
        assert pcm.dtype == np.float32 and pcm.flags.c_contiguous and pcm.ndim == 2
        n, c = pcm.shape
        p = plan(self.desc, cfg, n)
        if out is not None:
            assert out.dtype == np.float32 and out.ndim == 2 and out.shape[0] == self.desc.num_spks and out.shape[1] >= p.n_out \
                and out.strides[1] == 4
        hcfg = handoff_cfg(n_mels, pad_frames, drop_silence)
        ho = handoff if handoff is not None else self._session_handoff(cfg, n, n_mels, pad_frames, drop_silence)[1]
        check(self.h, self.lib.css_run_enqueue_handoff(self.h, _np_ptr(pcm), n, c, C.byref(cfg.c), None if out is None else _np_ptr(out),
                                                       0 if out is None else out.strides[0] // 4, C.byref(hcfg), C.byref(ho.c)))
        self._queued_keep = getattr(self, "_queued_keep", []) + [(pcm, out, cfg, ho)]
        return (None if out is None else out[:, :p.n_out]), ho

    def run_enqueue_pcm16_handoff(self, planes, cfg: RunCfg, out16: np.ndarray, peaks: Optional[np.ndarray] = None, n_mels: int = 80,
                                  pad_frames: int = 8, drop_silence: bool = True, handoff: Optional[SessionHandoff] = None):
        """run_enqueue_pcm16 plus the hand-off (css_run_enqueue_pcm16_handoff): the log-mel is that of the float waveforms before
        peak normalisation, i.e. what handoff_logmel sees.  Returns (view of `out16`, SessionHandoff)."""
        n = planes[0].shape[0]
        for p in planes:
            assert p.dtype == np.int16 and p.ndim == 1 and p.shape[0] == n and p.flags.c_contiguous
        c = len(planes)
        pl = plan(self.desc, cfg, n)
        S = int(self.desc.num_spks)
        assert out16.dtype == np.int16 and out16.ndim == 2 and out16.shape[0] == S and out16.shape[1] >= pl.n_out and out16.strides[1] == 2
        assert peaks is None or (peaks.dtype == np.float32 and peaks.shape == (S,) and peaks.flags.c_contiguous)
        ptrs = (C.c_void_p * c)(*[p.ctypes.data for p in planes])
        hcfg = handoff_cfg(n_mels, pad_frames, drop_silence)
        ho = handoff if handoff is not None else self._session_handoff(cfg, n, n_mels, pad_frames, drop_silence)[1]
        check(self.h, self.lib.css_run_enqueue_pcm16_handoff(self.h, ptrs, n, c, C.byref(cfg.c), out16.ctypes.data_as(C.c_void_p),
                                                             out16.strides[0] // 2,
                                                             peaks.ctypes.data_as(C.c_void_p) if peaks is not None else None,
                                                             C.byref(hcfg), C.byref(ho.c)))
        self._queued_keep = getattr(self, "_queued_keep", []) + [(planes, out16, peaks, cfg, ho)]
        return out16[:, :pl.n_out], ho

    # ---- the hand-off to NeMo hosts (include/css_mi355_nemo_handoff.h) ----
    def _nemo_handoff(self, cfg: RunCfg, n: int, ncfg: CssNemoCfg, pinned=True):
        frames, ranges = nemo_handoff_bounds(self.desc, cfg, ncfg, n)
        return NemoHandoff(int(self.desc.num_spks), int(ncfg.n_mels), frames, ranges, pinned=pinned)

    def handoff_nemo_all(self, wav_ptr: int, wav_ld: int, n_mels: int = 80, pad_frames: int = 8, drop_silence: bool = True,
                         preemphasis: float = 0.97, normalize: bool = True, out: Optional[NemoHandoff] = None) -> NemoHandoff:
        """After run_device: kept ranges and NeMo log-mel features of ALL streams (css_handoff_nemo_all).  `out`: a NemoHandoff
        to fill (any memory)."""
        ncfg = nemo_cfg(n_mels, pad_frames, drop_silence, preemphasis, normalize)
        if out is None:
            p = self.get_plan()
            TL = int(p.mix_frames)
            out = NemoHandoff(int(self.desc.num_spks), n_mels, int(p.n_out) // 160,
                              (TL - 1) // (2 * int(pad_frames) + 3) + 1 if drop_silence else 1, pinned=False)
        check(self.h, self.lib.css_handoff_nemo_all(self.h, C.c_void_p(wav_ptr), int(wav_ld), C.byref(ncfg), C.byref(out.c)))
        return out

    def run_enqueue_nemo(self, pcm: np.ndarray, cfg: RunCfg, out: Optional[np.ndarray], n_mels: int = 80, pad_frames: int = 8,
                         drop_silence: bool = True, preemphasis: float = 0.97, normalize: bool = True,
                         handoff: Optional[NemoHandoff] = None):
        """run_enqueue plus the hand-off to a NeMo host (css_run_enqueue_nemo): behind the session's waveforms, on the device, the
        kept ranges and NeMo's log-mel features of all streams (``stream.nemo_features`` states them).  `out` None: features only,
        no waveform leaves the GPU.  Returns (view of `out` or None, NemoHandoff); both are valid after wait() /
        wait_sessions().  Not in "split_f16"."""
        assert pcm.dtype == np.float32 and pcm.flags.c_contiguous and pcm.ndim == 2
        n, c = pcm.shape
        p = plan(self.desc, cfg, n)
        if out is not None:
            assert out.dtype == np.float32 and out.ndim == 2 and out.shape[0] == self.desc.num_spks and out.shape[1] >= p.n_out \
                and out.strides[1] == 4
        ncfg = nemo_cfg(n_mels, pad_frames, drop_silence, preemphasis, normalize)
        ho = handoff if handoff is not None else self._nemo_handoff(cfg, n, ncfg)
        check(self.h, self.lib.css_run_enqueue_nemo(self.h, _np_ptr(pcm), n, c, C.byref(cfg.c), None if out is None else _np_ptr(out),
                                                    0 if out is None else out.strides[0] // 4, C.byref(ncfg), C.byref(ho.c)))
        self._queued_keep = getattr(self, "_queued_keep", []) + [(pcm, out, cfg, ho)]
        return (None if out is None else out[:, :p.n_out]), ho

    def run_enqueue_pcm16_nemo(self, planes, cfg: RunCfg, out16: Optional[np.ndarray], peaks: Optional[np.ndarray] = None,
                               n_mels: int = 80, pad_frames: int = 8, drop_silence: bool = True, preemphasis: float = 0.97,
                               normalize: bool = True, handoff: Optional[NemoHandoff] = None):
        """run_enqueue_pcm16 plus the hand-off to a NeMo host (css_run_enqueue_pcm16_nemo): the features are those of the float
        waveforms before peak normalisation.  `out16` None: features only.  Returns (view of `out16` or None, NemoHandoff)."""
        n = planes[0].shape[0]
        for p in planes:
            assert p.dtype == np.int16 and p.ndim == 1 and p.shape[0] == n and p.flags.c_contiguous
        c = len(planes)
        pl = plan(self.desc, cfg, n)
        S = int(self.desc.num_spks)
        if out16 is not None:
            assert out16.dtype == np.int16 and out16.ndim == 2 and out16.shape[0] == S and out16.shape[1] >= pl.n_out and out16.strides[1] == 2
        assert peaks is None or (peaks.dtype == np.float32 and peaks.shape == (S,) and peaks.flags.c_contiguous)
        ptrs = (C.c_void_p * c)(*[p.ctypes.data for p in planes])
        ncfg = nemo_cfg(n_mels, pad_frames, drop_silence, preemphasis, normalize)
        ho = handoff if handoff is not None else self._nemo_handoff(cfg, n, ncfg)
        check(self.h, self.lib.css_run_enqueue_pcm16_nemo(self.h, ptrs, n, c, C.byref(cfg.c),
                                                          None if out16 is None else out16.ctypes.data_as(C.c_void_p),
                                                          0 if out16 is None else out16.strides[0] // 2,
                                                          peaks.ctypes.data_as(C.c_void_p) if peaks is not None else None,
                                                          C.byref(ncfg), C.byref(ho.c)))
        self._queued_keep = getattr(self, "_queued_keep", []) + [(planes, out16, peaks, cfg, ho)]
        return (None if out16 is None else out16[:, :pl.n_out]), ho

    def nemo_kernels(self, job):
        """The kernels of csrc/nemo.hip on caller data (css_nemo_kernels_host): gather, the product, mel, statistics and
        normalisation as the path launches them.  A job is a dict of the descriptor's scalar fields and its arrays (the WHOLE
        allocations); the arrays the launches write are copied first -> {operand, raw, mean, stdv, out} as the launches left them."""
        j = dict(job)
        d = CssNemoKernelsJob()
        keep, left = [], {}
        for (name, dtype), out in [(f, False) for f in NEMO_KERNEL_ARRAYS[0]] + [(f, True) for f in NEMO_KERNEL_ARRAYS[1]]:
            a = j.pop(name, None)
            if a is None:
                continue
            a = np.ascontiguousarray(a, dtype=dtype).reshape(-1)
            a = a.copy() if out else a
            getattr(d, name).p, getattr(d, name).elems = a.ctypes.data, a.size
            keep.append(a)
            if out:
                left[name] = a
        for k, v in j.items():
            setattr(d, k, float(v) if k == "preemphasis" else int(v))
        return self._rate_left(self.lib.css_nemo_kernels_host(self.h, C.byref(d)), left)

    # ---- encoder windows of whole sessions (include/css_mi355_session_window.h) ----
    def session_window_bounds(self, cfg: RunCfg, n: int, width: int = 3000, stride: int = 3000, n_mels: int = 80, pad_frames: int = 8,
                              drop_silence: bool = True):
        """(frames, ranges, windows) per stream that suffice for a window session of `n` samples"""
        return session_window_bounds(self.desc, cfg, handoff_cfg(n_mels, pad_frames, drop_silence), width, stride, n)

    def _session_windows(self, frames, ranges, nw, hcfg, width, stride, dtype, mel_host, seek, handoff, windows, pinned=True,
                         torch_sync=True):
        """the hand-off arrays and the window description for the bounds (frames, ranges, nw), made where the caller gave none ->
        (SessionHandoff, the CssSessionHandoffOut to pass, SessionWindows).  mel_host False: the struct's mel_host is NULL (the
        SessionHandoff's mel_all is not written); seek: also the whole log-mel, frames + 3000 columns a row."""
        S = int(self.desc.num_spks)
        if handoff is None:
            handoff = SessionHandoff(S, hcfg.n_mels, frames if mel_host else 1, ranges, pinned=pinned)
        c = CssSessionHandoffOut(handoff.c.mel_host if mel_host else None, handoff.c.cap_frames if mel_host else 0,
                                 handoff.c.ranges_host, handoff.c.cap_ranges, handoff.c.n_frames, handoff.c.n_ranges)
        if windows is None:
            windows = SessionWindows(self.device, S, hcfg.n_mels, width, stride, dtype, cap_windows=nw, mel=bool(seek),
                                     mel_ld=frames + WINDOW_MAX_WIDTH, pinned=pinned)
        if torch_sync:
            import torch
            torch.cuda.current_stream(self.device).synchronize()   # the caller's tensors: nothing of torch's still writes them
        return handoff, c, windows

    def handoff_windows_all(self, wav_ptr: int, wav_ld: int, width: int = 3000, stride: int = 3000, dtype="float16", n_mels: int = 80,
                            pad_frames: int = 8, drop_silence: bool = True, mel_host: bool = True, seek: bool = False,
                            out: Optional[SessionHandoff] = None, windows: Optional[SessionWindows] = None):
        """After run_device: handoff_logmel_all plus the encoder windows on the device (css_handoff_windows_all) ->
        (SessionHandoff, SessionWindows).  mel_host False: no log-mel goes to the host (``mel_all`` is not written)."""
        hcfg = handoff_cfg(n_mels, pad_frames, drop_silence)
        p = self.get_plan()
        frames = int(p.n_out) // 160
        ranges = (int(p.mix_frames) - 1) // (2 * int(pad_frames) + 3) + 1 if drop_silence else 1
        ho, c, win = self._session_windows(frames, ranges, -(-frames // max(int(stride), 1)), hcfg, width, stride, dtype, mel_host, seek,
                                           out, windows, pinned=False)
        check(self.h, self.lib.css_handoff_windows_all(self.h, C.c_void_p(wav_ptr), int(wav_ld), C.byref(hcfg), C.byref(c), C.byref(win.c)))
        return ho, win

    def run_enqueue_windows(self, pcm: np.ndarray, cfg: RunCfg, out: Optional[np.ndarray], width: int = 3000, stride: int = 3000,
                            dtype="float16", n_mels: int = 80, pad_frames: int = 8, drop_silence: bool = True, mel_host: bool = True,
                            seek: bool = False, handoff: Optional[SessionHandoff] = None, windows: Optional[SessionWindows] = None,
                            torch_sync: bool = True):
        """run_enqueue_handoff plus the encoder windows, written on the device behind the session's log-mel
        (css_run_enqueue_windows).  Returns (view of `out` or None, SessionHandoff, SessionWindows), valid after wait() /
        wait_sessions().  mel_host False: no log-mel crosses PCIe; seek: also the whole padded log-mel (``windows.mel``).
        torch's current stream is synchronised before the enqueue, so that nothing of torch's still writes the tensors; on the
        legacy default stream that waits for the handle's main stream too (DESIGN.md section 7 N4 has the cost) -- a caller whose
        tensors are idle passes torch_sync=False."""
        assert pcm.dtype == np.float32 and pcm.flags.c_contiguous and pcm.ndim == 2
        n, c = pcm.shape
        p = plan(self.desc, cfg, n)
        if out is not None:
            assert out.dtype == np.float32 and out.ndim == 2 and out.shape[0] == self.desc.num_spks and out.shape[1] >= p.n_out \
                and out.strides[1] == 4
        hcfg = handoff_cfg(n_mels, pad_frames, drop_silence)
        ho, hc, win = self._session_windows(*session_window_bounds(self.desc, cfg, hcfg, width, stride, n), hcfg, width, stride, dtype,
                                            mel_host, seek, handoff, windows, torch_sync=torch_sync)
        check(self.h, self.lib.css_run_enqueue_windows(self.h, _np_ptr(pcm), n, c, C.byref(cfg.c), None if out is None else _np_ptr(out),
                                                       0 if out is None else out.strides[0] // 4, C.byref(hcfg), C.byref(hc),
                                                       C.byref(win.c)))
        self._queued_keep = getattr(self, "_queued_keep", []) + [(pcm, out, cfg, ho, win)]
        return (None if out is None else out[:, :p.n_out]), ho, win

    def run_enqueue_pcm16_windows(self, planes, cfg: RunCfg, out16: np.ndarray, peaks: Optional[np.ndarray] = None, width: int = 3000,
                                  stride: int = 3000, dtype="float16", n_mels: int = 80, pad_frames: int = 8, drop_silence: bool = True,
                                  mel_host: bool = True, seek: bool = False, handoff: Optional[SessionHandoff] = None,
                                  windows: Optional[SessionWindows] = None, torch_sync: bool = True):
        """run_enqueue_pcm16_handoff plus the encoder windows (css_run_enqueue_pcm16_windows): windows of the float waveforms
        before peak normalisation.  Returns (view of `out16`, SessionHandoff, SessionWindows)."""
        n = planes[0].shape[0]
        for p in planes:
            assert p.dtype == np.int16 and p.ndim == 1 and p.shape[0] == n and p.flags.c_contiguous
        c = len(planes)
        pl = plan(self.desc, cfg, n)
        S = int(self.desc.num_spks)
        assert out16.dtype == np.int16 and out16.ndim == 2 and out16.shape[0] == S and out16.shape[1] >= pl.n_out and out16.strides[1] == 2
        assert peaks is None or (peaks.dtype == np.float32 and peaks.shape == (S,) and peaks.flags.c_contiguous)
        ptrs = (C.c_void_p * c)(*[p.ctypes.data for p in planes])
        hcfg = handoff_cfg(n_mels, pad_frames, drop_silence)
        ho, hc, win = self._session_windows(*session_window_bounds(self.desc, cfg, hcfg, width, stride, n), hcfg, width, stride, dtype,
                                            mel_host, seek, handoff, windows, torch_sync=torch_sync)
        check(self.h, self.lib.css_run_enqueue_pcm16_windows(self.h, ptrs, n, c, C.byref(cfg.c), out16.ctypes.data_as(C.c_void_p),
                                                             out16.strides[0] // 2,
                                                             peaks.ctypes.data_as(C.c_void_p) if peaks is not None else None,
                                                             C.byref(hcfg), C.byref(hc), C.byref(win.c)))
        self._queued_keep = getattr(self, "_queued_keep", []) + [(planes, out16, peaks, cfg, ho, win)]
        return out16[:, :pl.n_out], ho, win

    def session_window_stats(self):
        """(launches of the window kernel, sessions that asked for windows) on this handle so far"""
        a, b = C.c_int64(), C.c_int64()
        check(self.h, self.lib.css_session_window_stats(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def resample(self, x, input_rate: int, fs: int = 16000) -> np.ndarray:
        """A recording at `input_rate` -> float32 [n_out, C] at `fs` on the device (css_resample_host): the samples a stream opened
        with ``input_rate`` forms from the same input, bit for bit -- scipy.signal.resample_poly's default filter in float32.
        `x`: float32 or int16, [n, C] or [n]; a C-contiguous array and the planar view ``planes.T`` are passed on as they are
        (stream.pcm16_layout's rule), anything else is copied once.  int16 samples count as q / 32768."""
        a = np.asarray(x)
        if a.dtype not in (np.int16, np.float32):
            a = a.astype(np.float32)
        if a.ndim == 1:
            a = a[:, None]
        if a.ndim != 2:
            raise ValueError(f"expected [n, C] or [n] samples, got {a.shape}")
        n, c = a.shape
        up, down = rate_ratio(input_rate, fs)
        el = a.dtype.itemsize
        if a.flags.c_contiguous and a.flags.aligned:
            ss, cs = c, 1
        elif n >= 1 and a.flags.aligned and (n == 1 or a.strides[0] == el) and a.strides[1] % el == 0 and a.strides[1] // el >= n:
            ss, cs = 1, a.strides[1] // el
        else:
            a, ss, cs = np.ascontiguousarray(a), c, 1
        m = stream_rate_samples(up, down, n, True)
        out = np.empty((m, c), np.float32)
        n_out = C.c_int64()
        check(self.h, self.lib.css_resample_host(self.h, C.c_void_p(a.ctypes.data), int(a.dtype == np.int16), n, c, ss, cs, up, down,
                                                 _np_ptr(out), m, C.byref(n_out)))
        assert n_out.value == m
        return out

    def stream_output_stats(self):
        """(launches of the output kernel, rounds with a stream that has an output format) of the last push / finish on this handle"""
        a, b = C.c_int32(), C.c_int32()
        check(self.h, self.lib.css_stream_output_stats(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def stream_handoff_stats(self):
        """(hand-off launches, DFT products among them, operand frames) of the last stream call on this handle"""
        a, b, c = C.c_int32(), C.c_int32(), C.c_int64()
        check(self.h, self.lib.css_stream_handoff_stats(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def validation_loss(self, mix: np.ndarray, gt_spk0: np.ndarray, gt_noise0: np.ndarray, loss_name: str = "masked_mag",
                        base_loss: str = "mse", clip_gt_to_mixture: bool = False, noise_weight: float = 1.0):
        """train.py:411 _calc_loss for a validation batch: mix [B, n, C], gt_spk0 [B, S, n], gt_noise0 [B, n] (ground
        truths at microphone 0) -> (loss, spk_loss [B], noise_loss [B], perms [B, S])."""
        mix = np.ascontiguousarray(mix, dtype=np.float32)
        gs = np.ascontiguousarray(gt_spk0, dtype=np.float32)
        gn = np.ascontiguousarray(gt_noise0, dtype=np.float32)
        b, n, c = mix.shape
        s = int(self.desc.num_spks)
        assert gs.shape == (b, s, n) and gn.shape == (b, n)
        spk, noi = np.empty(b, np.float32), np.empty(b, np.float32)
        perms = np.empty((b, s), np.int32)
        loss = C.c_float()
        check(self.h, self.lib.css_validation_loss_host(
            self.h, _np_ptr(mix), _np_ptr(gs), _np_ptr(gn), b, n, c, {"masked_mag": 0, "mask": 1}[loss_name],
            {"l1": 0, "mse": 1}[base_loss], int(bool(clip_gt_to_mixture)), float(noise_weight), _np_ptr(spk), _np_ptr(noi),
            _np_ptr(perms), C.byref(loss)))
        return float(loss.value), spk, noi, perms

    def istft_host(self, planes: np.ndarray) -> np.ndarray:
        """planes [B, 2F, T] -> wav [B, (T-1)*hop + frame_len]."""
        planes = np.ascontiguousarray(planes, dtype=np.float32)
        b, _, t = planes.shape
        out = np.empty((b, (t - 1) * self.desc.frame_hop + self.desc.frame_len), dtype=np.float32)
        check(self.h, self.lib.css_istft_host(self.h, _np_ptr(planes), b, t, _np_ptr(out)))
        return out

    # ---- buffers
    def buffer_dims(self, which: int):
        dims = (C.c_int64 * 4)()
        el = C.c_int32()
        check(self.h, self.lib.css_buffer_dims(self.h, which, dims, C.byref(el)))
        shape = [int(x) for x in dims]
        rank = {BUF_X: 3, BUF_SCM: 4, BUF_BFW: 4, BUF_SEP: 4, BUF_MASK_ST: 3, BUF_Y: 3, BUF_WTA_OVERRIDE: 3, BUF_LEVEL: 1}.get(which, 2)
        return tuple(shape[:rank]), int(el.value)

    def read(self, which: int) -> np.ndarray:
        dims, el = self.buffer_dims(which)
        dt = _BUF_DTYPES.get(which, np.float32)
        out = np.empty(dims, dtype=dt)
        assert out.itemsize == el
        check(self.h, self.lib.css_read_buffer(self.h, which, _np_ptr(out), out.nbytes))
        return out

    def write(self, which: int, arr: np.ndarray):
        dims, el = self.buffer_dims(which)
        dt = _BUF_DTYPES.get(which, np.float32)
        arr = np.ascontiguousarray(arr, dtype=dt)
        assert arr.size == int(np.prod(dims)), (arr.shape, dims)
        check(self.h, self.lib.css_write_buffer(self.h, which, _np_ptr(arr), arr.nbytes))

    def devptr(self, which: int) -> int:
        p = C.c_void_p()
        check(self.h, self.lib.css_buffer_devptr(self.h, which, C.byref(p)))
        return int(p.value or 0)
