/* css_mi355_nemo_handoff.h -- the hand-off to NeMo-family consumers for whole sessions: kept ranges and NeMo log-mel features of
 * ALL separated streams, found and computed on the device behind a session's waveforms.
 *
 * An addition to css_mi355.h (included below; same library, same conventions).  The hand-off of css_mi355_session_handoff.h makes
 * Whisper's features; NeMo's speaker, VAD and recogniser models (TitaNet, MarbleNet, Conformer-CTC, Parakeet, Canary,
 * FastConformer) take another definition, the one of NeMo's AudioToMelSpectrogramPreprocessor, whose arithmetic is published as
 * ParakeetFeatureExtractor in transformers.  The calls here run it with no host decision between the kernels: the gate bytes are
 * scanned into the run table and the counts (the same kernel, the same rule and the same ranges as in
 * css_mi355_session_handoff.h), then gather, one exact float32 product, mel, statistics, normalisation.
 *
 * The definition, per separated stream k with x = the concatenation of its kept ranges (drop_silence == 0: the whole stream):
 *   1. pre-emphasis: y[0] = x[0], y[c] = x[c] - p x[c - 1] over the concatenation -- across a range seam x[c - 1] is the last
 *      sample of the range before; product and difference are rounded separately in float32 (no FMA); p == 0: y = x;
 *   2. framing: 256 zeros before and behind y; frame j is padded samples [160 j, 160 j + 512);
 *   3. window: zero on [0, 56) and [456, 512), 0.5 - 0.5 cos(2 pi n / 399) at offset 56 + n (symmetric 400-point Hann);
 *   4. a 512-point DFT, 257 bins;
 *   5. n_frames = len(x) / 160 (the one frame more that torch.stft produces is not computed: NeMo masks it);
 *   6. power re^2 + im^2, then the slaney mel bank [n_mels][257] (0 .. 8 kHz, slaney normalisation);
 *   7. ln(mel + 2^-24) in float32 -- no floor;
 *   8. with normalize: per band mean = sum / L and std = sqrt(sum (v - mean)^2 / (L - 1)) over the L = n_frames valid frames
 *      (float64 sums in a fixed order, each rounded to float32 once), then (v - mean) / (std + 1e-5).  For L == 1 the
 *      definition's std is NaN and is taken as 0 here, as NeMo does to a NaN std; for L == 0 nothing is written.
 *      normalize == 0: the raw ln values (a diarizer host normalises per embedding window itself: NeMo's speaker models
 *      normalise per segment).
 *
 * Frames of 512 samples at hop 256 only.  Streamed sessions: css_mi355_stream_nemo.h.  Out of scope: encoder-style windows, float16 output, rate
 * sessions, other frame geometries, CSS_LINEAR_SPLIT_F16 (CSS_ERR_STATE), and NeMo's pad_to / dither, which are host and
 * training concerns.  A session has one format, Whisper's or this one, not both. */
#ifndef CSS_MI355_NEMO_HANDOFF_H
#define CSS_MI355_NEMO_HANDOFF_H

#include "css_mi355.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

/* n_mels: 80 or 128.  pad_frames (0 .. 4096) and drop_silence (0 / 1): the range rule's.  preemphasis: finite, 0 <= p < 1, 0 = none
 * (NeMo's default is 0.97).  normalize: 1 = per band over the stream's valid frames, 0 = raw ln values. */
typedef struct CssNemoCfg {
    int32_t n_mels;
    int32_t pad_frames;
    int32_t drop_silence;
    float preemphasis;
    int32_t normalize;
} CssNemoCfg;

/* Caller-owned.  The queued forms need every array page-locked (css_host_alloc): the kernels store into them.  Speaker k's
 * results: mel_host[(k n_mels + m) cap_frames + j] for j < n_frames[k], ranges_host[(k cap_ranges + r) 2 + {0, 1}] for
 * r < n_ranges[k], and -- where they are not NULL, with either value of normalize, for speakers with n_frames[k] >= 1 --
 * mean_host[k n_mels + m] and std_host[k n_mels + m] of the raw ln values; nothing else of the arrays is written.  Capacities of
 * at least css_nemo_handoff_bounds cannot overflow. */
typedef struct CssNemoOut {
    float* mel_host;
    int64_t cap_frames;
    int64_t* ranges_host;
    int32_t cap_ranges;
    int64_t* n_frames;
    int32_t* n_ranges;
    float* mean_host;
    float* std_host;
} CssNemoOut;

/* Pure host arithmetic: frames = n_out / 160; ranges = (TL - 1) / (2 pad_frames + 3) + 1 (1 with drop_silence == 0), TL =
 * CssPlan.mix_frames, n_out = (TL + 1) 256 -- the counts of css_mi355_session_handoff.h's bounds. */
int css_nemo_handoff_bounds(const CssModelDesc* desc, const CssRunCfg* cfg, const CssNemoCfg* ncfg, int64_t n_samples,
                            int64_t* frames, int32_t* ranges);

/* Synchronous, after a finished pass on the handle (css_run_device): all S streams of wav_dev [S][wav_ld] on the handle's
 * stream, one synchronise at the end.  Pageable arrays are allowed. */
int css_handoff_nemo_all(css_handle_t h, const float* wav_dev, int64_t wav_ld, const CssNemoCfg* ncfg, CssNemoOut* out);

/* css_run_enqueue / css_run_enqueue_pcm16 plus this hand-off.  The waveforms keep their bits and lifetime rules; wav_host /
 * wav_pcm16_host may be NULL (features only; cap is then unused).  The arrays of `out` are valid once css_wait or
 * css_wait_sessions has returned for the session.  The PCM16 form hands off the float waveforms before peak normalisation.  Such
 * a session shares estimator batches and queue groups with every other kind of queued session.  Refused at the call, with nothing
 * allocated, queued or written: CSS_ERR_INVALID_ARG for capacities below the bounds, arrays that are not page-locked, n_mels
 * other than 80 / 128, pad_frames outside 0 .. 4096, a preemphasis that is not finite, negative or >= 1, frames other than
 * 512 / 256; CSS_ERR_STATE in CSS_LINEAR_SPLIT_F16. */
int css_run_enqueue_nemo(css_handle_t h, const float* pcm_host, int64_t n_samples, int32_t n_ch, const CssRunCfg* cfg,
                         float* wav_host, int64_t cap, const CssNemoCfg* ncfg, CssNemoOut* out);
int css_run_enqueue_pcm16_nemo(css_handle_t h, const int16_t* const* planes_host, int64_t n_samples, int32_t n_ch,
                               const CssRunCfg* cfg, int16_t* wav_pcm16_host, int64_t cap, float* peaks_host,
                               const CssNemoCfg* ncfg, CssNemoOut* out);

/* ---- the kernels of csrc/nemo.hip on caller data (unit tests of the kernels; not on the hot path): gather, the product, mel,
 * statistics and normalisation exactly as the path launches them, behind a run table the caller gives.  Every array is staged at
 * a 256-byte boundary with 256 bytes of room on both sides, uploaded whole and -- the outputs -- downloaded whole.
 * In: wav [S][wav_ld] float32 behind wav_off (0 .. 3) floats; the run table as the keep-scan leaves it: regs [S][cap_ranges][2]
 * int64 sample ranges, offs [S][cap_ranges] int64 samples before each run, st [S] rows {int64 A, int64 J, int32, int32} (kept
 * samples, frames), n_ranges [S] int32.  Speaker k has `rows` operand rows of 160 floats; the path's rows = n_out / 160 + 4.
 * Out, whole: operand, exactly S rows 160 + 512 floats; raw [S][n_mels][raw_ld], the ln values; mean and stdv [S][n_mels]; out
 * [S][n_mels][out_ld], the normalised rows (normalize == 0: the raw ones) of the frames below J.
 * Refused with CSS_ERR_INVALID_ARG and a message before anything is launched or written: a NULL handle, job or array, an array
 * shorter than its description, S outside 1 .. 4, rows outside 4 .. 2^20, cap_ranges < 1, n_mels other than 80 / 128, a
 * preemphasis as above, raw_ld < rows - 4, out_ld < 0, st[k].A < 0, st[k].J outside 0 .. rows - 4 or above (A + 352) / 160 (a frame
 * that reads past the zeros the gather writes), n_ranges[k] < 0, an offs row that is not monotone, and a table under which the
 * gather would read outside speaker k's wav row. */
typedef struct CssNemoArray { void* p; int64_t elems; } CssNemoArray;
typedef struct CssNemoKernelsJob {
    int32_t S, n_mels, normalize, cap_ranges, wav_off;
    float preemphasis;
    int64_t wav_ld, rows, raw_ld, out_ld;
    CssNemoArray wav, regs, offs, st, n_ranges, operand, raw, mean, stdv, out;
} CssNemoKernelsJob;
int css_nemo_kernels_host(css_handle_t h, CssNemoKernelsJob* job);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif

#endif /* CSS_MI355_NEMO_HANDOFF_H */
