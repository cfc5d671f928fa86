/* css_mi355_session_handoff.h -- the hand-off to Whisper for whole sessions: kept ranges and log-mel of ALL separated streams,
 * found and computed on the device behind a session's waveforms.
 *
 * An addition to css_mi355.h (included below; same library, same conventions).  css_handoff_logmel hands off one stream per
 * call and decides the ranges on the host in the middle, so a queued session (css_run_enqueue) could not use it.  The calls
 * here run five kernels with no host decision between them: the gate bytes are scanned into the run table and the counts on
 * the device, the kept samples of all S streams are gathered, one exact float32 product gives the spectra, then mel and
 * Whisper's normalisation.  The values are, bit for bit, css_handoff_logmel's for every stream: mel [n_mels][n_frames],
 * ranges [n_ranges][2], n_frames, n_ranges.
 *
 * Frames of 512 samples at hop 256 only.  With TL = CssPlan.mix_frames a stream has n_out = (TL + 1) 256 samples, blocks
 * q = 0 .. TL of 256 samples.  Block q is kept iff drop_silence == 0 or a frame t of [max(q - pad_frames - 1, 0),
 * min(q + pad_frames, TL - 1)] is active; ranges are the maximal runs of kept blocks times 256 -- the time map from the
 * concatenation back to the meeting: concatenated sample c lies in range r iff off_r <= c < off_r + (end_r - start_r), with
 * off_r the lengths of the ranges before r, and is meeting sample start_r + c - off_r.  n_frames = (256 kept blocks) / 160.
 *
 * Not covered: CSS_LINEAR_SPLIT_F16 (css_wait may repeat such sessions; CSS_ERR_STATE), other frame geometries, float16
 * log-mel, encoder windows. */
#ifndef CSS_MI355_SESSION_HANDOFF_H
#define CSS_MI355_SESSION_HANDOFF_H

#include "css_mi355.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

/* Caller-owned.  The queued forms need every array page-locked (css_host_alloc): the kernels store into them.  Speaker k's
 * results: mel_host[(k n_mels + m) cap_frames + j] for j < n_frames[k], ranges_host[(k cap_ranges + r) 2 + {0, 1}] for
 * r < n_ranges[k]; nothing else of the arrays is written.  Capacities of at least css_session_handoff_bounds cannot overflow. */
typedef struct CssSessionHandoffOut {
    float* mel_host;
    int64_t cap_frames;
    int64_t* ranges_host;
    int32_t cap_ranges;
    int64_t* n_frames;
    int32_t* n_ranges;
} CssSessionHandoffOut;

/* Scan step of the keep-scan kernel, in gate frames and in sample blocks (the sizes around it are where that kernel carries). */
#define CSS_SESSION_SCAN_CHUNK 1024

/* Pure host arithmetic: frames = n_out / 160; ranges = (TL - 1) / (2 pad_frames + 3) + 1 (1 with drop_silence == 0), which the
 * pattern "one active frame every 2 pad_frames + 3 frames from frame 0" attains. */
int css_session_handoff_bounds(const CssModelDesc* desc, const CssRunCfg* cfg, const CssStreamHandoffCfg* hcfg, int64_t n_samples,
                               int64_t* frames, int32_t* ranges);

/* Synchronous, after a finished pass on the handle (css_run_device; the state css_handoff_logmel needs): all S streams of
 * wav_dev [S][wav_ld] on the handle's stream, one synchronise at the end.  Pageable arrays are allowed. */
int css_handoff_logmel_all(css_handle_t h, const float* wav_dev, int64_t wav_ld, const CssStreamHandoffCfg* hcfg,
                           CssSessionHandoffOut* out);

/* css_run_enqueue / css_run_enqueue_pcm16 plus the hand-off.  The waveforms keep their bits and lifetime rules; wav_host may be
 * NULL (log-mel only; cap is then unused).  The hand-off arrays are valid once css_wait or css_wait_sessions has returned for
 * the session.  The PCM16 form hands off the float waveforms before peak normalisation.  Refused at the call, with nothing
 * queued and nothing written: CSS_ERR_INVALID_ARG for capacities below the bounds, arrays that are not page-locked, n_mels
 * other than 80 / 128, pad_frames outside 0 .. 4096, frames other than 512 / 256; CSS_ERR_STATE in CSS_LINEAR_SPLIT_F16. */
int css_run_enqueue_handoff(css_handle_t h, const float* pcm_host, int64_t n_samples, int32_t n_ch, const CssRunCfg* cfg,
                            float* wav_host, int64_t cap, const CssStreamHandoffCfg* hcfg, CssSessionHandoffOut* out);
int css_run_enqueue_pcm16_handoff(css_handle_t h, const int16_t* const* planes_host, int64_t n_samples, int32_t n_ch,
                                  const CssRunCfg* cfg, int16_t* wav_pcm16_host, int64_t cap, float* peaks_host,
                                  const CssStreamHandoffCfg* hcfg, CssSessionHandoffOut* out);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif

#endif /* CSS_MI355_SESSION_HANDOFF_H */
