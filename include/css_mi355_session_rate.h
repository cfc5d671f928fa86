/* css_mi355_session_rate.h -- whole recordings at the capture rate: both wav edges of a session resampled on the device.
 *
 * An addition to css_mi355.h and css_mi355_rate.h (included below; same library, same conventions).  css_run, css_run_pcm16 and
 * the queue take the recording's rate for the model's.  The calls below take a recording at the capture rate (48, 44.1, 32, 24,
 * 22.05, 8, 96 kHz against the 16 kHz model), cross PCIe with the samples as they were captured, and form the model-rate samples
 * in the session's slot of the sample buffer with one kernel launch for all rate sessions of a queue group; on the way out the
 * separated streams may be resampled to a playback rate, and -- for PCM16 output -- peak-normalised and encoded at that rate.
 *
 * Definition (what the tests hold the calls to, bit for bit):
 *   x16 = css_resample_host(input)               float32 [n_model][C]; int16 samples enter as q * 2^-15
 *   w   = css_run(x16, cfg)                      [S][n_out_model]
 *   y   = w                                      when out_up / out_down is 1 / 1, else
 *         css_resample_host of w's S rows as S planar channels at out_up / out_down      [S][n_out]
 *   PCM16 output: per stream  peak = max |y|,  z = y * 0.99 / (peak + 1e-7) in float32,  int16(clip(rint((double)z * 32767)));
 *   peaks_host[k] = that peak (of the samples at the output rate, before normalisation).
 * Accepted ratios on either side: those of css_mi355_rate.h, and 1 / 1 (no change on that side).
 */
#ifndef CSS_MI355_SESSION_RATE_H
#define CSS_MI355_SESSION_RATE_H

#include "css_mi355_rate.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef struct CssSessionRate {
    int32_t in_up, in_down;    /* model rate = capture rate * in_up / in_down, lowest terms; 1 / 1 = no change at the input  */
    int32_t out_up, out_down;  /* output rate = model rate * out_up / out_down;              1 / 1 = outputs at the model rate */
} CssSessionRate;

/* Pure host arithmetic, no GPU: the three counts of a recording of n_in capture-rate samples.
 *   n_model     = ceil(n_in in_up / in_down)            (css_stream_rate_samples, finished = 1; n_in itself at 1 / 1)
 *   n_out_model = css_plan's n_out for n_model samples
 *   n_out       = ceil(n_out_model out_up / out_down)   (n_out_model itself at 1 / 1)
 * CSS_ERR_INVALID_ARG (and no word written) for a null pointer, a ratio outside the rule, n_in < 1 or n_in > 2^40, or a
 * configuration css_plan refuses for n_model samples. */
int css_session_rate_samples(const CssModelDesc* desc, const CssRunCfg* cfg, const CssSessionRate* rate, int64_t n_in,
                             int64_t* n_model, int64_t* n_out_model, int64_t* n_out);

/* css_run of a recording at the capture rate: pcm_host [n_in][n_ch] float32 -> wav_host [S][cap] float32 at the output rate
 * (n_out samples per stream, cap >= n_out).  Synchronous.
 * Refused with CSS_ERR_INVALID_ARG before anything is allocated, uploaded or queued: a ratio outside the rule or one whose tile
 * does not fit a workgroup's LDS, n_in < 1 or n_in > 2^40, cap < n_out, a null pointer.  Whatever css_run refuses for n_model
 * samples is refused with css_run's status.  CSS_ERR_STATE in CSS_LINEAR_SPLIT_F16: css_wait may repeat a session from its
 * input buffers, a rate session cannot be repeated. */
int css_run_rate(css_handle_t h, const float* pcm_host, int64_t n_in, int32_t n_ch, const CssRunCfg* cfg,
                 const CssSessionRate* rate, float* wav_host, int64_t cap);

/* css_run_pcm16 of a recording at the capture rate: n_ch mono PCM16 planes of n_in samples -> wav_pcm16_host [S][cap] int16 at
 * the output rate, peak-normalised per stream at that rate; peaks_host (may be NULL) [S].  Synchronous; refusals as above, and a
 * null plane is CSS_ERR_INVALID_ARG. */
int css_run_pcm16_rate(css_handle_t h, const int16_t* const* planes_host, int64_t n_in, int32_t n_ch, const CssRunCfg* cfg,
                       const CssSessionRate* rate, int16_t* wav_pcm16_host, int64_t cap, float* peaks_host);

/* The queued forms: the lifetime rules of css_run_enqueue / css_run_enqueue_pcm16 (inputs valid and outputs untouched until
 * css_wait), the same grouping rule (same segmentation and windows, page-locked output), one queue: rate sessions, plain PCM16
 * sessions and float sessions may alternate and share one estimator batch.  All rate sessions of a group are converted by ONE
 * launch of the ingest kernel, which also writes each recording's level; a session with an output ratio keeps its waveforms in
 * device memory and leaves through the output kernel on the stream its tail runs on.  Frame geometries other than 512 / 256 run
 * to their end inside the call, as css_run_enqueue_pcm16 does. */
int css_run_enqueue_rate(css_handle_t h, const float* pcm_host, int64_t n_in, int32_t n_ch, const CssRunCfg* cfg,
                         const CssSessionRate* rate, float* wav_host, int64_t cap);
int css_run_enqueue_pcm16_rate(css_handle_t h, const int16_t* const* planes_host, int64_t n_in, int32_t n_ch, const CssRunCfg* cfg,
                               const CssSessionRate* rate, int16_t* wav_pcm16_host, int64_t cap, float* peaks_host);

/* Running counts on this handle since css_create: launches of the ingest kernel, launches of the output kernel, rate sessions
 * put on the streams.  CSS_ERR_INVALID_ARG for a null handle or pointer. */
int css_session_rate_stats(css_handle_t h, int64_t* ingest_launches, int64_t* output_launches, int64_t* sessions);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CSS_MI355_SESSION_RATE_H */
