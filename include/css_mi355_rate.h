/* css_mi355_rate.h -- pushes at the capture rate: the rate conversion of a stream's ingest and of whole recordings.
 *
 * An addition to css_mi355.h (included below; same library, same conventions).  The mask estimator is a 16 kHz model; capture
 * devices, WebRTC decoders and USB arrays deliver 48 kHz, sometimes 44.1, 32 or 8 kHz.  A stream that was given a rate ratio
 * takes its pushes at the capture rate: the samples cross PCIe as they were captured (int16 or float32) and one kernel launch
 * per round filters, decimates and de-interleaves them into the windows of all rate streams of the round.  Everything behind
 * the window is the stream it was: all counts of CssStreamInfo, the finality rule, max_lag, the hand-off and every refusal are
 * in model-rate samples, evaluated on the model-rate samples the inputs make available (css_stream_rate_samples).
 *
 * The conversion is scipy.signal.resample_poly(x, up, down, padtype='constant') with its default filter.  For the ratio
 * up / down in lowest terms (output rate = input rate * up / down: 48 kHz -> 16 kHz is 1 / 3, 44.1 kHz -> 16 kHz 160 / 441,
 * 8 kHz -> 16 kHz 2 / 1):
 *   half = 10 max(up, down),  L = 2 half + 1
 *   h    = up * firwin(L, 1 / max(up, down), window=('kaiser', 5.0))      computed in float64 on the host (I0 by its power
 *          series), rounded to float32 once; css_resample_taps returns exactly the taps the device uses
 *   y[m] = sum_i x[i] h[half + m down - i up]   over 0 <= half + m down - i up <= 2 half,   x[i] = 0 outside [0, n_in)
 *   a recording of n_in samples gives ceil(n_in up / down) samples
 * int16 samples enter as (float)q * 2^-15 (exact, the PCM16 push's scaling).  One output sample is one float32 fmaf chain over
 * its taps in ascending i from 0.0f, so its bits do not depend on where pushes were cut, and css_resample_host of a whole
 * recording gives the samples a stream forms from it, bit for bit.
 * Accepted ratios: up != down, gcd(up, down) = 1, ceil(L / up) <= 128 taps per output sample, L <= 16384; everything else is
 * CSS_ERR_INVALID_ARG.  (96, 48, 44.1, 32, 24, 22.05 and 8 kHz against 16 kHz are covered; 1 / 7 is not.)
 */
#ifndef CSS_MI355_RATE_H
#define CSS_MI355_RATE_H

#include "css_mi355.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

/* Gives an open stream its rate ratio: after css_stream_open (and css_stream_handoff_open, in either order) and before the
 * stream's first sample; later, or a second time, is CSS_ERR_STATE, a ratio outside the rule above CSS_ERR_INVALID_ARG, and on
 * any refusal the stream stays as it was.  From then on n_samples of css_stream_push(_many)(_pcm16) counts INPUT samples (for
 * the PCM16 layouts too: planar needs channel_stride >= n_samples input samples), float and PCM16 pushes may alternate across
 * calls, and items with and without a rate may share a grouped call.  After n_in input samples css_stream_rate_samples(up,
 * down, n_in, 0) model-rate samples have entered the window (CssStreamInfo.n_pushed), which is what the finality rule, the
 * capacity check, the zero-weight check and the hand-off bounds of a call are evaluated on; the resampler's own lag is half / up
 * input samples (30 samples, 0.6 ms, at 48 kHz).  css_stream_finish first completes the count to ceil(n_in up / down) with
 * zeros past the end, then finishes as before: what a finished stream returned is css_run of css_resample_host of the
 * recording, bit for bit.
 * Device memory, allocated here and counted in CssStreamInfo.device_bytes from here on: staging for one piece of input as
 * float32, two generations of the carried inputs (ceil(2 half / up) + 1 per channel) and the taps.  A stream without a rate
 * allocates and reports what it did. */
int css_stream_set_rate(css_handle_t h, int32_t id, int32_t up, int32_t down);

/* Pure host arithmetic, no GPU: model-rate samples after n_in input samples at the ratio up / down.
 *   finished = 0   those computable while the stream is open: max(0, ceil((n_in up - half) / down))
 *   finished = 1   those of the whole recording:              ceil(n_in up / down)
 * CSS_ERR_INVALID_ARG for a ratio outside the rule, n_in < 0 or a null pointer. */
int css_stream_rate_samples(int32_t up, int32_t down, int64_t n_in, int32_t finished, int64_t* n_model);

/* Pure host arithmetic, no GPU: the L float32 taps of the ratio into taps[cap].  *n_taps = L whenever the ratio is accepted;
 * a capacity below L (or taps == NULL) is CSS_ERR_INVALID_ARG and writes no tap. */
int css_resample_taps(int32_t up, int32_t down, float* taps, int32_t cap, int32_t* n_taps);

/* A whole recording host -> device -> host on the handle's stream: src is int16 (is_int16 != 0) or float32 samples, sample i
 * of channel c at src[i * sample_stride + c * channel_stride] (strides in elements of that type) in one of the PCM16 push's two
 * layouts -- interleaved (sample_stride == n_ch, channel_stride == 1) or planar (sample_stride == 1, channel_stride >= n_in).
 * out_host receives [n_out][n_ch] float32, css_run's input layout, *n_out = ceil(n_in up / down); cap < n_out is
 * CSS_ERR_INVALID_ARG.  Independent of the handle's session and streams (it allocates and frees its own device buffers and
 * ends with a synchronise of the handle's stream); 1 .. 64 channels. */
int css_resample_host(css_handle_t h, const void* src, int32_t is_int16, int64_t n_in, int32_t n_ch, int64_t sample_stride,
                      int64_t channel_stride, int32_t up, int32_t down, float* out_host, int64_t cap, int64_t* n_out);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CSS_MI355_RATE_H */
