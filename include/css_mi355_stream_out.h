/* css_mi355_stream_out.h -- final samples of a stream at the playback rate, float32 or PCM16, converted on the device.
 *
 * An addition to css_mi355.h (included below through css_mi355_rate.h; same library, same conventions).  The hosts that push
 * 48 kHz PCM16 -- conference bridges, WebRTC relays, monitoring desks, room recorders -- consume 48 kHz PCM16 as well.  A stream
 * that was given an output format writes, with every push and with css_stream_finish, the samples that became final into a bound
 * host buffer at the OUTPUT rate, as float32 or int16: one kernel launch per round for all such streams of the round resamples,
 * scales and rounds them on the device, and only the converted samples cross PCIe (the float32 out_host of the push may be NULL).
 *
 * Definition.  For separated stream k let w_k be css_run's waveform of the whole recording (of css_resample_host of it for a
 * stream with css_stream_set_rate), and up / down the output rate over the model's 16 kHz in lowest terms (48 kHz: 3 / 1,
 * 44.1 kHz: 441 / 160, 8 kHz: 1 / 2).
 *   float32   y_k = css_resample_host(w, is_int16 = 0, up, down) of the S waveforms as S planar channels: resample_poly's default
 *             filter (css_mi355_rate.h), one float32 fmaf chain per output sample, zeros outside the recording,
 *             ceil(n_out up / down) samples in all.  What all pushes and finish wrote, concatenated, is y_k bit for bit, however
 *             the pushes were cut.
 *   count     after n final model-rate samples exactly css_stream_rate_samples(up, down, n, 0) = max(0, ceil((n up - half) / down))
 *             output samples have been written; finish completes the count to ceil(n up / down).  (css_stream_output_samples.)
 *   1 / 1     up == down == 1 is no rate change: no filter, no lag, y = w.  Accepted here although css_stream_set_rate refuses it:
 *             it exists for PCM16 at the model rate.
 *   PCM16     v = y * gain in float32 (one rounding), q = (int16) clamp(rint((double) v * 32767.0), -32768, 32767): round half to
 *             even and the clamp of css_run_pcm16's encoder.  There is no peak normalisation -- a live host cannot know the
 *             recording's peak; n_clipped[k] counts the samples the clamp changed, so a host sees that its gain is too high.
 *   peak      with or without an output format every stream keeps max |w_k| over the final model-rate samples it has emitted,
 *             as float bits (css_stream_output_peaks).  After finish it is css_run_pcm16's peaks_host bit for bit, so a recorder
 *             can apply the wav writer's gain to what it stored.
 *
 * css_stream_preview* is unchanged: it returns float32 at the model rate and reads or moves none of the output state, because a
 * provisional tail cannot be taken back from a loudspeaker.  The split-f16 mode stays refused, as for every stream.
 */
#ifndef CSS_MI355_STREAM_OUT_H
#define CSS_MI355_STREAM_OUT_H

#include "css_mi355_rate.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef struct CssStreamOutputCfg {
    int32_t up, down;   /* output rate / model rate in lowest terms; 1 / 1: no rate change                       */
    int32_t pcm16;      /* 0: float32 samples, else int16                                                       */
    float gain;         /* PCM16 only: the factor before the rounding (finite, > 0; 1 for float32 is customary) */
} CssStreamOutputCfg;

/* Filled by every push / finish of a stream they are bound to (the struct and its arrays stay valid while bound). */
typedef struct CssStreamOutputCounts {
    int64_t n_written;      /* out: output-rate samples per separated stream the last call wrote                 */
    int64_t n_total;        /* out: ... all calls so far                                                        */
    int64_t* n_clipped;     /* [S], out: samples of all calls so far that the PCM16 clamp changed (float32: 0)  */
    uint32_t* peak_bits;    /* [S], out: max |w_k| over the final model-rate samples so far, as float bits      */
} CssStreamOutputCounts;

/* Gives an open stream its output format: after css_stream_open and before the stream's first sample, in any order with
 * css_stream_handoff_open and css_stream_set_rate.  Later, or a second time, is CSS_ERR_STATE; a ratio outside the resampler's
 * rule (css_mi355_rate.h) other than 1 / 1, a non-finite gain or a gain <= 0 is CSS_ERR_INVALID_ARG; on any refusal the stream
 * stays as it was.  Device memory, allocated here and counted in CssStreamInfo.device_bytes from here on: two generations of the
 * carried final samples (ceil(2 half / up) + 1 per separated stream), the taps, one round of output samples and the counters.
 * A stream without an output format allocates, launches and copies what it did. */
int css_stream_set_output(css_handle_t h, int32_t id, const CssStreamOutputCfg* cfg);

/* Binds the caller's buffer -- page-locked or pageable host memory, out_host [S][cap] at the output rate, int16 or float32 by
 * the cfg -- and the counts; may be called again between calls (out_host == NULL unbinds).  A stream with an output format and
 * nothing bound refuses pushes and finish with CSS_ERR_STATE; a capacity below what the call will write
 * (css_stream_output_samples of the final samples after the call, minus n_total) is CSS_ERR_INVALID_ARG; both come before
 * anything moves and leave every stream of the call as it was.  With an output format bound the float32 out_host of
 * css_stream_push*, css_stream_push*_pcm16 and css_stream_finish may be NULL: then nothing crosses PCIe at the model rate (n_out
 * still counts the model-rate samples that became final).  If it is given, both are written.  All push forms work, with or
 * without css_stream_set_rate, and such streams may share a grouped call with streams that have no output format.
 * CSS_ERR_STATE for a stream without an output format. */
int css_stream_output_bind(css_handle_t h, int32_t id, void* out_host, int64_t cap, CssStreamOutputCounts* counts);

/* Pure host arithmetic, no GPU: output samples written after n_final_model final model-rate samples (finished = 1: of a finished
 * stream that emitted n_final_model samples).  css_stream_rate_samples for the cfg's ratio; n_final_model for 1 / 1. */
int css_stream_output_samples(const CssStreamOutputCfg* cfg, int64_t n_final_model, int32_t finished, int64_t* n);

/* peak_bits [S]: the running peak of ANY open stream of the handle, with or without an output format (see above). */
int css_stream_output_peaks(css_handle_t h, int32_t id, uint32_t* peak_bits);

/* Of the last push / finish call on this handle: launches of the output kernel and the rounds that had at least one stream with
 * an output format (one launch per round and CSS_STREAM_OUTPUT_TABLE such streams).  Either pointer may be NULL. */
#define CSS_STREAM_OUTPUT_TABLE 16
int css_stream_output_stats(css_handle_t h, int32_t* launches, int32_t* rounds);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CSS_MI355_STREAM_OUT_H */
