/* css_mi355_preview.h -- the unfinished tail of a stream: css_run of what was pushed so far, without ending the stream.
 *
 * An addition to css_mi355.h (included below; same library, same conventions).  A push returns the samples that are FINAL, and
 * finality lags the input by up to CssStreamInfo.max_lag samples (3.6 s with 3 s / 1.5 s segments).  A preview returns the rest:
 * after n pushed samples, samples [n_emitted, css_plan(n).n_out) of css_run on those n samples, bit for bit -- what
 * css_stream_finish would return at this moment -- and leaves the stream as it was: n_pushed, n_emitted, the finality of later
 * pushes, every later returned sample and every later hand-off output are those of a stream that was never previewed.  The
 * samples are PROVISIONAL: the segment that is still open was closed with zeros and the last-segment window, and a later push
 * replaces them with other values once they become final.
 *
 * Cost: for every prefix exactly one segment is not done yet, so a preview passes ONE segment per stream through the mask
 * estimator; the grouped call passes the pending segments of all its streams as one batch, as a grouped push does.  The
 * hand-off takes no part in the calls of this header: no log-mel frame, range or gate byte is produced or moved.  The preview
 * that also returns the hand-off's outputs up to the present is declared in css_mi355_preview_handoff.h.
 */
#ifndef CSS_MI355_PREVIEW_H
#define CSS_MI355_PREVIEW_H

#include "css_mi355.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

/* Pure host arithmetic, no GPU: after n_pushed model-rate samples a preview returns samples [*first, *first + *count) per
 * separated stream; *first == css_stream_final_samples(n_pushed), *first + *count == css_plan(n_pushed).n_out.  Both are
 * written whenever the arguments are accepted; the return value is then the status css_run gives for this prefix: CSS_OK, or
 * CSS_ERR_ZERO_WEIGHT where the plan finds a frame without weight (css.py:297; with the default windows every prefix of at most
 * one segment).  count <= (segment_frames + dilation_frames + erosion_frames - 1) * 256 + 512 < CssStreamInfo.max_lag, so max_lag
 * is always a sufficient capacity.  (A stream with a rate ratio: n_pushed is css_stream_rate_samples(up, down, n_in, 1) for the
 * end and css_stream_rate_samples(up, down, n_in, 0) for the first sample.) */
int css_stream_preview_samples(const CssModelDesc* desc, const CssRunCfg* cfg, int64_t n_pushed, int64_t* first, int64_t* count);

/* Row k of out_host[S][cap] receives samples [n_emitted, css_plan(n).n_out) of separated stream k of css_run on the n samples
 * pushed so far (a stream with a rate ratio: css_run of css_resample_host of the inputs so far); *n_out their count,
 * *first_sample = n_emitted.  A prefix that css_run refuses returns css_run's status (CSS_ERR_ZERO_WEIGHT) and writes nothing.
 * Refused, with the stream and the buffers untouched: an unknown id (CSS_ERR_INVALID_ARG), a finished stream or queued sessions
 * outstanding (CSS_ERR_STATE), cap below the count or a NULL pointer (CSS_ERR_INVALID_ARG).
 * Device memory: the stream's output buffer may grow to the preview's length (counted in CssStreamInfo.device_bytes). */
int css_stream_preview(css_handle_t h, int32_t id, float* out_host, int64_t cap, int64_t* n_out, int64_t* first_sample);

typedef struct CssStreamPreview {
    int32_t id;
    float*  out_host; int64_t cap;      /* [S][cap] */
    int64_t n_out, first_sample;        /* written */
    int32_t status;                     /* written: CSS_OK, or the status css_run gives for this prefix */
} CssStreamPreview;

/* css_stream_preview of n_items distinct streams of one handle in one call: the pending segments of all items pass the mask
 * estimator as one batch per segmentation, and the call synchronises once.  Every item receives what its own css_stream_preview
 * would have written, bit for bit.  An item whose prefix css_run refuses gets that status in items[i].status and n_out = 0, its
 * buffer is not written, the other items proceed and the call returns CSS_OK.  Argument and state errors (see above; also an
 * id named twice) refuse the WHOLE call before anything moves; css_last_error names the item index and the id.
 * stats (may be NULL) counts estimator batches and segments as for css_stream_push_many. */
int css_stream_preview_many(css_handle_t h, CssStreamPreview* items, int32_t n_items, CssStreamGroupStats* stats);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CSS_MI355_PREVIEW_H */
