/* css_mi355_preview_handoff.h -- a preview that also hands off: log-mel frames, kept ranges and gate bits up to the present.
 *
 * An addition to css_mi355_preview.h (included below; same library, same conventions).  The hand-off of a stream
 * (css_stream_handoff_*, css_mi355.h) returns, with every push, what became FINAL; css_stream_preview returns the unfinished tail
 * as waveforms only.  A preview with hand-off returns both halves of what css_stream_finish would return at this moment: the
 * waveforms of css_stream_preview, and the hand-off outputs css_stream_finish would write into a bound CssStreamHandoffOut --
 *   gate bits    of frames [t_g, css_plan(n).mix_frames) of css_run on the n samples pushed so far; first_activity_frame = t_g,
 *                the number of frames whose gate bits the pushes returned;
 *   ranges       the kept sample ranges of [D, css_plan(n).n_out), D the decided samples, merged as a push merges them (the
 *                first one may start where the stream's last returned range ended);
 *   raw log-mel  frames J_k .. A'_k / 160 - 1 of stream k's concatenation, J_k the frames the pushes returned for k and A'_k the
 *                kept samples of the whole prefix, with the trailing reflection as at finish; first_frame[k] = J_k places them;
 *   raw_max[k]   the maximum of the stream's running maximum and these frames
 * -- and leaves the stream as it was, as css_stream_preview does: every later push, finish and hand-off output is that of a
 * stream that was never previewed.  With everything the pushes returned this is css_handoff_logmel after css_run_device of the
 * prefix, bit for bit: the ranges merge to regions_host, (max(concat(raw so far, these frames), raw_max - 8) + 4) / 4 is mel_host
 * and the gate bits are CSS_BUF_ACT_FINAL.  All of it is PROVISIONAL in the sense of css_mi355_preview.h.
 *
 * Capacities: a preview is a finish at this moment, so css_stream_handoff_bounds(desc, cfg, hcfg, -1, ...) suffices for every
 * prefix; there is no bounds function of its own.  Capacities below it are refused (CSS_ERR_INVALID_ARG) before anything moves.
 *
 * Cost: on top of css_stream_preview's one estimator segment per stream, the hand-off's three launches (append, ONE DFT product,
 * mel) per 16 items with hand-off outputs, which css_stream_handoff_stats counts after the call, and one more download under
 * the call's one synchronise.  Device memory: one scratch HandoffState table per handle, nothing per stream.
 */
#ifndef CSS_MI355_PREVIEW_HANDOFF_H
#define CSS_MI355_PREVIEW_HANDOFF_H

#include "css_mi355_preview.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

/* css_stream_preview, plus the hand-off's closing round without a commit.  ho is caller-owned and used for this call only
 * (nothing is bound or unbound: what css_stream_handoff_bind bound stays bound and is not written); first_frame [S] receives J_k.
 * Refused as css_stream_preview refuses, and: a stream whose hand-off is off (CSS_ERR_STATE); a NULL ho or first_frame, NULL
 * mel_host / ranges_host / n_frames / n_ranges / raw_max in *ho, or capacities below css_stream_handoff_bounds(..., -1, ...)
 * (CSS_ERR_INVALID_ARG).  activity_host may be NULL.  A prefix that css_run refuses returns its status and writes nothing. */
int css_stream_preview_handoff(css_handle_t h, int32_t id, float* out_host, int64_t cap, int64_t* n_out, int64_t* first_sample,
                               CssStreamHandoffOut* ho, int64_t* first_frame);

typedef struct CssStreamPreviewHandoff {
    CssStreamPreview p;            /* as css_stream_preview_many */
    CssStreamHandoffOut* ho;       /* NULL: waveforms only for this item (also on a stream with the hand-off on) */
    int64_t* first_frame;          /* [S], written when ho != NULL */
} CssStreamPreviewHandoff;

/* css_stream_preview_handoff of n_items distinct streams of one handle in one call, under the rules of css_stream_preview_many:
 * one estimator batch per segmentation, one synchronise, every item what its own call would have written, bit for bit.  An item
 * whose prefix css_run refuses gets that status in items[i].p.status; nothing of it is written, waveform or hand-off, the other
 * items proceed and the call returns CSS_OK.  Argument and state errors (above) refuse the WHOLE call before anything moves;
 * css_last_error names the item index and the id. */
int css_stream_preview_handoff_many(css_handle_t h, CssStreamPreviewHandoff* items, int32_t n_items, CssStreamGroupStats* stats);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CSS_MI355_PREVIEW_HANDOFF_H */
