/* css_mi355_present_window.h -- Whisper encoder windows that reach the present, assembled on the device.
 *
 * An addition to css_mi355_preview_handoff.h and css_mi355_window.h (both included below; same library, same conventions).
 * css_stream_windows writes encoder inputs out of a stream's frame history, which ends where the stream's FINAL frames end -- up
 * to CssStreamInfo.max_lag behind the input.  css_stream_preview_handoff computes the PROVISIONAL frames from there to the present,
 * into host memory.  The call of this header does both under one synchronise: it previews a set of streams exactly as
 * css_stream_preview_handoff_many does and, behind the preview's hand-off on the handle's stream, writes windows whose spans end
 * at the present frame -- final frames out of the ring, then the preview's provisional frames, normalised over the whole span by
 * the rule of css_mi355_window.h and padded -- into device memory of the caller's.  No stream moves.
 *
 * For stream `id` and speaker k at the moment of the call: J_k frames were returned by the pushes, the ring holds [R_k, J_k) with
 * R_k = max(J_k - history_frames, 0), the preview's hand-off makes P_k provisional frames J_k .. J_k + P_k - 1 (what
 * css_stream_preview_handoff writes to ho->mel_host with first_frame[k] = J_k), and E_k = J_k + P_k.  A window (k, n_frames, width,
 * dtype) covers  a = max(E_k - n_frames, R_k),  used = E_k - a  frames: the ring's [a, J_k), then the last min(used, P_k)
 * provisional ones.  P_k depends on the tail's gate bits, which exist on the device only until the synchronise, so the span is
 * resolved there and reported afterwards.
 */
#ifndef CSS_MI355_PRESENT_WINDOW_H
#define CSS_MI355_PRESENT_WINDOW_H

#include "css_mi355_preview_handoff.h"
#include "css_mi355_window.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef struct CssStreamPresentWindow {
    int32_t speaker;
    int32_t n_frames;        /* at most this many frames, counted back from the present: 1 .. width */
    int32_t width, dtype;    /* n_frames .. CSS_WINDOW_MAX_WIDTH; CSS_WINDOW_F32 / CSS_WINDOW_F16 */
    void*   out_dev;         /* device memory, [n_mels][ld] of dtype */
    int64_t ld;              /* >= width */
    int64_t first_frame;     /* out: first frame of the span, in the speaker's concatenation */
    int32_t n_used;          /* out: frames in the span */
    int32_t n_provisional;   /* out: how many of them are the preview's */
    float   window_max;      /* out: the maximum the clamp used */
} CssStreamPresentWindow;

typedef struct CssStreamPresentItem {
    CssStreamPreviewHandoff ph;        /* exactly as css_stream_preview_handoff_many takes it; ho != NULL */
    CssStreamPresentWindow* windows;   /* n_windows of them, any speakers, repeats allowed */
    int32_t n_windows;
} CssStreamPresentItem;

/* Previews n_items distinct streams of one handle (ph: every rule of css_stream_preview_handoff_many, whose outputs -- waveforms,
 * *ho, first_frame, p.status, p.n_out, p.first_sample -- are written exactly as that call writes them) and writes their windows.
 * Window w of an item, with the span above:
 *   used >= 1   out_dev[m * ld + c], m < n_mels, c < width, receives the window of the `used` raw frames by the rule at the top of
 *               css_mi355_window.h (stream.py whisper_window), bit for bit; nothing else of out_dev is written.  first_frame = a,
 *               n_used = used, n_provisional = min(used, P_k), window_max = the frames' maximum.
 *   used == 0   (no frame yet: J_k = P_k = 0) nothing is written at out_dev; first_frame = E_k, n_used = n_provisional = 0, and
 *               window_max is left as it was.
 * An item whose prefix css_run refuses gets that status in ph.p.status; none of its windows is written, none of their out fields
 * is touched, the other items proceed and the call returns CSS_OK.  Afterwards every stream, its device state, its ring, its
 * bound hand-off outputs and css_stream_window_range are as they were before the call.
 * Checked before anything moves, each refusing the WHOLE call (css_last_error names the item and the window index): everything
 * css_stream_preview_handoff_many refuses; n_items < 1 or NULL items (CSS_ERR_INVALID_ARG); a stream without a frame history
 * (css_stream_window_open; CSS_ERR_STATE); and with CSS_ERR_INVALID_ARG n_windows < 0, n_windows > 0 with windows or ph.ho
 * NULL, a speaker outside 0 .. S - 1, n_frames < 1 or > width, width > CSS_WINDOW_MAX_WIDTH, ld < width, an unknown dtype, an
 * out_dev that is NULL or not aligned to its element size.
 * Cost: the preview's estimator batch (stats, may be NULL, as css_stream_preview_many), the hand-off's three launches per 16
 * hand-off items (css_stream_handoff_stats, as css_stream_preview_handoff_many), one kernel launch per CSS_WINDOW_TABLE windows of
 * the whole call, whatever streams they name (*window_launches, may be NULL, receives the count), and ONE synchronise.  The
 * provisional frames live in scratch of the handle that the next hand-off round overwrites: they are not kept. */
int css_stream_present_windows(css_handle_t h, CssStreamPresentItem* items, int32_t n_items, CssStreamGroupStats* stats,
                               int32_t* window_launches);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CSS_MI355_PRESENT_WINDOW_H */
