/* css_mi355_window.h -- Whisper encoder windows assembled on the device, out of a stream's own frame history.
 *
 * An addition to css_mi355.h (included below; same library, same conventions).  The hand-off of a stream (css_stream_handoff_*)
 * returns, with every push, the RAW log-mel frames that became final, in host memory: the max - 8 clamp needs a maximum over a
 * span the consumer chooses.  This header lets the consumer choose that span on the device.  A stream that was given a frame
 * history keeps its last history_frames raw frames per separated stream in device memory, and css_stream_windows writes any
 * number of encoder inputs -- a span of those frames, clamped at the span's own maximum - 8, (x + 4) / 4, padded to the
 * encoder's width, as float32 or float16 -- straight into device memory of the caller's, for example a torch tensor that a
 * Whisper encoder consumes.  For the raw frames `raw` [n_mels][n_frames] of the span and their maximum M over all bands and frames:
 *   column c < n_frames of row m     (fmaxf(raw[m][c], M - 8.0f) + 4.0f) * 0.25f            in float32
 *   columns n_frames .. width - 1    (fmaxf(-10.0f,    M - 8.0f) + 4.0f) * 0.25f            (-10 = log10(1e-10): a frame of digital zeros)
 *   CSS_WINDOW_F16                   that float32 value rounded to nearest-even
 * which is, bit for bit, what the host makes of the frames the pushes returned (stream.py whisper_window).  Nothing of the
 * hand-off changes: the frames still arrive in the bound CssStreamHandoffOut as before, and a stream without a history holds
 * and returns what it did.
 *
 * Windows whose span goes on over a preview's provisional frames, up to the present, are css_mi355_present_window.h's (a preview
 * never writes the history).  Not covered: bfloat16, and spans longer than 3000 frames.
 */
#ifndef CSS_MI355_WINDOW_H
#define CSS_MI355_WINDOW_H

#include "css_mi355.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

enum { CSS_WINDOW_F32 = 0, CSS_WINDOW_F16 = 1 };
#define CSS_WINDOW_MAX_WIDTH 3000   /* columns of a window, at most (Whisper's 30 s) */
#define CSS_WINDOW_TABLE 32         /* windows per kernel launch of css_stream_windows */

/* Gives an open stream its frame history: after css_stream_handoff_open and before the stream's first sample.  A stream whose
 * hand-off is off, a stream that has taken samples or has finished, and a second call are CSS_ERR_STATE; history_frames outside
 * 32 .. 2^20 is CSS_ERR_INVALID_ARG; on any refusal the stream stays as it was.  From then on every push and css_stream_finish
 * also leaves the frames it completes in a ring on the device -- frame j of separated stream k's concatenation (the index
 * CssStreamHandoffOut counts frames in) in slot j mod history_frames, with the same float32 values it writes to mel_host -- so
 * that after any call the ring holds frames [max(J_k - history_frames, 0), J_k), J_k the frames returned for k so far.  A
 * preview never writes it.  The hand-off's launch count (css_stream_handoff_stats) is unchanged.
 * Device memory, allocated here and counted in CssStreamInfo.device_bytes from here on: the ring, float32
 * [S][n_mels][history_frames], and the frames' maxima over the bands, float32 [S][history_frames]. */
int css_stream_window_open(css_handle_t h, int32_t id, int32_t history_frames);

/* The frames the history of stream `id` holds now: [first_frame[k], end_frame[k]) for k < S.  A stream without a history is
 * CSS_ERR_STATE.  A finished stream that is not closed yet keeps its history. */
int css_stream_window_range(css_handle_t h, int32_t id, int64_t* first_frame /*[S]*/, int64_t* end_frame /*[S]*/);

typedef struct CssStreamWindow {
    int32_t id, speaker;
    int64_t first_frame;   /* frame of the speaker's concatenation */
    int32_t n_frames;      /* 1 .. width */
    int32_t width;         /* columns written, n_frames .. 3000 */
    int32_t dtype;         /* CSS_WINDOW_F32, CSS_WINDOW_F16 */
    void*   out_dev;       /* device memory, [n_mels][ld] elements of dtype */
    int64_t ld;            /* >= width */
    float   window_max;    /* out: the maximum the clamp used */
} CssStreamWindow;

/* Writes n_items windows, of any streams and speakers of the handle in any order (a stream or a span may appear many times), on
 * the handle's stream, and returns after ONE synchronise; no stream's state changes.  Item i: frames [first_frame, first_frame +
 * n_frames) of the speaker's history by the rule at the top into out_dev[m * ld + c], m < n_mels, c < width; nothing else of
 * out_dev is written, and out_dev may have any alignment its element size allows.
 * All items are checked before anything is launched: an id without an open stream or a stream without a history, a speaker
 * outside 0 .. S - 1, frames outside css_stream_window_range, n_frames < 1, width outside n_frames .. 3000, ld < width, an
 * unknown dtype, a NULL out_dev or one not aligned to the element size refuse the WHOLE call with CSS_ERR_INVALID_ARG;
 * css_last_error names the item's index, and nothing is written.
 * Cost: one kernel launch per CSS_WINDOW_TABLE items, whatever streams they name; *launches (may be NULL) receives the count. */
int css_stream_windows(css_handle_t h, CssStreamWindow* items, int32_t n_items, int32_t* launches);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CSS_MI355_WINDOW_H */
