/* css_mi355_session_window.h -- Whisper encoder inputs of whole sessions, written on the device: the last step of the session
 * hand-off (css_mi355_session_handoff.h, included below; same library, same conventions).
 *
 * The session hand-off stores the normalised log-mel of every separated stream into host arrays; a consumer then cuts 30 s
 * windows, pads them, converts them to float16 and uploads them again.  The calls here leave those encoder inputs in device
 * memory of the caller's (a torch tensor, for example) with ONE more kernel launch per session, whatever the number of windows.
 * For speaker k, with mel_k [n_mels][J_k] the hand-off's normalised log-mel (J_k = n_frames[k]), M_k the maximum its clamp used
 * and  fill_k = (fmaxf(-10.0f, M_k - 8.0f) + 4.0f) * 0.25f  (what a frame of digital zeros takes under that clamp):
 *
 *   windows      n_windows[k] = ceil(J_k / stride).  Window w holds the columns c < n = min(width, J_k - w stride), which are
 *                mel_k[m][w stride + c]; columns n .. width - 1 are fill_k.  Element (k, w, m, c) is
 *                windows_dev[((k cap_windows + w) n_mels + m) ld + c].  Windows w >= n_windows[k] and the columns >= width
 *                of a row are not written.
 *   whole        (optional; seek-based decoding) mel_dev[(k n_mels + m) mel_ld + j] = mel_k[m][j] for j < J_k and fill_k for
 *                J_k <= j < mel_ld: with mel_ld >= frames + 3000, columns [seek, seek + 3000) are Whisper's segment for any
 *                seek <= J_k.
 *   dtype        CSS_WINDOW_F32, or CSS_WINDOW_F16: the float32 value rounded to nearest-even (css_mi355_window.h's constants);
 *                one dtype for both outputs.
 *   empty        a speaker with J_k = 0 gets n_windows[k] = 0; none of its windows or mel_dev rows is written and its
 *                window_max is not specified.
 *
 * J_k and M_k are read from device memory by the kernel: no host decision is added to the session hand-off.
 * Not covered: sessions at the capture rate, windows normalised at their own maximum (css_mi355_window.h does that for
 * streams), bfloat16, CSS_LINEAR_SPLIT_F16 and frame geometries other than 512 / 256 (as the session hand-off). */
#ifndef CSS_MI355_SESSION_WINDOW_H
#define CSS_MI355_SESSION_WINDOW_H

#include "css_mi355_session_handoff.h"
#include "css_mi355_window.h"   /* CSS_WINDOW_F32, CSS_WINDOW_F16, CSS_WINDOW_MAX_WIDTH */

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

/* Caller-owned.  windows_dev and mel_dev are device memory on the handle's device, aligned to the element size; one of them may
 * be NULL (not both).  n_windows and window_max are host arrays of S elements; the queued forms need them page-locked
 * (css_host_alloc): the kernel stores into them.  window_max[k] is M_k. */
typedef struct CssSessionWindows {
    int32_t width;         /* 1 .. 3000 */
    int32_t stride;        /* 1 .. width */
    int32_t dtype;         /* CSS_WINDOW_F32, CSS_WINDOW_F16 */
    int32_t reserved;      /* 0 */
    void*   windows_dev;   /* [S][cap_windows][n_mels][ld], or NULL */
    int64_t ld;            /* >= width */
    int64_t cap_windows;   /* >= css_session_window_bounds' windows */
    void*   mel_dev;       /* [S][n_mels][mel_ld], or NULL */
    int64_t mel_ld;        /* >= css_session_window_bounds' frames */
    int32_t* n_windows;
    float*   window_max;
} CssSessionWindows;

/* Pure host arithmetic: frames and ranges are css_session_handoff_bounds', windows = ceil(frames / stride). */
int css_session_window_bounds(const CssModelDesc* desc, const CssRunCfg* cfg, const CssStreamHandoffCfg* hcfg, int32_t width,
                              int32_t stride, int64_t n_samples, int64_t* frames, int32_t* ranges, int64_t* windows);

/* css_handoff_logmel_all plus the windows: synchronous, after a finished pass.  Pageable host arrays are allowed. */
int css_handoff_windows_all(css_handle_t h, const float* wav_dev, int64_t wav_ld, const CssStreamHandoffCfg* hcfg,
                            CssSessionHandoffOut* out, CssSessionWindows* win);

/* css_run_enqueue_handoff / css_run_enqueue_pcm16_handoff plus the windows, written on the hand-off's stream behind the session's
 * log-mel; everything is valid once css_wait or css_wait_sessions has returned for the session.
 * In all three calls out->mel_host may be NULL (cap_frames is then ignored): no log-mel crosses PCIe and the launch that
 * normalises into host memory is not made, so the session's launch count is css_run_enqueue_handoff's.  ranges_host, n_frames
 * and n_ranges stay required.
 * Refused with nothing allocated, queued or written: everything css_run_enqueue_handoff refuses, with its codes; and with
 * CSS_ERR_INVALID_ARG a NULL win or count array, count arrays that are not page-locked (queued forms), both device outputs NULL,
 * width outside 1 .. 3000, stride outside 1 .. width, an unknown dtype, ld < width, cap_windows or mel_ld below the bounds, a
 * device pointer that is not device memory of the handle's device or not aligned to the element size. */
int css_run_enqueue_windows(css_handle_t h, const float* pcm_host, int64_t n_samples, int32_t n_ch, const CssRunCfg* cfg,
                            float* wav_host, int64_t cap, const CssStreamHandoffCfg* hcfg, CssSessionHandoffOut* out,
                            CssSessionWindows* win);
int css_run_enqueue_pcm16_windows(css_handle_t h, const int16_t* const* planes_host, int64_t n_samples, int32_t n_ch,
                                  const CssRunCfg* cfg, int16_t* wav_pcm16_host, int64_t cap, float* peaks_host,
                                  const CssStreamHandoffCfg* hcfg, CssSessionHandoffOut* out, CssSessionWindows* win);

/* Running counts of the handle: launches of the window kernel, and sessions (or synchronous calls) that asked for windows. */
int css_session_window_stats(css_handle_t h, int64_t* launches, int64_t* sessions);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif

#endif /* CSS_MI355_SESSION_WINDOW_H */
