/* css_mi355_handoff_kernels.h -- the window kernels and the hand-off kernels of queued sessions, on caller data.
 *
 * An addition to css_mi355_stream_kernels.h (included below; same library, same conventions, its CssKArray): one entry per launcher
 * of the part of csrc/handoff.hip that header leaves out -- session_keep_scan_kernel, session_gather_kernel, session_norm_kernel,
 * session_window_kernel and stream_window_kernel -- for unit tests of the kernels; not on the hot path.  Each entry checks first,
 * uploads the inputs and the WHOLE of every output allocation, makes the launcher call(s) exactly as the path makes them, downloads
 * everything a launch could have written and synchronises.  Every array is staged at a 256-byte boundary with 256 bytes of room on
 * both sides.  These kernels branch on the alignment of their arrays, so every array whose address a kernel looks at has an
 * ELEMENT OFFSET field (..._off): the kernel is given the address that many elements past the array's first one, which sits on the
 * 256-byte boundary; the array's length counts the elements in front.  Refused with CSS_ERR_INVALID_ARG and a message
 * (css_last_error) before anything is launched or written: a NULL handle, descriptor or array, an array shorter than its
 * description, and the preconditions named with each entry: what the kernels do not guard themselves, next to what the paths
 * guarantee in its place.  A state row is {int64 A, int64 J, int32 gmax, int32 pad}, as in css_mi355_stream_kernels.h.
 */
#ifndef CSS_MI355_HANDOFF_KERNELS_H
#define CSS_MI355_HANDOFF_KERNELS_H

#include "css_mi355_stream_kernels.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define CSS_WINDOW_KERNEL_ITEMS 64   /* items per call of css_stream_windows_host, at most */

/* ---- launch_session_keep_scan.  In: gate, S TL bytes behind gate_off (0 .. 3) bytes.  Out, all uploaded and downloaded whole:
 * psum [S][TL + 1] int32, regs [S][cap_ranges][2] int64, offs [S][cap_ranges] int64, st [S] state rows, n_new [S] int32,
 * n_ranges [S] int32, and the caller's three arrays ranges_out [S][cap_ranges][2] int64, n_frames_out [S] int64, n_ranges_out [S]
 * int32.  Refused: S outside 1 .. 4, TL outside 1 .. 2^24, pad outside 0 .. 4096, cap_ranges < 1, gate_off outside 0 .. 3.
 * ACCEPTED: a cap_ranges below the gate's run count (the path refuses capacities below (TL - 1) / (2 pad + 3) + 1, so there the
 * kernel's own guards never fire): only the first cap_ranges runs are tabulated, the counts are the true ones. */
typedef struct CssSessionScanJob {
    int32_t S, pad, drop, cap_ranges, gate_off, reserved;
    int64_t TL;
    CssKArray gate, psum, regs, offs, st, n_new, n_ranges, ranges_out, n_frames_out, n_ranges_out;
} CssSessionScanJob;
int css_session_scan_host(css_handle_t h, CssSessionScanJob* job);

/* ---- launch_session_gather on caller tables.  In: regs, offs, st, n_ranges as the keep-scan leaves them, wav [S][wav_ld] float32
 * behind wav_off (0 .. 3) floats.  Out: operand, exactly S rows 160 + 416 floats.  Speaker k reads min(n_ranges[k], cap_ranges)
 * table rows.  Refused: S outside 1 .. 4, rows outside 1 .. 2^20, cap_ranges < 1, st[k].A < 0, n_ranges[k] < 0, an offs row that
 * is not monotone, and a table under which the kernel would read outside speaker k's wav row: concatenation
 * sample j < A of the last run r with offs[r] <= j is wav[regs[r][0] + j - offs[r]] (the largest and the smallest index per run are
 * worked out on the host).  The path: the keep-scan's table, whose runs lie inside 256 (TL + 1) <= wav_ld samples. */
typedef struct CssSessionGatherJob {
    int32_t S, cap_ranges, wav_off, reserved;
    int64_t wav_ld, rows;
    CssKArray regs, offs, st, n_ranges, wav, operand;
} CssSessionGatherJob;
int css_session_gather_host(css_handle_t h, CssSessionGatherJob* job);

/* ---- launch_session_norm.  In: st [S], mel [S][n_mels][mel_ld] float32.  Out: out [S][n_mels][out_ld] float32, whole.  rows <= 0
 * launches nothing, as in the launcher.  Refused: S outside 1 .. 4, n_mels outside 1 .. 128, mel_ld < rows, out_ld < 0,
 * st[k].J < 0 or > rows: the kernel does not guard it (its grid covers `rows` columns rounded up to 256 and it reads mel below J);
 * on the path rows is the frame bound n_out / 160 >= J. */
typedef struct CssSessionNormJob {
    int32_t S, n_mels;
    int64_t mel_ld, out_ld, rows;
    CssKArray st, mel, out;
} CssSessionNormJob;
int css_session_norm_host(css_handle_t h, CssSessionNormJob* job);

/* ---- launch_session_windows.  The fields are SessionWindows' (csrc/kernels.hpp).  In: st [S], mel [S][n_mels][mel_ld] float32
 * behind mel_off (0 .. 3) floats.  Out, whole: win [S][cap_windows][n_mels][ld] behind win_off (0 .. 7) elements (has_win), whole
 * [S][n_mels][whole_ld] behind whole_off (0 .. 7) elements (has_whole), both of float32 or (f16) float16; n_windows_out [S] int32,
 * window_max_out [S] float32.  The entry computes n_win_jobs = ceil(max_frames / stride) or 0 and n_whole_jobs =
 * ceil(whole_ld / 4096) or 0 as the path does and returns them in the descriptor.
 * Accepted: n_mels 1 .. 128 (the kernel guards its bands), either output absent, st[k].J > max_frames (the kernel clamps).
 * Refused: S outside 1 .. 4, width or stride < 1 (or above 2^20), max_frames < 0, max_frames > mel_ld, with has_win ld < width
 * or cap_windows < ceil(max_frames / stride), whole_ld < 1 with has_whole, an offset outside its range, st[k].J < 0. */
typedef struct CssSessionWindowsJob {
    int32_t S, n_mels, width, stride, f16, has_win, has_whole, win_off, whole_off, mel_off;
    int64_t mel_ld, max_frames, ld, cap_windows, whole_ld, n_win_jobs, n_whole_jobs;
    CssKArray st, mel, win, whole, n_windows_out, window_max_out;
} CssSessionWindowsJob;
int css_session_windows_host(css_handle_t h, CssSessionWindowsJob* job);

/* ---- launch_stream_windows on a table of up to CSS_WINDOW_KERNEL_ITEMS items, CSS_WINDOW_TABLE (32) per launch as the path's
 * launch_windows chunks them (33 items: two launches).  The fields are WindowItem's.  In per item: ring [n_mels][hist] float32
 * behind ring_off (0 .. 3) floats, fmax [hist]; with has_pv also pv [n_mels][pv_ld] behind pv_off (0 .. 3) floats, pvmax [pv_ld]
 * and n_new, one int32.  Out per item: out [n_mels][ld] behind out_off (0 .. 7) elements, float32 or (f16) float16, whole; and row
 * i of res, res_rows rows of {int64 first_frame, int32 n_used, int32 n_provisional, float window_max, int32 pad}, uploaded and
 * downloaded whole.  Accepted: hist >= 1, n_mels 1 .. 128 and differing among the items (the grid is the largest), *n_new > pv_ld
 * (the kernel clamps).  Refused: width outside 1 .. 3000, n_frames outside 1 .. width, ld < width, J < 0, *n_new < 0, pv_ld < 1 with has_pv,
 * an offset outside its range, res_rows < n_items, and WITHOUT has_pv n_frames > min(J, hist): the host's check that the
 * kernel's "n_frames <= hist and J - hist <= first" relies on. */
typedef struct CssStreamWindowJob {
    int32_t n_frames, width, n_mels, f16, has_pv, ring_off, pv_off, out_off;
    int64_t hist, ld, J, pv_ld;
    CssKArray ring, fmax, pv, pvmax, n_new, out;
} CssStreamWindowJob;
int css_stream_windows_host(css_handle_t h, CssStreamWindowJob* items, int32_t n_items, void* res, int64_t res_rows);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CSS_MI355_HANDOFF_KERNELS_H */
