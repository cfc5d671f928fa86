/* css_mi355_rate_kernels.h -- the kernels of csrc/resample.hip on caller data.
 *
 * An addition to css_mi355.h (included below; same library, same conventions), the companion of css_mi355_frontend.h: one entry
 * per side of the rate conversion -- the ingest side (stream_ingest_resample_kernel, session_ingest_resample_kernel) and the
 * output side (stream_output_kernel, session_output_kernel) -- for unit tests of the arithmetic; not on the hot path.
 * (resample_kernel is css_resample_host of css_mi355_rate.h.)  Each entry takes a table of plain job descriptors that name
 * caller arrays, uploads the inputs and the WHOLE of every output allocation, builds the taps and the phase table as the handle
 * builds them, makes the launch exactly as the path makes it (one call of the launcher for the whole table, so a table longer
 * than the kernel's own crosses into a second launch), downloads everything a launch could have written and synchronises, so a
 * caller sees every element a launch did not own.  Refused with CSS_ERR_INVALID_ARG and a message (css_last_error) before
 * anything is launched or written: a NULL handle, table or array, an array shorter than its description, a ratio the library
 * refuses (css_mi355_rate.h) or whose tile does not fit a workgroup's LDS, and the preconditions named below.  The kernels read
 * inputs outside [N0 - H, N0 + n) as zero whatever H, N0 and m0 are, so those need not be consistent with each other.
 * Lengths are in elements of the array's type.
 */
#ifndef CSS_MI355_RATE_KERNELS_H
#define CSS_MI355_RATE_KERNELS_H

#include "css_mi355.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define CSS_RATE_KERNEL_JOBS 64   /* jobs per call, at most */

/* One job of the ingest side: outputs [m0, m0 + n_m) at up / down of the recording whose inputs [N0 - H, N0) are hist_in [C][H]
 * (float32) and [N0, N0 + n) the piece at src: int16 (is_int16; q 2^-15) or float32, interleaved [n][C] (plane_ld = 0) or planar
 * with channel c at src + c plane_ld.  src [src_elems] is staged at src_offset (0 .. 7) elements behind a 256-byte boundary.
 *   form 0  launch_stream_ingest_resample_multi: dst[dst_col + c dst_ld + (m - m0)], dst_col 0 .. 3 floats behind a 256-byte
 *           boundary; with has_hist_out the last H inputs of [hist_in | piece] go to hist_out [C][H]
 *   form 1  launch_session_ingest_multi: dst[m C + c] (dst_ld, dst_col and has_hist_out must be 0), and the level word holds
 *           level_before when the launch starts and level_after receives it: max(level, max |dst[m][:]| over m < n_peak) as
 *           float bits
 * dst [dst_floats] and hist_out [hist_elems] are uploaded and downloaded whole; hist_in and hist_out have hist_elems >= C H.
 * Refused: H, n, n_m, m0, N0, n_peak < 0 or any of them above 2^40, n_m above 2^24, hist_out == hist_in, C outside 1 .. 64,
 * 0 < plane_ld < n, dst_ld < dst_col + n_m (form 0). */
typedef struct CssRateIngestJob {
    int32_t up, down, C, is_int16, src_offset, H, dst_col, has_hist_out;
    uint32_t level_before, level_after;
    int64_t plane_ld, n, N0, m0, n_m, dst_ld, n_peak, src_elems, hist_elems, dst_floats;
    const void* src;
    const float* hist_in;
    float* hist_out;
    float* dst;
} CssRateIngestJob;
int css_rate_ingest_host(css_handle_t h, int32_t form, CssRateIngestJob* jobs, int32_t n_jobs);

/* One job of the output side: rows src [S][src_ld] of n model-rate samples (the recording's samples [N0, N0 + n)) -> outputs
 * [m0, m0 + n_m) at up / down in dst [S][dst_ld].
 *   form 0  launch_stream_output_multi (S is the launch's, shared by the table): inputs [N0 - H, N0) are hist_in [S][H]; dst is
 *           float32, or with pcm16 int16 by the two lines of css_mi355_stream_out.h with `gain`; up = down = 1 is the copy /
 *           conversion (then n_m <= n); with has_hist_out the last H inputs of [hist_in | src] go to hist_out [S][H];
 *           peak [S] (float bits) and clipped [S] hold the caller's values when the launch starts and receive the words afterwards
 *   form 1  launch_session_output (one job; H, N0, m0, pcm16, has_hist_out must be 0; clipped is not used): dst float32, peak [S]
 *           of the OUTPUT samples
 * dst [dst_elems] and hist_out [hist_elems] are uploaded and downloaded whole.  Refused: a dst_ld that is not a multiple of 16
 * bytes (the staging of dst is), dst_ld < n_m, src_ld < n, H, n, n_m, m0, N0 < 0 or above 2^40, n_m above 2^24,
 * hist_out == hist_in, S outside 1 .. 64. */
typedef struct CssRateOutputJob {
    int32_t up, down, H, pcm16, has_hist_out, reserved;
    float gain, reserved_f;
    int64_t src_ld, n, N0, m0, n_m, dst_ld, src_floats, hist_elems, dst_elems;
    const float* src;
    const float* hist_in;
    float* hist_out;
    void* dst;
    uint32_t* peak;
    uint64_t* clipped;
} CssRateOutputJob;
int css_rate_output_host(css_handle_t h, int32_t form, int32_t S, CssRateOutputJob* jobs, int32_t n_jobs);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CSS_MI355_RATE_KERNELS_H */
