/* css_mi355_backend.h -- the kernels of csrc/mvdr.hip and csrc/stitch.hip on caller data.
 *
 * An addition to css_mi355.h (included below; same library, same conventions), the companion of css_mi355_frontend.h: one entry
 * per kernel family -- covariances, MVDR solve, beamformer and power normalisation; stitching costs, permutation scan, the two
 * overlap-add kernels and the gate -- for unit tests of the arithmetic; not on the hot path.  Each entry takes caller arrays and
 * a plain descriptor, uploads the inputs and the WHOLE of every output allocation, makes the launch exactly as the path makes
 * it, downloads every allocation a launch could have written and synchronises, so a caller sees every element a launch did not
 * own.  Each form reads what the stage before it would have written FROM THE CALLER.  Whatever a kernel's own comment excludes is
 * refused with CSS_ERR_INVALID_ARG and a message (css_last_error) before anything is launched or written: a NULL handle or
 * descriptor, an array shorter than its description, and the preconditions named at each entry.  Lengths are in elements of the
 * array's type; a split-f16 output (split_f16.hpp) has the float count of its float32 form.
 */
#ifndef CSS_MI355_BACKEND_H
#define CSS_MI355_BACKEND_H

#include "css_mi355.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define CSS_BACKEND_MAX_SETS 16

/* One argument set of the multi-session solve (form 2): segments [seg_lo, seg_lo + nseg) of a session whose covariances start
 * at scm + scm_off and whose weights start at bfw + bfw_off (offsets in doubles). */
typedef struct CssMvdrSet {
    int64_t seg_lo, nseg, scm_off, bfw_off;
} CssMvdrSet;

/* The kernels of mvdr.hip (MvdrArgs, kernels.hpp).  X [C][2 F][T_ld] planes, masks [(S + 1) F][mask_ld] (segment s at column
 * s T), override [segments][F][T] bytes or NULL, scm [segments][S + 1][F][49] doubles, bfw [segments][S][F][7][2] doubles, sep
 * [segments][S][F][T][2] floats; `segments` = seg_lo + nseg.  form:
 *   0  launch_scm (its own dispatch: scm_kernel<4,192> / <4> / <8>, scm_long_kernel beyond 512 frames or with
 *      CSS_FORCE_LONG_PATH in the environment): reads X, masks, override; scm is uploaded and downloaded whole
 *   1  launch_mvdr_solve: reads scm; bfw is uploaded and downloaded whole
 *   2  launch_mvdr_solve_multi over sets[0 .. n_sets): as form 1 per set (seg_lo and nseg of the descriptor are not used)
 *   3  launch_beamform (use_mvdr 0 / 1, mask_floor): reads X, masks and, with use_mvdr, bfw; sep is uploaded and downloaded whole
 *   4  launch_segment_power_norm: reads X, scales sep in place (uploaded and downloaded whole)
 * Arrays a form does not read or write may be NULL.  Refused: C != 7 for forms 0 .. 2 and with use_mvdr (C >= 1 otherwise), S
 * outside 1 .. 3, F outside 1 .. 4096, T outside 1 .. 65535, hop < 1, nseg outside 1 .. 4096, seg_lo < 0,
 * mask_ld < (seg_lo + nseg) T, mask_ld or T_ld above 2^28, T_ld shorter than the last valid frame min(stft_frames, (seg_lo + nseg - 1) hop + T), an override
 * byte that is neither a winner index below S + 1 nor 16 | bits with a bit below S + 1 set, n_sets outside 1 ..
 * CSS_BACKEND_MAX_SETS, a set outside its arrays, short arrays. */
typedef struct CssMvdrDesc {
    int32_t form, C, F, S, T, hop, nseg, use_mvdr, n_sets, reserved;
    float mask_floor, reserved_f;
    int64_t seg_lo, stft_frames, T_ld, mask_ld;
    int64_t x_floats, mask_floats, override_bytes, scm_doubles, bfw_doubles, sep_floats;
    CssMvdrSet sets[CSS_BACKEND_MAX_SETS];
} CssMvdrDesc;
int css_mvdr_host(css_handle_t h, const CssMvdrDesc* d, const float* X, const float* masks, const uint8_t* wta_override,
                  double* scm, double* bfw, float* sep);

/* One session of the multi-session costs (form 1): num_segments segments whose masks start at masks + mask_off (floats; rows of
 * mask_ld), whose separated spectra start at sep + sep_off (floats) and whose costs [num_segments - 1][S S] start at
 * costs + costs_off (doubles). */
typedef struct CssStitchSet {
    int64_t num_segments, mask_off, sep_off, costs_off;
} CssStitchSet;

/* The kernels of stitch.hip (StitchArgs, kernels.hpp).  masks [S F][mask_ld] at least (segment s at column s T), sep
 * [num_segments][S][F][T][2], windows [3][T] (w_first | w_mid | w_last), costs [boundaries][S S] doubles, perms [segments][S]
 * int32, mask_st [S][F][T_long], activity [S][T_long], act_b / act_tmp / act_final [S][T_long] bytes, Y [S][T_long][KIp].  form:
 *   0  launch_pit_costs(loss, input, boundaries [lo, hi)): reads masks (input 0) or sep (input 1); costs whole
 *   1  launch_pit_costs_multi over sets[0 .. n_sets) (num_segments, lo, hi of the descriptor are not used); costs whole
 *   2  launch_pit_scan(boundaries [lo, hi)): reads costs; perms is uploaded (the resume reads row lo) and downloaded whole
 *   3  launch_ola_masks(frames [lo, hi)): reads masks, perms, windows; mask_st, activity, act_b whole
 *   4  launch_morphology(frames [lo, hi)): reads act_b; act_tmp and act_final whole
 *   5  launch_ola_stft(frames [lo, hi)): reads sep, perms, windows, act_final; Y whole (y_split 0 / 1; has_level = 1 passes a
 *      device word holding `level`, 0 passes NULL)
 * Arrays a form does not read or write may be NULL.  Refused: S outside 1 .. 4, F outside 1 .. 4096 (1 .. 511 for form 5: the
 * tile's LDS), T outside 1 .. 65535, hop < 1 or hop > T, hop == T for forms 0 and 1 (the mean divides by F (T - hop)), ranges
 * outside [0, T_long] (frames) or [0, num_segments - 1] (boundaries), num_segments < 1, T_long < 1 or beyond the segments'
 * coverage (num_segments - 1) hop + T, mask_ld < num_segments T or above 2^28, KIp < 2 F, KIp % 32 with y_split, a negative radius, a perms
 * row that is not a permutation of 0 .. S - 1 (form 2: row lo when lo > 0; forms 3 and 5: every row), n_sets outside 1 ..
 * CSS_BACKEND_MAX_SETS, a set outside its arrays, short arrays. */
typedef struct CssStitchDesc {
    int32_t form, S, F, T, hop, loss, input, KIp, y_split, has_level, dilation, erosion, n_sets;
    uint32_t level;
    float activity_th, reserved_f;
    int64_t num_segments, T_long, mask_ld, lo, hi;
    int64_t mask_floats, sep_floats, costs_doubles, perms_ints, mask_st_floats, activity_floats, act_bytes, y_floats;
    CssStitchSet sets[CSS_BACKEND_MAX_SETS];
} CssStitchDesc;
int css_stitch_host(css_handle_t h, const CssStitchDesc* d, const float* masks, const float* sep, const float* windows,
                    double* costs, int32_t* perms, float* mask_st, float* activity, uint8_t* act_b, uint8_t* act_tmp,
                    uint8_t* act_final, float* Y);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CSS_MI355_BACKEND_H */
