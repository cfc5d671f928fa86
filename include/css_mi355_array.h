/* css_mi355_array.h -- the MVDR kernels of csrc/mvdr.hip for microphone arrays of 2 to 8 channels, on caller data.
 *
 * An addition to css_mi355.h (included below; same library, same conventions), the companion of css_mi355_backend.h, whose
 * css_mvdr_host stays the entry of the 7-microphone kernels.  A model of `num_mics` 2 .. 8 runs every path of css_mi355.h
 * (css_run, queued sessions, streams); this entry makes the covariance, solve and beamformer launches of such a model on arrays
 * the caller chooses, for unit tests of the arithmetic; not on the hot path.  It uploads the inputs and the WHOLE of every output
 * allocation, makes the launch exactly as the path makes it, downloads every allocation a launch could have written and
 * synchronises.  Whatever a kernel's own comment excludes is refused with CSS_ERR_INVALID_ARG and a message (css_last_error)
 * before anything is launched or written.  Lengths are in elements of the array's type.
 *
 * Layouts for C microphones: a covariance matrix is packed Hermitian, C real diagonal entries, then (Re, Im) of the entries
 * (c, d), c < d, row by row -- C C doubles (49 at C = 7, the layout of css_mi355_backend.h); the beamformer weights of a
 * (segment, speaker, bin) are [C][2] doubles.
 */
#ifndef CSS_MI355_ARRAY_H
#define CSS_MI355_ARRAY_H

#include "css_mi355.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define CSS_ARRAY_MAX_SETS 16
#define CSS_ARRAY_MIN_MICS 2
#define CSS_ARRAY_MAX_MICS 8

/* One argument set of the multi-session solve (form 2): segments [seg_lo, seg_lo + nseg) of a session whose covariances start
 * at scm + scm_off and whose weights start at bfw + bfw_off (offsets in doubles). */
typedef struct CssMvdrArraySet {
    int64_t seg_lo, nseg, scm_off, bfw_off;
} CssMvdrArraySet;

/* X [C][2 F][T_ld] planes, masks [(S + 1) F][mask_ld] (segment s at column s T), override [segments][F][T] bytes or NULL, scm
 * [segments][S + 1][F][C C] doubles, bfw [segments][S][F][C][2] doubles, sep [segments][S][F][T][2] floats; `segments` =
 * seg_lo + nseg.  form:
 *   0  launch_scm (its own dispatch: the tile kernel of T <= 192, <= 256 or <= 512 frames, the any-length kernel beyond 512 frames
 *      or with CSS_FORCE_LONG_PATH in the environment): reads X, masks, override; scm is uploaded and downloaded whole
 *   1  launch_mvdr_solve: reads scm; bfw is uploaded and downloaded whole
 *   2  launch_mvdr_solve_multi over sets[0 .. n_sets): as form 1 per set (seg_lo and nseg of the descriptor are not used)
 *   3  launch_beamform (use_mvdr 0 / 1, mask_floor): reads X, masks and, with use_mvdr, bfw; sep is uploaded and downloaded whole
 * Arrays a form does not read or write may be NULL.  Refused: C outside 2 .. 8, S outside 1 .. 3, F outside 1 .. 4096, T outside
 * 1 .. 65535, hop < 1, nseg outside 1 .. 4096, seg_lo < 0, mask_ld < (seg_lo + nseg) T, mask_ld or T_ld above 2^28, T_ld shorter
 * than the last valid frame min(stft_frames, (seg_lo + nseg - 1) hop + T), an override byte that is neither a winner index below
 * S + 1 nor 16 | bits with a bit below S + 1 set, n_sets outside 1 .. CSS_ARRAY_MAX_SETS, a set outside its arrays, short arrays. */
typedef struct CssMvdrArrayDesc {
    int32_t form, C, F, S, T, hop, nseg, use_mvdr, n_sets, reserved;
    float mask_floor, reserved_f;
    int64_t seg_lo, stft_frames, T_ld, mask_ld;
    int64_t x_floats, mask_floats, override_bytes, scm_doubles, bfw_doubles, sep_floats;
    CssMvdrArraySet sets[CSS_ARRAY_MAX_SETS];
} CssMvdrArrayDesc;
int css_mvdr_array_host(css_handle_t h, const CssMvdrArrayDesc* d, const float* X, const float* masks, const uint8_t* wta_override,
                        double* scm, double* bfw, float* sep);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CSS_MI355_ARRAY_H */
