/* css_mi355_frontend.h -- the kernels of csrc/stft.hip and csrc/frontend.hip on caller data.
 *
 * An addition to css_mi355.h (included below; same library, same conventions), the companion of css_mi355_encoder.h: one entry
 * per kernel family -- the analysis FFT with its phase planes, the feature kernels, the synthesis tail (overlap-add, shard
 * join, planes to rows) and the PCM edges -- for unit tests of the arithmetic; not on the hot path.  Each entry takes caller
 * arrays and a plain descriptor, uploads the inputs and the WHOLE of every output allocation, makes the launch exactly as the
 * path makes it, downloads everything a launch could have written and synchronises, so a caller sees every float a launch did
 * not own.  Whatever a kernel's own comment excludes is refused with CSS_ERR_INVALID_ARG and a message (css_last_error) before
 * anything is launched or written: a NULL handle or descriptor, an array shorter than its description, and the preconditions
 * named at each entry.  Lengths are in elements of the array's type; a split-f16 output (split_f16.hpp) has the float count of
 * its float32 form.
 */
#ifndef CSS_MI355_FRONTEND_H
#define CSS_MI355_FRONTEND_H

#include "css_mi355.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

/* launch_stft_fft: frames [t_lo, t_hi) of C channels (frame t = samples [256 t, 256 t + 512) of x [C][x_stride]) into the planes
 * out[offset + (c 514 + r) row_ld + t], r = f (Re) / 257 + f (Im), and, with want_phase, the phase planes
 * phase[offset + (c 257 + f) row_ld + t].  The tables are stft_build_tables(window) (0: hann, 1: sqrt_hann / 16), as the handle
 * builds them.  offset (0 .. 3 floats) is added to the 256-byte-aligned staging of out AND of phase: offset 0 with
 * row_ld % 4 == 0 takes the float4 stores, anything else the scalar ones.  out [out_floats] and phase [phase_floats] are
 * uploaded and downloaded whole.  Refused: an odd x_stride (the kernel reads samples as float2), t_lo < 0, t_hi < t_lo,
 * row_ld < t_hi, x_stride < 256 (t_hi - 1) + 512. */
typedef struct CssAnalysisDesc {
    int32_t C, t_lo, t_hi, offset, window, want_phase;
    int64_t x_stride, row_ld, x_floats, out_floats, phase_floats;
} CssAnalysisDesc;
int css_analysis_host(css_handle_t h, const CssAnalysisDesc* d, const float* x, float* out, float* phase);

/* launch_features: segments [seg_lo, seg_lo + nseg) of T frames, hop frames apart, from the planes X [C][2 F][T_ld] (and the
 * phase planes PH [C][F][T_ld], or NULL) into feat [nseg T][Kp], float32 or split-f16 rows (split_out); in_bias and in_scale
 * [F (1 + pairs)].  Frames at or past stft_frames are X = 0 and are not read.  The dispatch between the tuned kernels and the
 * any-length one stays launch_features' own (T > 512, or CSS_FORCE_LONG_PATH in the environment).  feat [feat_floats] is
 * uploaded and downloaded whole.  Refused: T < 2, Kp < F (1 + pairs), Kp % 32 with split_out, more than 16 pairs, a pair
 * index outside [0, C), a version outside 1 .. 3 with ipd_mean_normalize, stft_frames > T_ld. */
typedef struct CssFeaturesDesc {
    int32_t C, F, nseg, T, hop, Kp, split_out, reserved;
    int64_t T_ld, stft_frames, seg_lo, x_floats, ph_floats, feat_floats;
    CssFeatureCfg cfg;
} CssFeaturesDesc;
int css_features_host(css_handle_t h, const CssFeaturesDesc* d, const float* X, const float* PH, const float* in_bias,
                      const float* in_scale, float* feat);

/* The kernels behind the synthesis GEMM.  form:
 *   0  launch_wave_ola: in = G [B][T_frames][L] -> out [B][out_ld], output blocks [q_lo, q_hi) of hop samples from the frames
 *      [f_lo, f_hi), block q at out + (q - out_q0) hop; has_level = 1 passes a device word holding `level` (float bits of the
 *      recording's peak, split_f16.hpp level_gain), 0 passes NULL
 *   1  launch_join_shards: in = gathered [world][S][ld], rank k holding blocks t_lo[k] .. t_hi[k] -> out [S][out_ld], n_out
 *      samples per stream
 *   2  launch_planes_to_rows: in = planes [B][F2][T_frames] -> out rows [B][T_frames][KIp]
 * out [out_floats] is uploaded and downloaded whole.  Refused: q_lo < out_q0, frames outside [0, T_frames], hop > L (form 0);
 * hop % 4 or ld % 4 (the join's float4 reads), world outside 1 .. 64, a rank whose blocks do not fit ld (form 1);
 * KIp < F2 (form 2). */
typedef struct CssSynthesisTailDesc {
    int32_t form, B, hop, L, world, S, F2, KIp, has_level;
    uint32_t level;
    int64_t T_frames, q_lo, q_hi, f_lo, f_hi, out_ld, out_q0, ld, n_out, in_floats, out_floats;
    int64_t t_lo[64], t_hi[64];
} CssSynthesisTailDesc;
int css_synthesis_tail_host(css_handle_t h, const CssSynthesisTailDesc* d, const float* in, float* out);

/* The PCM edges.  form:
 *   0  launch_deinterleave: in float [n][C] -> out float [C][n_pad], samples [i_lo, i_hi), zeros past n; split_out 0 / 1
 *   1  launch_pcm16_to_float: in int16 [C][n] -> out float [n][C]
 *   2  launch_pcm16_to_channel_major: in int16 [C][n] -> out float [C][n_pad], samples [i_lo, i_hi)
 *   3  launch_pcm_peak_f32: in float [src_offset + count]; the launch gets in + src_offset of a 16-byte-aligned staging
 *   4  launch_pcm_peak_i16: the same on int16
 *   5  launch_encode_pcm16: in float [S][n] -> out int16 [S][out_ld]; peak [S] receives the peaks as float bits
 * Forms 3 and 4: the peak word holds peak_before when the launch starts and *peak receives it afterwards; out is NULL.
 * in [in_elems] and out [out_elems] are in elements of their types; out is uploaded and downloaded whole.  Refused:
 * i_lo < 0, i_hi > n_pad, n_pad % 32 with split_out, src_offset outside 0 .. 7, out_ld < n. */
typedef struct CssPcmEdgesDesc {
    int32_t form, C, split_out, S, src_offset;
    uint32_t peak_before;
    int64_t n, n_pad, i_lo, i_hi, count, out_ld, in_elems, out_elems;
} CssPcmEdgesDesc;
int css_pcm_edges_host(css_handle_t h, const CssPcmEdgesDesc* d, const void* in, void* out, uint32_t* peak);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CSS_MI355_FRONTEND_H */
