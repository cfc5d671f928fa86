/* css_mi355_stream_kernels.h -- the kernels every live stream runs on every push, on caller data.
 *
 * An addition to css_mi355.h (included below; same library, same conventions), the companion of css_mi355_rate_kernels.h: one
 * entry per launcher of csrc/stream.hip (stream_activity_kernel, stream_gate_ola_kernel, stream_scatter_masks_kernel,
 * stream_ingest_pcm16_kernel) and of the streamed part of csrc/handoff.hip (handoff_append_kernel, handoff_mel_multi_kernel<false>
 * and <true>), for unit tests of the kernels; not on the hot path.  Each entry takes a table of plain job descriptors that name
 * caller arrays (CssKArray: address and length in elements of the array's type), uploads the inputs and the WHOLE of every output
 * allocation, makes ONE call of the launcher for the whole table exactly as tail() / handoff_round() / estimate_class() / the
 * PCM16 ingest make it (so a table longer than the kernel's own crosses into further launches), downloads everything a launch
 * could have written and synchronises, so a caller sees every element a launch did not own.  Every array is staged at a 256-byte
 * boundary with 256 bytes of room on both sides.  Refused with CSS_ERR_INVALID_ARG and a message (css_last_error) before
 * anything is launched or written: a NULL handle, table or array, an array shorter than its description, more than
 * CSS_STREAM_KERNEL_JOBS jobs, and the preconditions named with each entry: what the kernels do not guard themselves, next to
 * what the streaming path guarantees in its place.
 */
#ifndef CSS_MI355_STREAM_KERNELS_H
#define CSS_MI355_STREAM_KERNELS_H

#include "css_mi355.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define CSS_STREAM_KERNEL_JOBS 64   /* jobs per call, at most */

typedef struct CssKArray {
    void* p;
    int64_t elems;
} CssKArray;

/* ---- the stitching tail: launch_stream_activity_multi (form 0), launch_stream_gate_ola_multi (form 1) -------------------------
 * The fields are StreamStitchArgs' (csrc/kernels.hpp) and the local frame range [t_lo, t_hi).  In: masks [>= S F][mask_ld]
 * float32 (slot j at column j T), sep [num_slots][S][F][T][2], perms [num_slots][S] int32, w_first / w_mid / w_last [T].
 * act_b [S][ld_frames] bytes: out in form 0, in in form 1.  Y [S][ld_frames][KIp] float32: out of form 1.  ring [S][gate_ld]
 * bytes (has_ring; form 1): receives the gate byte of frame t at column (t + frame_base) & (gate_ld - 1).  act_b, Y and ring are
 * uploaded and downloaded whole in both forms.
 * Refused: S outside 1 .. 4, F outside 1 .. 1024, T outside 1 .. 4096, hop outside 1 .. T, jobs of one call with different S or
 * F (the launch's grid and LDS are entry 0's), KIp < 2 F, dilation or erosion outside 0 .. 4096, a gate_ld that is not a power
 * of two, num_slots T > mask_ld, a permutation entry outside 0 .. S - 1, seg_base, frame_base or num_slots < 0,
 * num_segments_global < seg_base + num_slots, t_lo < 0, t_hi < t_lo, t_hi > ld_frames, t_hi > T_long_global - frame_base, and
 * for form 1 a gate launch whose LDS, 64 (2 F + 1) + 16 + 2 (the largest erosion of the call) bytes, exceeds 64 KiB, and a range
 * under which the kernel reads act_b outside a row.  The frames of [t_lo, t_hi) take their gate from the local frames
 *     [ max(t_lo - erosion - dilation, -frame_base),  min(t_hi - 1 + erosion + dilation, T_long_global - frame_base - 1) ]
 * and both ends must lie in [0, ld_frames).  The path: rebase() keeps max(halo, 1) frames below t_g in the window (halo = dilation +
 * erosion), which is the left condition; on the right t_hi + halo = a_hi <= K <= WF for the K transformed frames of the window
 * (fit_window).  Every lane of a block of 16 frames dilates, whether or not its frame lies below t_hi, so the last block looks up
 * to 15 frames further; the path does NOT keep those inside the row (fit_window lets K reach WF = ld_frames), so the kernel itself
 * reads frames at or above ld_frames as 0.  No output depends on what lies in act_b at or above t_hi + erosion + dilation
 * (tests/test_hip_stream_kernels.py toggles it). */
typedef struct CssStreamTailJob {
    int32_t S, F, T, hop, KIp, dilation, erosion, has_ring;
    float activity_th, reserved_f;
    int64_t num_slots, seg_base, frame_base, num_segments_global, T_long_global, mask_ld, ld_frames, gate_ld, t_lo, t_hi;
    CssKArray masks, sep, perms, w_first, w_mid, w_last, act_b, Y, ring;
} CssStreamTailJob;
int css_stream_tail_host(css_handle_t h, int32_t form, CssStreamTailJob* jobs, int32_t n_jobs);

/* ---- launch_stream_scatter_masks: rows 0 .. rows - 1, columns [src_col, src_col + n_cols) of src [rows][src_ld] float32 go to
 * dst[dst_off + row dst_ld + c], c < n_cols, for every entry; dst is uploaded and downloaded whole.  Refused: rows outside
 * 1 .. 65536, src_col or n_cols < 0, src_col + n_cols > src_ld, dst_ld < n_cols, dst_off outside 0 .. 63. */
typedef struct CssStreamScatterJob {
    int64_t dst_off, dst_ld, src_col, n_cols;
    CssKArray dst;
} CssStreamScatterJob;
int css_stream_scatter_host(css_handle_t h, const float* src, int64_t src_elems, int64_t src_ld, int32_t rows, CssStreamScatterJob* jobs,
                            int32_t n_jobs);

/* ---- launch_stream_ingest_pcm16_multi: src int16, interleaved [n][C] (plane_ld = 0) or planar with channel c at src + c plane_ld,
 * staged 16-byte aligned as on the path -> dst[dst_col + c dst_ld + i] = (float)q[i][c] * 2^-15; dst is uploaded and downloaded
 * whole.  Refused: C outside 1 .. 64, jobs of one call with different C (the path's rule: the launch's tile is sized by the
 * largest), n outside 0 .. 2^24, 0 < plane_ld < n, dst_col outside 0 .. 3, dst_ld < dst_col + n. */
typedef struct CssStreamIngestJob {
    int32_t C, dst_col;
    int64_t plane_ld, n, dst_ld;
    CssKArray src, dst;
} CssStreamIngestJob;
int css_stream_ingest_host(css_handle_t h, CssStreamIngestJob* jobs, int32_t n_jobs);

/* ---- launch_handoff_append_multi.  The fields are HandoffAppend's (csrc/kernels.hpp); a state row is {int64 A, int64 J, int32 gmax,
 * int32 pad}.  In: gate [S][gate_ld] bytes (the ring; gate_mask = gate_ld - 1), out [S][out_ld] float32 (column 0 is sample
 * out_base), carry_in [S][carry_ld], tail_in [S][512], st [S] state rows.  Out: carry_out [S][carry_ld], tail_out [S][512],
 * act_out [S][t_g1 - t_g0] bytes, n_new [S] int32, and the state rows after the round: st itself (preview = 0, a push) or st_out
 * (preview = 1: gmax is copied across, st keeps its bits).  The entry computes rows = (D1 - D0 + 200) / 160 + 5 and row0 = the rows
 * of the jobs before times S, as handoff_round does, and returns them in the job; `operand` is the ONE frame operand of the call,
 * (sum of S rows) 160 + 1024 floats exactly, uploaded and downloaded whole.
 * Refused -- what the path cannot produce and the kernel does not guard: S outside 1 .. 4 or different among the jobs, pad outside
 * 0 .. 4096, a gate_ld that is not a power of two, t_g0 < 0, t_g1 < t_g0, D0 < 0, D1 < D0, D0 not a multiple of 256 (an open round
 * decides whole blocks; nothing follows a closing one), D1 - D0 above 2^24, out_base < 0, max(D1, 256 t_g1) - out_base > out_ld,
 * min(out_base, max(D1, 256 t_g1)) - D0 > carry_ld (undecided samples the carry cannot hold), 256 t_g1 - D1 > carry_ld,
 * an open round with drop and D1 > 256 max(t_g1 - pad, 0) (blocks whose keeping frames are not gated-final), a ring shorter than
 * the frames the round reads: t_g1 - min(t_g0, max(D0 / 256 - pad - 1, 0)) > gate_ld (with drop; t_g1 - t_g0 without), and a state
 * row that is not a state of an open stream: A < 0 or J != (A >= 201 ? (A - 200) / 160 + 1 : 0) (the tail is indexed from
 * 160 J - 200). */
typedef struct CssStreamAppendJob {
    int32_t pad, drop, closing, S, preview, reserved;
    int64_t gate_ld, out_ld, out_base, carry_ld, t_g0, t_g1, D0, D1, row0, rows;
    CssKArray gate, out, carry_in, carry_out, tail_in, tail_out, st, st_out, act_out, n_new;
} CssStreamAppendJob;
int css_stream_append_host(css_handle_t h, CssStreamAppendJob* jobs, int32_t n_jobs, float* operand, int64_t operand_floats);

/* ---- launch_handoff_mel_multi on caller spectra spec [402][ld] float32 (rows f: Re, 201 + f: Im; time fastest), S speakers per job.
 * Speaker k of a job owns the columns [row0 + k rows, row0 + (k + 1) rows) and writes min(n_new[k], rows) frames:
 * mel[(k n_mels + m) mel_ld + j] = log10(max(sum_f w[m][f] |X|^2, 1e-10)) with the filterbank built as the handle builds it
 * (handoff_build_mel), and folds their maximum into st[k].gmax (order-preserving integer form).  With has_ring the last `hist`
 * frames also go to ring [S][n_mels][hist] and their maxima over the bands to fmax [S][hist], frame j at slot
 * (st[k].J - n_new[k] + j) % hist; with has_pvmax the maxima over the bands go to pvmax [S][rows] instead and the table takes the
 * <true> instance, as on the path.  st, mel, ring, fmax and pvmax are uploaded and downloaded whole.
 * Refused: S outside 1 .. 4, n_mels other than 80 or 128, row0 < 0, rows outside 1 .. 2^20, row0 + S rows > ld, mel_ld < rows,
 * n_new < 0, has_ring with has_pvmax, hist < 1 with has_ring, st[k].J < n_new[k] with has_ring. */
typedef struct CssStreamMelJob {
    int32_t n_mels, has_ring, has_pvmax, reserved;
    int64_t row0, rows, hist, mel_ld;
    CssKArray n_new, st, mel, ring, fmax, pvmax;
} CssStreamMelJob;
int css_stream_mel_host(css_handle_t h, int32_t S, const float* spec, int64_t spec_elems, int64_t ld, CssStreamMelJob* jobs, int32_t n_jobs);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CSS_MI355_STREAM_KERNELS_H */
