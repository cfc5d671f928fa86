/* css_mi355_stream_nemo.h -- the NeMo hand-off of a stream: raw NeMo log-mel frames as samples become final.
 *
 * An addition to css_mi355.h (included below; same library, same conventions): the streamed counterpart of
 * css_mi355_nemo_handoff.h, as css_stream_handoff_* is the streamed counterpart of css_handoff_logmel.  A stream opened with
 * css_stream_nemo_open returns with every push (css_stream_push*, every item of css_stream_push_many*) and with css_stream_finish,
 * per separated stream k:
 *   - the gate bits that became final in the call and the sample ranges the call appended to k's concatenation of kept samples:
 *     the range rule, the decided samples D, pad_frames and drop_silence are EXACTLY the Whisper stream hand-off's
 *     (css_mi355.h "the hand-off of a stream");
 *   - the RAW NeMo frames ln(mel + 2^-24) that became complete, [n_mels][n] float32, time fastest: the features of NeMo's
 *     AudioToMelSpectrogramPreprocessor with `normalize: NA` -- what cache-aware streaming FastConformer, streaming diarizers
 *     and frame-level VAD take, or normalise per short window themselves.
 * With A kept samples appended so far and y their pre-emphasised concatenation (y[0] = x[0], y[c] = x[c] - p x[c - 1], product
 * and difference rounded apart; x[c - 1] is the last kept sample before, across a seam and across calls), frame j reads
 * y[160 j - 256, 160 j + 256) with zeros below 0.  An open stream emits frame j once A >= 160 j + 256 -- J = A >= 256 ?
 * (A - 256) / 160 + 1 : 0 frames -- and finish emits the rest up to A / 160, with zeros from y[A] on.  (The window's taps are
 * zero outside [56, 456): a frame waits for at most 56 samples it multiplies by zero, so that every emitted operand row is the
 * offline gather's row, float for float.)
 * For a finished stream all frames of k are the raw (normalize = 0) frames the session call of css_mi355_nemo_handoff.h returns
 * for k after css_run_device on the whole recording, bit for bit, over any cutting into pushes; the merged ranges and the gate
 * bits are that call's too.
 *
 * The results use CssStreamHandoffOut and css_stream_handoff_bind (css_mi355.h): raw_max is never written for a NeMo stream and
 * may be NULL.  The bind, the refusal of an unbound stream and "capacities below the bounds leave every stream of the call
 * unchanged" are the Whisper hand-off's rules.  A stream has ONE format: css_stream_nemo_open on a stream with either hand-off
 * on, and css_stream_handoff_open on a NeMo stream, are CSS_ERR_STATE.  A NeMo stream takes float and PCM16 pushes, a rate ratio
 * (css_mi355_rate.h) and an output format (css_mi355_stream_out.h) as a Whisper hand-off stream does -- the hand-off reads the
 * model-rate output behind those stages -- and pushes alone or in groups mixed with plain and Whisper streams: a round costs
 * three launches for all its NeMo streams (append, ONE product, mel; tables of 16 streams), besides Whisper's three where the
 * round has Whisper streams; css_stream_handoff_stats counts both.
 * Refused with CSS_ERR_STATE and a message, for a NeMo stream: a preview with hand-off (css_mi355_preview_handoff.h; a plain
 * preview, css_mi355_preview.h, works and leaves the NeMo state untouched), Whisper's frame history and encoder windows
 * (css_mi355_window.h) and windows up to the present (css_mi355_present_window.h).  A NeMo stream's own frame history, and chunks
 * of it written on the device, are css_mi355_nemo_chunk.h's.
 * Out of scope: per-band normalisation over the whole recording (a live consumer cannot have it before the end), float16 frames,
 * other frame geometries.
 */
#ifndef CSS_MI355_STREAM_NEMO_H
#define CSS_MI355_STREAM_NEMO_H

#include "css_mi355.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

/* n_mels 80 / 128, pad_frames 0 .. 4096, preemphasis finite with 0 <= p < 1 (0: y = x) */
typedef struct CssStreamNemoCfg {
    int32_t n_mels, pad_frames, drop_silence;
    float preemphasis;
} CssStreamNemoCfg;

/* Before the stream's first sample and once.  CSS_ERR_STATE after the first sample, when a hand-off of either format is on
 * already, and in CSS_LINEAR_SPLIT_F16; CSS_ERR_INVALID_ARG for other values. */
int css_stream_nemo_open(css_handle_t h, int32_t id, const CssStreamNemoCfg* cfg);
/* Pure host arithmetic: capacities that suffice for a push of n_samples (css_stream_finish: n_samples = -1). */
int css_stream_nemo_bounds(const CssModelDesc* desc, const CssRunCfg* cfg, const CssStreamNemoCfg* ncfg, int64_t n_samples,
                           int64_t* frames, int32_t* ranges, int64_t* activity);
/* Pure, drop_silence = 0 only: NeMo frames that are final after n_pushed samples of an open stream. */
int css_stream_nemo_final_frames(const CssModelDesc* desc, const CssRunCfg* cfg, const CssStreamNemoCfg* ncfg, int64_t n_pushed,
                                 int64_t* n_frames);

/* ---- the two kernels of a NeMo round on caller data (unit tests of the kernels; the conventions of css_mi355_stream_kernels.h:
 * a job names caller arrays by address and length in elements, the inputs and the WHOLE of every output allocation are uploaded,
 * ONE launcher call is made for the table, everything a launch could have written is downloaded; refusals with
 * CSS_ERR_INVALID_ARG and a message before anything is launched or written; at most 64 jobs) -------------------------------------
 * launch_nemo_append_multi.  The job is the Whisper append entry's (that header; csrc/kernels.hpp NemoAppend), field for field,
 * and so are its refusals, with these differences: tail_in / tail_out are [S][512] floats of y[160 J - 256, A) (zeros where that
 * lies before the recording's start); a state row {int64 A, int64 J, int32, int32} of an open stream has
 * J = A >= 256 ? (A - 256) / 160 + 1 : 0; there is no preview (st is written in place, its two int32 words are left alone); the
 * entry computes rows = (D1 - D0 + 256) / 160 + 6 and row0 and returns them in the job; `operand` holds (sum of S rows) 160 + 1024
 * floats exactly.  xlast_in / xlast_out [S] float32: the last kept sample before / after the round (another array; xlast_in is
 * not read for a speaker with A = 0).  preemphasis as in CssStreamNemoCfg. */
typedef struct CssStreamNemoArray {
    void* p;
    int64_t elems;
} CssStreamNemoArray;
typedef struct CssStreamNemoAppendJob {
    int32_t pad, drop, closing, S;
    float preemphasis;
    int32_t reserved;
    int64_t gate_ld, out_ld, out_base, carry_ld, t_g0, t_g1, D0, D1, row0, rows;
    CssStreamNemoArray gate, out, carry_in, carry_out, tail_in, tail_out, st, act_out, n_new, xlast_in, xlast_out;
} CssStreamNemoAppendJob;
int css_stream_nemo_append_host(css_handle_t h, CssStreamNemoAppendJob* jobs, int32_t n_jobs, float* operand, int64_t operand_floats);

/* launch_nemo_mel_multi on caller spectra spec [514][ld] float32 (rows f: Re, 257 + f: Im; time fastest), S speakers per job.
 * Speaker k of a job owns the columns [row0 + k rows, row0 + (k + 1) rows) and writes min(n_new[k], rows) frames:
 * mel[(k n_mels + m) mel_ld + j] = ln(sum_f w[m][f] |X|^2 + 2^-24) with the handle's slaney bank at 257 bins.  mel is uploaded
 * and downloaded whole.  Refused: S outside 1 .. 4, n_mels other than 80 or 128, row0 < 0, rows outside 1 .. 2^20,
 * row0 + S rows > ld, mel_ld < rows, n_new < 0. */
typedef struct CssStreamNemoMelJob {
    int32_t n_mels, reserved;
    int64_t row0, rows, mel_ld;
    CssStreamNemoArray n_new, mel;
} CssStreamNemoMelJob;
int css_stream_nemo_mel_host(css_handle_t h, int32_t S, const float* spec, int64_t spec_elems, int64_t ld, CssStreamNemoMelJob* jobs,
                             int32_t n_jobs);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CSS_MI355_STREAM_NEMO_H */
