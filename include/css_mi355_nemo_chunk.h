/* css_mi355_nemo_chunk.h -- NeMo feature chunks assembled on the device, out of a NeMo stream's own frame history.
 *
 * An addition to css_mi355_stream_nemo.h (included below; same library, same conventions): the NeMo counterpart of
 * css_mi355_window.h.  The NeMo hand-off of a stream returns, with every push, the RAW frames ln(mel + 2^-24) that became
 * complete, in host memory.  A live NeMo consumer takes CHUNKS of them on the GPU: cache-aware streaming FastConformer takes
 * [n_mels][pre-encode cache + chunk] raw frames per step (`normalize: NA`); buffered inference (FrameBatchASR, the streaming
 * diarizer, frame-level VAD) takes a buffer of some seconds normalised PER FEATURE OVER THE BUFFER.  A NeMo stream that was given
 * a frame history keeps its last history_frames raw frames per separated stream in device memory, and css_stream_nemo_chunks
 * writes any number of chunks -- a span of those frames, raw or normalised per band over the span, padded to a width, as float32
 * or float16 -- straight into device memory of the caller's, for example a torch tensor.  For the raw frames raw[m][0 .. n) of the
 * span, n = n_frames:
 *   CSS_NEMO_CHUNK_RAW           column c < n of row m is raw[m][c], bit for bit what the pushes returned
 *   CSS_NEMO_CHUNK_PER_FEATURE   column c < n of row m is (raw[m][c] - mean[m]) / (std[m] + 1e-5f) in float32, each step rounded
 *                                once (the session call's expression, css_mi355_nemo_handoff.h)
 *   columns n .. width - 1       pad_value, never normalised (NeMo's pad_value: 0)
 *   float16                      that float32 value rounded to nearest-even
 * mean[m] and std[m] (unbiased; 0 for n = 1) are float64 sums in ONE fixed order, each result rounded to float32 once:
 *   pass one   lane l of 64 adds frames l, l + 64, ... in increasing order, then x[l] += x[l + s] for s = 32, 16, .. 1;
 *              mean = x[0] / n
 *   pass two   d = (double)raw - mean, d * d and the addition rounded apart, in the same order; std = sqrt(x[0] / (n - 1))
 * so they depend on the span's values and n alone -- not on the ring slot the span starts in, on a wrap inside the span, on width,
 * ld, dtype, the alignment of out_dev, the item's place in the table or the other items -- and a numpy statement of them is exact
 * (stream.py nemo_chunk_features).  Nothing of the hand-off changes: the frames still arrive in the bound CssStreamHandoffOut, and
 * a stream without a history holds and returns what it did.
 *
 * Not covered: chunks that go on over a preview's provisional frames (previews with hand-off of a NeMo stream stay refused; a
 * plain preview never writes the history), caller-supplied or running statistics, bfloat16, spans longer than 3000 frames.
 */
#ifndef CSS_MI355_NEMO_CHUNK_H
#define CSS_MI355_NEMO_CHUNK_H

#include "css_mi355_stream_nemo.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

enum { CSS_NEMO_CHUNK_RAW = 0, CSS_NEMO_CHUNK_PER_FEATURE = 1 };
#define CSS_NEMO_CHUNK_MAX_WIDTH 3000   /* columns of a chunk, at most */
#define CSS_NEMO_CHUNK_TABLE 32         /* chunks per kernel launch of css_stream_nemo_chunks */

/* Gives a NeMo stream its frame history: after the NeMo hand-off was switched on (css_mi355_stream_nemo.h) and before the stream's
 * first sample.  A stream without the NeMo hand-off (the message names a Whisper hand-off stream: its history is
 * css_stream_window_open's), a stream that has taken samples or has finished, and a second call are CSS_ERR_STATE;
 * history_frames outside 32 .. 2^20 is CSS_ERR_INVALID_ARG; on any refusal the stream stays as it was.  From then on every push and
 * css_stream_finish also leaves the frames it completes in a ring on the device -- frame j of separated stream k's concatenation
 * (the index CssStreamHandoffOut counts frames in) in slot j mod history_frames, with the same float32 values it writes to
 * mel_host -- so that after any call the ring holds frames [max(J_k - history_frames, 0), J_k), J_k the frames returned for k so
 * far.  A preview never writes it.  The launch count of a round (css_stream_handoff_stats) is unchanged: three for all its NeMo
 * streams.
 * Device memory, allocated here and counted in CssStreamInfo.device_bytes from here on: the ring, float32
 * [S][n_mels][history_frames]. */
int css_stream_nemo_history_open(css_handle_t h, int32_t id, int32_t history_frames);

/* The frames the history of stream `id` holds now: [first_frame[k], end_frame[k]) for k < S.  A stream without a NeMo history is
 * CSS_ERR_STATE.  A finished stream that is not closed yet keeps its history. */
int css_stream_nemo_history_range(css_handle_t h, int32_t id, int64_t* first_frame /*[S]*/, int64_t* end_frame /*[S]*/);

typedef struct CssStreamNemoChunk {
    int32_t id, speaker;
    int64_t first_frame;   /* frame of the speaker's concatenation, the index CssStreamHandoffOut counts in */
    int32_t n_frames;      /* 1 .. width */
    int32_t width;         /* columns written, n_frames .. 3000 */
    int32_t dtype;         /* 0: float32, 1: float16 (the values of CSS_WINDOW_F32 / CSS_WINDOW_F16, css_mi355_window.h) */
    int32_t normalize;     /* CSS_NEMO_CHUNK_RAW, CSS_NEMO_CHUNK_PER_FEATURE */
    float   pad_value;     /* finite; columns n_frames .. width - 1 */
    int32_t reserved;      /* 0 */
    void*   out_dev;       /* device memory, [n_mels][ld] elements of dtype, aligned to the element size only */
    int64_t ld;            /* >= width */
    float*  mean_host;     /* [n_mels] each, may be NULL: the statistics of a PER_FEATURE chunk, written after the call's */
    float*  std_host;      /* synchronise (left alone for a RAW chunk) */
} CssStreamNemoChunk;

/* Writes n_items chunks, of any NeMo streams and speakers of the handle in any order (a stream or a span may appear many times),
 * on the handle's stream, and returns after ONE synchronise; no stream's state changes.  Item i: frames [first_frame, first_frame +
 * n_frames) of the speaker's history by the rule at the top into out_dev[m * ld + c], m < n_mels, c < width; nothing else of
 * out_dev is written.
 * All items are checked before anything is launched: an id without an open stream or a stream without a NeMo history (a Whisper
 * stream's windows are css_stream_windows'), a speaker outside 0 .. S - 1, frames outside css_stream_nemo_history_range,
 * n_frames < 1, width outside n_frames .. 3000, ld < width, an unknown dtype or normalize, a pad_value that is not finite, a
 * reserved that is not 0, a NULL out_dev or one not aligned to the element size refuse the WHOLE call with CSS_ERR_INVALID_ARG;
 * css_last_error names the item's index and id, and nothing is written.
 * Cost: one kernel launch per CSS_NEMO_CHUNK_TABLE items, whatever streams they name; *launches (may be NULL) receives the count. */
int css_stream_nemo_chunks(css_handle_t h, CssStreamNemoChunk* items, int32_t n_items, int32_t* launches);

/* ---- the two kernels on caller data (unit tests of the kernels; the conventions of css_mi355_stream_kernels.h: a job names caller
 * arrays by address and length in elements, the inputs and the WHOLE of every output allocation are uploaded, ONE launcher call is
 * made per table, everything a launch could have written is downloaded; refusals with CSS_ERR_INVALID_ARG and a message before
 * anything is launched or written; at most 64 jobs) ----------------------------------------------------------------------------
 * nemo_chunk_kernel on a caller ring [n_mels][hist] float32, hist >= 1, that holds frames [max(end_frame - hist, 0), end_frame) of
 * one speaker, frame j in slot j mod hist: the chunk of frames [first_frame, first_frame + n_frames) by CssStreamNemoChunk's rule
 * and refusals (n_mels 80 or 128; frames outside the ring's are refused) into out[out_offset + m ld + c] -- out is float32 words,
 * or 16-bit words of float16, uploaded and downloaded whole.  mean / std [n_mels] float32 are uploaded and downloaded whole too: a
 * PER_FEATURE chunk writes them, a RAW chunk leaves them.  One launch per 32 jobs. */
typedef struct CssNemoChunkArray {
    void* p;
    int64_t elems;
} CssNemoChunkArray;
typedef struct CssNemoChunkJob {
    int32_t n_mels, n_frames, width, dtype, normalize;
    float pad_value;
    int64_t hist, end_frame, first_frame, ld, out_offset;
    CssNemoChunkArray ring, out, mean, std;
} CssNemoChunkJob;
int css_nemo_chunk_host(css_handle_t h, CssNemoChunkJob* jobs, int32_t n_jobs);

/* The mel kernel of a NeMo round with a frame history, on caller data: the mel entry of css_mi355_stream_nemo.h -- its spectra, its
 * fields n_mels, row0, rows, mel_ld, n_new, mel, its rules and its refusals -- with a caller ring [S][n_mels][hist] float32,
 * hist >= 1, uploaded and downloaded whole, and frames_after [S] int64, every speaker's frame count AFTER the round (>= n_new): the
 * round's frame j < min(n_new, rows) of speaker k is frame frames_after[k] - n_new[k] + j and goes to slot (that) mod hist iff
 * j >= n_new[k] - hist.  mel is what that entry writes for the same job, bit for bit. */
typedef struct CssStreamNemoMelHistoryJob {
    int32_t n_mels, reserved;
    int64_t row0, rows, mel_ld, hist;
    CssNemoChunkArray n_new, mel, ring, frames_after;
} CssStreamNemoMelHistoryJob;
int css_stream_nemo_mel_history_host(css_handle_t h, int32_t S, const float* spec, int64_t spec_elems, int64_t ld,
                                     CssStreamNemoMelHistoryJob* jobs, int32_t n_jobs);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CSS_MI355_NEMO_CHUNK_H */
