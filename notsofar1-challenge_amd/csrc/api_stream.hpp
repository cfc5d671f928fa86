// Internal header of the host side of streamed sessions: what api_stream.hip (the window, the rounds, push / finish / preview),
// api_stream_handoff.hip (hand-off, frame history, encoder windows), api_nemo_chunk.hip (a NeMo stream's history and chunks) and
// api_stream_io.hip (rate ratio, output format, the ways samples reach the window and leave it) share.  Nothing here is exported.
#pragma once
#include "api_ctx.hpp"
#include "../../include/css_mi355_rate.h"
#include "../../include/css_mi355_preview.h"
#include "../../include/css_mi355_preview_handoff.h"
#include "../../include/css_mi355_window.h"
#include "../../include/css_mi355_present_window.h"
#include "../../include/css_mi355_stream_out.h"
#include "../../include/css_mi355_stream_nemo.h"
#include "../../include/css_mi355_nemo_chunk.h"

#include <climits>

// The host's mirrors of a hand-off stream: gate bytes of frames [hist_base, t_g) per speaker, samples appended, frames emitted,
// running maximum.  (A preview collects on a copy.)
struct HandoffMirror {
    std::vector<std::vector<uint8_t>> hist;
    int64_t hist_base = 0;
    std::vector<int64_t> A, J;
    std::vector<float> raw_max;
};

// Per stream with the hand-off on.  Nothing here is part of the window: the rebase never touches it.
struct HandoffStream {
    CssStreamHandoffCfg cfg{};
    int pad = 0;                        // pad_frames with drop_silence, else 0 (nothing waits for the gate)
    CssStreamHandoffOut* bound = nullptr;
    // gate ring [S][gate_ld] (frame t at t & gate_mask); undecided samples and concatenation tail in two generations
    DevBuf gate, carry[2], tail[2];
    int64_t gate_ld = 0, gate_mask = 0, carry_ld = 1;
    int cur = 0;
    int64_t D = 0;                      // decided samples
    HandoffMirror m;
    // the frame history (css_stream_window_open, include/css_mi355_window.h): raw frames [S][n_mels][hist_frames], frame j in slot
    // j mod hist_frames, and their maxima over the bands [S][hist_frames]; one generation, written by committed rounds only
    DevBuf ring, fmax;
    int64_t hist_frames = 0;
    // the NeMo format (css_stream_nemo_open, include/css_mi355_stream_nemo.h): everything above but the history serves it as it
    // serves Whisper's (cfg holds n_mels, pad_frames, drop_silence; tail at NEMO_TAIL_LD); the last kept sample per speaker
    // travels in two generations beside carry and tail.  A NeMo stream's history (css_stream_nemo_history_open,
    // include/css_mi355_nemo_chunk.h; api_nemo_chunk.hip) is `ring` and `hist_frames` above, without the maxima.
    bool nemo = false;
    float preemph = 0.f;
    DevBuf xlast[2];
};

// Per handle, made when the first stream switches the hand-off on.
struct HandoffCtx {
    DevBuf tab, operand, spec, res, state;   // DFT matrix + both filterbanks; frame operand; spectra; a round's results; HandoffState per (id, k)
    DevBuf state_pv;                         // a preview's closing round writes its counts and maximum here, never into `state`
    std::vector<PinnedBuf> pinned;           // staging of round r of a call
    DevBuf present; PinnedBuf present_pin;   // css_stream_windows / css_stream_present_windows: a WindowOut per window of one call, and its staging
    int32_t launches = 0, products = 0;
    int64_t frames = 0;
    // the same for the NeMo streams of a round (their own operand, spectra, results and staging: a round may have both formats)
    DevBuf nemo_operand, nemo_spec, nemo_res;
    std::vector<PinnedBuf> nemo_pinned;
    // css_stream_nemo_chunks: mean and std [2][n_mels] per chunk of one call, and their staging
    DevBuf chunk_stats; PinnedBuf chunk_pin;
};

// Per stream with a rate ratio (css_stream_set_rate; resample.hip).  Nothing here is part of the window: the rebase never touches
// it.  n_in inputs have arrived and all avail(n_in) model-rate samples they make computable are in the window (that count IS
// the stream's n_pushed); hist[cur] holds inputs [n_in - H, n_in) as float, channel-major (zeros before the recording's start),
// and every later output reads no earlier input: output avail(n_in) needs an input that has not arrived, and a chain is P <= H
// inputs long.
struct RateStream {
    ResampleRatio r{};
    int H = 0;                          // carried inputs per channel: ceil(2 half / up) + 1
    int64_t n_in = 0, max_in = 0;       // inputs so far; the most a piece takes
    int cur = 0;
    DevBuf stage, hist[2], tab;         // one piece as the caller laid it out (sized for float32); the carried inputs; the taps by phase
};

// Per stream with an output format (css_stream_set_output; resample.hip stream_output_kernel).  Nothing here is part of the
// window.  The stream's n_emitted final samples have passed the kernel and all css_stream_output_samples(n_emitted) output samples
// they make computable were written (n_total); hist[cur] holds final samples [n_emitted - H, n_emitted) per separated stream
// (zeros before the recording's start).  The launch of a round writes the other generation and only a round that makes samples
// final flips `cur`: a refused call and one that makes nothing final leave all of it alone.
struct OutputCounters { unsigned long long clipped[SMAX]; unsigned int peak[SMAX]; };
struct OutputStream {
    CssStreamOutputCfg cfg{};
    bool unity = false;
    ResampleRatio r{};                  // (1 / 1: all zero but up = down = 1)
    int H = 0;                          // carried samples per separated stream: ceil(2 half / up) + 1
    int cur = 0;
    DevBuf hist[2], tab, stage, ctr;    // the carried samples; the taps by phase; one round's output [S][stage_ld]; OutputCounters
    int64_t stage_ld = 0, n_total = 0;
    PinnedBuf pin;                      // the counters after a call
    void* bound = nullptr; int64_t cap = 0; CssStreamOutputCounts* counts = nullptr;
};

struct StreamState {
    std::unique_ptr<HandoffStream> ho;
    std::unique_ptr<RateStream> rate;
    std::unique_ptr<OutputStream> outp;
    uint32_t peak_bits[SMAX] = {};  // max |w_k| over the n_emitted final samples, as float bits
    CssRunCfg cfg{};
    std::vector<float> w;          // the three windows (cfg.w_* point here)
    int n_ch = 0, T = 0, hop = 0, halo = 0;
    int64_t n_pushed = 0, n_emitted = 0;
    bool finished = false;
    // progress in frames / segments of the recording: K frames transformed, sd segments done, act_b of frames < t_st,
    // synthesis rows and output blocks of frames < t_g
    int64_t K = 0, sd = 0, t_st = 0, t_g = 0;
    int64_t seg_base = 0;
    int64_t WF = 0, WS = 0, SC = 0, piece = 0;   // window: frames, samples, segment slots; samples per piece
    int cur = 0;
    DevBuf pcm[2], X[2], masks[2], sep[2], perms[2], act_b[2], G[2];
    DevBuf scm, bfw, pnorm, costs, pit_part, Y, out, segw;
    std::vector<float> host_cm;    // one piece, channel-major (float pushes)
    DevBuf pcm16_stage;            // one piece of int16 as the caller laid it out, from the first PCM16 push on
};

inline StreamState* get_stream(css_ctx* h, int32_t id) { return id < 0 || id >= CSS_MAX_STREAMS ? nullptr : h->streams[id]; }

inline int64_t frames_of(int64_t n) { return n < 512 ? 0 : (n - 512) / 256 + 1; }
// segments whose frames are all known and which are not the last segment of the recording, whatever follows
inline int64_t segments_done(int64_t K, int T, int hop) { return K > T ? (K - 1 - T) / hop + 1 : 0; }
inline int64_t final_frames(int64_t n, int T, int hop, int halo) {
    return std::max<int64_t>(segments_done(frames_of(n), T, hop) * hop - halo, 0);
}

// One item of a push: its samples come as float32 [n][C] or as int16 with strides.
struct PushItem {
    int32_t id;
    const float* f32;                                   // float call: [n_samples][C]
    const int16_t* i16; int64_t sample_stride, channel_stride;   // PCM16 call
    int64_t n_samples; float* out_host; int64_t cap; int64_t* n_out;
};

// What the host needs after the call's synchronise to hand out the results of one stream's share of a hand-off round (handoff_round).
struct HandoffRec {
    StreamState* s; int item; int64_t t_g0, t_g1, D0, D1, n_out; bool closing;
    const uint8_t* act; const int32_t* n_new; const float* mel; int64_t mel_ld; const HandoffState* st;   // in page-locked staging
    const int32_t* n_new_dev; const float* mel_dev; const float* pvmax_dev;   // the round's results on the device (pvmax_dev: a round with windows)
};

// One stream's share of a round, from "its samples are in the window" to "its downloads are queued" (api_stream.hip stream_round).
// The caller says where the round takes the stream: K1 frames transformed, segments below nseg done, activity bits of frames below
// a_hi, gate and synthesis of frames below t_hi, output blocks below q_hi, n_new more final samples.  A closing round ends the
// recording by its plan (nseg, TL = mix_frames, n_out) behind zeroed planes of the local frames [K1 - frame base, z_hi) and moves
// nothing of the stream; any other round moves K and sd where a push always moved them.
struct RoundJob {
    StreamState* s; int item;
    int64_t K1, nseg, a_hi, t_hi, q_hi, n_new;
    bool closing = false; int64_t TL = 0, n_out = 0, z_hi = 0;
    bool handoff = true;                           // the gate ring receives the round's gate bytes and the hand-off round takes the stream
    float* out_host = nullptr; int64_t cap = 0;    // the n_new samples -> out_host[S][cap] at column `done`, the samples final earlier in the call
    int64_t done = 0, written = 0;                 // (written: the same count at the output format's rate, the bound buffer's column)
    int64_t n_m = 0;                               // <- output samples the round wrote to the bound buffer
    CssStreamPresentWindow* windows = nullptr;     // css_stream_present_windows: the item's windows up to the present,
    int32_t n_windows = 0; size_t win0 = 0;        // and the index of its first one among the call's
};

// What one css_stream_present_windows call launches: `total` windows over all jobs, `launches` kernel launches; after the call's
// synchronise `res` (page-locked) holds the spans the kernel resolved, window RoundJob::win0 + w of a job at that index.
struct PresentCall { size_t total = 0; int32_t launches = 0; const WindowOut* res = nullptr; };

// ---- api_stream.hip
int check_stream_cfg(const CssModelDesc& d, const CssRunCfg* cfg);
const char* queued_refusal(const css_ctx* h);
int check_stream_call(css_ctx* h, int32_t id, StreamState** out);
int refuse_item(css_ctx* h, int code, size_t i, int32_t id, const std::string& msg);

// ---- api_stream_handoff.hip
int check_handoff_out(const StreamState* s, const CssStreamHandoffOut* o, int64_t n_samples, std::string* why);
int check_handoff_call(const StreamState* s, int64_t n_samples, std::string* why);
void handoff_begin_call(css_ctx* h);
int handoff_round(css_ctx* h, const std::vector<RoundJob>& all, size_t round, std::vector<HandoffRec>* recs, bool commit);
int handoff_collect(css_ctx* h, StreamState* s, int item, int64_t t_g_before, const std::vector<HandoffRec>& recs, HandoffMirror& mir,
                    CssStreamHandoffOut* out, bool commit);
template <typename W>
const char* window_refusal(const css_ctx* h, const HandoffStream* o, const W& w, const int64_t* first_frame);
int present_windows(css_ctx* h, const std::vector<RoundJob>& jobs, const std::vector<HandoffRec>& recs, PresentCall* pc);

// ---- api_stream_io.hip
int64_t model_samples_after(const StreamState* s, int64_t more);
ResampleJob rate_job(StreamState* s, bool i16, bool planar, int64_t n_in, int64_t m1, float* win, bool flush);
int stage_piece(css_ctx* h, StreamState* s, const PushItem& p, bool pcm16, bool planar, int64_t done, int64_t n_in, int64_t n, float* win,
                std::vector<ResampleJob>* rsj, std::vector<StreamIngestPcm16>* ing, bool* host_staging);
int check_output_call(const StreamState* s, int64_t need, bool finished, std::string* why);
int output_job(css_ctx* h, StreamState* s, int64_t done, int64_t n, int64_t src_ld, bool finished, StreamOutputJob* j, int64_t* n_m);
int output_download(css_ctx* h, StreamState* s, int64_t n_m, int64_t at);
int output_counters(css_ctx* h, StreamState* s);
void output_report(css_ctx* h, StreamState* s, int64_t written);
void output_report_idle(css_ctx* h, StreamState* s);
void host_peak(css_ctx* h, StreamState* s, const float* out, int64_t cap, int64_t n);
