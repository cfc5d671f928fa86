// libcss_mi355.so, host side of streamed sessions (css_stream_*): samples arrive in chunks of any size, every push returns the
// output samples that became final, and what a finished stream returned is css_run's result bit for bit.  (DESIGN.md
// "Streaming separation": the finality rule, the window, what is refused.)
//
// A stream keeps a linear WINDOW of the recording on the device: local frame 0 is frame seg_base * hop of the recording,
// local segment slot j is segment seg_base + j.  Every buffer (samples, analysis planes, masks, spectra, permutations,
// activity bits, synthesis rows) is indexed locally; when a piece would run past the window's end, the live tail is copied
// to the front of a second set of buffers (rebase) and the two sets swap.  The window's size follows from the segmentation
// alone, so an 8-hour stream holds what a 1-minute one holds.  A push is cut into pieces of at most PIECE_SEGMENTS
// segments' worth of samples, so a push of any length fits the window too.
//
// What runs per piece is the offline path's own code on the window: the analysis FFT over the new frames, the mask estimator
// over the segments the piece completed (one batch), covariances / MVDR / power normalisation, the stitching costs and the
// permutation scan (continued from the last segment's permutation), then stream.hip's two stitching kernels and the
// synthesis GEMM + overlap-add over the newly final frames.
//
// There is one push path: push_items, behind css_stream_push_many (float32 samples) and css_stream_push_many_pcm16 (int16
// samples, converted on the device).  It takes piece r of every item in round r, and the segments a round completes
// in all streams of one segmentation pass the estimator as ONE batch (every estimator kernel is batch invariant in exact
// float32, as for queued sessions: api_queue.hip run_group), so N live meetings cost about one estimator pass per tick
// instead of N.  css_stream_push(_pcm16) is a group of one item; css_stream_finish and the previews (css_stream_preview*,
// include/css_mi355_preview.h, css_mi355_preview_handoff.h) run the same segments() / tail() in closing_pass: finish with one job,
// a preview with N and no commit.
//
// The hand-off (css_stream_handoff_*): a stream that has it switched on also returns, with every call, the gate
// bits, the kept sample ranges and the raw Whisper log-mel frames that became final.  The step sits between tail() and the
// downloads of a round: three launches for all streams of the round (handoff.hip: append, ONE DFT product, mel), results
// into page-locked staging under the call's final synchronise, where the host trims them into the caller's buffers.
//
// A stream with a rate ratio (css_stream_set_rate, include/css_mi355_rate.h) takes its pushes at the capture rate:
// a piece is copied as the caller laid it out into the stream's device staging and ONE launch per round (resample.hip) filters,
// decimates and de-interleaves the rate streams' pieces into their windows.  Everything behind the window is unchanged and
// counts model-rate samples; the call's checks are evaluated on the model-rate samples its inputs make computable.
//
// A hand-off stream with a frame history (css_stream_window_open, include/css_mi355_window.h) also keeps its last raw
// log-mel frames in a ring on the device: the mel launch of a committed round leaves them there.  css_stream_windows turns spans
// of them into Whisper encoder inputs in the caller's device memory, css_stream_present_windows spans that end in a preview's
// provisional frames: one kernel (handoff.hip stream_window_kernel), one table launch per WINDOW_MULTI_MAX windows (launch_windows).
//
// A stream with an output format (css_stream_set_output, include/css_mi355_stream_out.h) also writes the samples
// that became final at the playback rate, as float32 or PCM16, into the buffer bound to it: ONE table launch per round
// (resample.hip stream_output_kernel) between tail() and the downloads reads the round's final samples where tail() left them,
// and the converted samples go from the stream's device staging to the caller's memory.  The float download is skipped when
// the call's out_host is NULL.  Every stream keeps the running peak of its final samples: the kernel forms it for a stream with
// an output format, the host from the downloaded samples for every other one (no launch, no copy is added to that path).
#include "api_ctx.hpp"
#include "../../include/css_mi355_rate.h"
#include "../../include/css_mi355_preview.h"
#include "../../include/css_mi355_preview_handoff.h"
#include "../../include/css_mi355_window.h"
#include "../../include/css_mi355_present_window.h"
#include "../../include/css_mi355_stream_out.h"

#include <climits>

namespace {

constexpr int PIECE_SEGMENTS = 8;

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
};

// Per handle, made when the first stream switches the hand-off on.
struct HandoffCtx {
    DevBuf tab, operand, spec, res, state;   // DFT matrix + both filterbanks; frame operand; spectra; a round's results; HandoffState per (id, k)
    DevBuf state_pv;                         // a preview's closing round writes its counts and maximum here, never into `state`
    std::vector<PinnedBuf> pinned;           // staging of round r of a call
    DevBuf present; PinnedBuf present_pin;   // css_stream_windows / css_stream_present_windows: a WindowOut per window of one call, and its staging
    int32_t launches = 0, products = 0;
    int64_t frames = 0;
};
constexpr size_t HO_DFT_F = (size_t)402 * 416, HO_MEL80_F = (size_t)80 * 201, HO_MEL128_F = (size_t)128 * 201;

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

StreamState* get_stream(css_ctx* h, int32_t id) {
    if (id < 0 || id >= CSS_MAX_STREAMS) return nullptr;
    return static_cast<StreamState*>(h->streams[id]);
}

int64_t frames_of(int64_t n) { return n < 512 ? 0 : (n - 512) / 256 + 1; }
// segments whose frames are all known and which are not the last segment of the recording, whatever follows
int64_t segments_done(int64_t K, int T, int hop) { return K > T ? (K - 1 - T) / hop + 1 : 0; }
int64_t final_frames(int64_t n, int T, int hop, int halo) {
    return std::max<int64_t>(segments_done(frames_of(n), T, hop) * hop - halo, 0);
}

// every device buffer of a stream, its hand-off and its rate conversion (css_stream_info: what the stream holds on the device)
template <class Fn>
void for_each_buffer(const StreamState* s, Fn fn) {
    for (int b = 0; b < 2; ++b)
        for (const DevBuf* d : {&s->pcm[b], &s->X[b], &s->masks[b], &s->sep[b], &s->perms[b], &s->act_b[b], &s->G[b]}) fn(*d);
    for (const DevBuf* d : {&s->scm, &s->bfw, &s->pnorm, &s->costs, &s->pit_part, &s->Y, &s->out, &s->segw, &s->pcm16_stage}) fn(*d);
    if (s->ho)
        for (const DevBuf* d : {&s->ho->gate, &s->ho->carry[0], &s->ho->carry[1], &s->ho->tail[0], &s->ho->tail[1], &s->ho->ring, &s->ho->fmax}) fn(*d);
    if (s->rate)
        for (const DevBuf* d : {&s->rate->stage, &s->rate->hist[0], &s->rate->hist[1], &s->rate->tab}) fn(*d);
    if (s->outp)
        for (const DevBuf* d : {&s->outp->hist[0], &s->outp->hist[1], &s->outp->tab, &s->outp->stage, &s->outp->ctr}) fn(*d);
}

int64_t device_bytes(const StreamState* s) {
    int64_t n = s->ho ? (int64_t)(SMAX * sizeof(HandoffState)) : 0;   // (its rows of the handle's hand-off state)
    for_each_buffer(s, [&](const DevBuf& d) { n += (int64_t)d.cap; });
    return n;
}

int check_cfg(const CssModelDesc& d, const CssRunCfg* cfg) {
    if (!cfg || !cfg->w_first || !cfg->w_mid || !cfg->w_last) return CSS_ERR_INVALID_ARG;
    if (d.frame_len != 512 || d.frame_hop != 256) return CSS_ERR_INVALID_ARG;
    if (cfg->segment_frames < 2 || cfg->segment_frames > CSS_MAX_SEGMENT_FRAMES || cfg->hop_frames < 1 ||
        cfg->hop_frames >= cfg->segment_frames || cfg->dilation_frames < 0 || cfg->erosion_frames < 0)
        return CSS_ERR_INVALID_ARG;
    return CSS_OK;
}

// css.py:297 on the frames [t_lo, t_hi) a push finalises: segments covering them are done and not the last one, so their
// total weight (summed as plan_impl sums it) is what css_run finds for every recording that reaches them
bool zero_weight_frames(const StreamState* s, int64_t t_lo, int64_t t_hi) {
    const int T = s->T, hop = s->hop;
    for (int64_t t = t_lo; t < t_hi; ++t) {
        float ws = 0.f;
        for (int64_t seg = std::max<int64_t>(0, (t - T + hop) / hop); seg <= t / hop; ++seg) {
            const int64_t tl = t - seg * hop;
            if (tl < 0 || tl >= T) continue;
            ws += (seg == 0 ? s->cfg.w_first : s->cfg.w_mid)[tl];
        }
        if (!(ws > 1e-5f)) return true;
    }
    return false;
}

StreamStitchArgs stitch_view(css_ctx* h, StreamState* s, bool closing, int64_t nseg, int64_t TL) {
    StreamStitchArgs a{};
    const int c = s->cur;
    a.masks = (const float*)s->masks[c].p; a.mask_ld = s->SC * s->T;
    a.sep = (const float*)s->sep[c].p;
    a.perms = (const int32_t*)s->perms[c].p + h->d.num_spks;   // (slot -1 is the scan's guard)
    a.S = h->d.num_spks; a.F = h->d.num_bins; a.T = s->T; a.hop = s->hop;
    a.seg_base = s->seg_base; a.frame_base = s->seg_base * s->hop;
    a.num_slots = (closing ? nseg : s->sd) - s->seg_base;
    a.num_segments_global = closing ? nseg : INT64_MAX;
    a.T_long_global = closing ? TL : INT64_MAX;
    a.w_first = (const float*)s->segw.p; a.w_mid = a.w_first + s->T; a.w_last = a.w_mid + s->T;
    a.act_b = (uint8_t*)s->act_b[c].p;
    a.Y = (float*)s->Y.p; a.KIp = h->KIp;
    a.ld_frames = s->WF;
    a.activity_th = s->cfg.activity_th; a.dilation = s->cfg.dilation_frames; a.erosion = s->cfg.erosion_frames;
    if (s->ho) { a.gate_out = (uint8_t*)s->ho->gate.p; a.gate_ld = s->ho->gate_ld; a.gate_mask = s->ho->gate_mask; }
    return a;
}

int copy_rows(css_ctx* h, void* dst, const void* src, size_t pitch, size_t width, size_t rows) {
    if (!width || !rows) return CSS_OK;
    if (rows == 1) {
        HIPCHK(h, hipMemcpyAsync(dst, src, width, hipMemcpyDeviceToDevice, h->stream));
        return CSS_OK;
    }
    HIPCHK(h, hipMemcpy2DAsync(dst, pitch, src, pitch, width, rows, hipMemcpyDeviceToDevice, h->stream));
    return CSS_OK;
}

// Moves the window forward as far as the live state allows (whole segments): what is still read later -- the samples of
// frames not yet transformed, the planes of segments not yet done, the segments covering frames not yet gated, the
// permutation the scan continues from, the activity halo of the gate and the synthesis rows of the frame before the next
// output block -- is copied to the front of the other buffer set.
int rebase(css_ctx* h, StreamState* s) {
    const int T = s->T, hop = s->hop;
    const int64_t first_cover = s->t_g - T + 1 <= 0 ? 0 : (s->t_g - T + 1 + hop - 1) / hop;
    const int64_t frame_need = s->t_g - std::max(s->halo, 1);
    int64_t nb = std::min<int64_t>(s->sd - 1, first_cover);
    nb = std::min<int64_t>(nb, frame_need < 0 ? 0 : frame_need / hop);
    nb = std::max<int64_t>(nb, 0);
    const int64_t d = nb - s->seg_base;
    if (d <= 0) return CSS_OK;
    const int c = s->cur, o = 1 - c;
    const int F = h->d.num_bins, S = h->d.num_spks, C = s->n_ch, N = h->d.frame_len;
    const int64_t df = d * hop, fb = s->seg_base * hop;
    const int64_t ds = df * h->d.frame_hop, sb = fb * h->d.frame_hop;
    const size_t f4 = sizeof(float);
    int rc;
    if ((rc = copy_rows(h, s->pcm[o].p, (float*)s->pcm[c].p + ds, s->WS * f4, (size_t)(s->n_pushed - sb - ds) * f4, C)) != CSS_OK) return rc;
    if ((rc = copy_rows(h, s->X[o].p, (float*)s->X[c].p + df, s->WF * f4, (size_t)(s->K - fb - df) * f4,
                        (size_t)C * X_ROWS_PER_BIN * F)) != CSS_OK) return rc;
    const int64_t keep_seg = s->sd - s->seg_base - d;   // slots d .. sd - seg_base
    if ((rc = copy_rows(h, s->masks[o].p, (float*)s->masks[c].p + d * T, s->SC * T * f4, (size_t)keep_seg * T * f4,
                        (size_t)(S + 1) * F)) != CSS_OK) return rc;
    if ((rc = copy_rows(h, s->sep[o].p, (float*)s->sep[c].p + d * (int64_t)S * F * T * 2, 0, (size_t)keep_seg * S * F * T * 2 * f4, 1)) != CSS_OK) return rc;
    if ((rc = copy_rows(h, (int32_t*)s->perms[o].p + S, (int32_t*)s->perms[c].p + S + d * S, 0, (size_t)keep_seg * S * sizeof(int32_t), 1)) != CSS_OK) return rc;
    if ((rc = copy_rows(h, s->act_b[o].p, (uint8_t*)s->act_b[c].p + df, s->WF, (size_t)(s->t_st - fb - df), S)) != CSS_OK) return rc;
    if ((rc = copy_rows(h, s->G[o].p, (float*)s->G[c].p + df * N, s->WF * N * f4, (size_t)(s->t_g - fb - df) * N * f4, S)) != CSS_OK) return rc;
    s->cur = o;
    s->seg_base = nb;
    return CSS_OK;
}

// One stream's share of a round: segments [g_lo, g_hi) of its recording became complete; k_local frames of its window are transformed.
struct SegJob { StreamState* s; int64_t g_lo, g_hi, k_local; };

// The mask estimator over the segments of `jobs` (streams of ONE segmentation T / hop) as shared batches: batch segment c
// belongs to the job whose range holds it.  The feature kernel takes a session-local first segment, and a stream's first new
// segment is window slot g_lo - seg_base: time is the fastest axis of the planes, so a GroupSess whose planes start at frame
// slot * hop (and whose frame count is shorter by as much) makes that slot its segment 0.  The mask head writes the batch
// matrix into the stream code's own buffer; stream_scatter_masks_kernel moves each stream's columns into its window.
int estimate_class(css_ctx* h, const std::vector<SegJob>& jobs, CssStreamGroupStats* stats) {
    const int T = jobs[0].s->T, hop = jobs[0].s->hop, F = h->d.num_bins, S = h->d.num_spks;
    int64_t total = 0;
    for (const SegJob& j : jobs) total += j.g_hi - j.g_lo;
    const int64_t cap = batch_len(total, batch_cap(h, T));
    int rc;
    if ((rc = ensure_activations(h, cap, T)) != CSS_OK) return rc;
    if ((rc = ensure(h, h->stream_masks, (size_t)(S + 1) * F * cap * T * sizeof(float))) != CSS_OK) return rc;
    std::vector<GroupSess> gs;
    std::vector<MaskScatter> sc;
    for (int64_t b0 = 0; b0 < total; b0 += cap) {
        const int nb = (int)std::min<int64_t>(cap, total - b0);
        gs.clear(); sc.clear();
        int64_t off = 0;   // the job's first segment in the class's numbering
        for (const SegJob& j : jobs) {
            const int64_t n = j.g_hi - j.g_lo;
            const int64_t lo = std::max(b0, off), hi = std::min<int64_t>(b0 + nb, off + n);
            if (hi > lo) {
                StreamState* s = j.s;
                const int64_t slot = j.g_lo + (lo - off) - s->seg_base;
                const float* X = (const float*)s->X[s->cur].p + slot * hop;
                gs.push_back(GroupSess{X, s->WF, j.k_local - slot * hop, lo - b0, (int)(hi - lo), X + (int64_t)s->n_ch * 2 * F * s->WF});
                sc.push_back(MaskScatter{(float*)s->masks[s->cur].p + slot * T, s->SC * T, (lo - b0) * T, (hi - lo) * T});
            }
            off += n;
        }
        MaskIo io{nullptr, 0, 0, hop, T, (float*)h->stream_masks.p, (int64_t)nb * T, &gs};
        if ((rc = masknet_batch(h, io, 0, nb)) != CSS_OK) return rc;
        launch_stream_scatter_masks((const float*)h->stream_masks.p, (int64_t)nb * T, (S + 1) * F, sc.data(), (int)sc.size(), h->stream);
        if (stats) { stats->estimator_batches += 1; stats->estimator_segments += nb; }
    }
    HIPCHK(h, hipGetLastError());
    return CSS_OK;
}

// The segments the jobs completed: the estimator per (T, hop) class, then per stream covariances, MVDR (one table launch
// for all streams), beamformer, power normalisation, the stitching costs of the boundaries that ended and the permutation
// scan.  (The costs stay per stream: launch_pit_costs_multi computes a session's boundaries from 0, a stream needs a range.)
int segments(css_ctx* h, const std::vector<SegJob>& all, CssStreamGroupStats* stats) {
    std::vector<SegJob> jobs;
    for (const SegJob& j : all)
        if (j.g_hi > j.g_lo) jobs.push_back(j);
    if (jobs.empty()) return CSS_OK;
    int rc;
    std::vector<char> taken(jobs.size(), 0);
    std::vector<SegJob> cls;
    for (size_t i = 0; i < jobs.size(); ++i) {
        if (taken[i]) continue;
        cls.clear();
        for (size_t k = i; k < jobs.size(); ++k)
            if (!taken[k] && jobs[k].s->T == jobs[i].s->T && jobs[k].s->hop == jobs[i].s->hop) { cls.push_back(jobs[k]); taken[k] = 1; }
        if ((rc = estimate_class(h, cls, stats)) != CSS_OK) return rc;
    }
    const int F = h->d.num_bins, S = h->d.num_spks;
    std::vector<MvdrArgs> mv(jobs.size()), solve;
    for (size_t i = 0; i < jobs.size(); ++i) {
        StreamState* s = jobs[i].s;
        const int c = s->cur;
        MvdrArgs& a = mv[i];
        a = MvdrArgs{};
        a.X = (const float*)s->X[c].p; a.T_ld = s->WF; a.stft_frames = jobs[i].k_local;
        a.C = s->n_ch; a.F = F;
        a.masks = (const float*)s->masks[c].p; a.mask_ld = s->SC * s->T;
        a.S = S; a.T = s->T; a.hop = s->hop;
        a.seg_lo = jobs[i].g_lo - s->seg_base; a.nseg = (int)(jobs[i].g_hi - jobs[i].g_lo);
        a.wta_override = nullptr;
        a.scm = (double*)s->scm.p; a.bfw = (double*)s->bfw.p; a.sep = (float*)s->sep[c].p;
        a.mask_floor = s->cfg.mask_floor;
        a.use_mvdr = (s->n_ch > 1 && s->cfg.mc_mvdr) ? 1 : 0;
        if (a.use_mvdr) {
            if (!launch_scm(a, h->stream)) return fail(h, CSS_ERR_HIP, "the covariance kernel's LDS could not be reserved");
            solve.push_back(a);
        }
    }
    if (!solve.empty()) launch_mvdr_solve_multi(solve.data(), (int)solve.size(), h->stream);
    for (size_t i = 0; i < jobs.size(); ++i) {
        StreamState* s = jobs[i].s;
        const int c = s->cur, T = s->T;
        const int64_t lo = mv[i].seg_lo, hi = lo + mv[i].nseg;
        launch_beamform(mv[i], h->stream);
        if (s->cfg.normalize_segment_power) launch_segment_power_norm(mv[i], (double*)s->pnorm.p, h->stream);
        // boundaries b (segments b, b + 1) that end in these segments (the costs' chunking is one constant: stitch.hip pit_chunks)
        const int64_t b_lo = std::max<int64_t>(lo - 1, 0), b_hi = hi - 1;
        if (b_hi > b_lo) {
            StitchArgs sa{};
            sa.masks = (const float*)s->masks[c].p; sa.mask_ld = s->SC * T; sa.sep = (const float*)s->sep[c].p;
            sa.S = S; sa.F = F; sa.T = T; sa.hop = s->hop;
            sa.num_segments = hi; sa.T_long = s->WF;
            launch_pit_costs(sa, s->cfg.stitching_loss, s->cfg.stitching_input, b_lo, b_hi, (double*)s->pit_part.p,
                             (double*)s->costs.p + S * S, h->stream);
            // slot j's permutation lives at perms + (j + 1) S and boundary b's costs at costs + (b + 1) S S: the scan starts
            // at its index 1 + b_lo and continues from slot b_lo's permutation (never the identity it writes for index 0)
            launch_pit_scan((const double*)s->costs.p, 1 + b_lo, 1 + b_hi, S, (int32_t*)s->perms[c].p, h->stream);
        }
    }
    HIPCHK(h, hipGetLastError());
    return CSS_OK;
}

// One stream's frames [t_lo, t_hi) of the recording: activity bits of [a_lo, a_hi), gate + overlap-add + synthesis of [t_lo, t_hi),
// output blocks [t_lo, q_hi) into the stream's output buffer (block t_lo at column 0)
// (gate: whether a hand-off stream's gate ring receives the gate bytes; a preview's closing pass leaves it alone)
struct TailJob { StreamState* s; bool closing; int64_t nseg, TL, a_lo, a_hi, t_lo, t_hi, q_hi; bool gate = true; };

int tail(css_ctx* h, const std::vector<TailJob>& jobs) {
    std::vector<StreamStitchArgs> a(jobs.size());
    std::vector<StreamFrames> ra(jobs.size()), rg(jobs.size());
    for (size_t i = 0; i < jobs.size(); ++i) {
        const TailJob& j = jobs[i];
        const int64_t fb = j.s->seg_base * j.s->hop;
        a[i] = stitch_view(h, j.s, j.closing, j.nseg, j.TL);
        if (!j.gate) { a[i].gate_out = nullptr; a[i].gate_ld = 0; a[i].gate_mask = 0; }
        ra[i] = StreamFrames{j.a_lo - fb, j.a_hi - fb};
        rg[i] = StreamFrames{j.t_lo - fb, j.t_hi - fb};
    }
    launch_stream_activity_multi(a.data(), ra.data(), (int)jobs.size(), h->stream);
    launch_stream_gate_ola_multi(a.data(), rg.data(), (int)jobs.size(), h->stream);
    const int S = h->d.num_spks, N = h->d.frame_len;
    for (const TailJob& j : jobs) {
        StreamState* s = j.s;
        const int64_t fb = s->seg_base * s->hop, t_lo = j.t_lo, t_hi = j.t_hi;
        const int c = s->cur;
        if (t_hi > t_lo) {
            GemmArgs g{};
            g.A = (const float*)s->Y.p + (t_lo - fb) * h->KIp; g.lda = h->KIp; g.strideA = s->WF * h->KIp;
            g.B = h->dft_inv_t.as(); g.ldb = h->KIp; g.strideB = 0;
            g.C = (float*)s->G[c].p + (t_lo - fb) * N; g.ldc = N; g.strideC = s->WF * N;
            g.M = (int)(t_hi - t_lo); g.N = N; g.K = h->KIp; g.batch = S;
            g.bias = nullptr; g.act = ACT_NONE; g.residual = nullptr; g.alpha = 1.f;
            launch_gemm(g, h->stream);
        }
        if (j.q_hi > t_lo)
            launch_wave_ola((const float*)s->G[c].p, (float*)s->out.p, S, s->WF, h->d.frame_hop, N, t_lo - fb, j.q_hi - fb, 0,
                            (j.closing ? j.TL : t_hi) - fb, (j.q_hi - t_lo) * h->d.frame_hop, t_lo - fb, nullptr, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return CSS_OK;
}

int download(css_ctx* h, StreamState* s, int64_t n, float* out_host, int64_t cap, int64_t at) {
    if (n <= 0) return CSS_OK;
    HIPCHK(h, hipMemcpy2DAsync(out_host + at, (size_t)cap * sizeof(float), s->out.p, (size_t)n * sizeof(float), (size_t)n * sizeof(float),
                               (size_t)h->d.num_spks, hipMemcpyDeviceToHost, h->stream));
    return CSS_OK;
}

// ---- output format ---------------------------------------------------------------------------------------------------------
// output samples written once `n_final` model-rate samples are final (finished: of the whole recording)
int64_t output_count(const OutputStream* o, int64_t n_final, bool finished) {
    return o->unity ? n_final : resample_count(o->r, n_final, finished);
}
size_t output_el(const OutputStream* o) { return o->cfg.pcm16 ? sizeof(int16_t) : sizeof(float); }
// a row of the staging that holds what `n` final samples can make in one round (the resampler's lag released at finish included)
int64_t output_stage_ld(const OutputStream* o, int64_t n) {
    const int64_t most = o->unity ? n : (n * o->r.up + o->r.half) / o->r.down + 2;
    return (most + 7) / 8 * 8;
}

// what a call that makes `need` more samples final must find bound to a stream with an output format
int check_output_call(const StreamState* s, int64_t need, bool finished, std::string* why) {
    const OutputStream* o = s->outp.get();
    if (!o) return CSS_OK;
    if (!o->bound) { *why = "the stream has an output format and nothing is bound (css_stream_output_bind)"; return CSS_ERR_STATE; }
    if (o->cap < output_count(o, s->n_emitted + need, finished) - o->n_total) {
        *why = "the bound output capacity is below what this call writes (css_stream_output_samples)";
        return CSS_ERR_INVALID_ARG;
    }
    return CSS_OK;
}

// The entry of the round's output launch for a stream whose tail() left `n` new final samples per separated stream in s->out
// (row pitch src_ld), `done` samples after the n_emitted of the call's start; flips the carried samples' generation.
// *n_m: the output samples the round writes (at column 0 of the staging).
int output_job(css_ctx* h, StreamState* s, int64_t done, int64_t n, int64_t src_ld, bool finished, StreamOutputJob* j, int64_t* n_m) {
    OutputStream* o = s->outp.get();
    const int S = h->d.num_spks;
    const int64_t N0 = s->n_emitted + done, m0 = output_count(o, N0, false);
    *n_m = output_count(o, N0 + n, finished) - m0;
    const int64_t ld = output_stage_ld(o, n);
    if (ld > o->stage_ld) {   // (finish can make more samples final than a round of a push)
        const int rc = ensure(h, o->stage, (size_t)S * ld * output_el(o));
        if (rc != CSS_OK) return rc;
        o->stage_ld = ld;
    }
    *j = StreamOutputJob{};
    j->src = (const float*)s->out.p; j->src_ld = src_ld; j->n = n;
    j->N0 = N0; j->m0 = m0; j->n_m = *n_m;
    j->up = o->r.up; j->down = o->r.down; j->half = o->r.half; j->P = o->r.P; j->P_ld = o->r.P_ld; j->tab = (const float*)o->tab.p;
    j->pcm16 = o->cfg.pcm16; j->gain = o->cfg.gain;
    j->dst = o->stage.p; j->dst_ld = o->stage_ld;
    OutputCounters* c = (OutputCounters*)o->ctr.p;
    j->peak = c->peak; j->clipped = c->clipped;
    if (!o->unity) {
        j->hist_in = (const float*)o->hist[o->cur].p; j->H = o->H;
        if (!finished) { j->hist_out = (float*)o->hist[1 - o->cur].p; o->cur = 1 - o->cur; }
    }
    return CSS_OK;
}

// the round's `n_m` output samples from the staging to column `at` of the bound buffer
int output_download(css_ctx* h, StreamState* s, int64_t n_m, int64_t at) {
    OutputStream* o = s->outp.get();
    if (n_m <= 0) return CSS_OK;
    const size_t el = output_el(o);
    HIPCHK(h, hipMemcpy2DAsync((char*)o->bound + (size_t)at * el, (size_t)o->cap * el, o->stage.p, (size_t)o->stage_ld * el, (size_t)n_m * el,
                               (size_t)h->d.num_spks, hipMemcpyDeviceToHost, h->stream));
    return CSS_OK;
}

// behind a call's last round: the counters to page-locked memory (read after the call's synchronise by output_report)
int output_counters(css_ctx* h, StreamState* s) {
    HIPCHK(h, hipMemcpyAsync(s->outp->pin.p, s->outp->ctr.p, sizeof(OutputCounters), hipMemcpyDeviceToHost, h->stream));
    return CSS_OK;
}
void output_report(css_ctx* h, StreamState* s, int64_t written) {
    OutputStream* o = s->outp.get();
    const OutputCounters* c = o->pin.as<OutputCounters>();
    o->n_total += written;
    for (int k = 0; k < h->d.num_spks; ++k) s->peak_bits[k] = c->peak[k];
    if (CssStreamOutputCounts* q = o->counts) {
        q->n_written = written; q->n_total = o->n_total;
        for (int k = 0; k < h->d.num_spks; ++k) { q->n_clipped[k] = (int64_t)c->clipped[k]; q->peak_bits[k] = c->peak[k]; }
    }
}
// a call that moved nothing still reports (n_written = 0)
void output_report_idle(css_ctx* h, StreamState* s) {
    if (!s->outp || !s->outp->counts) return;
    s->outp->counts->n_written = 0; s->outp->counts->n_total = s->outp->n_total;
}

// a stream without an output format: the running peak from the `n` samples per separated stream a call downloaded to out[S][cap].
// fmaxf(m, |x|) from 0 as the kernels form it, on the bits: non-negative floats order like unsigned integers and a NaN, which
// fmaxf never lets raise the peak, counts as 0 -- an integer maximum, which the compiler vectorises (the scan is bound by the
// host's memory: about 0.3 ms per 1.15 M samples, a tick of 16 rooms)
void host_peak(css_ctx* h, StreamState* s, const float* out, int64_t cap, int64_t n) {
    for (int k = 0; k < h->d.num_spks; ++k) {
        const int32_t* w = reinterpret_cast<const int32_t*>(out + (size_t)k * cap);
        int32_t m = (int32_t)s->peak_bits[k];   // (|x| bits are below 2^31: signed compares, which every x86-64 has for vectors)
        for (int64_t i = 0; i < n; ++i) {
            const int32_t a = w[i] & 0x7fffffff;
            const int32_t v = a > 0x7f800000 ? 0 : a;
            m = v > m ? v : m;
        }
        s->peak_bits[k] = (uint32_t)m;
    }
}

// ---- hand-off ----------------------------------------------------------------------------------------------------------
// Capacities that suffice for one call.  A push of n samples adds at most n / 256 + 1 frames to the transform, hence at most
// that plus hop_frames to the segments' frames, the gated-final frames and the decided blocks; finish decides what is left:
// fewer than T + halo + pad + 2 blocks (t_g >= K - T - halo, n_out = (max(K, T) + 1) blocks).  J frames need 160 J + 40
// samples, so a call that appends dn samples completes at most dn / 160 + 1 frames -- (dn + 200) / 160 + 1 at finish, which
// also emits the frames the trailing reflection completes.  Two ranges of a call have a dropped block between them.
struct HandoffNeed { int64_t frames; int32_t ranges; int64_t activity; };
HandoffNeed handoff_need(int T, int hop, int halo, const CssStreamHandoffCfg& c, int64_t n_samples) {
    const int pad = c.drop_silence ? c.pad_frames : 0;
    const int64_t blocks = n_samples < 0 ? (int64_t)T + hop + halo + pad + 3 : n_samples / 256 + 1 + hop;
    HandoffNeed n;
    n.frames = (blocks * 256 + 200) / 160 + 2;
    n.ranges = c.drop_silence ? (int32_t)std::min<int64_t>(blocks / 2 + 1, INT32_MAX) : 1;
    n.activity = blocks;
    return n;
}
// frames of the operand a round reserves for one speaker that appends at most dn samples: the frames it can complete, the
// rows the last frame's 416 columns reach into, and the gap to the next owner
int64_t handoff_rows(int64_t dn) { return (dn + 200) / 160 + 2 + 3; }

int check_handoff_cfg(const CssStreamHandoffCfg* c) {
    if (!c || (c->n_mels != 80 && c->n_mels != 128) || c->pad_frames < 0 || c->pad_frames > 4096) return CSS_ERR_INVALID_ARG;
    return CSS_OK;
}

// what a call must find in the hand-off outputs `o` of a stream with the hand-off on
int check_handoff_out(const StreamState* s, const CssStreamHandoffOut* o, int64_t n_samples, std::string* why) {
    const HandoffNeed n = handoff_need(s->T, s->hop, s->halo, s->ho->cfg, n_samples);
    if (!o->mel_host || !o->ranges_host || !o->n_frames || !o->n_ranges || !o->raw_max || o->cap_frames < n.frames ||
        o->cap_ranges < n.ranges || (o->activity_host && o->cap_activity < n.activity)) {
        *why = "hand-off capacities below css_stream_handoff_bounds for this call";
        return CSS_ERR_INVALID_ARG;
    }
    return CSS_OK;
}
// ... bound to it
int check_handoff_call(css_ctx* h, const StreamState* s, int64_t n_samples, std::string* why) {
    if (!s->ho) return CSS_OK;
    if (!s->ho->bound) { *why = "the hand-off is on and nothing is bound (css_stream_handoff_bind)"; return CSS_ERR_STATE; }
    return check_handoff_out(s, s->ho->bound, n_samples, why);
}

HandoffCtx* handoff_ctx(css_ctx* h) { return static_cast<HandoffCtx*>(h->handoff); }

void handoff_begin_call(css_ctx* h) {
    if (HandoffCtx* c = handoff_ctx(h)) { c->launches = c->products = 0; c->frames = 0; }
}

// One stream's share of a round's hand-off: frames [t_g0, t_g1) became gated-final, the output buffer holds out_ld samples per
// speaker from sample t_g0 * hop on.  HandoffRec is what the host needs after the call's synchronise to hand the round's results out.
// pvmax (a preview's round only): also leave the maxima over the bands of the frames the round makes, for windows up to the present.
struct HandoffJob { StreamState* s; int item; int64_t t_g0, t_g1, out_ld; bool closing; int64_t n_out; bool pvmax = false; };
struct HandoffRec {
    StreamState* s; int item; int64_t t_g0, t_g1, D0, D1, n_out; bool closing;
    const uint8_t* act; const int32_t* n_new; const float* mel; int64_t mel_ld; const HandoffState* st;   // in page-locked staging
    const int32_t* n_new_dev; const float* mel_dev; const float* pvmax_dev;   // the round's results on the device (pvmax_dev: with HandoffJob::pvmax)
};

// commit: the streams' decided counts, generations and device state move (a push, finish).  Without it (a preview with hand-off)
// the round reads the same inputs and writes only what is scratch until a commit: the other generation of carry and tail, the
// handle's operand / spectra / results and the state_pv rows.
int handoff_round(css_ctx* h, const std::vector<HandoffJob>& all, size_t round, std::vector<HandoffRec>* recs, bool commit = true) {
    HandoffCtx* c = handoff_ctx(h);
    std::vector<HandoffJob> jobs;
    for (const HandoffJob& j : all)
        if (j.s->ho && (j.t_g1 > j.t_g0 || j.closing)) jobs.push_back(j);
    if (jobs.empty() || !c) return CSS_OK;
    const int S = h->d.num_spks, hopS = h->d.frame_hop;
    const size_t n = jobs.size();
    std::vector<HandoffAppend> ap(n);
    std::vector<HandoffMel> me(n);
    std::vector<size_t> act_off(n), new_off(n), mel_off(n), pvm_off(n, 0);
    int64_t rows_total = 0;
    size_t res_b = 0;
    auto al = [](size_t v) { return (v + 63) / 64 * 64; };
    for (size_t i = 0; i < n; ++i) {
        const HandoffJob& j = jobs[i];
        HandoffStream* o = j.s->ho.get();
        const int64_t D1 = j.closing ? j.n_out : std::max<int64_t>(j.t_g1 - o->pad, 0) * hopS;
        HandoffAppend& a = ap[i];
        a = HandoffAppend{};
        a.gate = (const uint8_t*)o->gate.p; a.gate_ld = o->gate_ld; a.gate_mask = o->gate_mask;
        a.out = (const float*)j.s->out.p; a.out_ld = j.out_ld; a.out_base = j.t_g0 * hopS;
        a.carry_in = (const float*)o->carry[o->cur].p; a.carry_out = (float*)o->carry[1 - o->cur].p; a.carry_ld = o->carry_ld;
        a.tail_in = (const float*)o->tail[o->cur].p; a.tail_out = (float*)o->tail[1 - o->cur].p;
        a.t_g0 = j.t_g0; a.t_g1 = j.t_g1; a.D0 = o->D; a.D1 = D1;
        a.pad = o->pad; a.drop = o->cfg.drop_silence ? 1 : 0; a.closing = j.closing ? 1 : 0; a.S = S;
        a.rows = handoff_rows(D1 - o->D); a.row0 = rows_total;
        rows_total += a.rows * S;
        act_off[i] = res_b; res_b = al(res_b + (size_t)S * (size_t)(j.t_g1 - j.t_g0));
        new_off[i] = res_b; res_b = al(res_b + (size_t)S * sizeof(int32_t));
        mel_off[i] = res_b; res_b = al(res_b + (size_t)S * o->cfg.n_mels * (size_t)a.rows * sizeof(float));
        if (j.pvmax && !commit) { pvm_off[i] = res_b; res_b = al(res_b + (size_t)S * (size_t)a.rows * sizeof(float)); }
    }
    const size_t state_b = (size_t)CSS_MAX_STREAMS * SMAX * sizeof(HandoffState);
    const int64_t ld = (rows_total + 3) / 4 * 4;
    int rc;
    // The product reads 416 columns from every row; columns 400 .. 415 meet zeros of the matrix, so what they read only has to
    // be finite.  The append kernel rewrites ALL rows of every owner each round, the floats behind the last row are zeros
    // from the allocation or finite values an earlier, larger round left there.
    if ((rc = ensure(h, c->operand, ((size_t)rows_total * 160 + 1024) * sizeof(float), true)) != CSS_OK) return rc;
    if ((rc = ensure(h, c->spec, (size_t)402 * ld * sizeof(float))) != CSS_OK) return rc;
    if ((rc = ensure(h, c->res, res_b)) != CSS_OK) return rc;
    if (c->pinned.size() <= round) c->pinned.resize(round + 1);
    PinnedBuf& pin = c->pinned[round];
    if (pin.cap < res_b + state_b) HIPCHK(h, pin.alloc(res_b + state_b));
    const float* dftm = (const float*)c->tab.p;
    for (size_t i = 0; i < n; ++i) {
        const HandoffJob& j = jobs[i];
        HandoffStream* o = j.s->ho.get();
        int id = 0;
        while (h->streams[id] != j.s) ++id;
        ap[i].st = (const HandoffState*)c->state.p + (size_t)id * SMAX;
        HandoffState* st = (HandoffState*)(commit ? c->state.p : c->state_pv.p) + (size_t)id * SMAX;
        ap[i].st_out = st;
        ap[i].act_out = (uint8_t*)c->res.p + act_off[i];
        ap[i].n_new = (int32_t*)((char*)c->res.p + new_off[i]);
        me[i] = HandoffMel{ap[i].row0, ap[i].rows, ap[i].n_new, st, dftm + HO_DFT_F + (o->cfg.n_mels == 80 ? 0 : HO_MEL80_F), o->cfg.n_mels,
                           (float*)((char*)c->res.p + mel_off[i]), ap[i].rows, nullptr, nullptr, 0};
        if (commit && o->hist_frames) { me[i].ring = (float*)o->ring.p; me[i].fmax = (float*)o->fmax.p; me[i].hist = o->hist_frames; }
        if (j.pvmax && !commit) me[i].pvmax = (float*)((char*)c->res.p + pvm_off[i]);
        HandoffRec r{};
        r.s = j.s; r.item = j.item; r.t_g0 = j.t_g0; r.t_g1 = j.t_g1; r.D0 = ap[i].D0; r.D1 = ap[i].D1; r.n_out = j.n_out; r.closing = j.closing;
        r.act = (const uint8_t*)pin.p + act_off[i];
        r.n_new = (const int32_t*)((const char*)pin.p + new_off[i]);
        r.mel = (const float*)((const char*)pin.p + mel_off[i]);
        r.mel_ld = ap[i].rows;
        r.st = (const HandoffState*)((const char*)pin.p + res_b) + (size_t)id * SMAX;
        r.n_new_dev = ap[i].n_new; r.mel_dev = me[i].mel; r.pvmax_dev = me[i].pvmax;
        recs->push_back(r);
        if (commit) {
            o->D = ap[i].D1;
            o->cur = 1 - o->cur;
        }
    }
    launch_handoff_append_multi(ap.data(), (int)n, (float*)c->operand.p, h->stream);
    GemmArgs g{};
    g.A = dftm; g.lda = 416; g.B = (const float*)c->operand.p; g.ldb = 160; g.C = (float*)c->spec.p; g.ldc = ld;
    g.M = 402; g.N = (int)rows_total; g.K = 416; g.batch = 1; g.alpha = 1.f;
    launch_gemm(g, h->stream);
    launch_handoff_mel_multi(me.data(), (int)n, S, (const float*)c->spec.p, ld, h->stream);
    const int tables = (int)((n + HANDOFF_MULTI_MAX - 1) / HANDOFF_MULTI_MAX);
    c->launches += 2 * tables + 1; c->products += 1; c->frames += rows_total;
    HIPCHK(h, hipMemcpyAsync(pin.p, c->res.p, res_b, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync((char*)pin.p + res_b, commit ? c->state.p : c->state_pv.p, state_b, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipGetLastError());
    return CSS_OK;
}

// After the call's synchronise: the rounds' results of ONE stream, in order, trimmed into `out`, on the mirrors `mir`: the
// stream's own and what is bound to it (a push, finish: a failure ends the stream, which has moved already), or a copy and the
// caller's outputs (a preview: the failure is that call's error, the stream has not moved).
int handoff_collect(css_ctx* h, StreamState* s, int item, int64_t t_g_before, const std::vector<HandoffRec>& recs, HandoffMirror& mir,
                    CssStreamHandoffOut* out, bool commit) {
    const HandoffStream* o = s->ho.get();
    const int S = h->d.num_spks, hopS = h->d.frame_hop, N = h->d.frame_len, nm = o->cfg.n_mels;
    std::vector<std::vector<int64_t>> reg((size_t)S);
    std::vector<int64_t> nfr((size_t)S, 0);
    int64_t n_act = 0;
    for (const HandoffRec& r : recs) {
        if (r.s != s || r.item != item) continue;
        const int64_t nt = r.t_g1 - r.t_g0;
        for (int k = 0; k < S; ++k) {
            std::vector<uint8_t>& hist = mir.hist[(size_t)k];
            hist.insert(hist.end(), r.act + (size_t)k * nt, r.act + (size_t)(k + 1) * nt);
            if (out->activity_host && nt > 0)
                std::memcpy(out->activity_host + (size_t)k * out->cap_activity + n_act, r.act + (size_t)k * nt, (size_t)nt);
            std::vector<int64_t>& g = reg[(size_t)k];
            const size_t before = g.size();
            const int64_t last_end = before ? g.back() : -1;
            if (!o->cfg.drop_silence) {
                if (r.D1 > r.D0) {
                    if (before && g.back() == r.D0) g.back() = r.D1;
                    else { g.push_back(r.D0); g.push_back(r.D1); }
                }
            } else {
                handoff_kept_ranges(hist.data(), mir.hist_base, r.t_g1, o->pad, hopS, N, r.D0, r.D1, r.closing ? r.n_out : INT64_MAX, g);
            }
            int64_t added = 0;   // samples this round appended: the new ranges, and what the last old one grew by
            for (size_t i = before; i + 1 < g.size(); i += 2) added += g[i + 1] - g[i];
            if (before) added += g[before - 1] - last_end;
            const int64_t A1 = mir.A[(size_t)k] + added;
            const int64_t J1 = r.closing ? A1 / 160 : (A1 >= 201 ? (A1 - 200) / 160 + 1 : 0);
            const int64_t nj = J1 - mir.J[(size_t)k];
            // internal consistency, not refusals: a stream that has moved already ends here (only css_stream_close is left)
            if (nj != r.n_new[k] || r.st[k].A != A1 || r.st[k].J != J1) {
                if (!commit) return fail(h, CSS_ERR_STATE, "hand-off: the device's counts differ from the host's range rule in this preview");
                s->finished = true;
                return fail(h, CSS_ERR_STATE, "hand-off: the device's counts differ from the host's range rule; the stream is closed to further calls");
            }
            if (nfr[(size_t)k] + nj > out->cap_frames || (int64_t)(g.size() / 2) > out->cap_ranges) {
                if (!commit) return fail(h, CSS_ERR_STATE, "hand-off: the capacities were exceeded in this preview");
                s->finished = true;
                return fail(h, CSS_ERR_STATE, "hand-off: the bound capacities were exceeded; the stream is closed to further calls");
            }
            for (int m = 0; m < nm && nj > 0; ++m)
                std::memcpy(out->mel_host + ((size_t)k * nm + m) * out->cap_frames + nfr[(size_t)k],
                            r.mel + ((size_t)k * nm + m) * r.mel_ld, (size_t)nj * sizeof(float));
            nfr[(size_t)k] += nj;
            mir.A[(size_t)k] = A1; mir.J[(size_t)k] = J1;
            const int b = r.st[k].gmax;
            const int bits = b >= 0 ? b : b ^ 0x7fffffff;
            std::memcpy(&mir.raw_max[(size_t)k], &bits, sizeof(float));
        }
        n_act += nt;
        // frames that can still keep an undecided sample: from t_g - 2 pad - 2 on
        const int64_t keep_from = std::max<int64_t>(r.t_g1 - 2 * (int64_t)o->pad - 3, mir.hist_base);
        if (keep_from > mir.hist_base) {
            for (int k = 0; k < S; ++k) mir.hist[(size_t)k].erase(mir.hist[(size_t)k].begin(), mir.hist[(size_t)k].begin() + (keep_from - mir.hist_base));
            mir.hist_base = keep_from;
        }
    }
    for (int k = 0; k < S; ++k) {
        const std::vector<int64_t>& g = reg[(size_t)k];
        std::memcpy(out->ranges_host + (size_t)k * out->cap_ranges * 2, g.data(), g.size() * sizeof(int64_t));
        out->n_ranges[k] = (int32_t)(g.size() / 2);
        out->n_frames[k] = nfr[(size_t)k];
        out->raw_max[k] = mir.raw_max[(size_t)k];
    }
    out->n_activity = n_act;
    out->first_activity_frame = t_g_before;
    return CSS_OK;
}

// ---- rate streams -----------------------------------------------------------------------------------------------------------
// model-rate samples in the window once `more` further inputs have arrived (a rate-less stream: its samples are the inputs)
int64_t model_samples_after(const StreamState* s, int64_t more) {
    return s->rate ? resample_count(s->rate->r, s->rate->n_in + more, false) : s->n_pushed + more;
}

// The entry of the resample launch that takes `n_in` inputs staged in s->rate->stage (0 with `flush`: zeros past the end) and
// writes outputs [n_pushed, m1) at `win`; flips the history's generation (the launch writes the other one).
ResampleJob rate_job(StreamState* s, bool i16, bool planar, int64_t n_in, int64_t m1, float* win, bool flush) {
    RateStream* q = s->rate.get();
    ResampleJob j{};
    j.src = q->stage.p; j.is_i16 = i16 ? 1 : 0; j.plane_ld = planar ? q->max_in : 0; j.n = n_in;
    j.hist_in = (const float*)q->hist[q->cur].p; j.hist_out = flush ? nullptr : (float*)q->hist[1 - q->cur].p; j.H = q->H;
    j.N0 = q->n_in; j.m0 = s->n_pushed; j.n_m = m1 - s->n_pushed;
    j.up = q->r.up; j.down = q->r.down; j.half = q->r.half; j.P = q->r.P; j.P_ld = q->r.P_ld; j.tab = (const float*)q->tab.p;
    j.C = s->n_ch; j.dst = win; j.dst_ld = s->WS;
    if (!flush) q->cur = 1 - q->cur;
    q->n_in += n_in;
    return j;
}

int check_stream_call(css_ctx* h, int32_t id, StreamState** out) {
    if (!h) return CSS_ERR_INVALID_ARG;
    StreamState* s = get_stream(h, id);
    if (!s) return fail(h, CSS_ERR_INVALID_ARG, "no open stream with this id");
    if (h->queued || !h->pending.empty())
        return fail(h, CSS_ERR_STATE, "queued sessions (css_run_enqueue*) are outstanding: css_wait before using a stream");
    *out = s;
    return CSS_OK;
}

// What opens every item of a grouped push or preview, item i of a call whose item k names stream id_of(k): the stream is open,
// no queued session is outstanding, no earlier item names it, it has not finished.  -> CSS_OK and *out, or the code and *why.
template <typename IdOf>
int check_group_item(css_ctx* h, size_t i, IdOf id_of, StreamState** out, std::string* why) {
    StreamState* s = get_stream(h, id_of(i));
    if (!s) { *why = "no open stream with this id"; return CSS_ERR_INVALID_ARG; }
    if (h->queued || !h->pending.empty()) {
        *why = "queued sessions (css_run_enqueue*) are outstanding: css_wait before using a stream";
        return CSS_ERR_STATE;
    }
    for (size_t k = 0; k < i; ++k)
        if (id_of(k) == id_of(i)) { *why = "the stream is named twice in one call"; return CSS_ERR_INVALID_ARG; }
    if (s->finished) { *why = "the stream has finished"; return CSS_ERR_STATE; }
    *out = s;
    return CSS_OK;
}

// What is wrong with a window request (CssStreamWindow, CssStreamPresentWindow) of a stream with the history `o`, or null.
// first_frame: of a request that names its span (css_stream_windows); null where the device resolves it.  `o` is read only with
// first_frame (either way the caller has refused a stream without a history before).
template <typename W>
const char* window_refusal(const css_ctx* h, const HandoffStream* o, const W& w, const int64_t* first_frame) {
    if (w.speaker < 0 || w.speaker >= h->d.num_spks) return "speaker out of range";
    if (w.dtype != CSS_WINDOW_F32 && w.dtype != CSS_WINDOW_F16) return "dtype is CSS_WINDOW_F32 or CSS_WINDOW_F16";
    if (w.n_frames < 1 || w.width < w.n_frames || w.width > CSS_WINDOW_MAX_WIDTH) return "1 <= n_frames <= width <= 3000";
    if (w.ld < w.width) return "ld < width";
    if (first_frame) {
        const int64_t J = o->m.J[(size_t)w.speaker], first = std::max<int64_t>(J - o->hist_frames, 0);
        if (*first_frame < first || *first_frame > J - w.n_frames) return "frames outside the history (css_stream_window_range)";
    }
    const size_t el = w.dtype == CSS_WINDOW_F16 ? 2 : 4;
    if (!w.out_dev || (uintptr_t)w.out_dev % el) return "out_dev is null or not aligned to its element size";
    return nullptr;
}

// The history half of an accepted request's kernel item; the caller adds the span (J, and the provisional frames if it has any).
template <typename W>
WindowItem history_item(const HandoffStream* o, const W& w) {
    WindowItem e{};
    const int64_t H = o->hist_frames, nm = o->cfg.n_mels;
    e.ring = (const float*)o->ring.p + w.speaker * nm * H;
    e.fmax = (const float*)o->fmax.p + w.speaker * H;
    e.out = w.out_dev;
    e.hist = H; e.ld = w.ld;
    e.n_frames = w.n_frames; e.width = w.width; e.n_mels = (int32_t)nm; e.f16 = w.dtype == CSS_WINDOW_F16 ? 1 : 0;
    return e;
}

// The windows of one call on the handle's stream, WINDOW_MULTI_MAX per launch, and the download of what the kernel resolved: after
// the call's synchronise (*res)[i] (page-locked) is window i's.  Every call that gets here ends in that synchronise, so one
// staging serves them all.
int launch_windows(css_ctx* h, std::vector<WindowItem>& w, int32_t* launches, const WindowOut** res) {
    static_assert(WINDOW_MULTI_MAX == CSS_WINDOW_TABLE, "the header states the table's size");
    HandoffCtx* c = handoff_ctx(h);   // (a stream with a frame history has the hand-off on)
    const size_t bytes = w.size() * sizeof(WindowOut);
    int rc;
    if ((rc = ensure(h, c->present, bytes)) != CSS_OK) return rc;
    if (c->present_pin.cap < bytes) HIPCHK(h, c->present_pin.alloc(bytes));
    for (size_t i = 0; i < w.size(); ++i) w[i].res = (WindowOut*)c->present.p + i;
    for (size_t i0 = 0; i0 < w.size(); i0 += WINDOW_MULTI_MAX, ++*launches)
        launch_stream_windows(w.data() + i0, (int)std::min<size_t>(WINDOW_MULTI_MAX, w.size() - i0), h->stream);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(c->present_pin.p, c->present.p, bytes, hipMemcpyDeviceToHost, h->stream));
    *res = c->present_pin.as<WindowOut>();
    return CSS_OK;
}

}  // namespace

void stream_destroy_all(css_ctx* h) {
    for (int i = 0; i < CSS_MAX_STREAMS; ++i)
        if (h->streams[i]) { delete static_cast<StreamState*>(h->streams[i]); h->streams[i] = nullptr; }
    h->stream_masks.reset();
    delete handoff_ctx(h);
    h->handoff = nullptr;
}
int stream_open_count(const css_ctx* h) {
    int n = 0;
    for (int i = 0; i < CSS_MAX_STREAMS; ++i) n += h->streams[i] != nullptr;
    return n;
}

int css_stream_final_samples(const CssModelDesc* desc, const CssRunCfg* cfg, int64_t n_pushed, int64_t* n_final) {
    if (!desc || !n_final || n_pushed < 0) return CSS_ERR_INVALID_ARG;
    const int rc = check_cfg(*desc, cfg);
    if (rc != CSS_OK) return rc;
    *n_final = final_frames(n_pushed, cfg->segment_frames, cfg->hop_frames, cfg->dilation_frames + cfg->erosion_frames) * desc->frame_hop;
    return CSS_OK;
}

int css_stream_open(css_handle_t h, const CssRunCfg* cfg, int32_t n_ch, int32_t* stream_id) {
    if (!h) return CSS_ERR_INVALID_ARG;
    if (!cfg || !stream_id) return fail(h, CSS_ERR_INVALID_ARG, "null argument");
    if (h->queued || !h->pending.empty())
        return fail(h, CSS_ERR_STATE, "queued sessions (css_run_enqueue*) are outstanding: css_wait before opening a stream");
    if (h->split) return fail(h, CSS_ERR_STATE, "streams run in CSS_LINEAR_EXACT_F32 only (the split-f16 mode takes whole-session decisions)");
    if (h->d.frame_len != 512 || h->d.frame_hop != 256 || !h->fft512)
        return fail(h, CSS_ERR_INVALID_ARG, "streams support frame_len 512 / frame_hop 256 only");
    // channels, windows, mask floor, segmentation (the weights are checked frame by frame as frames become final: push, finish)
    if (n_ch != h->d.num_mics)
        return fail(h, CSS_ERR_SHAPE, "input has " + std::to_string(n_ch) + " channels, the model expects " + std::to_string(h->d.num_mics));
    if (cfg->mask_floor > 1.0f || cfg->mask_floor < 0.f) return fail(h, CSS_ERR_MASK_FLOOR, "mask_floor_db must be <= 0");
    if (cfg->stitching_loss < 0 || cfg->stitching_loss > 1 || cfg->stitching_input < 0 || cfg->stitching_input > 1)
        return fail(h, CSS_ERR_INVALID_ARG, "unexpected stitching_loss / stitching_input");
    if (check_cfg(h->d, cfg) != CSS_OK) return fail(h, CSS_ERR_INVALID_ARG, "segment weights missing / bad segmentation / gate");
    int rc = CSS_OK;
    int id = -1;
    for (int i = 0; i < CSS_MAX_STREAMS && id < 0; ++i)
        if (!h->streams[i]) id = i;
    if (id < 0) return fail(h, CSS_ERR_STATE, "too many open streams on this handle (CSS_MAX_STREAMS)");
    HIPCHK(h, hipSetDevice(h->device));
    std::unique_ptr<StreamState> owner(new StreamState());
    StreamState* s = owner.get();
    const int T = cfg->segment_frames, hop = cfg->hop_frames, F = h->d.num_bins, S = h->d.num_spks, N = h->d.frame_len;
    s->cfg = *cfg;
    s->w.resize(3 * (size_t)T);
    std::memcpy(s->w.data(), cfg->w_first, T * sizeof(float));
    std::memcpy(s->w.data() + T, cfg->w_mid, T * sizeof(float));
    std::memcpy(s->w.data() + 2 * T, cfg->w_last, T * sizeof(float));
    s->cfg.w_first = s->w.data(); s->cfg.w_mid = s->w.data() + T; s->cfg.w_last = s->w.data() + 2 * T;
    s->n_ch = n_ch; s->T = T; s->hop = hop; s->halo = cfg->dilation_frames + cfg->erosion_frames;
    const int64_t piece_frames = (int64_t)PIECE_SEGMENTS * hop;
    s->piece = piece_frames * h->d.frame_hop;
    s->WF = ((2 * (int64_t)T + 2 * s->halo + 3 * (int64_t)hop + piece_frames + 16) + 3) / 4 * 4;
    s->WS = (s->WF * h->d.frame_hop + N + 31) / 32 * 32;
    s->SC = s->WF / hop + 3;
    const int64_t out_ld = (piece_frames + T + s->halo + 4) * h->d.frame_hop;
    s->host_cm.resize((size_t)n_ch * s->piece);
    auto alloc = [&](DevBuf& b, size_t bytes) { return ensure(h, b, bytes, true); };
    for (int b = 0; b < 2 && rc == CSS_OK; ++b) {
        if ((rc = alloc(s->pcm[b], (size_t)n_ch * s->WS * sizeof(float))) != CSS_OK) break;
        if ((rc = alloc(s->X[b], (size_t)n_ch * X_ROWS_PER_BIN * F * s->WF * sizeof(float))) != CSS_OK) break;
        if ((rc = alloc(s->masks[b], (size_t)(S + 1) * F * s->SC * T * sizeof(float))) != CSS_OK) break;
        if ((rc = alloc(s->sep[b], (size_t)s->SC * S * F * T * 2 * sizeof(float))) != CSS_OK) break;
        if ((rc = alloc(s->perms[b], (size_t)(s->SC + 1) * S * sizeof(int32_t))) != CSS_OK) break;
        if ((rc = alloc(s->act_b[b], (size_t)S * s->WF)) != CSS_OK) break;
        if ((rc = alloc(s->G[b], (size_t)S * s->WF * N * sizeof(float))) != CSS_OK) break;
    }
    if (rc == CSS_OK) rc = alloc(s->scm, (size_t)s->SC * (S + 1) * F * 49 * sizeof(double));
    if (rc == CSS_OK) rc = alloc(s->bfw, (size_t)s->SC * S * F * 7 * 2 * sizeof(double));
    if (rc == CSS_OK) rc = alloc(s->pnorm, (size_t)s->SC * sizeof(double));
    if (rc == CSS_OK) rc = alloc(s->costs, (size_t)(s->SC + 1) * S * S * sizeof(double));
    if (rc == CSS_OK) rc = alloc(s->pit_part, pit_cost_scratch_bytes(s->SC));
    if (rc == CSS_OK) rc = alloc(s->Y, (size_t)S * s->WF * h->KIp * sizeof(float));
    if (rc == CSS_OK) rc = alloc(s->out, (size_t)S * out_ld * sizeof(float));
    if (rc == CSS_OK) rc = alloc(s->segw, 3 * (size_t)T * sizeof(float));
    if (rc != CSS_OK) return rc;
    std::vector<int32_t> ident(S);
    for (int k = 0; k < S; ++k) ident[k] = k;
    hipError_t e = hipMemcpyAsync((int32_t*)s->perms[0].p + S, ident.data(), S * sizeof(int32_t), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(s->segw.p, s->w.data(), 3 * (size_t)T * sizeof(float), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, CSS_ERR_HIP, std::string("stream setup: ") + hipGetErrorString(e));
    h->streams[id] = owner.release();
    *stream_id = id;
    return CSS_OK;
}

// The one push path (css_stream_push_many, css_stream_push_many_pcm16 and their single-item forms).  An item's samples come as
// float32 [n][C] or as int16 with strides; the source of a piece is the only thing the two kinds of call differ in.  Every
// item is checked against its stream's state before anything moves (ids are distinct, so the checks are those of the
// item-by-item calls); then the call works in rounds: round r takes piece r of every item that still has one -- the samples
// into the windows, analysis transforms, the estimator over all segments the round completed (segments), the stitching tail
// of all streams (tail), the downloads.
//   float32: the piece is transposed on the host into the stream's staging buffer and uploaded from there; one synchronise
//            per round, because the next round reuses that buffer.
//   int16:   the piece is copied as it is from the caller's memory into the stream's device staging (one contiguous copy
//            for an interleaved piece, one 2-D copy for a planar one) and ONE table launch per round converts all streams'
//            pieces into their windows (stream.hip stream_ingest_pcm16_kernel).  No host buffer is reused, the next round's
//            copy into the staging is ordered behind the launch on the stream: no synchronise but the one that ends the call.
//            (Nothing else leans on the per-round synchronise: the hand-off's page-locked staging is per round of a call, and
//            every device buffer the rounds share is written and read in stream order.)
//   a rate stream (either kind of call): the piece, cut in INPUT samples, is copied as it is into the stream's device staging
//            and ONE table launch per round resamples all rate streams' pieces into their windows (resample.hip
//            stream_ingest_resample_kernel); the rate-less items of the call take their own route above.  No host buffer,
//            no synchronise of its own.
namespace {

struct PushItem {
    int32_t id;
    const float* f32;                                   // float call: [n_samples][C]
    const int16_t* i16; int64_t sample_stride, channel_stride;   // PCM16 call
    int64_t n_samples; float* out_host; int64_t cap; int64_t* n_out;
};

int push_items(css_ctx* h, const std::vector<PushItem>& items, bool pcm16, CssStreamGroupStats* stats) {
    struct Item { StreamState* s; const PushItem* p; int64_t done, emitted, n, t_g1, t_g_before; bool planar; int64_t n_in, written; };
    std::vector<Item> its(items.size());
    for (size_t i = 0; i < items.size(); ++i) {
        const PushItem& p = items[i];
        auto refuse = [&](int code, const std::string& msg) {
            return fail(h, code, "item " + std::to_string(i) + " (stream " + std::to_string(p.id) + "): " + msg);
        };
        StreamState* s = nullptr;
        std::string why;
        const int irc = check_group_item(h, i, [&](size_t k) { return items[k].id; }, &s, &why);
        if (irc != CSS_OK) return refuse(irc, why);
        const void* src = pcm16 ? (const void*)p.i16 : (const void*)p.f32;
        if (p.n_samples < 0 || (p.n_samples > 0 && !src)) return refuse(CSS_ERR_INVALID_ARG, "bad argument");
        bool planar = false;
        if (pcm16 && p.n_samples > 0) {   // (an item without samples takes no part, whatever its strides say)
            // (one channel: consecutive samples are both layouts, whatever channel_stride says, and are copied as one run)
            const bool inter = (p.sample_stride == s->n_ch && p.channel_stride == 1) || (s->n_ch == 1 && p.sample_stride == 1);
            planar = !inter && p.sample_stride == 1 && p.channel_stride >= p.n_samples;
            if (!inter && !planar)
                return refuse(CSS_ERR_INVALID_ARG, "PCM16 strides: interleaved (sample_stride = channels, channel_stride = 1) or planar "
                                                   "(sample_stride = 1, channel_stride >= n_samples)");
        }
        if (h->split) return refuse(CSS_ERR_STATE, "streams run in CSS_LINEAR_EXACT_F32 only");
        // (a rate stream: n_samples counts inputs; every check below is on the model-rate samples they make available)
        const int64_t n_after = model_samples_after(s, p.n_samples);
        const int64_t need = final_frames(n_after, s->T, s->hop, s->halo) * h->d.frame_hop - s->n_emitted;
        // (a stream with an output format may leave the model-rate out_host out)
        if (need > 0 && (p.out_host ? p.cap < need : !s->outp))
            return refuse(CSS_ERR_INVALID_ARG, "output capacity too small for the samples this push finalises");
        if (zero_weight_frames(s, s->t_st, segments_done(frames_of(n_after), s->T, s->hop) * s->hop))
            return refuse(CSS_ERR_ZERO_WEIGHT, "zero weights found. check hop_size, segment_size or m0, m1");
        const int hrc = check_handoff_call(h, s, n_after - s->n_pushed, &why);
        if (hrc != CSS_OK) return refuse(hrc, why);
        const int orc = check_output_call(s, std::max<int64_t>(need, 0), false, &why);
        if (orc != CSS_OK) return refuse(orc, why);
        its[i] = Item{s, &p, 0, 0, 0, 0, s->t_g, planar, 0, 0};
    }
    if (stats) *stats = CssStreamGroupStats{};
    h->stream_out_launches = h->stream_out_rounds = 0;
    handoff_begin_call(h);
    std::vector<HandoffJob> hj;
    std::vector<HandoffRec> recs;
    auto hand_out = [&]() {   // (a call that moved nothing still reports its empty hand-off)
        for (size_t i = 0; i < its.size(); ++i)
            if (its[i].written == 0) output_report_idle(h, its[i].s);
        for (size_t i = 0; i < its.size(); ++i)
            if (its[i].s->ho) {
                const int hrc = handoff_collect(h, its[i].s, (int)i, its[i].t_g_before, recs, its[i].s->ho->m, its[i].s->ho->bound, true);
                if (hrc != CSS_OK) return hrc;
            }
        return (int)CSS_OK;
    };
    bool any = false;
    for (Item& it : its) { *it.p->n_out = 0; any = any || it.p->n_samples > 0; }
    if (!any) return hand_out();
    HIPCHK(h, hipSetDevice(h->device));
    const int hopS = h->d.frame_hop;
    int rc;
    // a stream's first PCM16 push: device staging for one piece, [piece][C] interleaved or C planes of `piece` values
    if (pcm16)
        for (Item& it : its)
            if (it.p->n_samples > 0 && !it.s->rate &&
                (rc = ensure(h, it.s->pcm16_stage, (size_t)it.s->n_ch * it.s->piece * sizeof(int16_t))) != CSS_OK) return rc;
    std::vector<Item*> act;
    std::vector<SegJob> sj;
    std::vector<TailJob> tj;
    std::vector<StreamIngestPcm16> ing;
    std::vector<ResampleJob> rsj;
    std::vector<StreamOutputJob> oj;
    std::vector<int64_t> o_nm;
    for (size_t round = 0;; ++round) {
        act.clear();
        for (Item& it : its)
            if (it.done < it.p->n_samples) act.push_back(&it);
        if (act.empty()) break;
        ing.clear(); rsj.clear();
        bool host_staging = false;
        for (Item* it : act) {
            StreamState* s = it->s;
            const int C = s->n_ch;
            // a rate stream's piece is cut in inputs so that the outputs it makes available are at most `piece` window samples:
            // avail(N) <= n_pushed + piece  <=>  N <= ((n_pushed + piece) down + half) / up
            if (RateStream* q = s->rate.get())
                it->n_in = std::min<int64_t>(it->p->n_samples - it->done, ((s->n_pushed + s->piece) * q->r.down + q->r.half) / q->r.up - q->n_in);
            else
                it->n_in = std::min<int64_t>(s->piece, it->p->n_samples - it->done);
            const int64_t n = it->n = model_samples_after(s, it->n_in) - s->n_pushed;
            const int64_t N1 = s->n_pushed + n, K1 = frames_of(N1);
            if (K1 - s->seg_base * s->hop > s->WF || N1 - s->seg_base * s->hop * hopS > s->WS) {
                if ((rc = rebase(h, s)) != CSS_OK) return rc;
                if (K1 - s->seg_base * s->hop > s->WF || N1 - s->seg_base * s->hop * hopS > s->WS)
                    return fail(h, CSS_ERR_STATE, "stream window overflow");
            }
            const int64_t sb = s->seg_base * s->hop * hopS;
            float* win = (float*)s->pcm[s->cur].p + (s->n_pushed - sb);
            if (RateStream* q = s->rate.get()) {
                // the caller's samples as they are into the device staging, then the round's resample launch
                const int64_t ni = it->n_in;
                const size_t el = pcm16 ? sizeof(int16_t) : sizeof(float);
                const char* src = pcm16 ? (const char*)it->p->i16 : (const char*)it->p->f32;
                if (it->planar)
                    HIPCHK(h, hipMemcpy2DAsync(q->stage.p, (size_t)q->max_in * el, src + (size_t)it->done * el, (size_t)it->p->channel_stride * el,
                                               (size_t)ni * el, (size_t)C, hipMemcpyHostToDevice, h->stream));
                else
                    HIPCHK(h, hipMemcpyAsync(q->stage.p, src + (size_t)it->done * C * el, (size_t)ni * C * el, hipMemcpyHostToDevice, h->stream));
                rsj.push_back(rate_job(s, pcm16, it->planar, ni, s->n_pushed + n, win, false));
                continue;
            }
            if (pcm16) {
                int16_t* stage = (int16_t*)s->pcm16_stage.p;
                if (it->planar)
                    HIPCHK(h, hipMemcpy2DAsync(stage, (size_t)s->piece * sizeof(int16_t), it->p->i16 + it->done,
                                               (size_t)it->p->channel_stride * sizeof(int16_t), (size_t)n * sizeof(int16_t), (size_t)C,
                                               hipMemcpyHostToDevice, h->stream));
                else
                    HIPCHK(h, hipMemcpyAsync(stage, it->p->i16 + it->done * C, (size_t)n * C * sizeof(int16_t), hipMemcpyHostToDevice, h->stream));
                ing.push_back(StreamIngestPcm16{stage, it->planar ? s->piece : 0, n, C, win, s->WS});
                continue;
            }
            // samples -> the window, channel-major (a plain copy: the transform reads the same values css_run's does)
            host_staging = true;
            const float* src = it->p->f32 + it->done * C;
            for (int ch = 0; ch < C; ++ch) {
                float* d = s->host_cm.data() + (size_t)ch * n;
                for (int64_t i = 0; i < n; ++i) d[i] = src[i * C + ch];
            }
            HIPCHK(h, hipMemcpy2DAsync(win, (size_t)s->WS * sizeof(float), s->host_cm.data(),
                                       (size_t)n * sizeof(float), (size_t)n * sizeof(float), (size_t)C, hipMemcpyHostToDevice, h->stream));
        }
        if (!rsj.empty() && !launch_stream_ingest_resample_multi(rsj.data(), (int)rsj.size(), h->stream))
            return fail(h, CSS_ERR_HIP, "the resampling kernel's LDS could not be reserved");
        if (pcm16) {
            launch_stream_ingest_pcm16_multi(ing.data(), (int)ing.size(), h->stream);
        } else if (host_staging) {
            // the host staging buffers are reused by the next round (a rate stream has none: its piece went from the caller's memory)
            HIPCHK(h, hipStreamSynchronize(h->stream));
        }
        sj.clear(); tj.clear();
        for (Item* it : act) {
            StreamState* s = it->s;
            const int c = s->cur;
            const int64_t fb = s->seg_base * s->hop;
            s->n_pushed += it->n;
            const int64_t K1 = frames_of(s->n_pushed);
            bool ph = false;
            if (K1 > s->K &&
                !analysis_transform(h, (const float*)s->pcm[c].p, s->WS, s->n_ch, s->K - fb, K1 - fb, (float*)s->X[c].p, s->WF, h->stream,
                                    (float*)s->X[c].p + (int64_t)s->n_ch * 2 * h->d.num_bins * s->WF, &ph))
                return fail(h, CSS_ERR_HIP, "the analysis transform's LDS could not be reserved");
            s->K = std::max(s->K, K1);
            const int64_t sd1 = segments_done(s->K, s->T, s->hop);
            sj.push_back(SegJob{s, s->sd, sd1, s->K - fb});
            const int64_t t_st1 = sd1 * s->hop;
            it->t_g1 = std::max<int64_t>(t_st1 - s->halo, 0);
            tj.push_back(TailJob{s, false, 0, 0, s->t_st, t_st1, s->t_g, it->t_g1, it->t_g1});
        }
        if ((rc = segments(h, sj, stats)) != CSS_OK) return rc;
        for (const SegJob& j : sj) j.s->sd = j.g_hi;
        if ((rc = tail(h, tj)) != CSS_OK) return rc;
        hj.clear();
        for (Item* it : act)
            if (it->s->ho) hj.push_back(HandoffJob{it->s, (int)(it - its.data()), it->s->t_g, it->t_g1, (it->t_g1 - it->s->t_g) * hopS, false, 0});
        if ((rc = handoff_round(h, hj, round, &recs)) != CSS_OK) return rc;
        // the streams with an output format whose tail() made samples final: one launch for all of them
        oj.clear(); o_nm.clear();
        for (Item* it : act) {
            const int64_t n_new = (it->t_g1 - it->s->t_g) * hopS;
            if (!it->s->outp || n_new <= 0) continue;
            oj.emplace_back(); o_nm.push_back(0);
            if ((rc = output_job(h, it->s, it->emitted, n_new, n_new, false, &oj.back(), &o_nm.back())) != CSS_OK) return rc;
        }
        if (!oj.empty()) {
            if (!launch_stream_output_multi(oj.data(), (int)oj.size(), h->d.num_spks, h->stream, &h->stream_out_launches))
                return fail(h, CSS_ERR_HIP, "the output kernel's LDS could not be reserved");
            h->stream_out_rounds += 1;
            HIPCHK(h, hipGetLastError());
        }
        size_t oi = 0;
        for (Item* it : act) {
            StreamState* s = it->s;
            const int64_t n_new = (it->t_g1 - s->t_g) * hopS;
            if (s->outp && n_new > 0) {
                if ((rc = output_download(h, s, o_nm[oi], it->written)) != CSS_OK) return rc;
                it->written += o_nm[oi++];
            }
            if (it->p->out_host && (rc = download(h, s, n_new, it->p->out_host, it->p->cap, it->emitted)) != CSS_OK) return rc;
            it->emitted += n_new;
            s->t_st = s->sd * s->hop;
            s->t_g = it->t_g1;
            it->done += it->n_in;
        }
    }
    for (Item& it : its)
        if (it.s->outp && it.emitted > 0 && (rc = output_counters(h, it.s)) != CSS_OK) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (Item& it : its) {
        if (it.s->outp) {
            if (it.emitted > 0) output_report(h, it.s, it.written);
        } else if (it.emitted > 0) {
            host_peak(h, it.s, it.p->out_host, it.p->cap, it.emitted);
        }
        it.s->n_emitted += it.emitted;
        *it.p->n_out = it.emitted;
    }
    return hand_out();
}

}  // namespace

int css_stream_push_many(css_handle_t h, CssStreamPush* items, int32_t n_items, CssStreamGroupStats* stats) {
    if (!h) return CSS_ERR_INVALID_ARG;
    if (n_items < 0 || (n_items > 0 && !items)) return fail(h, CSS_ERR_INVALID_ARG, "bad argument");
    std::vector<PushItem> v((size_t)n_items);
    for (int32_t i = 0; i < n_items; ++i) {
        CssStreamPush& p = items[i];
        v[(size_t)i] = PushItem{p.id, p.pcm_host, nullptr, 0, 0, p.n_samples, p.out_host, p.cap, &p.n_out};
    }
    return push_items(h, v, false, stats);
}

int css_stream_push_many_pcm16(css_handle_t h, CssStreamPushPcm16* items, int32_t n_items, CssStreamGroupStats* stats) {
    if (!h) return CSS_ERR_INVALID_ARG;
    if (n_items < 0 || (n_items > 0 && !items)) return fail(h, CSS_ERR_INVALID_ARG, "bad argument");
    std::vector<PushItem> v((size_t)n_items);
    for (int32_t i = 0; i < n_items; ++i) {
        CssStreamPushPcm16& p = items[i];
        v[(size_t)i] = PushItem{p.id, nullptr, p.pcm16_host, p.sample_stride, p.channel_stride, p.n_samples, p.out_host, p.cap, &p.n_out};
    }
    return push_items(h, v, true, stats);
}

// a group of one item
int css_stream_push(css_handle_t h, int32_t id, const float* pcm_host, int64_t n_samples, float* out_host, int64_t cap, int64_t* n_out) {
    if (!h) return CSS_ERR_INVALID_ARG;
    if (!n_out) return fail(h, CSS_ERR_INVALID_ARG, "bad argument");
    CssStreamPush p{id, pcm_host, n_samples, out_host, cap, 0};
    const int rc = css_stream_push_many(h, &p, 1, nullptr);
    if (rc == CSS_OK) *n_out = p.n_out;
    return rc;
}

int css_stream_push_pcm16(css_handle_t h, int32_t id, const int16_t* pcm16_host, int64_t n_samples, int64_t sample_stride,
                          int64_t channel_stride, float* out_host, int64_t cap, int64_t* n_out) {
    if (!h) return CSS_ERR_INVALID_ARG;
    if (!n_out) return fail(h, CSS_ERR_INVALID_ARG, "bad argument");
    CssStreamPushPcm16 p{id, pcm16_host, n_samples, sample_stride, channel_stride, out_host, cap, 0};
    const int rc = css_stream_push_many_pcm16(h, &p, 1, nullptr);
    if (rc == CSS_OK) *n_out = p.n_out;
    return rc;
}

// ---- the closing pass: css_stream_finish and the previews (include/css_mi355_preview.h) ------------------------------------------
// What ends a recording after its last pushed sample, for a vector of streams: a rate stream's resampler is flushed into the
// window (one table launch for all of them) and the frames the flushed samples complete are transformed; the frames the one
// pending segment reads past the last transformed one are zeroed (css.py:159-164 pads a short recording; the last segment's
// tail); segments() runs that segment of every stream (the estimator as one batch per segmentation) and tail() closes every
// stream's output with the last-segment window; then the downloads and ONE synchronise.
//   commit      css_stream_finish: the hand-off's closing round runs, and the progress counters move to the recording's end.
//   no commit   a preview: nothing of StreamState, RateStream or HandoffStream changes but the window's generation, if a rebase
//               was needed.  Without hand-off outputs (CloseJob::ho null) StreamStitchArgs::gate_out stays null, so the gate
//               ring is not written.  With them (css_mi355_preview_handoff.h) the gate bytes of frames [t_g, mix_frames) go
//               into the stream's own ring and the hand-off's closing round runs without a commit (handoff_round): D, cur, the
//               device's HandoffState rows and the host mirrors stay, the results are collected on a copy of the mirrors into
//               the caller's outputs.  The ring holds >= WF + 2 pad + 8 frames and mix_frames - t_g <= WF (both lie in the
//               window and the window starts at or before t_g), so the provisional bytes replace no frame from
//               t_g - 2 pad - 3 on, the oldest a later round reads; a later round writes frames [t_g, its t_g1) again before
//               its append kernel reads them, and reads none from its t_g1 on.  Every
//               device region written here is written again before a later pass reads it, because sd, t_st and t_g stay:
//               mask / sep / permutation / cost slots from sd - seg_base on, act_b from t_st on, G rows from t_g on, the window
//               samples from n_pushed and the planes from frame K on (the next push's ingest and transform), and the scratch
//               (scm, bfw, pnorm, pit_part, Y, out).  The flush passes no hist_out, so the carried inputs stay too.
// finish zero-fills to the window's end, once; a preview, which runs every tick, only the frames its segment reads.
namespace {

struct CloseJob {
    StreamState* s; CssPlan p; int64_t n_total;   // the recording's length in model-rate samples, its plan
    float* out_host; int64_t cap, need;           // samples [n_emitted, p.n_out) -> out_host[S][cap]
    CssStreamHandoffOut* ho = nullptr;            // a preview with hand-off: the caller's outputs and first_frame [S]
    int64_t* first_frame = nullptr;
    CssStreamPresentWindow* windows = nullptr;    // ... that also writes windows up to the present (css_mi355_present_window.h):
    int32_t n_windows = 0; size_t win0 = 0;       // the item's windows; the index of its first one among the call's
};

// What one css_stream_present_windows call launches: `total` windows over all jobs, `launches` kernel launches; after the call's
// synchronise `res` (page-locked) holds the spans the kernel resolved, window CloseJob::win0 + w of a job at that index.
struct PresentCall { size_t total = 0; int32_t launches = 0; const WindowOut* res = nullptr; };

// The windows of a preview's jobs, behind the hand-off round `recs` on the handle's stream: the provisional frames, their maxima
// and their counts are that round's results, which the next round overwrites.
int present_windows(css_ctx* h, const std::vector<CloseJob>& jobs, const std::vector<HandoffRec>& recs, PresentCall* pc) {
    std::vector<WindowItem> w(pc->total);
    for (size_t i = 0; i < jobs.size(); ++i) {
        const CloseJob& j = jobs[i];
        if (!j.n_windows) continue;
        const HandoffRec* r = nullptr;
        for (const HandoffRec& x : recs)
            if (x.s == j.s && x.item == (int)i) r = &x;
        if (!r || !r->pvmax_dev) return fail(h, CSS_ERR_STATE, "windows up to the present without the preview's hand-off round");
        const HandoffStream* o = j.s->ho.get();
        for (int32_t q = 0; q < j.n_windows; ++q) {
            WindowItem& e = w[j.win0 + (size_t)q];
            e = history_item(o, j.windows[q]);
            const int64_t k = j.windows[q].speaker;
            e.pv = r->mel_dev + k * o->cfg.n_mels * r->mel_ld;
            e.pvmax = r->pvmax_dev + k * r->mel_ld;
            e.n_new = r->n_new_dev + k;
            e.J = o->m.J[(size_t)k]; e.pv_ld = r->mel_ld;
        }
    }
    return launch_windows(h, w, &pc->launches, &pc->res);
}

int closing_pass(css_ctx* h, const std::vector<CloseJob>& jobs, bool commit, CssStreamGroupStats* stats, PresentCall* pc = nullptr) {
    if (jobs.empty()) return CSS_OK;
    int rc;
    std::vector<HandoffRec> recs;
    std::vector<int64_t> t_g_before(jobs.size());
    bool any_ho = commit;
    for (const CloseJob& j : jobs) any_ho = any_ho || j.ho;
    if (any_ho) handoff_begin_call(h);
    HIPCHK(h, hipSetDevice(h->device));
    const int hopS = h->d.frame_hop, F = h->d.num_bins, S = h->d.num_spks;
    std::vector<ResampleJob> rsj;
    for (size_t i = 0; i < jobs.size(); ++i) {
        StreamState* s = jobs[i].s;
        t_g_before[i] = s->t_g;
        const int64_t n_total = jobs[i].n_total, K1 = std::max(s->K, frames_of(n_total));
        const int64_t TL = jobs[i].p.mix_frames, nseg = jobs[i].p.num_segments;
        auto past_window = [&]() {
            const int64_t fb = s->seg_base * s->hop;
            return K1 - fb > s->WF || n_total - fb * hopS > s->WS || TL - fb > s->WF || nseg - s->seg_base > s->SC;
        };
        if (past_window()) {
            if ((rc = rebase(h, s)) != CSS_OK) return rc;
            if (past_window()) return fail(h, CSS_ERR_STATE, "stream window overflow");
        }
        // flush the resampler: the samples that waited for inputs, into the window (fewer than a frame's worth: half / down + 1)
        if (n_total > s->n_pushed)
            rsj.push_back(rate_job(s, false, false, 0, n_total, (float*)s->pcm[s->cur].p + (s->n_pushed - s->seg_base * s->hop * hopS), true));
    }
    if (!rsj.empty() && !launch_stream_ingest_resample_multi(rsj.data(), (int)rsj.size(), h->stream))
        return fail(h, CSS_ERR_HIP, "the resampling kernel's LDS could not be reserved");
    std::vector<SegJob> sj;
    std::vector<TailJob> tj;
    for (const CloseJob& j : jobs) {
        StreamState* s = j.s;
        const int c = s->cur;
        const int64_t fb = s->seg_base * s->hop, K1 = std::max(s->K, frames_of(j.n_total));
        const int64_t TL = j.p.mix_frames, nseg = j.p.num_segments;
        bool ph = false;
        if (K1 > s->K &&
            !analysis_transform(h, (const float*)s->pcm[c].p, s->WS, s->n_ch, s->K - fb, K1 - fb, (float*)s->X[c].p, s->WF, h->stream,
                                (float*)s->X[c].p + (int64_t)s->n_ch * 2 * F * s->WF, &ph))
            return fail(h, CSS_ERR_HIP, "the analysis transform's LDS could not be reserved");
        // frames past the last transformed one are zero: to the window's end, or to the end of the pending segment
        const int64_t z_hi = commit ? s->WF : std::min<int64_t>(s->WF, (nseg - 1) * s->hop + s->T - fb);
        if (z_hi > K1 - fb)
            HIPCHK(h, hipMemset2DAsync((float*)s->X[c].p + (K1 - fb), (size_t)s->WF * sizeof(float), 0,
                                       (size_t)(z_hi - (K1 - fb)) * sizeof(float), (size_t)s->n_ch * X_ROWS_PER_BIN * F, h->stream));
        sj.push_back(SegJob{s, s->sd, nseg, K1 - fb});
        // the rest of the output: blocks up to mix_frames (frame_len = 2 hop: block TL holds the last frame's second half)
        const int64_t q_hi = TL + 1;
        if ((q_hi - s->t_g) * hopS > (int64_t)(s->out.cap / (sizeof(float) * S)) &&
            (rc = ensure(h, s->out, (size_t)S * (q_hi - s->t_g) * hopS * sizeof(float))) != CSS_OK) return rc;
        TailJob t{s, true, nseg, TL, s->t_st, TL, s->t_g, TL, q_hi};
        t.gate = commit || j.ho;
        tj.push_back(t);
    }
    if ((rc = segments(h, sj, stats)) != CSS_OK) return rc;
    if ((rc = tail(h, tj)) != CSS_OK) return rc;
    if (any_ho) {
        std::vector<HandoffJob> hj;
        for (size_t i = 0; i < jobs.size(); ++i) {
            StreamState* s = jobs[i].s;
            const int64_t TL = jobs[i].p.mix_frames;
            if (commit || jobs[i].ho)
                hj.push_back(HandoffJob{s, (int)i, s->t_g, TL, (TL + 1 - s->t_g) * hopS, true, jobs[i].p.n_out, jobs[i].n_windows > 0});
        }
        if ((rc = handoff_round(h, hj, 0, &recs, commit)) != CSS_OK) return rc;
        if (pc && pc->total && (rc = present_windows(h, jobs, recs, pc)) != CSS_OK) return rc;
    }
    // finish of a stream with an output format: the rest of its samples, and the outputs that waited for inputs past the end
    std::vector<int64_t> o_nm(jobs.size(), 0);
    if (commit) {
        h->stream_out_launches = h->stream_out_rounds = 0;
        std::vector<StreamOutputJob> oj;
        for (size_t i = 0; i < jobs.size(); ++i) {
            StreamState* s = jobs[i].s;
            if (!s->outp || jobs[i].need <= 0) continue;
            oj.emplace_back();
            if ((rc = output_job(h, s, 0, jobs[i].need, (jobs[i].p.mix_frames + 1 - s->t_g) * hopS, true, &oj.back(), &o_nm[i])) != CSS_OK) return rc;
        }
        if (!oj.empty()) {
            if (!launch_stream_output_multi(oj.data(), (int)oj.size(), S, h->stream, &h->stream_out_launches))
                return fail(h, CSS_ERR_HIP, "the output kernel's LDS could not be reserved");
            h->stream_out_rounds += 1;
            HIPCHK(h, hipGetLastError());
        }
        for (size_t i = 0; i < jobs.size(); ++i)
            if (jobs[i].s->outp && jobs[i].need > 0) {
                if ((rc = output_download(h, jobs[i].s, o_nm[i], 0)) != CSS_OK) return rc;
                if ((rc = output_counters(h, jobs[i].s)) != CSS_OK) return rc;
            }
    }
    for (const CloseJob& j : jobs)
        if (j.out_host && (rc = download(h, j.s, j.need, j.out_host, j.cap, 0)) != CSS_OK) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (!commit) {
        for (size_t i = 0; i < jobs.size(); ++i) {
            if (!jobs[i].ho) continue;
            HandoffMirror m = jobs[i].s->ho->m;
            for (int k = 0; k < S; ++k) jobs[i].first_frame[k] = m.J[(size_t)k];
            if ((rc = handoff_collect(h, jobs[i].s, (int)i, t_g_before[i], recs, m, jobs[i].ho, false)) != CSS_OK) return rc;
        }
        return CSS_OK;
    }
    for (size_t i = 0; i < jobs.size(); ++i) {
        StreamState* s = jobs[i].s;
        if (s->ho && (rc = handoff_collect(h, s, (int)i, t_g_before[i], recs, s->ho->m, s->ho->bound, true)) != CSS_OK) return rc;
        if (s->outp) {
            if (jobs[i].need > 0) output_report(h, s, o_nm[i]);
            else output_report_idle(h, s);
        } else if (jobs[i].need > 0) {
            host_peak(h, s, jobs[i].out_host, jobs[i].cap, jobs[i].need);
        }
        s->n_pushed = jobs[i].n_total;
        s->K = std::max(s->K, frames_of(jobs[i].n_total));
        s->sd = jobs[i].p.num_segments; s->t_st = s->t_g = jobs[i].p.mix_frames;
        s->n_emitted += jobs[i].need;
        s->finished = true;
    }
    return CSS_OK;
}

// the recording a closing pass ends: ceil(n_in up / down) model-rate samples for a rate stream (the last of them read zeros past the end)
int64_t closing_samples(const StreamState* s) { return s->rate ? resample_count(s->rate->r, s->rate->n_in, true) : s->n_pushed; }

}  // namespace

int css_stream_finish(css_handle_t h, int32_t id, float* out_host, int64_t cap, int64_t* n_out) {
    StreamState* s = nullptr;
    int rc = check_stream_call(h, id, &s);
    if (rc != CSS_OK) return rc;
    if (s->finished) return fail(h, CSS_ERR_STATE, "the stream has finished");
    if (!n_out) return fail(h, CSS_ERR_INVALID_ARG, "null argument");
    if (h->split) return fail(h, CSS_ERR_STATE, "streams run in CSS_LINEAR_EXACT_F32 only");
    CloseJob j{s, CssPlan{}, closing_samples(s), out_host, cap, 0};
    plan_impl(h->d, s->cfg, j.n_total, &j.p);
    if (j.p.zero_weight) return fail(h, CSS_ERR_ZERO_WEIGHT, "zero weights found. check hop_size, segment_size or m0, m1");
    j.need = j.p.n_out - s->n_emitted;
    // (a stream with an output format may leave the model-rate out_host out)
    if (out_host ? cap < j.need : !s->outp) return fail(h, CSS_ERR_INVALID_ARG, "output capacity too small for the rest of the stream");
    std::string why;
    if ((rc = check_handoff_call(h, s, -1, &why)) != CSS_OK) return fail(h, rc, why);
    if ((rc = check_output_call(s, j.need, true, &why)) != CSS_OK) return fail(h, rc, why);
    if ((rc = closing_pass(h, {j}, true, nullptr)) != CSS_OK) return rc;
    *n_out = j.need;
    return CSS_OK;
}

// ---- previews (include/css_mi355_preview.h) ------------------------------------------------------------------------------------
int css_stream_preview_samples(const CssModelDesc* desc, const CssRunCfg* cfg, int64_t n_pushed, int64_t* first, int64_t* count) {
    if (!desc || !first || !count || n_pushed < 0) return CSS_ERR_INVALID_ARG;
    const int rc = check_cfg(*desc, cfg);
    if (rc != CSS_OK) return rc;
    CssPlan p{};
    if (plan_impl(*desc, *cfg, n_pushed, &p) != CSS_OK) return CSS_ERR_INVALID_ARG;
    *first = final_frames(n_pushed, cfg->segment_frames, cfg->hop_frames, cfg->dilation_frames + cfg->erosion_frames) * desc->frame_hop;
    *count = p.n_out - *first;
    return p.zero_weight ? CSS_ERR_ZERO_WEIGHT : CSS_OK;
}

namespace {

// one item of a grouped preview: the waveform item and, for a preview with hand-off, the caller's outputs
// ... and, for css_stream_present_windows (`present`), its windows
struct PreviewItem {
    CssStreamPreview* p; CssStreamHandoffOut* ho; int64_t* first_frame;
    bool present = false; CssStreamPresentWindow* windows = nullptr; int32_t n_windows = 0;
};

int preview_items(css_ctx* h, const std::vector<PreviewItem>& items, CssStreamGroupStats* stats, int32_t* window_launches = nullptr) {
    PresentCall pc;
    const int32_t n_items = (int32_t)items.size();
    std::vector<CloseJob> jobs;
    std::vector<int32_t> status((size_t)n_items, CSS_OK);
    std::vector<int64_t> first((size_t)n_items, 0);
    for (int32_t i = 0; i < n_items; ++i) {
        const CssStreamPreview& p = *items[(size_t)i].p;
        auto refuse = [&](int code, const std::string& msg) {
            return fail(h, code, "item " + std::to_string(i) + " (stream " + std::to_string(p.id) + "): " + msg);
        };
        StreamState* s = nullptr;
        std::string why;
        const int irc = check_group_item(h, (size_t)i, [&](size_t k) { return items[k].p->id; }, &s, &why);
        if (irc != CSS_OK) return refuse(irc, why);
        if (h->split) return refuse(CSS_ERR_STATE, "streams run in CSS_LINEAR_EXACT_F32 only");
        CloseJob j{s, CssPlan{}, closing_samples(s), p.out_host, p.cap, 0};
        if (CssStreamHandoffOut* ho = items[(size_t)i].ho) {
            if (!s->ho) return refuse(CSS_ERR_STATE, "the hand-off of this stream is off (css_stream_handoff_open)");
            if (!items[(size_t)i].first_frame) return refuse(CSS_ERR_INVALID_ARG, "hand-off outputs without first_frame");
            const int hrc = check_handoff_out(s, ho, -1, &why);   // a preview is a finish at this moment
            if (hrc != CSS_OK) return refuse(hrc, why);
            j.ho = ho; j.first_frame = items[(size_t)i].first_frame;
        }
        if (items[(size_t)i].present) {
            const PreviewItem& it = items[(size_t)i];
            if (!s->ho || !s->ho->hist_frames) return refuse(CSS_ERR_STATE, "the stream has no frame history (css_stream_window_open)");
            if (it.n_windows < 0 || (it.n_windows > 0 && (!it.windows || !it.ho)))
                return refuse(CSS_ERR_INVALID_ARG, "n_windows < 0, or windows without `windows` or without hand-off outputs (ph.ho)");
            for (int32_t q = 0; q < it.n_windows; ++q) {
                if (const char* bad = window_refusal(h, s->ho.get(), it.windows[q], nullptr))
                    return refuse(CSS_ERR_INVALID_ARG, "window " + std::to_string(q) + ": " + bad);
            }
            j.windows = it.windows; j.n_windows = it.n_windows;
        }
        plan_impl(h->d, s->cfg, j.n_total, &j.p);
        first[(size_t)i] = s->n_emitted;
        if (j.p.zero_weight) { status[(size_t)i] = CSS_ERR_ZERO_WEIGHT; continue; }   // (css_run's refusal of this prefix: the item's own)
        j.need = j.p.n_out - s->n_emitted;
        if (!p.out_host || p.cap < j.need) return refuse(CSS_ERR_INVALID_ARG, "output capacity too small for the preview (css_stream_preview_samples)");
        j.win0 = pc.total;
        pc.total += (size_t)j.n_windows;
        jobs.push_back(j);
    }
    if (stats) *stats = CssStreamGroupStats{};
    const int rc = closing_pass(h, jobs, false, stats, &pc);
    if (rc != CSS_OK) return rc;
    for (const CloseJob& j : jobs)
        for (int32_t q = 0; q < j.n_windows; ++q) {
            const WindowOut& r = pc.res[j.win0 + (size_t)q];
            CssStreamPresentWindow& w = j.windows[q];
            w.first_frame = r.first_frame; w.n_used = r.n_used; w.n_provisional = r.n_provisional;
            if (r.n_used > 0) w.window_max = r.window_max;
        }
    if (window_launches) *window_launches = pc.launches;
    size_t k = 0;
    for (int32_t i = 0; i < n_items; ++i) {
        CssStreamPreview& p = *items[(size_t)i].p;
        p.status = status[(size_t)i];
        p.first_sample = first[(size_t)i];
        p.n_out = status[(size_t)i] == CSS_OK ? jobs[k++].need : 0;
    }
    return CSS_OK;
}

}  // namespace

int css_stream_preview_many(css_handle_t h, CssStreamPreview* items, int32_t n_items, CssStreamGroupStats* stats) {
    if (!h) return CSS_ERR_INVALID_ARG;
    if (n_items < 0 || (n_items > 0 && !items)) return fail(h, CSS_ERR_INVALID_ARG, "bad argument");
    std::vector<PreviewItem> v;
    for (int32_t i = 0; i < n_items; ++i) v.push_back(PreviewItem{&items[i], nullptr, nullptr});
    return preview_items(h, v, stats);
}

// ---- previews with hand-off (include/css_mi355_preview_handoff.h) -------------------------------------------------------------
int css_stream_preview_handoff_many(css_handle_t h, CssStreamPreviewHandoff* items, int32_t n_items, CssStreamGroupStats* stats) {
    if (!h) return CSS_ERR_INVALID_ARG;
    if (n_items < 0 || (n_items > 0 && !items)) return fail(h, CSS_ERR_INVALID_ARG, "bad argument");
    std::vector<PreviewItem> v;
    for (int32_t i = 0; i < n_items; ++i) v.push_back(PreviewItem{&items[i].p, items[i].ho, items[i].first_frame});
    return preview_items(h, v, stats);
}

// ---- previews that also write windows up to the present (include/css_mi355_present_window.h) -----------------------------------
int css_stream_present_windows(css_handle_t h, CssStreamPresentItem* items, int32_t n_items, CssStreamGroupStats* stats,
                               int32_t* window_launches) {
    if (!h) return CSS_ERR_INVALID_ARG;
    if (n_items < 1 || !items) return fail(h, CSS_ERR_INVALID_ARG, "bad argument");
    std::vector<PreviewItem> v;
    for (int32_t i = 0; i < n_items; ++i)
        v.push_back(PreviewItem{&items[i].ph.p, items[i].ph.ho, items[i].ph.first_frame, true, items[i].windows, items[i].n_windows});
    return preview_items(h, v, stats, window_launches);
}

// a group of one item
int css_stream_preview_handoff(css_handle_t h, int32_t id, float* out_host, int64_t cap, int64_t* n_out, int64_t* first_sample,
                               CssStreamHandoffOut* ho, int64_t* first_frame) {
    if (!h) return CSS_ERR_INVALID_ARG;
    if (!n_out || !first_sample || !ho || !first_frame) return fail(h, CSS_ERR_INVALID_ARG, "null argument");
    CssStreamPreviewHandoff it{CssStreamPreview{id, out_host, cap, 0, 0, CSS_OK}, ho, first_frame};
    const int rc = css_stream_preview_handoff_many(h, &it, 1, nullptr);
    if (rc != CSS_OK) return rc;
    if (it.p.status != CSS_OK) return fail(h, it.p.status, "zero weights found. check hop_size, segment_size or m0, m1");
    *n_out = it.p.n_out; *first_sample = it.p.first_sample;
    return CSS_OK;
}

// a group of one item
int css_stream_preview(css_handle_t h, int32_t id, float* out_host, int64_t cap, int64_t* n_out, int64_t* first_sample) {
    if (!h) return CSS_ERR_INVALID_ARG;
    if (!n_out || !first_sample) return fail(h, CSS_ERR_INVALID_ARG, "null argument");
    CssStreamPreview p{id, out_host, cap, 0, 0, CSS_OK};
    const int rc = css_stream_preview_many(h, &p, 1, nullptr);
    if (rc != CSS_OK) return rc;
    if (p.status != CSS_OK) return fail(h, p.status, "zero weights found. check hop_size, segment_size or m0, m1");
    *n_out = p.n_out; *first_sample = p.first_sample;
    return CSS_OK;
}

int css_stream_close(css_handle_t h, int32_t id) {
    if (!h) return CSS_ERR_INVALID_ARG;
    StreamState* s = get_stream(h, id);
    if (!s) return fail(h, CSS_ERR_INVALID_ARG, "no open stream with this id");
    hipSetDevice(h->device);
    hipStreamSynchronize(h->stream);
    delete s;
    h->streams[id] = nullptr;
    return CSS_OK;
}

int css_stream_info(css_handle_t h, int32_t id, CssStreamInfo* out) {
    if (!h) return CSS_ERR_INVALID_ARG;
    StreamState* s = get_stream(h, id);
    if (!s || !out) return fail(h, CSS_ERR_INVALID_ARG, "no open stream with this id / null argument");
    out->n_pushed = s->n_pushed;
    out->n_emitted = s->n_emitted;
    out->max_lag = (int64_t)(s->T + s->halo + 2) * h->d.frame_hop + h->d.frame_len;
    out->device_bytes = device_bytes(s);
    out->finished = s->finished ? 1 : 0;
    return CSS_OK;
}

// ---- the rate ratio of a stream (include/css_mi355_rate.h) -----------------------------------------------------------------------
int css_stream_set_rate(css_handle_t h, int32_t id, int32_t up, int32_t down) {
    StreamState* s = nullptr;
    int rc = check_stream_call(h, id, &s);
    if (rc != CSS_OK) return rc;
    ResampleRatio r;
    if (!resample_ratio(up, down, &r) || !resample_fits(r, s->n_ch))
        return fail(h, CSS_ERR_INVALID_ARG, "rate ratio: up != down in lowest terms, at most 128 taps per output sample and 16384 taps");
    if (s->rate) return fail(h, CSS_ERR_STATE, "this stream has a rate ratio already");
    if (s->n_pushed > 0 || s->finished) return fail(h, CSS_ERR_STATE, "the rate ratio is set before the stream's first sample");
    HIPCHK(h, hipSetDevice(h->device));
    std::unique_ptr<RateStream> q(new RateStream());
    q->r = r;
    q->H = (2 * r.half + r.up - 1) / r.up + 1;
    q->max_in = (s->piece * r.down + r.half) / r.up + 1;
    std::vector<float> taps((size_t)r.L), tab((size_t)r.up * r.P_ld);
    resample_taps_f32(r, taps.data());
    resample_phase_table(r, taps.data(), tab.data());
    rc = ensure(h, q->stage, (size_t)s->n_ch * q->max_in * sizeof(float));
    for (int b = 0; b < 2 && rc == CSS_OK; ++b) rc = ensure(h, q->hist[b], (size_t)s->n_ch * q->H * sizeof(float), true);
    if (rc == CSS_OK) rc = ensure(h, q->tab, tab.size() * sizeof(float));
    hipError_t e = hipSuccess;
    if (rc == CSS_OK) {
        e = hipMemcpyAsync(q->tab.p, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    }
    if (rc != CSS_OK) return rc;
    if (e != hipSuccess) return fail(h, CSS_ERR_HIP, std::string("rate setup: ") + hipGetErrorString(e));
    s->rate = std::move(q);
    return CSS_OK;
}

// ---- the output format of a stream (include/css_mi355_stream_out.h) --------------------------------------------------------------
int css_stream_set_output(css_handle_t h, int32_t id, const CssStreamOutputCfg* cfg) {
    StreamState* s = nullptr;
    int rc = check_stream_call(h, id, &s);
    if (rc != CSS_OK) return rc;
    if (!cfg) return fail(h, CSS_ERR_INVALID_ARG, "null argument");
    static_assert(STREAM_MULTI_MAX == CSS_STREAM_OUTPUT_TABLE, "the header states the table's size");
    const bool unity = cfg->up == 1 && cfg->down == 1;
    ResampleRatio r{1, 1, 0, 0, 0, 0};
    if (!unity && (!resample_ratio(cfg->up, cfg->down, &r) || !stream_output_fits(r)))
        return fail(h, CSS_ERR_INVALID_ARG, "output ratio: 1 / 1, or up != down in lowest terms, at most 128 taps per output sample and 16384 taps");
    if (!std::isfinite(cfg->gain) || !(cfg->gain > 0.f)) return fail(h, CSS_ERR_INVALID_ARG, "the gain is finite and > 0");
    if (s->outp) return fail(h, CSS_ERR_STATE, "this stream has an output format already");
    if (s->n_pushed > 0 || s->finished || (s->rate && s->rate->n_in > 0))
        return fail(h, CSS_ERR_STATE, "the output format is set before the stream's first sample");
    HIPCHK(h, hipSetDevice(h->device));
    const int S = h->d.num_spks;
    std::unique_ptr<OutputStream> o(new OutputStream());
    o->cfg = *cfg;
    o->cfg.pcm16 = cfg->pcm16 ? 1 : 0;
    o->unity = unity;
    o->r = r;
    // a round of a push makes at most as many samples final as the stream's output buffer holds per separated stream
    o->stage_ld = output_stage_ld(o.get(), (int64_t)(s->out.cap / (sizeof(float) * S)));
    rc = ensure(h, o->stage, (size_t)S * o->stage_ld * output_el(o.get()));
    if (rc == CSS_OK) rc = ensure(h, o->ctr, sizeof(OutputCounters), true);
    hipError_t e = o->pin.alloc(sizeof(OutputCounters));
    if (rc == CSS_OK && e == hipSuccess && !unity) {
        o->H = (2 * r.half + r.up - 1) / r.up + 1;
        std::vector<float> taps((size_t)r.L), tab((size_t)r.up * r.P_ld);
        resample_taps_f32(r, taps.data());
        resample_phase_table(r, taps.data(), tab.data());
        for (int b = 0; b < 2 && rc == CSS_OK; ++b) rc = ensure(h, o->hist[b], (size_t)S * o->H * sizeof(float), true);
        if (rc == CSS_OK) rc = ensure(h, o->tab, tab.size() * sizeof(float));
        if (rc == CSS_OK) e = hipMemcpyAsync(o->tab.p, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice, h->stream);
    }
    const hipError_t es = hipStreamSynchronize(h->stream);   // (the zero fills, and `tab` above leaves scope)
    if (rc != CSS_OK) return rc;
    if (e != hipSuccess || es != hipSuccess) return fail(h, CSS_ERR_HIP, std::string("output setup: ") + hipGetErrorString(e != hipSuccess ? e : es));
    s->outp = std::move(o);
    return CSS_OK;
}

int css_stream_output_bind(css_handle_t h, int32_t id, void* out_host, int64_t cap, CssStreamOutputCounts* counts) {
    if (!h) return CSS_ERR_INVALID_ARG;
    StreamState* s = get_stream(h, id);
    if (!s) return fail(h, CSS_ERR_INVALID_ARG, "no open stream with this id");
    if (!s->outp) return fail(h, CSS_ERR_STATE, "this stream has no output format (css_stream_set_output)");
    if (out_host && (cap < 0 || !counts || !counts->n_clipped || !counts->peak_bits))
        return fail(h, CSS_ERR_INVALID_ARG, "a buffer without counts, or counts without their arrays");
    s->outp->bound = out_host;
    s->outp->cap = out_host ? cap : 0;
    s->outp->counts = out_host ? counts : nullptr;
    return CSS_OK;
}

int css_stream_output_peaks(css_handle_t h, int32_t id, uint32_t* peak_bits) {
    if (!h) return CSS_ERR_INVALID_ARG;
    StreamState* s = get_stream(h, id);
    if (!s || !peak_bits) return fail(h, CSS_ERR_INVALID_ARG, "no open stream with this id / null argument");
    for (int k = 0; k < h->d.num_spks; ++k) peak_bits[k] = s->peak_bits[k];
    return CSS_OK;
}

int css_stream_output_stats(css_handle_t h, int32_t* launches, int32_t* rounds) {
    if (!h) return CSS_ERR_INVALID_ARG;
    if (launches) *launches = h->stream_out_launches;
    if (rounds) *rounds = h->stream_out_rounds;
    return CSS_OK;
}

// ---- hand-off entry points ------------------------------------------------------------------------------------------------
int css_stream_handoff_bounds(const CssModelDesc* desc, const CssRunCfg* cfg, const CssStreamHandoffCfg* hcfg, int64_t n_samples,
                              int64_t* frames, int32_t* ranges, int64_t* activity) {
    if (!desc || !frames || !ranges || !activity || n_samples < -1) return CSS_ERR_INVALID_ARG;
    int rc = check_cfg(*desc, cfg);
    if (rc == CSS_OK) rc = check_handoff_cfg(hcfg);
    if (rc != CSS_OK) return rc;
    const HandoffNeed n = handoff_need(cfg->segment_frames, cfg->hop_frames, cfg->dilation_frames + cfg->erosion_frames, *hcfg, n_samples);
    *frames = n.frames; *ranges = n.ranges; *activity = n.activity;
    return CSS_OK;
}

int css_stream_handoff_final_frames(const CssModelDesc* desc, const CssRunCfg* cfg, const CssStreamHandoffCfg* hcfg, int64_t n_pushed,
                                    int64_t* n_frames) {
    if (!desc || !n_frames || n_pushed < 0) return CSS_ERR_INVALID_ARG;
    int rc = check_cfg(*desc, cfg);
    if (rc == CSS_OK) rc = check_handoff_cfg(hcfg);
    if (rc != CSS_OK) return rc;
    if (hcfg->drop_silence) return CSS_ERR_INVALID_ARG;   // with the gate in play the count depends on the audio
    const int64_t fin = final_frames(n_pushed, cfg->segment_frames, cfg->hop_frames, cfg->dilation_frames + cfg->erosion_frames) * desc->frame_hop;
    *n_frames = fin >= 201 ? (fin - 200) / 160 + 1 : 0;
    return CSS_OK;
}

int css_stream_handoff_open(css_handle_t h, int32_t id, const CssStreamHandoffCfg* cfg) {
    StreamState* s = nullptr;
    int rc = check_stream_call(h, id, &s);
    if (rc != CSS_OK) return rc;
    if (check_handoff_cfg(cfg) != CSS_OK) return fail(h, CSS_ERR_INVALID_ARG, "n_mels is 80 or 128, pad_frames 0 .. 4096");
    if (s->ho) return fail(h, CSS_ERR_STATE, "the hand-off of this stream is on already");
    if (s->n_pushed > 0 || s->finished) return fail(h, CSS_ERR_STATE, "the hand-off is switched on before the stream's first sample");
    HIPCHK(h, hipSetDevice(h->device));
    const int S = h->d.num_spks;
    HandoffCtx* c = handoff_ctx(h);
    if (!c) {
        c = new HandoffCtx();
        h->handoff = c;
    }
    if (!c->tab.p || !c->state.p || !c->state_pv.p) {
        std::vector<float> t(HO_DFT_F + HO_MEL80_F + HO_MEL128_F, 0.f);
        handoff_build_dft(t.data());
        handoff_build_mel(t.data() + HO_DFT_F, 80);
        handoff_build_mel(t.data() + HO_DFT_F + HO_MEL80_F, 128);
        if ((rc = ensure(h, c->state, (size_t)CSS_MAX_STREAMS * SMAX * sizeof(HandoffState), true)) != CSS_OK) return rc;
        if ((rc = ensure(h, c->state_pv, (size_t)CSS_MAX_STREAMS * SMAX * sizeof(HandoffState), true)) != CSS_OK) return rc;
        if ((rc = ensure(h, c->tab, t.size() * sizeof(float))) != CSS_OK) return rc;
        HIPCHK(h, hipMemcpy(c->tab.p, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    std::unique_ptr<HandoffStream> o(new HandoffStream());
    o->cfg = *cfg;
    o->cfg.drop_silence = cfg->drop_silence ? 1 : 0;
    o->pad = o->cfg.drop_silence ? cfg->pad_frames : 0;
    // the ring holds a round's frames (at most the window) and the 2 pad + 2 frames before them that can keep its blocks
    int64_t ring = 64;
    while (ring < s->WF + 2 * (int64_t)o->pad + 8) ring *= 2;
    o->gate_ld = ring; o->gate_mask = ring - 1;
    o->carry_ld = std::max<int64_t>((int64_t)o->pad * h->d.frame_hop, 1);
    rc = ensure(h, o->gate, (size_t)S * ring, true);
    for (int b = 0; b < 2 && rc == CSS_OK; ++b) {
        rc = ensure(h, o->carry[b], (size_t)S * o->carry_ld * sizeof(float), true);
        if (rc == CSS_OK) rc = ensure(h, o->tail[b], (size_t)S * HANDOFF_TAIL_LD * sizeof(float), true);
    }
    std::vector<HandoffState> init((size_t)SMAX, HandoffState{0, 0, HANDOFF_GMAX_NONE, 0});
    hipError_t e = hipSuccess;
    if (rc == CSS_OK) {
        e = hipMemcpyAsync((HandoffState*)c->state.p + (size_t)id * SMAX, init.data(), init.size() * sizeof(HandoffState), hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    }
    if (rc != CSS_OK) return rc;
    if (e != hipSuccess) return fail(h, CSS_ERR_HIP, std::string("hand-off setup: ") + hipGetErrorString(e));
    o->m.hist.assign((size_t)S, std::vector<uint8_t>());
    o->m.A.assign((size_t)S, 0); o->m.J.assign((size_t)S, 0);
    o->m.raw_max.assign((size_t)S, -INFINITY);
    s->ho = std::move(o);
    return CSS_OK;
}

int css_stream_handoff_bind(css_handle_t h, int32_t id, CssStreamHandoffOut* out) {
    if (!h) return CSS_ERR_INVALID_ARG;
    StreamState* s = get_stream(h, id);
    if (!s) return fail(h, CSS_ERR_INVALID_ARG, "no open stream with this id");
    if (!s->ho) return fail(h, CSS_ERR_STATE, "the hand-off of this stream is off (css_stream_handoff_open)");
    s->ho->bound = out;
    return CSS_OK;
}

int css_stream_handoff_stats(css_handle_t h, int32_t* launches, int32_t* products, int64_t* frames) {
    if (!h) return CSS_ERR_INVALID_ARG;
    const HandoffCtx* c = handoff_ctx(h);
    if (launches) *launches = c ? c->launches : 0;
    if (products) *products = c ? c->products : 0;
    if (frames) *frames = c ? c->frames : 0;
    return CSS_OK;
}

// ---- encoder windows out of the frame history (include/css_mi355_window.h) -------------------------------------------------------
int css_stream_window_open(css_handle_t h, int32_t id, int32_t history_frames) {
    StreamState* s = nullptr;
    int rc = check_stream_call(h, id, &s);
    if (rc != CSS_OK) return rc;
    if (history_frames < 32 || history_frames > (1 << 20)) return fail(h, CSS_ERR_INVALID_ARG, "history_frames is 32 .. 2^20");
    if (!s->ho) return fail(h, CSS_ERR_STATE, "the hand-off of this stream is off (css_stream_handoff_open)");
    if (s->ho->hist_frames) return fail(h, CSS_ERR_STATE, "this stream has a frame history already");
    if (s->n_pushed > 0 || s->finished || (s->rate && s->rate->n_in > 0))
        return fail(h, CSS_ERR_STATE, "the frame history is switched on before the stream's first sample");
    HIPCHK(h, hipSetDevice(h->device));
    HandoffStream* o = s->ho.get();
    const size_t S = (size_t)h->d.num_spks, H = (size_t)history_frames;
    DevBuf ring, fmax;
    if ((rc = ensure(h, ring, S * o->cfg.n_mels * H * sizeof(float), true)) != CSS_OK) return rc;
    if ((rc = ensure(h, fmax, S * H * sizeof(float), true)) != CSS_OK) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    o->ring = std::move(ring); o->fmax = std::move(fmax);
    o->hist_frames = history_frames;
    return CSS_OK;
}

int css_stream_window_range(css_handle_t h, int32_t id, int64_t* first_frame, int64_t* end_frame) {
    if (!h) return CSS_ERR_INVALID_ARG;
    StreamState* s = get_stream(h, id);
    if (!s || !first_frame || !end_frame) return fail(h, CSS_ERR_INVALID_ARG, "no open stream with this id / null argument");
    if (!s->ho || !s->ho->hist_frames) return fail(h, CSS_ERR_STATE, "this stream has no frame history (css_stream_window_open)");
    for (int k = 0; k < h->d.num_spks; ++k) {
        const int64_t J = s->ho->m.J[(size_t)k];
        first_frame[k] = std::max<int64_t>(J - s->ho->hist_frames, 0);
        end_frame[k] = J;
    }
    return CSS_OK;
}

int css_stream_windows(css_handle_t h, CssStreamWindow* items, int32_t n_items, int32_t* launches) {
    if (!h) return CSS_ERR_INVALID_ARG;
    if (n_items < 0 || (n_items > 0 && !items)) return fail(h, CSS_ERR_INVALID_ARG, "bad argument");
    if (h->queued || !h->pending.empty())
        return fail(h, CSS_ERR_STATE, "queued sessions (css_run_enqueue*) are outstanding: css_wait before using a stream");
    std::vector<WindowItem> w((size_t)n_items);
    for (int32_t i = 0; i < n_items; ++i) {
        const CssStreamWindow& p = items[i];
        auto refuse = [&](const std::string& msg) {
            return fail(h, CSS_ERR_INVALID_ARG, "item " + std::to_string(i) + " (stream " + std::to_string(p.id) + "): " + msg);
        };
        const StreamState* s = get_stream(h, p.id);
        if (!s) return refuse("no open stream with this id");
        const HandoffStream* o = s->ho.get();
        if (!o || !o->hist_frames) return refuse("the stream has no frame history (css_stream_window_open)");
        if (const char* bad = window_refusal(h, o, p, &p.first_frame)) return refuse(bad);
        w[(size_t)i] = history_item(o, p);
        w[(size_t)i].J = p.first_frame + p.n_frames;   // (no provisional frames: the span the kernel resolves is the request's)
    }
    if (launches) *launches = 0;
    if (n_items == 0) return CSS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    int32_t n_launch = 0;
    const WindowOut* res = nullptr;
    const int rc = launch_windows(h, w, &n_launch, &res);
    if (rc != CSS_OK) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int32_t i = 0; i < n_items; ++i) items[i].window_max = res[i].window_max;
    if (launches) *launches = n_launch;
    return CSS_OK;
}

int css_handoff_kept_ranges(const uint8_t* act, int64_t first_frame, int64_t n_known, int32_t pad_frames, int64_t a, int64_t b,
                            int64_t n_out, int64_t* ranges, int32_t n_ranges_in, int32_t cap_ranges, int32_t* n_ranges) {
    if (!ranges || !n_ranges || pad_frames < 0 || first_frame < 0 || n_known < first_frame || a < 0 || b < a || n_out < 0 ||
        n_ranges_in < 0 || n_ranges_in > cap_ranges || (n_known > first_frame && !act))
        return CSS_ERR_INVALID_ARG;
    if (a / 256 - pad_frames - 2 < first_frame && first_frame > 0) return CSS_ERR_INVALID_ARG;   // a frame that can keep a sample of [a, b) is missing
    std::vector<int64_t> reg(ranges, ranges + 2 * (size_t)n_ranges_in);
    handoff_kept_ranges(act, first_frame, n_known, pad_frames, 256, 512, a, b, n_out, reg);
    *n_ranges = (int32_t)(reg.size() / 2);
    if ((int64_t)(reg.size() / 2) > cap_ranges) return CSS_ERR_INVALID_ARG;
    std::memcpy(ranges, reg.data(), reg.size() * sizeof(int64_t));
    return CSS_OK;
}
