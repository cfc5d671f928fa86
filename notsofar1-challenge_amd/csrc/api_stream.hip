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
// include/css_mi355_preview.h, css_mi355_preview_handoff.h) run the same round body (stream_round) in closing_pass: finish with
// one job, a preview with N and no commit.  A stream's optional parts are api_stream_handoff.hip's (hand-off, frame history,
// encoder windows) and api_stream_io.hip's (rate ratio, output format); api_stream.hpp holds what the three files share.
#include "api_stream.hpp"

namespace {

constexpr int PIECE_SEGMENTS = 8;

// every device buffer of a stream, its hand-off and its rate conversion (css_stream_info: what the stream holds on the device)
template <class Fn>
void for_each_buffer(const StreamState* s, Fn fn) {
    for (int b = 0; b < 2; ++b)
        for (const DevBuf* d : {&s->pcm[b], &s->X[b], &s->masks[b], &s->sep[b], &s->perms[b], &s->act_b[b], &s->G[b]}) fn(*d);
    for (const DevBuf* d : {&s->scm, &s->bfw, &s->pnorm, &s->costs, &s->pit_part, &s->Y, &s->out, &s->segw, &s->pcm16_stage}) fn(*d);
    if (s->ho)
        for (const DevBuf* d : {&s->ho->gate, &s->ho->carry[0], &s->ho->carry[1], &s->ho->tail[0], &s->ho->tail[1], &s->ho->ring, &s->ho->fmax,
                                &s->ho->xlast[0], &s->ho->xlast[1]}) fn(*d);
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

// One stream's frames [t_g, t_hi) of the recording: activity bits of [t_st, a_hi), gate + overlap-add + synthesis of [t_g, t_hi),
// output blocks [t_g, q_hi) into the stream's output buffer (block t_g at column 0)
// (RoundJob::handoff: whether a hand-off stream's gate ring receives the gate bytes; a preview's closing pass leaves it alone)
int tail(css_ctx* h, const std::vector<RoundJob>& jobs) {
    std::vector<StreamStitchArgs> a(jobs.size());
    std::vector<StreamFrames> ra(jobs.size()), rg(jobs.size());
    for (size_t i = 0; i < jobs.size(); ++i) {
        const RoundJob& j = jobs[i];
        const int64_t fb = j.s->seg_base * j.s->hop;
        a[i] = stitch_view(h, j.s, j.closing, j.nseg, j.TL);
        if (!j.handoff) { a[i].gate_out = nullptr; a[i].gate_ld = 0; a[i].gate_mask = 0; }
        ra[i] = StreamFrames{j.s->t_st - fb, j.a_hi - fb};
        rg[i] = StreamFrames{j.s->t_g - fb, j.t_hi - fb};
    }
    launch_stream_activity_multi(a.data(), ra.data(), (int)jobs.size(), h->stream);
    launch_stream_gate_ola_multi(a.data(), rg.data(), (int)jobs.size(), h->stream);
    const int S = h->d.num_spks, N = h->d.frame_len;
    for (const RoundJob& j : jobs) {
        StreamState* s = j.s;
        const int64_t fb = s->seg_base * s->hop, t_lo = s->t_g, t_hi = j.t_hi;
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

// The window holds frames below K1 and samples below N1 of the recording -- and, for a closing pass, frames below TL and segments
// below nseg (a push passes 0 for both: it has no such bound) -- after a rebase if it takes one.
int fit_window(css_ctx* h, StreamState* s, int64_t K1, int64_t N1, int64_t TL, int64_t nseg) {
    auto past_window = [&]() {
        const int64_t fb = s->seg_base * s->hop;
        return K1 - fb > s->WF || N1 - fb * h->d.frame_hop > s->WS || TL - fb > s->WF || nseg - s->seg_base > s->SC;
    };
    if (!past_window()) return CSS_OK;
    const int rc = rebase(h, s);
    if (rc != CSS_OK) return rc;
    return past_window() ? fail(h, CSS_ERR_STATE, "stream window overflow") : CSS_OK;
}

// The round body: what a round of a push and a closing pass (css_stream_finish: commit; a preview: none) both run between "the
// samples are in the window" and "the downloads are queued", for all streams of the round at once: the analysis transform of the
// frames that became computable (a closing round: and the zero fill behind them), segments(), tail(), the hand-off round, the
// windows up to the present where a preview asks for them, the output format's launch and download (with a commit only) and the
// model-rate download.
int stream_round(css_ctx* h, std::vector<RoundJob>& jobs, size_t round, bool commit, CssStreamGroupStats* stats,
                 std::vector<HandoffRec>* recs, PresentCall* pc) {
    const int hopS = h->d.frame_hop, F = h->d.num_bins, S = h->d.num_spks;
    int rc;
    std::vector<SegJob> sj;
    for (const RoundJob& j : jobs) {
        StreamState* s = j.s;
        const int c = s->cur;
        const int64_t fb = s->seg_base * s->hop, k1 = j.K1 - fb;
        bool ph = false;
        if (j.K1 > s->K &&
            !analysis_transform(h, (const float*)s->pcm[c].p, s->WS, s->n_ch, s->K - fb, k1, (float*)s->X[c].p, s->WF, h->stream,
                                (float*)s->X[c].p + (int64_t)s->n_ch * 2 * F * s->WF, &ph))
            return fail(h, CSS_ERR_HIP, "the analysis transform's LDS could not be reserved");
        if (j.z_hi > k1)
            HIPCHK(h, hipMemset2DAsync((float*)s->X[c].p + k1, (size_t)s->WF * sizeof(float), 0, (size_t)(j.z_hi - k1) * sizeof(float),
                                       (size_t)s->n_ch * X_ROWS_PER_BIN * F, h->stream));
        if (!j.closing) s->K = j.K1;
        sj.push_back(SegJob{s, s->sd, j.nseg, k1});
        const int64_t out_ld = (j.q_hi - s->t_g) * hopS;   // what tail() leaves in s->out per separated stream (finish: past a round's)
        if (out_ld > (int64_t)(s->out.cap / (sizeof(float) * S)) && (rc = ensure(h, s->out, (size_t)S * out_ld * sizeof(float))) != CSS_OK)
            return rc;
    }
    if ((rc = segments(h, sj, stats)) != CSS_OK) return rc;
    for (const RoundJob& j : jobs)
        if (!j.closing) j.s->sd = j.nseg;
    if ((rc = tail(h, jobs)) != CSS_OK) return rc;
    if ((rc = handoff_round(h, jobs, round, recs, commit)) != CSS_OK) return rc;
    if (pc && pc->total && (rc = present_windows(h, jobs, *recs, pc)) != CSS_OK) return rc;
    // the streams with an output format whose tail() made samples final: one launch for all of them (finish: the rest of their
    // samples, and the outputs that waited for inputs past the end)
    std::vector<StreamOutputJob> oj;
    for (RoundJob& j : jobs) {
        if (!commit || !j.s->outp || j.n_new <= 0) continue;
        oj.emplace_back();
        if ((rc = output_job(h, j.s, j.done, j.n_new, (j.q_hi - j.s->t_g) * hopS, j.closing, &oj.back(), &j.n_m)) != CSS_OK) return rc;
    }
    if (!oj.empty()) {
        if (!launch_stream_output_multi(oj.data(), (int)oj.size(), S, h->stream, &h->stream_out_launches))
            return fail(h, CSS_ERR_HIP, "the output kernel's LDS could not be reserved");
        h->stream_out_rounds += 1;
        HIPCHK(h, hipGetLastError());
    }
    for (const RoundJob& j : jobs) {
        if (j.n_m > 0 && (rc = output_download(h, j.s, j.n_m, j.written)) != CSS_OK) return rc;
        if (j.out_host && (rc = download(h, j.s, j.n_new, j.out_host, j.cap, j.done)) != CSS_OK) return rc;
    }
    return CSS_OK;
}

// After the call's synchronise, for a stream the call made `emitted` more samples final of (`written` at its output format's
// rate): the output format's report (a call that moved nothing still reports) or the host's peak scan of the samples in
// out_host[S][cap], then the rounds' hand-off into what is bound to the stream.
int commit_report(css_ctx* h, StreamState* s, int item, int64_t t_g_before, const std::vector<HandoffRec>& recs, const float* out_host,
                  int64_t cap, int64_t emitted, int64_t written) {
    if (s->outp && emitted > 0) output_report(h, s, written);
    else if (s->outp) output_report_idle(h, s);
    else if (emitted > 0) host_peak(h, s, out_host, cap, emitted);
    return s->ho ? handoff_collect(h, s, item, t_g_before, recs, s->ho->m, s->ho->bound, true) : CSS_OK;
}

}  // namespace

int check_stream_cfg(const CssModelDesc& d, const CssRunCfg* cfg) {
    if (!cfg || !cfg->w_first || !cfg->w_mid || !cfg->w_last) return CSS_ERR_INVALID_ARG;
    if (d.frame_len != 512 || d.frame_hop != 256) return CSS_ERR_INVALID_ARG;
    if (cfg->segment_frames < 2 || cfg->segment_frames > CSS_MAX_SEGMENT_FRAMES || cfg->hop_frames < 1 ||
        cfg->hop_frames >= cfg->segment_frames || cfg->dilation_frames < 0 || cfg->erosion_frames < 0)
        return CSS_ERR_INVALID_ARG;
    return CSS_OK;
}

// the one test that no queued session is outstanding, and its words
const char* queued_refusal(const css_ctx* h) {
    return h->queued || !h->pending.empty() ? "queued sessions (css_run_enqueue*) are outstanding: css_wait before using a stream" : nullptr;
}

int check_stream_call(css_ctx* h, int32_t id, StreamState** out) {
    if (!h) return CSS_ERR_INVALID_ARG;
    StreamState* s = get_stream(h, id);
    if (!s) return fail(h, CSS_ERR_INVALID_ARG, "no open stream with this id");
    if (const char* q = queued_refusal(h)) return fail(h, CSS_ERR_STATE, q);
    *out = s;
    return CSS_OK;
}

// the refusal of item i of a grouped call, which names stream `id`
int refuse_item(css_ctx* h, int code, size_t i, int32_t id, const std::string& msg) {
    return fail(h, code, "item " + std::to_string(i) + " (stream " + std::to_string(id) + "): " + msg);
}

// What opens every item of a grouped push or preview, item i of a call whose item k names stream id_of(k): the stream is open,
// no queued session is outstanding, no earlier item names it, it has not finished.  -> CSS_OK and *out, or the item's refusal.
template <typename IdOf>
static int check_group_item(css_ctx* h, size_t i, IdOf id_of, StreamState** out) {
    StreamState* s = get_stream(h, id_of(i));
    if (!s) return refuse_item(h, CSS_ERR_INVALID_ARG, i, id_of(i), "no open stream with this id");
    if (const char* q = queued_refusal(h)) return refuse_item(h, CSS_ERR_STATE, i, id_of(i), q);
    for (size_t k = 0; k < i; ++k)
        if (id_of(k) == id_of(i)) return refuse_item(h, CSS_ERR_INVALID_ARG, i, id_of(i), "the stream is named twice in one call");
    if (s->finished) return refuse_item(h, CSS_ERR_STATE, i, id_of(i), "the stream has finished");
    *out = s;
    return CSS_OK;
}

void stream_destroy_all(css_ctx* h) {
    for (int i = 0; i < CSS_MAX_STREAMS; ++i)
        if (h->streams[i]) { delete h->streams[i]; h->streams[i] = nullptr; }
    h->stream_masks.reset();
    delete h->handoff;
    h->handoff = nullptr;
}
int stream_open_count(const css_ctx* h) {
    int n = 0;
    for (int i = 0; i < CSS_MAX_STREAMS; ++i) n += h->streams[i] != nullptr;
    return n;
}

int css_stream_final_samples(const CssModelDesc* desc, const CssRunCfg* cfg, int64_t n_pushed, int64_t* n_final) {
    if (!desc || !n_final || n_pushed < 0) return CSS_ERR_INVALID_ARG;
    const int rc = check_stream_cfg(*desc, cfg);
    if (rc != CSS_OK) return rc;
    *n_final = final_frames(n_pushed, cfg->segment_frames, cfg->hop_frames, cfg->dilation_frames + cfg->erosion_frames) * desc->frame_hop;
    return CSS_OK;
}

int css_stream_open(css_handle_t h, const CssRunCfg* cfg, int32_t n_ch, int32_t* stream_id) {
    if (!h) return CSS_ERR_INVALID_ARG;
    if (!cfg || !stream_id) return fail(h, CSS_ERR_INVALID_ARG, "null argument");
    if (const char* q = queued_refusal(h)) return fail(h, CSS_ERR_STATE, q);
    if (h->split) return fail(h, CSS_ERR_STATE, "streams run in CSS_LINEAR_EXACT_F32 only (the split-f16 mode takes whole-session decisions)");
    if (h->d.frame_len != 512 || h->d.frame_hop != 256 || !h->fft512)
        return fail(h, CSS_ERR_INVALID_ARG, "streams support frame_len 512 / frame_hop 256 only");
    // channels, windows, mask floor, segmentation (the weights are checked frame by frame as frames become final: push, finish)
    if (n_ch != h->d.num_mics)
        return fail(h, CSS_ERR_SHAPE, "input has " + std::to_string(n_ch) + " channels, the model expects " + std::to_string(h->d.num_mics));
    if (cfg->mask_floor > 1.0f || cfg->mask_floor < 0.f) return fail(h, CSS_ERR_MASK_FLOOR, "mask_floor_db must be <= 0");
    if (cfg->stitching_loss < 0 || cfg->stitching_loss > 1 || cfg->stitching_input < 0 || cfg->stitching_input > 1)
        return fail(h, CSS_ERR_INVALID_ARG, "unexpected stitching_loss / stitching_input");
    if (check_stream_cfg(h->d, cfg) != CSS_OK) return fail(h, CSS_ERR_INVALID_ARG, "segment weights missing / bad segmentation / gate");
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
    if (rc == CSS_OK) rc = alloc(s->scm, (size_t)s->SC * (S + 1) * F * s->n_ch * s->n_ch * sizeof(double));
    if (rc == CSS_OK) rc = alloc(s->bfw, (size_t)s->SC * S * F * s->n_ch * 2 * sizeof(double));
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
// The three ways a piece reaches its window are api_stream_io.hip's (stage_piece); what follows them is the round body above.
static int push_items(css_ctx* h, const std::vector<PushItem>& items, bool pcm16, CssStreamGroupStats* stats) {
    struct Item { StreamState* s; const PushItem* p; int64_t done, emitted, n, t_g_before; bool planar; int64_t n_in, written; };
    std::vector<Item> its(items.size());
    int rc;
    for (size_t i = 0; i < items.size(); ++i) {
        const PushItem& p = items[i];
        auto refuse = [&](int code, const std::string& msg) { return refuse_item(h, code, i, p.id, msg); };
        StreamState* s = nullptr;
        std::string why;
        if ((rc = check_group_item(h, i, [&](size_t k) { return items[k].id; }, &s)) != CSS_OK) return rc;
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
        if ((rc = check_handoff_call(s, n_after - s->n_pushed, &why)) != CSS_OK) return refuse(rc, why);
        if ((rc = check_output_call(s, std::max<int64_t>(need, 0), false, &why)) != CSS_OK) return refuse(rc, why);
        its[i] = Item{s, &p, 0, 0, 0, s->t_g, planar, 0, 0};
    }
    if (stats) *stats = CssStreamGroupStats{};
    h->stream_out_launches = h->stream_out_rounds = 0;
    handoff_begin_call(h);
    std::vector<HandoffRec> recs;
    auto report = [&]() {   // (a call that moved nothing still reports: its empty hand-off, the output format's idle counts)
        for (size_t i = 0; i < its.size(); ++i) {
            const Item& it = its[i];
            if ((rc = commit_report(h, it.s, (int)i, it.t_g_before, recs, it.p->out_host, it.p->cap, it.emitted, it.written)) != CSS_OK) return rc;
        }
        return (int)CSS_OK;
    };
    bool any = false;
    for (Item& it : its) { *it.p->n_out = 0; any = any || it.p->n_samples > 0; }
    if (!any) return report();
    HIPCHK(h, hipSetDevice(h->device));
    const int hopS = h->d.frame_hop;
    // a stream's first PCM16 push: device staging for one piece, [piece][C] interleaved or C planes of `piece` values
    if (pcm16)
        for (Item& it : its)
            if (it.p->n_samples > 0 && !it.s->rate &&
                (rc = ensure(h, it.s->pcm16_stage, (size_t)it.s->n_ch * it.s->piece * sizeof(int16_t))) != CSS_OK) return rc;
    std::vector<Item*> act;
    std::vector<RoundJob> rj;
    std::vector<StreamIngestPcm16> ing;
    std::vector<ResampleJob> rsj;
    for (size_t round = 0;; ++round) {
        act.clear();
        for (Item& it : its)
            if (it.done < it.p->n_samples) act.push_back(&it);
        if (act.empty()) break;
        ing.clear(); rsj.clear();
        bool host_staging = false;
        for (Item* it : act) {
            StreamState* s = it->s;
            // a rate stream's piece is cut in inputs so that the outputs it makes available are at most `piece` window samples:
            // avail(N) <= n_pushed + piece  <=>  N <= ((n_pushed + piece) down + half) / up
            if (RateStream* q = s->rate.get())
                it->n_in = std::min<int64_t>(it->p->n_samples - it->done, ((s->n_pushed + s->piece) * q->r.down + q->r.half) / q->r.up - q->n_in);
            else
                it->n_in = std::min<int64_t>(s->piece, it->p->n_samples - it->done);
            const int64_t n = it->n = model_samples_after(s, it->n_in) - s->n_pushed;
            if ((rc = fit_window(h, s, frames_of(s->n_pushed + n), s->n_pushed + n, 0, 0)) != CSS_OK) return rc;
            float* win = (float*)s->pcm[s->cur].p + (s->n_pushed - s->seg_base * s->hop * hopS);
            if ((rc = stage_piece(h, s, *it->p, pcm16, it->planar, it->done, it->n_in, n, win, &rsj, &ing, &host_staging)) != CSS_OK) return rc;
        }
        if (!rsj.empty() && !launch_stream_ingest_resample_multi(rsj.data(), (int)rsj.size(), h->stream))
            return fail(h, CSS_ERR_HIP, "the resampling kernel's LDS could not be reserved");
        if (pcm16) {
            launch_stream_ingest_pcm16_multi(ing.data(), (int)ing.size(), h->stream);
        } else if (host_staging) {
            // the host staging buffers are reused by the next round (a rate stream has none: its piece went from the caller's memory)
            HIPCHK(h, hipStreamSynchronize(h->stream));
        }
        // where the round takes each stream: the frames its samples complete, the segments those complete, the frames those make final
        rj.clear();
        for (Item* it : act) {
            StreamState* s = it->s;
            s->n_pushed += it->n;
            RoundJob j{s, (int)(it - its.data())};
            j.K1 = std::max(s->K, frames_of(s->n_pushed));
            j.nseg = segments_done(j.K1, s->T, s->hop);
            j.a_hi = j.nseg * s->hop;
            j.t_hi = j.q_hi = std::max<int64_t>(j.a_hi - s->halo, 0);
            j.n_new = (j.t_hi - s->t_g) * hopS;
            j.out_host = it->p->out_host; j.cap = it->p->cap; j.done = it->emitted; j.written = it->written;
            rj.push_back(j);
        }
        if ((rc = stream_round(h, rj, round, true, stats, &recs, nullptr)) != CSS_OK) return rc;
        for (size_t k = 0; k < act.size(); ++k) {
            Item* it = act[k];
            it->written += rj[k].n_m; it->emitted += rj[k].n_new; it->done += it->n_in;
            it->s->t_st = it->s->sd * it->s->hop;
            it->s->t_g = rj[k].t_hi;
        }
    }
    for (Item& it : its)
        if (it.s->outp && it.emitted > 0 && (rc = output_counters(h, it.s)) != CSS_OK) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (Item& it : its) { it.s->n_emitted += it.emitted; *it.p->n_out = it.emitted; }
    return report();
}

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

int closing_pass(css_ctx* h, const std::vector<CloseJob>& jobs, bool commit, CssStreamGroupStats* stats, PresentCall* pc = nullptr) {
    if (jobs.empty()) return CSS_OK;
    int rc;
    std::vector<HandoffRec> recs;
    bool any_ho = commit;
    for (const CloseJob& j : jobs) any_ho = any_ho || j.ho;
    if (any_ho) handoff_begin_call(h);
    HIPCHK(h, hipSetDevice(h->device));
    const int hopS = h->d.frame_hop, S = h->d.num_spks;
    std::vector<ResampleJob> rsj;
    std::vector<RoundJob> rj;
    for (size_t i = 0; i < jobs.size(); ++i) {
        const CloseJob& c = jobs[i];
        StreamState* s = c.s;
        RoundJob j{s, (int)i};
        j.K1 = std::max(s->K, frames_of(c.n_total));
        j.closing = true; j.nseg = c.p.num_segments; j.TL = j.a_hi = j.t_hi = c.p.mix_frames; j.n_out = c.p.n_out;
        if ((rc = fit_window(h, s, j.K1, c.n_total, j.TL, j.nseg)) != CSS_OK) return rc;
        // flush the resampler: the samples that waited for inputs, into the window (fewer than a frame's worth: half / down + 1)
        if (c.n_total > s->n_pushed)
            rsj.push_back(rate_job(s, false, false, 0, c.n_total, (float*)s->pcm[s->cur].p + (s->n_pushed - s->seg_base * s->hop * hopS), true));
        // frames past the last transformed one are zero: to the window's end, or to the end of the pending segment
        j.z_hi = commit ? s->WF : std::min<int64_t>(s->WF, (j.nseg - 1) * s->hop + s->T - s->seg_base * s->hop);
        // the rest of the output: blocks up to mix_frames (frame_len = 2 hop: block TL holds the last frame's second half)
        j.q_hi = j.TL + 1;
        j.n_new = c.need; j.out_host = c.out_host; j.cap = c.cap;
        j.handoff = commit || c.ho;
        j.windows = c.windows; j.n_windows = c.n_windows; j.win0 = c.win0;
        rj.push_back(j);
    }
    if (!rsj.empty() && !launch_stream_ingest_resample_multi(rsj.data(), (int)rsj.size(), h->stream))
        return fail(h, CSS_ERR_HIP, "the resampling kernel's LDS could not be reserved");
    if (commit) h->stream_out_launches = h->stream_out_rounds = 0;
    if ((rc = stream_round(h, rj, 0, commit, stats, &recs, pc)) != CSS_OK) return rc;
    for (const RoundJob& j : rj)
        if (commit && j.s->outp && j.n_new > 0 && (rc = output_counters(h, j.s)) != CSS_OK) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < jobs.size(); ++i) {
        StreamState* s = jobs[i].s;
        if (!commit && jobs[i].ho) {   // a preview with hand-off collects on a copy of the mirrors, into the caller's outputs
            HandoffMirror m = s->ho->m;
            for (int k = 0; k < S; ++k) jobs[i].first_frame[k] = m.J[(size_t)k];
            if ((rc = handoff_collect(h, s, (int)i, s->t_g, recs, m, jobs[i].ho, false)) != CSS_OK) return rc;
        }
        if (!commit) continue;
        if ((rc = commit_report(h, s, (int)i, s->t_g, recs, jobs[i].out_host, jobs[i].cap, jobs[i].need, rj[i].n_m)) != CSS_OK) return rc;
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
    if ((rc = check_handoff_call(s, -1, &why)) != CSS_OK) return fail(h, rc, why);
    if ((rc = check_output_call(s, j.need, true, &why)) != CSS_OK) return fail(h, rc, why);
    if ((rc = closing_pass(h, {j}, true, nullptr)) != CSS_OK) return rc;
    *n_out = j.need;
    return CSS_OK;
}

// ---- previews (include/css_mi355_preview.h) ------------------------------------------------------------------------------------
int css_stream_preview_samples(const CssModelDesc* desc, const CssRunCfg* cfg, int64_t n_pushed, int64_t* first, int64_t* count) {
    if (!desc || !first || !count || n_pushed < 0) return CSS_ERR_INVALID_ARG;
    const int rc = check_stream_cfg(*desc, cfg);
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
        auto refuse = [&](int code, const std::string& msg) { return refuse_item(h, code, (size_t)i, p.id, msg); };
        StreamState* s = nullptr;
        std::string why;
        const int irc = check_group_item(h, (size_t)i, [&](size_t k) { return items[k].p->id; }, &s);
        if (irc != CSS_OK) return irc;
        if (h->split) return refuse(CSS_ERR_STATE, "streams run in CSS_LINEAR_EXACT_F32 only");
        CloseJob j{s, CssPlan{}, closing_samples(s), p.out_host, p.cap, 0};
        if (CssStreamHandoffOut* ho = items[(size_t)i].ho) {
            if (!s->ho) return refuse(CSS_ERR_STATE, "the hand-off of this stream is off (css_stream_handoff_open)");
            if (s->ho->nemo) return refuse(CSS_ERR_STATE, "a preview with hand-off of a NeMo stream is not supported (css_stream_preview works)");
            if (!items[(size_t)i].first_frame) return refuse(CSS_ERR_INVALID_ARG, "hand-off outputs without first_frame");
            const int hrc = check_handoff_out(s, ho, -1, &why);   // a preview is a finish at this moment
            if (hrc != CSS_OK) return refuse(hrc, why);
            j.ho = ho; j.first_frame = items[(size_t)i].first_frame;
        }
        if (items[(size_t)i].present) {
            const PreviewItem& it = items[(size_t)i];
            if (s->ho && s->ho->nemo) return refuse(CSS_ERR_STATE, "windows up to the present of a NeMo stream are not supported");
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

