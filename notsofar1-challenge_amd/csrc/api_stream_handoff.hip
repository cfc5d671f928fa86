// The hand-off (css_stream_handoff_*): a stream that has it switched on also returns, with every call, the gate
// bits, the kept sample ranges and the raw Whisper log-mel frames that became final.  The step sits between tail() and the
// downloads of a round: three launches for all streams of the round (handoff.hip: append, ONE DFT product, mel), results
// into page-locked staging under the call's final synchronise, where the host trims them into the caller's buffers.
// The NeMo format (css_stream_nemo_*; include/css_mi355_stream_nemo.h) is the same step with nemo_stream.hip's kernels and the
// offline NeMo path's tables: raw ln(mel + 2^-24) frames instead, no running maximum, no previews with hand-off.  Its frame history
// and the chunks out of it are api_nemo_chunk.hip's (include/css_mi355_nemo_chunk.h); the mel launch below fills that ring too.
// A hand-off stream with a frame history (css_stream_window_open, include/css_mi355_window.h) also keeps its last raw
// log-mel frames in a ring on the device: the mel launch of a committed round leaves them there.  css_stream_windows turns spans
// of them into Whisper encoder inputs in the caller's device memory, css_stream_present_windows spans that end in a preview's
// provisional frames: one kernel (handoff.hip stream_window_kernel), one table launch per WINDOW_MULTI_MAX windows (launch_windows).
#include "api_stream.hpp"

constexpr size_t HO_DFT_F = (size_t)402 * 416, HO_MEL80_F = (size_t)80 * 201, HO_MEL128_F = (size_t)128 * 201;

// ---- hand-off ----------------------------------------------------------------------------------------------------------
// Capacities that suffice for one call.  A push of n samples adds at most n / 256 + 1 frames to the transform, hence at most
// that plus hop_frames to the segments' frames, the gated-final frames and the decided blocks; finish decides what is left:
// fewer than T + halo + pad + 2 blocks (t_g >= K - T - halo, n_out = (max(K, T) + 1) blocks).  J frames need 160 J + 40
// samples, so a call that appends dn samples completes at most dn / 160 + 1 frames -- (dn + 200) / 160 + 1 at finish, which
// also emits the frames the trailing reflection completes.  Two ranges of a call have a dropped block between them.
// The NeMo format (include/css_mi355_stream_nemo.h) differs in `lead`, the samples of the next hop a frame waits for: Whisper's
// frame j reads concatenated samples below 160 j + 200 (+ 1: the reflection), NeMo's below 160 j + 256.
constexpr int64_t WHISPER_LEAD = 200, NEMO_LEAD = NEMO_NFFT / 2;
struct HandoffNeed { int64_t frames; int32_t ranges; int64_t activity; };
static HandoffNeed handoff_need(int T, int hop, int halo, const CssStreamHandoffCfg& c, int64_t n_samples, int64_t lead = WHISPER_LEAD) {
    const int pad = c.drop_silence ? c.pad_frames : 0;
    const int64_t blocks = n_samples < 0 ? (int64_t)T + hop + halo + pad + 3 : n_samples / 256 + 1 + hop;
    HandoffNeed n;
    n.frames = (blocks * 256 + lead) / 160 + 2;
    n.ranges = c.drop_silence ? (int32_t)std::min<int64_t>(blocks / 2 + 1, INT32_MAX) : 1;
    n.activity = blocks;
    return n;
}
// frames of the operand a round reserves for one speaker that appends at most dn samples: the frames it can complete, the
// rows the last frame's 416 columns reach into, and the gap to the next owner
static int64_t handoff_rows(int64_t dn) { return (dn + 200) / 160 + 2 + 3; }
// the same for NeMo's 512 columns (api_stream_kernels.hip states it again for the kernel entry)
static int64_t nemo_rows(int64_t dn) { return (dn + NEMO_LEAD) / NEMO_HOP + 2 + 4; }
// frames of a concatenation of A samples: of a finished stream, or complete while it is open
static int64_t frames_complete(bool nemo, bool closing, int64_t A) {
    if (closing) return A / 160;
    return nemo ? (A >= NEMO_LEAD ? (A - NEMO_LEAD) / NEMO_HOP + 1 : 0) : (A >= 201 ? (A - 200) / 160 + 1 : 0);
}

static int check_handoff_cfg(const CssStreamHandoffCfg* c) {
    if (!c || (c->n_mels != 80 && c->n_mels != 128) || c->pad_frames < 0 || c->pad_frames > 4096) return CSS_ERR_INVALID_ARG;
    return CSS_OK;
}

// what a call must find in the hand-off outputs `o` of a stream with the hand-off on
int check_handoff_out(const StreamState* s, const CssStreamHandoffOut* o, int64_t n_samples, std::string* why) {
    const HandoffNeed n = handoff_need(s->T, s->hop, s->halo, s->ho->cfg, n_samples, s->ho->nemo ? NEMO_LEAD : WHISPER_LEAD);
    if (!o->mel_host || !o->ranges_host || !o->n_frames || !o->n_ranges || (!o->raw_max && !s->ho->nemo) || o->cap_frames < n.frames ||
        o->cap_ranges < n.ranges || (o->activity_host && o->cap_activity < n.activity)) {
        *why = "hand-off capacities below css_stream_handoff_bounds for this call";
        return CSS_ERR_INVALID_ARG;
    }
    return CSS_OK;
}
// ... bound to it
int check_handoff_call(const StreamState* s, int64_t n_samples, std::string* why) {
    if (!s->ho) return CSS_OK;
    if (!s->ho->bound) { *why = "the hand-off is on and nothing is bound (css_stream_handoff_bind)"; return CSS_ERR_STATE; }
    return check_handoff_out(s, s->ho->bound, n_samples, why);
}

void handoff_begin_call(css_ctx* h) {
    if (HandoffCtx* c = h->handoff) { c->launches = c->products = 0; c->frames = 0; }
}

// commit: the streams' decided counts, generations and device state move (a push, finish).  Without it (a preview with hand-off)
// the round reads the same inputs and writes only what is scratch until a commit: the other generation of carry and tail, the
// handle's operand / spectra / results and the state_pv rows.
// A stream's share (RoundJob::handoff): frames [t_g, t_hi) became gated-final, the output buffer holds (q_hi - t_g) hop samples per
// speaker from sample t_g * hop on.  A preview's round with windows up to the present (n_windows) also leaves the maxima over the
// bands of the frames it makes (pvmax).
// One format's streams of the round: Whisper's (handoff.hip) or, `nemo`, NeMo's (nemo_stream.hip) -- the same three steps on the
// format's own operand, spectra, results and staging.
static int handoff_round_format(css_ctx* h, const std::vector<RoundJob>& all, size_t round, std::vector<HandoffRec>* recs, bool commit, bool nemo) {
    HandoffCtx* c = h->handoff;
    std::vector<RoundJob> jobs;
    for (const RoundJob& j : all)
        if (j.handoff && j.s->ho && j.s->ho->nemo == nemo && (j.t_hi > j.s->t_g || j.closing)) jobs.push_back(j);
    if (jobs.empty() || !c) return CSS_OK;
    DevBuf& operand = nemo ? c->nemo_operand : c->operand;
    DevBuf& spec = nemo ? c->nemo_spec : c->spec;
    DevBuf& res = nemo ? c->nemo_res : c->res;
    std::vector<PinnedBuf>& pinned = nemo ? c->nemo_pinned : c->pinned;
    const int spec_rows = nemo ? 2 * NEMO_BINS : 402;
    const int S = h->d.num_spks, hopS = h->d.frame_hop;
    const size_t n = jobs.size();
    std::vector<HandoffAppend> ap(n);
    std::vector<HandoffMel> me(n);
    std::vector<size_t> act_off(n), new_off(n), mel_off(n), pvm_off(n, 0);
    int64_t rows_total = 0;
    size_t res_b = 0;
    auto al = [](size_t v) { return (v + 63) / 64 * 64; };
    for (size_t i = 0; i < n; ++i) {
        const RoundJob& j = jobs[i];
        HandoffStream* o = j.s->ho.get();
        const int64_t t_g0 = j.s->t_g, D1 = j.closing ? j.n_out : std::max<int64_t>(j.t_hi - o->pad, 0) * hopS;
        HandoffAppend& a = ap[i];
        a = HandoffAppend{};
        a.gate = (const uint8_t*)o->gate.p; a.gate_ld = o->gate_ld; a.gate_mask = o->gate_mask;
        a.out = (const float*)j.s->out.p; a.out_ld = (j.q_hi - t_g0) * hopS; a.out_base = t_g0 * hopS;
        a.carry_in = (const float*)o->carry[o->cur].p; a.carry_out = (float*)o->carry[1 - o->cur].p; a.carry_ld = o->carry_ld;
        a.tail_in = (const float*)o->tail[o->cur].p; a.tail_out = (float*)o->tail[1 - o->cur].p;
        a.t_g0 = t_g0; a.t_g1 = j.t_hi; a.D0 = o->D; a.D1 = D1;
        a.pad = o->pad; a.drop = o->cfg.drop_silence ? 1 : 0; a.closing = j.closing ? 1 : 0; a.S = S;
        a.rows = nemo ? nemo_rows(D1 - o->D) : handoff_rows(D1 - o->D); a.row0 = rows_total;
        rows_total += a.rows * S;
        act_off[i] = res_b; res_b = al(res_b + (size_t)S * (size_t)(j.t_hi - t_g0));
        new_off[i] = res_b; res_b = al(res_b + (size_t)S * sizeof(int32_t));
        mel_off[i] = res_b; res_b = al(res_b + (size_t)S * o->cfg.n_mels * (size_t)a.rows * sizeof(float));
        if (j.n_windows > 0 && !commit) { pvm_off[i] = res_b; res_b = al(res_b + (size_t)S * (size_t)a.rows * sizeof(float)); }
    }
    const size_t state_b = (size_t)CSS_MAX_STREAMS * SMAX * sizeof(HandoffState);
    const int64_t ld = (rows_total + 3) / 4 * 4;
    int rc;
    // The product reads 416 columns from every row (NeMo: 512); columns 400 .. 415 meet zeros of the matrix, so what they read only
    // has to be finite.  The append kernel rewrites ALL rows of every owner each round, the floats behind the last row are zeros
    // from the allocation or finite values an earlier, larger round left there.
    if ((rc = ensure(h, operand, ((size_t)rows_total * 160 + 1024) * sizeof(float), true)) != CSS_OK) return rc;
    if ((rc = ensure(h, spec, (size_t)spec_rows * ld * sizeof(float))) != CSS_OK) return rc;
    if ((rc = ensure(h, res, res_b)) != CSS_OK) return rc;
    if (pinned.size() <= round) pinned.resize(round + 1);
    PinnedBuf& pin = pinned[round];
    if (pin.cap < res_b + state_b) HIPCHK(h, pin.alloc(res_b + state_b));
    const float* dftm = (const float*)(nemo ? h->nemo_tab.p : c->tab.p);
    std::vector<NemoAppend> nap(nemo ? n : 0);
    std::vector<NemoMel> nme(nemo ? n : 0);
    for (size_t i = 0; i < n; ++i) {
        const RoundJob& j = jobs[i];
        HandoffStream* o = j.s->ho.get();
        int id = 0;
        while (h->streams[id] != j.s) ++id;
        ap[i].st = (const HandoffState*)c->state.p + (size_t)id * SMAX;
        HandoffState* st = (HandoffState*)(commit ? c->state.p : c->state_pv.p) + (size_t)id * SMAX;
        ap[i].st_out = st;
        ap[i].act_out = (uint8_t*)res.p + act_off[i];
        ap[i].n_new = (int32_t*)((char*)res.p + new_off[i]);
        if (nemo) {
            nap[i] = NemoAppend{ap[i], (const float*)o->xlast[o->cur].p, (float*)o->xlast[1 - o->cur].p, o->preemph, 0};
            nme[i] = NemoMel{ap[i].row0, ap[i].rows, ap[i].n_new, nemo_bank(h, o->cfg.n_mels), (float*)((char*)res.p + mel_off[i]), ap[i].rows,
                             o->cfg.n_mels, 0};
            if (commit && o->hist_frames) { nme[i].ring = (float*)o->ring.p; nme[i].hist = o->hist_frames; nme[i].st = st; }
            me[i].mel = nme[i].mel;
        } else {
            me[i] = HandoffMel{ap[i].row0, ap[i].rows, ap[i].n_new, st, dftm + HO_DFT_F + (o->cfg.n_mels == 80 ? 0 : HO_MEL80_F), o->cfg.n_mels,
                               (float*)((char*)res.p + mel_off[i]), ap[i].rows, nullptr, nullptr, 0};
            if (commit && o->hist_frames) { me[i].ring = (float*)o->ring.p; me[i].fmax = (float*)o->fmax.p; me[i].hist = o->hist_frames; }
            if (j.n_windows > 0 && !commit) me[i].pvmax = (float*)((char*)res.p + pvm_off[i]);
        }
        HandoffRec r{};
        r.s = j.s; r.item = j.item; r.t_g0 = ap[i].t_g0; r.t_g1 = ap[i].t_g1; r.D0 = ap[i].D0; r.D1 = ap[i].D1; r.n_out = j.n_out; r.closing = j.closing;
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
    if (nemo) launch_nemo_append_multi(nap.data(), (int)n, (float*)operand.p, h->stream);
    else launch_handoff_append_multi(ap.data(), (int)n, (float*)operand.p, h->stream);
    GemmArgs g{};
    g.A = dftm; g.lda = nemo ? NEMO_NFFT : 416; g.B = (const float*)operand.p; g.ldb = 160; g.C = (float*)spec.p; g.ldc = ld;
    g.M = spec_rows; g.N = (int)rows_total; g.K = nemo ? NEMO_NFFT : 416; g.batch = 1; g.alpha = 1.f;
    launch_gemm(g, h->stream);   // (exact float32: a k-ordered chain per element, whatever the product's shape)
    if (nemo) launch_nemo_mel_multi(nme.data(), (int)n, S, (const float*)spec.p, ld, h->stream);
    else launch_handoff_mel_multi(me.data(), (int)n, S, (const float*)spec.p, ld, h->stream);
    const int tables = (int)((n + HANDOFF_MULTI_MAX - 1) / HANDOFF_MULTI_MAX);
    c->launches += 2 * tables + 1; c->products += 1; c->frames += rows_total;
    HIPCHK(h, hipMemcpyAsync(pin.p, res.p, res_b, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync((char*)pin.p + res_b, commit ? c->state.p : c->state_pv.p, state_b, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipGetLastError());
    return CSS_OK;
}

int handoff_round(css_ctx* h, const std::vector<RoundJob>& all, size_t round, std::vector<HandoffRec>* recs, bool commit) {
    const int rc = handoff_round_format(h, all, round, recs, commit, false);
    return rc != CSS_OK ? rc : handoff_round_format(h, all, round, recs, commit, true);
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
            const int64_t J1 = frames_complete(o->nemo, r.closing, A1);
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
            if (o->nemo) continue;   // (no running maximum: raw_max is never written)
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
        if (!o->nemo) out->raw_max[k] = mir.raw_max[(size_t)k];
    }
    out->n_activity = n_act;
    out->first_activity_frame = t_g_before;
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
template const char* window_refusal(const css_ctx*, const HandoffStream*, const CssStreamPresentWindow&, const int64_t*);

// The history half of an accepted request's kernel item; the caller adds the span (J, and the provisional frames if it has any).
template <typename W>
static WindowItem history_item(const HandoffStream* o, const W& w) {
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
static int launch_windows(css_ctx* h, std::vector<WindowItem>& w, int32_t* launches, const WindowOut** res) {
    static_assert(WINDOW_MULTI_MAX == CSS_WINDOW_TABLE, "the header states the table's size");
    HandoffCtx* c = h->handoff;   // (a stream with a frame history has the hand-off on)
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

// The windows of a preview's jobs, behind the hand-off round `recs` on the handle's stream: the provisional frames, their maxima
// and their counts are that round's results, which the next round overwrites.
int present_windows(css_ctx* h, const std::vector<RoundJob>& jobs, const std::vector<HandoffRec>& recs, PresentCall* pc) {
    std::vector<WindowItem> w(pc->total);
    for (const RoundJob& j : jobs) {
        if (!j.n_windows) continue;
        const HandoffRec* r = nullptr;
        for (const HandoffRec& x : recs)
            if (x.s == j.s && x.item == j.item) r = &x;
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

// ---- hand-off entry points ------------------------------------------------------------------------------------------------
int css_stream_handoff_bounds(const CssModelDesc* desc, const CssRunCfg* cfg, const CssStreamHandoffCfg* hcfg, int64_t n_samples,
                              int64_t* frames, int32_t* ranges, int64_t* activity) {
    if (!desc || !frames || !ranges || !activity || n_samples < -1) return CSS_ERR_INVALID_ARG;
    int rc = check_stream_cfg(*desc, cfg);
    if (rc == CSS_OK) rc = check_handoff_cfg(hcfg);
    if (rc != CSS_OK) return rc;
    const HandoffNeed n = handoff_need(cfg->segment_frames, cfg->hop_frames, cfg->dilation_frames + cfg->erosion_frames, *hcfg, n_samples);
    *frames = n.frames; *ranges = n.ranges; *activity = n.activity;
    return CSS_OK;
}

int css_stream_handoff_final_frames(const CssModelDesc* desc, const CssRunCfg* cfg, const CssStreamHandoffCfg* hcfg, int64_t n_pushed,
                                    int64_t* n_frames) {
    if (!desc || !n_frames || n_pushed < 0) return CSS_ERR_INVALID_ARG;
    int rc = check_stream_cfg(*desc, cfg);
    if (rc == CSS_OK) rc = check_handoff_cfg(hcfg);
    if (rc != CSS_OK) return rc;
    if (hcfg->drop_silence) return CSS_ERR_INVALID_ARG;   // with the gate in play the count depends on the audio
    const int64_t fin = final_frames(n_pushed, cfg->segment_frames, cfg->hop_frames, cfg->dilation_frames + cfg->erosion_frames) * desc->frame_hop;
    *n_frames = fin >= 201 ? (fin - 200) / 160 + 1 : 0;
    return CSS_OK;
}

// What both formats' open calls do once the configuration is accepted: the handle's shared part on first use (the state rows; the
// format's tables), the stream's buffers, its state rows and mirrors.  nemo: the pre-emphasis coefficient, else null.
static int open_handoff(css_ctx* h, StreamState* s, int32_t id, const CssStreamHandoffCfg* cfg, const float* nemo) {
    int rc;
    if (s->ho) return fail(h, CSS_ERR_STATE, "the hand-off of this stream is on already");
    if (s->n_pushed > 0 || s->finished || (nemo && s->rate && s->rate->n_in > 0))
        return fail(h, CSS_ERR_STATE, "the hand-off is switched on before the stream's first sample");
    HIPCHK(h, hipSetDevice(h->device));
    const int S = h->d.num_spks;
    HandoffCtx* c = h->handoff;
    if (!c) {
        c = new HandoffCtx();
        h->handoff = c;
    }
    if (!c->state.p || !c->state_pv.p) {
        if ((rc = ensure(h, c->state, (size_t)CSS_MAX_STREAMS * SMAX * sizeof(HandoffState), true)) != CSS_OK) return rc;
        if ((rc = ensure(h, c->state_pv, (size_t)CSS_MAX_STREAMS * SMAX * sizeof(HandoffState), true)) != CSS_OK) return rc;
    }
    if (nemo) {
        if ((rc = nemo_ensure_tables(h)) != CSS_OK) return rc;
    } else if (!c->tab.p) {
        std::vector<float> t(HO_DFT_F + HO_MEL80_F + HO_MEL128_F, 0.f);
        handoff_build_dft(t.data());
        handoff_build_mel(t.data() + HO_DFT_F, 80);
        handoff_build_mel(t.data() + HO_DFT_F + HO_MEL80_F, 128);
        if ((rc = ensure(h, c->tab, t.size() * sizeof(float))) != CSS_OK) return rc;
        HIPCHK(h, hipMemcpy(c->tab.p, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    std::unique_ptr<HandoffStream> o(new HandoffStream());
    o->cfg = *cfg;
    o->cfg.drop_silence = cfg->drop_silence ? 1 : 0;
    o->pad = o->cfg.drop_silence ? cfg->pad_frames : 0;
    o->nemo = nemo != nullptr;
    o->preemph = nemo ? *nemo : 0.f;
    static_assert(NEMO_TAIL_LD == HANDOFF_TAIL_LD, "one allocation size serves both tails (each kernel indexes by its own constant)");
    // the ring holds a round's frames (at most the window) and the 2 pad + 2 frames before them that can keep its blocks
    int64_t ring = 64;
    while (ring < s->WF + 2 * (int64_t)o->pad + 8) ring *= 2;
    o->gate_ld = ring; o->gate_mask = ring - 1;
    o->carry_ld = std::max<int64_t>((int64_t)o->pad * h->d.frame_hop, 1);
    rc = ensure(h, o->gate, (size_t)S * ring, true);
    for (int b = 0; b < 2 && rc == CSS_OK; ++b) {
        rc = ensure(h, o->carry[b], (size_t)S * o->carry_ld * sizeof(float), true);
        if (rc == CSS_OK) rc = ensure(h, o->tail[b], (size_t)S * (nemo ? NEMO_TAIL_LD : HANDOFF_TAIL_LD) * sizeof(float), true);
        if (rc == CSS_OK && nemo) rc = ensure(h, o->xlast[b], (size_t)SMAX * sizeof(float), true);
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

int css_stream_handoff_open(css_handle_t h, int32_t id, const CssStreamHandoffCfg* cfg) {
    StreamState* s = nullptr;
    const int rc = check_stream_call(h, id, &s);
    if (rc != CSS_OK) return rc;
    if (check_handoff_cfg(cfg) != CSS_OK) return fail(h, CSS_ERR_INVALID_ARG, "n_mels is 80 or 128, pad_frames 0 .. 4096");
    return open_handoff(h, s, id, cfg, nullptr);
}

// ---- the NeMo format (include/css_mi355_stream_nemo.h) ------------------------------------------------------------------------
static bool nemo_cfg_ok(const CssStreamNemoCfg* c, CssStreamHandoffCfg* as) {
    if (!c || !std::isfinite(c->preemphasis) || c->preemphasis < 0.f || c->preemphasis >= 1.f) return false;
    *as = CssStreamHandoffCfg{c->n_mels, c->pad_frames, c->drop_silence};
    return check_handoff_cfg(as) == CSS_OK;
}

int css_stream_nemo_open(css_handle_t h, int32_t id, const CssStreamNemoCfg* cfg) {
    StreamState* s = nullptr;
    const int rc = check_stream_call(h, id, &s);
    if (rc != CSS_OK) return rc;
    CssStreamHandoffCfg as{};
    if (!nemo_cfg_ok(cfg, &as)) return fail(h, CSS_ERR_INVALID_ARG, "n_mels is 80 or 128, pad_frames 0 .. 4096, preemphasis finite in [0, 1)");
    if (h->split) return fail(h, CSS_ERR_STATE, "streams run in CSS_LINEAR_EXACT_F32 only");
    return open_handoff(h, s, id, &as, &cfg->preemphasis);
}

int css_stream_nemo_bounds(const CssModelDesc* desc, const CssRunCfg* cfg, const CssStreamNemoCfg* ncfg, int64_t n_samples,
                           int64_t* frames, int32_t* ranges, int64_t* activity) {
    CssStreamHandoffCfg as{};
    if (!desc || !frames || !ranges || !activity || n_samples < -1 || !nemo_cfg_ok(ncfg, &as)) return CSS_ERR_INVALID_ARG;
    const int rc = check_stream_cfg(*desc, cfg);
    if (rc != CSS_OK) return rc;
    const HandoffNeed n = handoff_need(cfg->segment_frames, cfg->hop_frames, cfg->dilation_frames + cfg->erosion_frames, as, n_samples, NEMO_LEAD);
    *frames = n.frames; *ranges = n.ranges; *activity = n.activity;
    return CSS_OK;
}

int css_stream_nemo_final_frames(const CssModelDesc* desc, const CssRunCfg* cfg, const CssStreamNemoCfg* ncfg, int64_t n_pushed,
                                 int64_t* n_frames) {
    CssStreamHandoffCfg as{};
    if (!desc || !n_frames || n_pushed < 0 || !nemo_cfg_ok(ncfg, &as)) return CSS_ERR_INVALID_ARG;
    const int rc = check_stream_cfg(*desc, cfg);
    if (rc != CSS_OK) return rc;
    if (as.drop_silence) return CSS_ERR_INVALID_ARG;   // with the gate in play the count depends on the audio
    const int64_t fin = final_frames(n_pushed, cfg->segment_frames, cfg->hop_frames, cfg->dilation_frames + cfg->erosion_frames) * desc->frame_hop;
    *n_frames = frames_complete(true, false, fin);
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
    const HandoffCtx* c = h->handoff;
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
    if (s->ho->nemo) return fail(h, CSS_ERR_STATE, "a NeMo stream has no frame history: encoder windows are Whisper's");
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
    if (!s->ho || !s->ho->hist_frames || s->ho->nemo) return fail(h, CSS_ERR_STATE, "this stream has no frame history (css_stream_window_open)");
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
    if (const char* q = queued_refusal(h)) return fail(h, CSS_ERR_STATE, q);
    std::vector<WindowItem> w((size_t)n_items);
    for (int32_t i = 0; i < n_items; ++i) {
        const CssStreamWindow& p = items[i];
        auto refuse = [&](const std::string& msg) { return refuse_item(h, CSS_ERR_INVALID_ARG, (size_t)i, p.id, msg); };
        const StreamState* s = get_stream(h, p.id);
        if (!s) return refuse("no open stream with this id");
        const HandoffStream* o = s->ho.get();
        if (!o || !o->hist_frames || o->nemo) return refuse("the stream has no frame history (css_stream_window_open)");
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
