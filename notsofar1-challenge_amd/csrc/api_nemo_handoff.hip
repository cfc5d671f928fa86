// libcss_mi355.so: the hand-off to NeMo-family consumers for whole sessions (include/css_mi355_nemo_handoff.h; DESIGN.md 7 "N4 for
// NeMo hosts") -- a hand-off session (api_session_handoff.hip) with another tail.  Six steps on the stream the waveforms were made
// on, with no host decision in between: keep-scan (the session hand-off's kernel: run table, counts), gather (all speakers,
// pre-emphasis across the seams, zero pads), the product (launch_gemm, exact float32, over the frame bound), mel (raw ln rows),
// statistics (float64 sums in a fixed order, one block per stream and band), normalisation (columns below the count only, stored
// straight into the caller's page-locked arrays).  The queue sees a SessHandoffReq whose nemo part is on: session_handoff_prepare /
// session_handoff_on hand it over, so such a session shares groups and batches with every other kind.  css_nemo_kernels_host runs
// steps two to six on caller data, staged through kstage::Stager.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "api_ctx.hpp"
#include "api_kernel_stage.hpp"
#include "../../include/css_mi355_nemo_handoff.h"

using namespace css::kstage;

namespace {
constexpr size_t NM_DFT_F = (size_t)2 * NEMO_BINS * NEMO_NFFT, NM_MEL80_F = (size_t)80 * NEMO_BINS, NM_MEL128_F = (size_t)128 * NEMO_BINS;

struct Bounds { int64_t frames; int32_t ranges; };
Bounds nemo_bounds(const CssPlan& pl, const CssNemoCfg& c) {
    const int64_t TL = pl.mix_frames;
    return Bounds{pl.n_out / NEMO_HOP, c.drop_silence ? (int32_t)((TL - 1) / (2 * (int64_t)c.pad_frames + 3) + 1) : 1};
}

bool preemph_ok(float p) { return std::isfinite(p) && p >= 0.f && p < 1.f; }
const char* cfg_refusal(const CssNemoCfg* c) {
    if (!c) return "null argument";
    if (c->n_mels != 80 && c->n_mels != 128) return "n_mels must be 80 or 128";
    if (c->pad_frames < 0 || c->pad_frames > 4096) return "pad_frames must lie in [0, 4096]";
    if (!preemph_ok(c->preemphasis)) return "preemphasis must be finite, at least 0 and below 1";
    return nullptr;
}

// one session's share of sh_work, every part at a 256-byte boundary
struct Layout {
    int64_t rows, ld;   // operand rows per speaker (the frame bound + the rows the last frames' 512 columns reach into); spectra row stride
    size_t st, n_new, n_ranges, psum, regs, offs, operand, spec, raw, mean, stdv, bytes;
};
Layout layout(int S, const CssPlan& pl, int n_mels, int32_t cap_ranges) {
    auto al = [](size_t b) { return (b + 255) / 256 * 256; };
    Layout L{};
    L.rows = pl.n_out / NEMO_HOP + 4;
    L.ld = (L.rows * S + 3) / 4 * 4;
    size_t o = 0;
    L.st = o; o = al(o + (size_t)S * sizeof(HandoffState));
    L.n_new = o; o = al(o + (size_t)S * sizeof(int32_t));
    L.n_ranges = o; o = al(o + (size_t)S * sizeof(int32_t));
    L.psum = o; o = al(o + (size_t)S * (size_t)(pl.mix_frames + 1) * sizeof(int32_t));
    L.regs = o; o = al(o + (size_t)S * (size_t)cap_ranges * 2 * sizeof(int64_t));
    L.offs = o; o = al(o + (size_t)S * (size_t)cap_ranges * sizeof(int64_t));
    L.operand = o; o = al(o + ((size_t)S * (size_t)L.rows * NEMO_HOP + NEMO_NFFT + 64) * sizeof(float));
    L.spec = o; o = al(o + (size_t)2 * NEMO_BINS * (size_t)L.ld * sizeof(float));
    L.raw = o; o = al(o + (size_t)S * (size_t)n_mels * (size_t)L.rows * sizeof(float));
    L.mean = o; o = al(o + (size_t)S * (size_t)n_mels * sizeof(float));
    L.stdv = o; o = al(o + (size_t)S * (size_t)n_mels * sizeof(float));
    L.bytes = o;
    return L;
}

// the request for the caller's arrays, by the device addresses `dev` of mel, ranges, n_frames, n_ranges, mean, std
SessHandoffReq make_req(const CssNemoCfg& c, void* const dev[6], int64_t cap_frames, int32_t cap_ranges) {
    SessHandoffReq r;
    r.on = true;
    r.cfg = CssStreamHandoffCfg{c.n_mels, c.pad_frames, c.drop_silence ? 1 : 0};
    r.ranges = (int64_t*)dev[1]; r.cap_ranges = cap_ranges;
    r.n_frames = (int64_t*)dev[2]; r.n_ranges = (int32_t*)dev[3];
    r.nemo.on = true; r.nemo.preemph = c.preemphasis; r.nemo.normalize = c.normalize ? 1 : 0;
    r.nemo.mel = (float*)dev[0]; r.nemo.cap_frames = cap_frames;
    r.nemo.mean = (float*)dev[4]; r.nemo.stdv = (float*)dev[5];
    return r;
}

bool out_complete(const CssNemoOut* o) { return o && o->mel_host && o->ranges_host && o->n_frames && o->n_ranges; }

// steps two to six on `st`: e holds the run table and the counts, f the rest
void features_on(css_ctx* h, const SessionHandoff& e, NemoFeatures f, const float* wav, int64_t wav_ld, float* operand, float* spec, int64_t ld,
                 float preemph, hipStream_t st) {
    launch_nemo_gather(e, wav, wav_ld, operand, f.rows, preemph, st);
    GemmArgs g{};
    g.A = (const float*)h->nemo_tab.p; g.lda = NEMO_NFFT; g.B = operand; g.ldb = NEMO_HOP; g.C = spec; g.ldc = ld;
    g.M = 2 * NEMO_BINS; g.N = (int)(f.rows * e.S); g.K = NEMO_NFFT; g.batch = 1; g.alpha = 1.f;
    launch_gemm(g, st);                                     // exact float32 matrix cores
    f.w = nemo_bank(h, f.n_mels);
    launch_nemo_mel(f, spec, ld, st);
    launch_nemo_stats(f, st);
    launch_nemo_norm(f, st);
}

// what the two queued entry points check alike; on CSS_OK `req` is the request and `n_out` the session's samples per stream
int enqueue_check(css_ctx* h, int64_t n_samples, int32_t n_ch, const CssRunCfg* cfg, const CssNemoCfg* ncfg, const CssNemoOut* out,
                  SessHandoffReq* req, int64_t* n_out) {
    if (!ncfg || !out_complete(out)) return fail(h, CSS_ERR_INVALID_ARG, "null argument");
    if (h->split) return fail(h, CSS_ERR_STATE, "CSS_LINEAR_SPLIT_F16: css_wait may repeat a queued session, a hand-off session cannot be repeated");
    if (!h->fft512) return fail(h, CSS_ERR_INVALID_ARG, "the NeMo hand-off needs frames of 512 samples at hop 256");
    if (const char* why = cfg_refusal(ncfg)) return fail(h, CSS_ERR_INVALID_ARG, why);
    CssPlan pl{};
    int rc = check_run_args(h, n_samples, n_ch, cfg, &pl);
    if (rc != CSS_OK) return rc;
    const Bounds b = nemo_bounds(pl, *ncfg);
    if (out->cap_frames < b.frames || out->cap_ranges < b.ranges)
        return fail(h, CSS_ERR_INVALID_ARG, "hand-off capacities below css_nemo_handoff_bounds: need " + std::to_string(b.frames) + " frames, " +
                                                std::to_string(b.ranges) + " ranges");
    void* dev[6] = {mapped_host(out->mel_host), mapped_host(out->ranges_host), mapped_host(out->n_frames), mapped_host(out->n_ranges),
                    out->mean_host ? mapped_host(out->mean_host) : nullptr, out->std_host ? mapped_host(out->std_host) : nullptr};
    if (!dev[0] || !dev[1] || !dev[2] || !dev[3] || (out->mean_host && !dev[4]) || (out->std_host && !dev[5]))
        return fail(h, CSS_ERR_INVALID_ARG, "the hand-off arrays of a queued session must be page-locked (css_host_alloc)");
    *req = make_req(*ncfg, dev, out->cap_frames, out->cap_ranges);
    *n_out = pl.n_out;
    return CSS_OK;
}
}  // namespace

int nemo_ensure_tables(css_ctx* h) {
    if (h->nemo_tab.p) return CSS_OK;
    std::vector<float> t(NM_DFT_F + NM_MEL80_F + NM_MEL128_F, 0.f);
    nemo_build_dft(t.data());
    handoff_build_mel(t.data() + NM_DFT_F, 80, NEMO_BINS);
    handoff_build_mel(t.data() + NM_DFT_F + NM_MEL80_F, 128, NEMO_BINS);
    int rc;
    if ((rc = ensure(h, h->nemo_tab, t.size() * sizeof(float))) != CSS_OK) return rc;
    HIPCHK(h, hipMemcpy(h->nemo_tab.p, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));   // (nothing reads it yet)
    return CSS_OK;
}
const float* nemo_bank(const css_ctx* h, int n_mels) { return (const float*)h->nemo_tab.p + NM_DFT_F + (n_mels == 80 ? 0 : NM_MEL80_F); }

int nemo_handoff_prepare(css_ctx* h, const CssPlan& pl, const SessHandoffReq& r) {
    int rc;
    if ((rc = nemo_ensure_tables(h)) != CSS_OK) return rc;
    return ensure(h, h->sh_work, layout(h->d.num_spks, pl, r.cfg.n_mels, r.cap_ranges).bytes);
}

int nemo_handoff_on(css_ctx* h, const float* wav, int64_t wav_ld, const SessHandoffReq& r, hipStream_t st) {
    const int S = h->d.num_spks;
    const Layout L = layout(S, h->plan, r.cfg.n_mels, r.cap_ranges);
    if (!h->nemo_tab.p || h->sh_work.cap < L.bytes) return fail(h, CSS_ERR_STATE, "internal: the NeMo hand-off was not prepared");
    char* base = (char*)h->sh_work.p;
    SessionHandoff e{};
    e.gate = (const uint8_t*)h->act_final.p; e.TL = h->plan.mix_frames;
    e.pad = r.cfg.pad_frames; e.drop = r.cfg.drop_silence ? 1 : 0; e.S = S; e.cap_ranges = r.cap_ranges;
    e.psum = (int32_t*)(base + L.psum);
    e.regs = (int64_t*)(base + L.regs); e.offs = (int64_t*)(base + L.offs);
    e.st = (HandoffState*)(base + L.st); e.n_new = (int32_t*)(base + L.n_new); e.n_ranges = (int32_t*)(base + L.n_ranges);
    e.ranges_out = r.ranges; e.n_frames_out = r.n_frames; e.n_ranges_out = r.n_ranges;
    NemoFeatures f{};
    f.st = e.st; f.S = S; f.n_mels = r.cfg.n_mels; f.normalize = r.nemo.normalize; f.rows = L.rows;
    f.raw = (float*)(base + L.raw); f.raw_ld = L.rows;
    f.mean = (float*)(base + L.mean); f.stdv = (float*)(base + L.stdv);
    f.mean_out = r.nemo.mean; f.std_out = r.nemo.stdv;
    f.out = r.nemo.mel; f.out_ld = r.nemo.cap_frames;
    launch_session_keep_scan(e, st);
    features_on(h, e, f, wav, wav_ld, (float*)(base + L.operand), (float*)(base + L.spec), L.ld, r.nemo.preemph, st);
    HIPCHK(h, hipGetLastError());
    return CSS_OK;
}

extern "C" {

int css_nemo_handoff_bounds(const CssModelDesc* desc, const CssRunCfg* cfg, const CssNemoCfg* ncfg, int64_t n_samples, int64_t* frames,
                            int32_t* ranges) {
    if (!desc || !cfg || !frames || !ranges || n_samples < 1 || cfg_refusal(ncfg)) return CSS_ERR_INVALID_ARG;
    if (validate_desc(*desc) || desc->frame_len != 512 || desc->frame_hop != 256) return CSS_ERR_INVALID_ARG;
    CssPlan pl{};
    CssRunCfg c = *cfg;
    c.w_first = c.w_mid = c.w_last = nullptr;   // (the plan's sizes do not depend on the windows)
    if (plan_impl(*desc, c, n_samples, &pl) != CSS_OK) return CSS_ERR_INVALID_ARG;
    const Bounds b = nemo_bounds(pl, *ncfg);
    *frames = b.frames; *ranges = b.ranges;
    return CSS_OK;
}

int css_handoff_nemo_all(css_handle_t h, const float* wav_dev, int64_t wav_ld, const CssNemoCfg* ncfg, CssNemoOut* out) {
    CSS_DRAIN(h);
    int rc = check_session(h);
    if (rc) return rc;
    if (!wav_dev || !ncfg || !out_complete(out)) return fail(h, CSS_ERR_INVALID_ARG, "null argument");
    if (!h->fft512) return fail(h, CSS_ERR_INVALID_ARG, "the NeMo hand-off needs frames of 512 samples at hop 256");
    if (const char* why = cfg_refusal(ncfg)) return fail(h, CSS_ERR_INVALID_ARG, why);
    if (!h->perms_done) return fail(h, CSS_ERR_STATE, "no finished pass in this session");
    if (wav_ld < h->plan.n_out) return fail(h, CSS_ERR_INVALID_ARG, "wav_ld shorter than the streams");
    const Bounds b = nemo_bounds(h->plan, *ncfg);
    if (out->cap_frames < b.frames || out->cap_ranges < b.ranges)
        return fail(h, CSS_ERR_INVALID_ARG, "hand-off capacities below css_nemo_handoff_bounds: need " + std::to_string(b.frames) + " frames, " +
                                                std::to_string(b.ranges) + " ranges");
    const int S = h->d.num_spks, nm = ncfg->n_mels;
    HIPCHK(h, hipSetDevice(h->device));
    // page-locked arrays take the kernels' stores themselves; pageable ones get them through a page-locked staging block of
    // the bounds' size, copied out -- the written parts only -- after the synchronise
    void* dev[6] = {mapped_host(out->mel_host), mapped_host(out->ranges_host), mapped_host(out->n_frames), mapped_host(out->n_ranges),
                    out->mean_host ? mapped_host(out->mean_host) : nullptr, out->std_host ? mapped_host(out->std_host) : nullptr};
    const bool direct = dev[0] && dev[1] && dev[2] && dev[3] && (!out->mean_host || dev[4]) && (!out->std_host || dev[5]);
    const int64_t fr_ld = std::max<int64_t>(b.frames, 1);
    const size_t mel_b = (size_t)S * nm * fr_ld * sizeof(float), reg_b = (size_t)S * b.ranges * 2 * sizeof(int64_t);
    // n_frames | n_ranges (int32 rows in a block of the same size: what follows stays 8-byte aligned) | mean | std
    const size_t nf_b = (size_t)S * sizeof(int64_t), nr_b = nf_b, ms_b = (size_t)S * nm * sizeof(float);
    SessHandoffReq req;
    if (direct) {
        req = make_req(*ncfg, dev, out->cap_frames, out->cap_ranges);
    } else {
        const size_t need = mel_b + reg_b + nf_b + nr_b + 2 * ms_b + 64;
        if (h->sh_pin.cap < need) HIPCHK(h, h->sh_pin.alloc(need));
        char* p = (char*)mapped_host(h->sh_pin.p);
        if (!p) return fail(h, CSS_ERR_HIP, "the staging block has no device address");
        void* stage[6] = {p, p + mel_b, p + mel_b + reg_b, p + mel_b + reg_b + nf_b, p + mel_b + reg_b + nf_b + nr_b,
                          p + mel_b + reg_b + nf_b + nr_b + ms_b};
        req = make_req(*ncfg, stage, fr_ld, b.ranges);
    }
    if ((rc = nemo_handoff_prepare(h, h->plan, req)) != CSS_OK) return rc;
    if ((rc = nemo_handoff_on(h, wav_dev, wav_ld, req, h->stream)) != CSS_OK) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    if (!direct) {
        const char* p = (const char*)h->sh_pin.p;
        const float* mel = (const float*)p;
        const int64_t* reg = (const int64_t*)(p + mel_b);
        const int64_t* nf = (const int64_t*)(p + mel_b + reg_b);
        const int32_t* nr = (const int32_t*)(p + mel_b + reg_b + nf_b);
        const float* mean = (const float*)(p + mel_b + reg_b + nf_b + nr_b);
        const float* stdv = (const float*)(p + mel_b + reg_b + nf_b + nr_b + ms_b);
        for (int k = 0; k < S; ++k) {
            out->n_frames[k] = nf[k];
            out->n_ranges[k] = nr[k];
            for (int m = 0; m < nm && nf[k] > 0; ++m)
                std::memcpy(out->mel_host + ((size_t)k * nm + m) * out->cap_frames, mel + ((size_t)k * nm + m) * fr_ld, (size_t)nf[k] * sizeof(float));
            if (nr[k] > 0)
                std::memcpy(out->ranges_host + (size_t)k * out->cap_ranges * 2, reg + (size_t)k * b.ranges * 2, (size_t)nr[k] * 2 * sizeof(int64_t));
            if (nf[k] > 0 && out->mean_host) std::memcpy(out->mean_host + (size_t)k * nm, mean + (size_t)k * nm, (size_t)nm * sizeof(float));
            if (nf[k] > 0 && out->std_host) std::memcpy(out->std_host + (size_t)k * nm, stdv + (size_t)k * nm, (size_t)nm * sizeof(float));
        }
    }
    return CSS_OK;
}

int css_run_enqueue_nemo(css_handle_t h, const float* pcm_host, int64_t n_samples, int32_t n_ch, const CssRunCfg* cfg, float* wav_host,
                         int64_t cap, const CssNemoCfg* ncfg, CssNemoOut* out) {
    if (!h || !pcm_host) return fail(h, CSS_ERR_INVALID_ARG, "null argument");
    SessHandoffReq req;
    int64_t n_out = 0;
    const int rc = enqueue_check(h, n_samples, n_ch, cfg, ncfg, out, &req, &n_out);
    if (rc != CSS_OK) return rc;
    return enqueue_impl(h, pcm_host, nullptr, n_samples, n_ch, cfg, wav_host, nullptr, nullptr, wav_host ? cap : n_out, &req);
}

int css_run_enqueue_pcm16_nemo(css_handle_t h, const int16_t* const* planes_host, int64_t n_samples, int32_t n_ch, const CssRunCfg* cfg,
                               int16_t* wav_pcm16_host, int64_t cap, float* peaks_host, const CssNemoCfg* ncfg, CssNemoOut* out) {
    if (!h || !planes_host || n_samples < 1 || n_ch < 1) return fail(h, CSS_ERR_INVALID_ARG, "bad argument");
    SessHandoffReq req;
    int64_t n_out = 0;
    const int rc = enqueue_check(h, n_samples, n_ch, cfg, ncfg, out, &req, &n_out);
    if (rc != CSS_OK) return rc;
    return enqueue_impl(h, nullptr, planes_host, n_samples, n_ch, cfg, nullptr, wav_pcm16_host, wav_pcm16_host ? peaks_host : nullptr,
                        wav_pcm16_host ? cap : n_out, &req);
}

int css_nemo_kernels_host(css_handle_t h, CssNemoKernelsJob* job) {
    CSS_DRAIN(h);
    if (!h) return CSS_ERR_INVALID_ARG;
    auto bad = [&](const char* what) { return fail(h, CSS_ERR_INVALID_ARG, std::string("css_nemo_kernels_host: ") + what); };
    if (!job) return bad("null argument");
    static_assert(sizeof(HandoffState) == 24, "the header states the state row");
    static_assert(sizeof(CssNemoArray) == sizeof(CssKArray), "the stager's array descriptor");
    const CssNemoKernelsJob& j = *job;
    constexpr int64_t POS_MAX = (int64_t)1 << 40;
    if (j.S < 1 || j.S > 4) return bad("S must be 1 .. 4");
    if (j.n_mels != 80 && j.n_mels != 128) return bad("n_mels must be 80 or 128");
    if (j.normalize != 0 && j.normalize != 1) return bad("normalize is 0 or 1");
    if (!preemph_ok(j.preemphasis)) return bad("preemphasis must be finite, at least 0 and below 1");
    if (j.rows < 4 || j.rows > (1 << 20)) return bad("rows must be 4 .. 2^20");
    if (j.cap_ranges < 1 || j.cap_ranges > (1 << 24)) return bad("cap_ranges must be at least 1");
    if (j.wav_off < 0 || j.wav_off > 3) return bad("wav_off must be 0 .. 3");
    if (j.wav_ld < 1 || j.wav_ld > HOST_CAP) return bad("wav_ld must be at least 1");
    const int64_t frames = j.rows - 4;
    if (j.raw_ld < frames || j.raw_ld > HOST_CAP) return bad("raw_ld must cover rows - 4");
    if (j.out_ld < 0 || j.out_ld > HOST_CAP) return bad("out_ld must not be negative");
    auto ka = [](const CssNemoArray& a) { return CssKArray{a.p, a.elems}; };
    const CssKArray wav = ka(j.wav), regs = ka(j.regs), offs = ka(j.offs), st = ka(j.st), n_ranges = ka(j.n_ranges), operand = ka(j.operand),
                    raw = ka(j.raw), mean = ka(j.mean), stdv = ka(j.stdv), out = ka(j.out);
    const int64_t S = j.S, cap = j.cap_ranges, SM = S * j.n_mels;
    if (!arr_ok(regs, S * cap * 2) || !regs.p || !arr_ok(offs, S * cap) || !offs.p || !arr_ok(st, S) || !st.p || !arr_ok(n_ranges, S) || !n_ranges.p ||
        !arr_ok(wav, j.wav_off + S * j.wav_ld) || !wav.p || !arr_ok(raw, SM * j.raw_ld) || !arr_ok(mean, SM) || !mean.p || !arr_ok(stdv, SM) || !stdv.p ||
        !arr_ok(out, SM * j.out_ld))
        return bad("an array is null or shorter than its description");
    if (!operand.p || operand.elems != S * j.rows * NEMO_HOP + NEMO_NFFT) return bad("operand must hold S rows 160 + 512 floats");
    const HandoffState* stv = (const HandoffState*)st.p;
    const int32_t* nrv = (const int32_t*)n_ranges.p;
    for (int k = 0; k < j.S; ++k) {
        const int64_t A = stv[k].A, J = stv[k].J;
        if (A < 0 || A > POS_MAX) return bad("a sample count A below 0");
        if (J < 0 || J > frames || (J > 0 && J > (A + 352) / NEMO_HOP)) return bad("a frame count J outside 0 .. rows - 4, or beyond the zeros behind A");
        if (nrv[k] < 0) return bad("a run count below 0");
        const int64_t nr = std::min<int64_t>(nrv[k], cap);
        if (A == 0 || nr == 0) continue;
        const int64_t* reg = (const int64_t*)regs.p + (int64_t)k * cap * 2;
        const int64_t* off = (const int64_t*)offs.p + (int64_t)k * cap;
        for (int64_t r = 0; r < nr; ++r) {
            if (off[r] < -POS_MAX || off[r] > POS_MAX || reg[2 * r] < -POS_MAX || reg[2 * r] > POS_MAX) return bad("a table entry out of range");
            if (r > 0 && off[r] < off[r - 1]) return bad("offs is not monotone");
        }
        for (int64_t r = 0; r < nr; ++r) {   // run r serves the concatenation samples [j_lo, j_hi]
            const int64_t j_lo = r == 0 ? 0 : std::max<int64_t>(off[r], 0);
            const int64_t j_hi = r == nr - 1 ? A - 1 : std::min(off[r + 1], A) - 1;
            if (j_lo > j_hi) continue;
            if (reg[2 * r] + (j_lo - off[r]) < 0 || reg[2 * r] + (j_hi - off[r]) >= j.wav_ld) return bad("the table reads outside a wav row");
        }
    }
    int rc;
    HIPCHK(h, hipSetDevice(h->device));
    if ((rc = nemo_ensure_tables(h)) != CSS_OK) return rc;
    const int64_t ld = (j.rows * S + 3) / 4 * 4;
    Stager sg;
    const size_t a_regs = sg.take(regs, 8, false), a_offs = sg.take(offs, 8, false), a_st = sg.take(st, sizeof(HandoffState), false),
                 a_nr = sg.take(n_ranges, 4, false), a_wav = sg.take(wav, 4, false), a_op = sg.take(operand, 4, true),
                 a_spec = sg.scratch((int64_t)2 * NEMO_BINS * ld, 4), a_raw = sg.take(raw, 4, true), a_mean = sg.take(mean, 4, true),
                 a_std = sg.take(stdv, 4, true), a_out = sg.take(out, 4, true);
    char* base = nullptr;
    if ((rc = stage_and_upload(h, sg, &base)) != CSS_OK) return rc;
    SessionHandoff e{};
    e.S = j.S; e.cap_ranges = j.cap_ranges;
    e.regs = (int64_t*)(base + a_regs); e.offs = (int64_t*)(base + a_offs); e.st = (HandoffState*)(base + a_st); e.n_ranges = (int32_t*)(base + a_nr);
    NemoFeatures f{};
    f.st = e.st; f.S = j.S; f.n_mels = j.n_mels; f.normalize = j.normalize; f.rows = j.rows;
    f.raw = (float*)(base + a_raw); f.raw_ld = j.raw_ld;
    f.mean = (float*)(base + a_mean); f.stdv = (float*)(base + a_std);
    f.out = out.elems > 0 ? (float*)(base + a_out) : nullptr; f.out_ld = j.out_ld;
    features_on(h, e, f, (const float*)(base + a_wav) + j.wav_off, j.wav_ld, (float*)(base + a_op), (float*)(base + a_spec), ld, j.preemphasis,
                h->stream);
    return download_all(h, sg, base);
}

}  // extern "C"
