// libcss_mi355.so: the hand-off to Whisper for whole sessions (include/css_mi355_session_handoff.h) -- kept ranges and
// normalised log-mel of all S separated streams, behind a session's waveforms on the stream they were made on, with no host
// decision in between.  Five steps (kernels.hpp): keep-scan (gate bytes -> run table, counts, the reset maximum), gather (all
// speakers, counts from the device), the product (launch_gemm, exact float32, over the frame bound), mel (the streams'
// handoff_mel_multi_kernel<false>: its frame counts come from device memory), normalisation (columns below the count only,
// stored straight into the caller's page-locked arrays).  Bit for bit css_handoff_logmel's values per stream: the gather is a
// copy, the product's elements do not depend on N, handoff_mel_tile is the one place of re re + im im and log10f, the maximum is
// an order-free atomicMax, and the normalisation is handoff_norm_kernel's expression.  A window session (api_session_window.hip)
// adds a sixth step, the encoder windows out of the raw mel rows, and may leave out the fifth (mel_host == NULL).
#include "api_ctx.hpp"
#include "../../include/css_mi355_session_handoff.h"

static_assert(CSS_SESSION_SCAN_CHUNK == SESSION_SCAN_CHUNK, "the header states the kernel's scan step");

namespace {
constexpr size_t SH_DFT_F = (size_t)402 * 416, SH_MEL80_F = (size_t)80 * 201, SH_MEL128_F = (size_t)128 * 201;

struct Bounds { int64_t frames; int32_t ranges; };
Bounds session_bounds(const CssPlan& pl, const CssStreamHandoffCfg& c) {
    const int64_t TL = pl.mix_frames;
    return Bounds{pl.n_out / 160, c.drop_silence ? (int32_t)((TL - 1) / (2 * (int64_t)c.pad_frames + 3) + 1) : 1};
}

bool handoff_cfg_ok(const CssStreamHandoffCfg* c) {
    return c && (c->n_mels == 80 || c->n_mels == 128) && c->pad_frames >= 0 && c->pad_frames <= 4096;
}

// one session's share of sh_work, every part at a 256-byte boundary
struct Layout {
    int64_t rows, ld;   // operand rows per speaker (the frame bound + the rows the last frames' 416 columns reach into); spectra row stride
    size_t st, n_new, n_ranges, psum, regs, offs, operand, spec, mel, bytes;
};
Layout layout(int S, const CssPlan& pl, const SessHandoffReq& r) {
    auto al = [](size_t b) { return (b + 255) / 256 * 256; };
    Layout L{};
    L.rows = pl.n_out / 160 + 3;
    L.ld = (L.rows * S + 3) / 4 * 4;
    size_t o = 0;
    L.st = o; o = al(o + (size_t)S * sizeof(HandoffState));
    L.n_new = o; o = al(o + (size_t)S * sizeof(int32_t));
    L.n_ranges = o; o = al(o + (size_t)S * sizeof(int32_t));
    L.psum = o; o = al(o + (size_t)S * (size_t)(pl.mix_frames + 1) * sizeof(int32_t));
    L.regs = o; o = al(o + (size_t)S * (size_t)r.cap_ranges * 2 * sizeof(int64_t));
    L.offs = o; o = al(o + (size_t)S * (size_t)r.cap_ranges * sizeof(int64_t));
    L.operand = o; o = al(o + ((size_t)S * (size_t)L.rows * 160 + 416 + 64) * sizeof(float));
    L.spec = o; o = al(o + (size_t)402 * (size_t)L.ld * sizeof(float));
    L.mel = o; o = al(o + (size_t)S * (size_t)r.cfg.n_mels * (size_t)L.rows * sizeof(float));
    L.bytes = o;
    return L;
}

// the request for the caller's arrays `out`, by the device addresses `dev` of mel, ranges, n_frames, n_ranges
SessHandoffReq make_req(const CssStreamHandoffCfg& c, void* const dev[4], int64_t cap_frames, int32_t cap_ranges) {
    SessHandoffReq r;
    r.on = true; r.cfg = c;
    r.mel = (float*)dev[0]; r.cap_frames = cap_frames;
    r.ranges = (int64_t*)dev[1]; r.cap_ranges = cap_ranges;
    r.n_frames = (int64_t*)dev[2]; r.n_ranges = (int32_t*)dev[3];
    return r;
}

bool out_complete(const CssSessionHandoffOut* o, bool mel_optional) {
    return o && (o->mel_host || mel_optional) && o->ranges_host && o->n_frames && o->n_ranges;
}
}  // namespace

// what the queued entry points check alike; on CSS_OK `req` is the request, `n_out` the session's samples per stream and
// `frames` its frame bound
int session_handoff_enqueue_check(css_ctx* h, int64_t n_samples, int32_t n_ch, const CssRunCfg* cfg, const CssStreamHandoffCfg* hcfg,
                                  const CssSessionHandoffOut* out, bool mel_optional, SessHandoffReq* req, int64_t* n_out, int64_t* frames) {
    if (!hcfg || !out_complete(out, mel_optional)) return fail(h, CSS_ERR_INVALID_ARG, "null argument");
    if (h->split) return fail(h, CSS_ERR_STATE, "CSS_LINEAR_SPLIT_F16: css_wait may repeat a queued session, a hand-off session cannot be repeated");
    if (!h->fft512) return fail(h, CSS_ERR_INVALID_ARG, "the session hand-off needs frames of 512 samples at hop 256");
    if (!handoff_cfg_ok(hcfg)) return fail(h, CSS_ERR_INVALID_ARG, "n_mels must be 80 or 128, pad_frames in [0, 4096]");
    CssPlan pl{};
    int rc = check_run_args(h, n_samples, n_ch, cfg, &pl);
    if (rc != CSS_OK) return rc;
    const Bounds b = session_bounds(pl, *hcfg);
    if ((out->mel_host && out->cap_frames < b.frames) || out->cap_ranges < b.ranges)
        return fail(h, CSS_ERR_INVALID_ARG, "hand-off capacities below css_session_handoff_bounds: need " + std::to_string(b.frames) +
                                                " frames, " + std::to_string(b.ranges) + " ranges");
    void* dev[4] = {out->mel_host ? mapped_host(out->mel_host) : nullptr, mapped_host(out->ranges_host), mapped_host(out->n_frames),
                    mapped_host(out->n_ranges)};
    for (int i = out->mel_host ? 0 : 1; i < 4; ++i)
        if (!dev[i]) return fail(h, CSS_ERR_INVALID_ARG, "the hand-off arrays of a queued session must be page-locked (css_host_alloc)");
    *req = make_req(*hcfg, dev, out->mel_host ? out->cap_frames : 0, out->cap_ranges);
    *n_out = pl.n_out;
    *frames = b.frames;
    return CSS_OK;
}

int session_handoff_prepare(css_ctx* h, const CssPlan& pl, const SessHandoffReq& r) {
    if (r.nemo.on) return nemo_handoff_prepare(h, pl, r);   // (a session has one format)
    int rc;
    if (!h->sh_tab.p) {
        std::vector<float> t(SH_DFT_F + SH_MEL80_F + SH_MEL128_F, 0.f);
        handoff_build_dft(t.data());
        handoff_build_mel(t.data() + SH_DFT_F, 80);
        handoff_build_mel(t.data() + SH_DFT_F + SH_MEL80_F, 128);
        if ((rc = ensure(h, h->sh_tab, t.size() * sizeof(float))) != CSS_OK) return rc;
        HIPCHK(h, hipMemcpy(h->sh_tab.p, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));   // (nothing reads it yet)
    }
    return ensure(h, h->sh_work, layout(h->d.num_spks, pl, r).bytes);
}

int session_handoff_on(css_ctx* h, const float* wav, int64_t wav_ld, const SessHandoffReq& r, hipStream_t st) {
    if (r.nemo.on) return nemo_handoff_on(h, wav, wav_ld, r, st);
    const int S = h->d.num_spks;
    const Layout L = layout(S, h->plan, r);
    if (!h->sh_tab.p || h->sh_work.cap < L.bytes) return fail(h, CSS_ERR_STATE, "internal: the session hand-off was not prepared");
    char* base = (char*)h->sh_work.p;
    SessionHandoff e{};
    e.gate = (const uint8_t*)h->act_final.p; e.TL = h->plan.mix_frames;
    e.pad = r.cfg.pad_frames; e.drop = r.cfg.drop_silence ? 1 : 0; e.S = S; e.cap_ranges = r.cap_ranges;
    e.psum = (int32_t*)(base + L.psum);
    e.regs = (int64_t*)(base + L.regs); e.offs = (int64_t*)(base + L.offs);
    e.st = (HandoffState*)(base + L.st); e.n_new = (int32_t*)(base + L.n_new); e.n_ranges = (int32_t*)(base + L.n_ranges);
    e.ranges_out = r.ranges; e.n_frames_out = r.n_frames; e.n_ranges_out = r.n_ranges;
    float* operand = (float*)(base + L.operand);
    float* spec = (float*)(base + L.spec);
    float* mel = (float*)(base + L.mel);
    const float* dftm = (const float*)h->sh_tab.p;
    launch_session_keep_scan(e, st);
    launch_session_gather(e, wav, wav_ld, operand, L.rows, st);
    GemmArgs g{};
    g.A = dftm; g.lda = 416; g.B = operand; g.ldb = 160; g.C = spec; g.ldc = L.ld;
    g.M = 402; g.N = (int)(L.rows * S); g.K = 416; g.batch = 1; g.alpha = 1.f;
    launch_gemm(g, st);                                     // exact float32 matrix cores, as css_handoff_logmel's product
    HandoffMel me{0, L.rows, e.n_new, e.st, dftm + SH_DFT_F + (r.cfg.n_mels == 80 ? 0 : SH_MEL80_F), r.cfg.n_mels, mel, L.rows,
                  nullptr, nullptr, 0, nullptr};
    launch_handoff_mel_multi(&me, 1, S, spec, L.ld, st);
    if (r.mel) launch_session_norm(e, mel, L.rows, r.cfg.n_mels, r.mel, r.cap_frames, L.rows - 3, st);
    if (r.win.on) {   // the encoder windows, out of the raw rows before the next session reuses them
        const SessWindowReq& w = r.win;
        SessionWindows sw{};
        sw.st = e.st; sw.mel = mel; sw.mel_ld = L.rows; sw.max_frames = L.rows - 3;
        sw.S = S; sw.n_mels = r.cfg.n_mels; sw.width = w.width; sw.stride = w.stride; sw.f16 = w.f16;
        sw.win = w.windows; sw.ld = w.ld; sw.cap_windows = w.cap_windows;
        sw.n_win_jobs = w.windows ? (sw.max_frames + w.stride - 1) / w.stride : 0;
        sw.whole = w.whole; sw.whole_ld = w.whole_ld;
        sw.n_whole_jobs = w.whole ? (w.whole_ld + SESSION_WINDOW_CHUNK - 1) / SESSION_WINDOW_CHUNK : 0;
        sw.n_windows_out = w.n_windows; sw.window_max_out = w.window_max;
        launch_session_windows(sw, st);
        h->window_launches += 1;
    }
    HIPCHK(h, hipGetLastError());
    return CSS_OK;
}

int css_session_handoff_bounds(const CssModelDesc* desc, const CssRunCfg* cfg, const CssStreamHandoffCfg* hcfg, int64_t n_samples,
                               int64_t* frames, int32_t* ranges) {
    if (!desc || !cfg || !frames || !ranges || n_samples < 1 || !handoff_cfg_ok(hcfg)) return CSS_ERR_INVALID_ARG;
    if (validate_desc(*desc) || desc->frame_len != 512 || desc->frame_hop != 256) return CSS_ERR_INVALID_ARG;
    CssPlan pl{};
    CssRunCfg c = *cfg;
    c.w_first = c.w_mid = c.w_last = nullptr;   // (the plan's sizes do not depend on the windows)
    if (plan_impl(*desc, c, n_samples, &pl) != CSS_OK) return CSS_ERR_INVALID_ARG;
    const Bounds b = session_bounds(pl, *hcfg);
    *frames = b.frames; *ranges = b.ranges;
    return CSS_OK;
}

int session_handoff_all_check(css_ctx* h, const float* wav_dev, int64_t wav_ld, const CssStreamHandoffCfg* hcfg,
                              const CssSessionHandoffOut* out, bool mel_optional, int64_t* frames) {
    CSS_DRAIN(h);
    int rc = check_session(h);
    if (rc) return rc;
    if (!wav_dev || !hcfg || !out_complete(out, mel_optional)) return fail(h, CSS_ERR_INVALID_ARG, "null argument");
    if (!h->fft512) return fail(h, CSS_ERR_INVALID_ARG, "the session hand-off needs frames of 512 samples at hop 256");
    if (!handoff_cfg_ok(hcfg)) return fail(h, CSS_ERR_INVALID_ARG, "n_mels must be 80 or 128, pad_frames in [0, 4096]");
    if (!h->perms_done) return fail(h, CSS_ERR_STATE, "no finished pass in this session");
    if (wav_ld < h->plan.n_out) return fail(h, CSS_ERR_INVALID_ARG, "wav_ld shorter than the streams");
    const Bounds b = session_bounds(h->plan, *hcfg);
    if ((out->mel_host && out->cap_frames < b.frames) || out->cap_ranges < b.ranges)
        return fail(h, CSS_ERR_INVALID_ARG, "hand-off capacities below css_session_handoff_bounds: need " + std::to_string(b.frames) +
                                                " frames, " + std::to_string(b.ranges) + " ranges");
    *frames = b.frames;
    return CSS_OK;
}

int session_handoff_all_run(css_ctx* h, const float* wav_dev, int64_t wav_ld, const CssStreamHandoffCfg* hcfg, CssSessionHandoffOut* out,
                            const SessWindowReq* win) {
    int rc;
    const int S = h->d.num_spks, nm = hcfg->n_mels;
    const Bounds b = session_bounds(h->plan, *hcfg);
    const bool has_mel = out->mel_host != nullptr;
    HIPCHK(h, hipSetDevice(h->device));
    // page-locked arrays take the kernels' stores themselves; pageable ones get them through a page-locked staging block of
    // the bounds' size, copied out -- the written parts only -- after the synchronise
    void* dev[4] = {has_mel ? mapped_host(out->mel_host) : nullptr, mapped_host(out->ranges_host), mapped_host(out->n_frames),
                    mapped_host(out->n_ranges)};
    void* wdev[2] = {win ? mapped_host(win->n_windows) : nullptr, win ? mapped_host(win->window_max) : nullptr};
    const bool direct = (dev[0] || !has_mel) && dev[1] && dev[2] && dev[3] && (!win || (wdev[0] && wdev[1]));
    const int64_t fr_ld = std::max<int64_t>(b.frames, 1);
    const size_t mel_b = has_mel ? (size_t)S * nm * fr_ld * sizeof(float) : 0, reg_b = (size_t)S * b.ranges * 2 * sizeof(int64_t);
    const size_t cnt_b = (size_t)S * (sizeof(int64_t) + sizeof(int32_t));   // n_frames | n_ranges, then (a window call) n_windows | window_max
    SessHandoffReq req;
    if (direct) {
        req = make_req(*hcfg, dev, has_mel ? out->cap_frames : 0, out->cap_ranges);
    } else {
        const size_t need = mel_b + reg_b + cnt_b + (size_t)S * (sizeof(int32_t) + sizeof(float)) + 64;
        if (h->sh_pin.cap < need) HIPCHK(h, h->sh_pin.alloc(need));
        char* p = (char*)mapped_host(h->sh_pin.p);
        if (!p) return fail(h, CSS_ERR_HIP, "the staging block has no device address");
        void* stage[4] = {has_mel ? p : nullptr, p + mel_b, p + mel_b + reg_b, p + mel_b + reg_b + (size_t)S * sizeof(int64_t)};
        req = make_req(*hcfg, stage, has_mel ? fr_ld : 0, b.ranges);
        wdev[0] = p + mel_b + reg_b + cnt_b;
        wdev[1] = p + mel_b + reg_b + cnt_b + (size_t)S * sizeof(int32_t);
    }
    if (win) {
        req.win = *win;
        req.win.on = true;
        req.win.n_windows = (int32_t*)wdev[0];
        req.win.window_max = (float*)wdev[1];
    }
    if ((rc = session_handoff_prepare(h, h->plan, req)) != CSS_OK) return rc;
    if ((rc = session_handoff_on(h, wav_dev, wav_ld, req, h->stream)) != CSS_OK) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    if (!direct) {
        const char* p = (const char*)h->sh_pin.p;
        const float* mel = (const float*)p;
        const int64_t* reg = (const int64_t*)(p + mel_b);
        const int64_t* nf = (const int64_t*)(p + mel_b + reg_b);
        const int32_t* nr = (const int32_t*)(p + mel_b + reg_b + (size_t)S * sizeof(int64_t));
        for (int k = 0; k < S; ++k) {
            out->n_frames[k] = nf[k];
            out->n_ranges[k] = nr[k];
            for (int m = 0; m < nm && nf[k] > 0 && has_mel; ++m)
                std::memcpy(out->mel_host + ((size_t)k * nm + m) * out->cap_frames, mel + ((size_t)k * nm + m) * fr_ld, (size_t)nf[k] * sizeof(float));
            if (nr[k] > 0)
                std::memcpy(out->ranges_host + (size_t)k * out->cap_ranges * 2, reg + (size_t)k * b.ranges * 2, (size_t)nr[k] * 2 * sizeof(int64_t));
        }
        if (win) {
            std::memcpy(win->n_windows, p + mel_b + reg_b + cnt_b, (size_t)S * sizeof(int32_t));
            std::memcpy(win->window_max, p + mel_b + reg_b + cnt_b + (size_t)S * sizeof(int32_t), (size_t)S * sizeof(float));
        }
    }
    return CSS_OK;
}

int css_handoff_logmel_all(css_handle_t h, const float* wav_dev, int64_t wav_ld, const CssStreamHandoffCfg* hcfg,
                           CssSessionHandoffOut* out) {
    int64_t frames = 0;
    const int rc = session_handoff_all_check(h, wav_dev, wav_ld, hcfg, out, false, &frames);
    return rc != CSS_OK ? rc : session_handoff_all_run(h, wav_dev, wav_ld, hcfg, out, nullptr);
}

int css_run_enqueue_handoff(css_handle_t h, const float* pcm_host, int64_t n_samples, int32_t n_ch, const CssRunCfg* cfg,
                            float* wav_host, int64_t cap, const CssStreamHandoffCfg* hcfg, CssSessionHandoffOut* out) {
    if (!h || !pcm_host) return fail(h, CSS_ERR_INVALID_ARG, "null argument");
    SessHandoffReq req;
    int64_t n_out = 0, frames = 0;
    const int rc = session_handoff_enqueue_check(h, n_samples, n_ch, cfg, hcfg, out, false, &req, &n_out, &frames);
    if (rc != CSS_OK) return rc;
    return enqueue_impl(h, pcm_host, nullptr, n_samples, n_ch, cfg, wav_host, nullptr, nullptr, wav_host ? cap : n_out, &req);
}

int css_run_enqueue_pcm16_handoff(css_handle_t h, const int16_t* const* planes_host, int64_t n_samples, int32_t n_ch,
                                  const CssRunCfg* cfg, int16_t* wav_pcm16_host, int64_t cap, float* peaks_host,
                                  const CssStreamHandoffCfg* hcfg, CssSessionHandoffOut* out) {
    if (!h || !planes_host || !wav_pcm16_host || n_samples < 1 || n_ch < 1) return fail(h, CSS_ERR_INVALID_ARG, "bad argument");
    SessHandoffReq req;
    int64_t n_out = 0, frames = 0;
    const int rc = session_handoff_enqueue_check(h, n_samples, n_ch, cfg, hcfg, out, false, &req, &n_out, &frames);
    if (rc != CSS_OK) return rc;
    return enqueue_impl(h, nullptr, planes_host, n_samples, n_ch, cfg, nullptr, wav_pcm16_host, peaks_host, cap, &req);
}
