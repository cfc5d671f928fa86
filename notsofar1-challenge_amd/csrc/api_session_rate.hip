// libcss_mi355.so: whole sessions at the capture rate (include/css_mi355_session_rate.h; DESIGN.md 7 "N1 / N2 at the capture
// rate") -- css_run, css_run_pcm16 and the queue for recordings at 48 / 44.1 / ... kHz, with the separated streams at the model's
// rate or at a playback rate.
// The ingest edge: the recording crosses PCIe as it was captured, into staging beside the session's slot of the sample buffer,
// and session_ingest_resample_kernel (one launch for all rate sessions of a queue group) writes the model-rate float32 [n_model][C]
// and the recording's level.  From there the session is a float session: nothing downstream of the sample buffer changes.
// The output edge: the waveforms stay in HBM (the hand-off sessions' form), session_output_kernel writes [S][n_out] and the rows'
// peaks on the tail's stream, and -- PCM16 -- the encode pass of css_run_pcm16 follows with those peaks.
// Bit for bit css_resample_host -> css_run -> css_resample_host: every sample is resample_sample's one fmaf chain.
#include "api_ctx.hpp"
#include "../../include/css_mi355_session_rate.h"

static_assert(SESSION_RATE_TABLE == css_ctx::MAX_GROUP, "one ingest launch holds a whole queue group");

namespace {
constexpr int64_t RATE_N_MAX = (int64_t)1 << 40;
const char* const kRatioRule = "rate ratio: 1 / 1, or up != down in lowest terms with at most 128 taps per output sample and 16384 taps";

bool unity(int32_t up, int32_t down) { return up == 1 && down == 1; }

// the ratio of one side: 1 / 1 (on = false) or one of resample_ratio's
bool side_ratio(int32_t up, int32_t down, bool* on, ResampleRatio* r) {
    *on = !unity(up, down);
    return !*on || resample_ratio(up, down, r);
}

int64_t pad4(int64_t n) { return (n + 3) / 4 * 4; }
size_t al256(size_t b) { return (b + 255) / 256 * 256; }

// the phase table of a ratio on the device, made on first use
int rate_tab(css_ctx* h, const ResampleRatio& r, const float** tab) {
    for (const auto& t : h->rate_tabs)
        if (t->up == r.up && t->down == r.down) { *tab = t->tab.as(); return CSS_OK; }
    std::vector<float> taps((size_t)r.L), host((size_t)r.up * r.P_ld);
    resample_taps_f32(r, taps.data());
    resample_phase_table(r, taps.data(), host.data());
    auto t = std::make_unique<css_ctx::RateTab>();
    t->up = r.up; t->down = r.down;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, dev_alloc(t->tab, host.size() * sizeof(float)));
    HIPCHK(h, hipMemcpy(t->tab.p, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));   // (nothing reads it yet)
    *tab = t->tab.as();
    h->rate_tabs.push_back(std::move(t));
    return CSS_OK;
}

// What the four calls check alike, before anything is allocated, uploaded or queued.  On CSS_OK `sr` is the session's rate
// (without its sink) and `pl` the plan of its n_model samples.
int check_rate(css_ctx* h, int64_t n_in, int32_t n_ch, const CssRunCfg* cfg, const CssSessionRate* rate, int64_t cap,
               const int16_t* const* planes, SessRate* sr, CssPlan* pl) {
    if (!cfg || !rate) return fail(h, CSS_ERR_INVALID_ARG, "null argument");
    if (h->split)
        return fail(h, CSS_ERR_STATE, "CSS_LINEAR_SPLIT_F16: css_wait may repeat a queued session, a rate session cannot be repeated");
    SessRate r;
    r.on = true;
    if (!side_ratio(rate->in_up, rate->in_down, &r.in_on, &r.in) || !side_ratio(rate->out_up, rate->out_down, &r.out_on, &r.out))
        return fail(h, CSS_ERR_INVALID_ARG, kRatioRule);
    if (n_in < 1 || n_in > RATE_N_MAX) return fail(h, CSS_ERR_INVALID_ARG, "n_in must be in [1, 2^40]");
    if (n_ch < 1 || n_ch > 64) return fail(h, CSS_ERR_INVALID_ARG, "bad argument");
    if ((r.in_on && (!resample_fits(r.in, n_ch) || !session_ingest_fits(r.in, n_ch))) || (r.out_on && !stream_output_fits(r.out)))
        return fail(h, CSS_ERR_INVALID_ARG, "rate ratio: its tile does not fit a workgroup's LDS");
    r.n_in = n_in;
    const int64_t n_model = r.in_on ? resample_count(r.in, n_in, true) : n_in;
    int rc = check_run_args(h, n_model, n_ch, cfg, pl);
    if (rc != CSS_OK) return rc;
    r.n_out = r.out_on ? resample_count(r.out, pl->n_out, true) : pl->n_out;
    if (cap < r.n_out) return fail(h, CSS_ERR_INVALID_ARG, "output buffer too small: need " + std::to_string(r.n_out) + " samples per stream");
    if (planes)
        for (int c = 0; c < n_ch; ++c)
            if (!planes[c]) return fail(h, CSS_ERR_INVALID_ARG, "null channel plane");
    if (r.in_on && (rc = rate_tab(h, r.in, &r.in_tab)) != CSS_OK) return rc;
    if (r.out_on && (rc = rate_tab(h, r.out, &r.out_tab)) != CSS_OK) return rc;
    *sr = r;
    return CSS_OK;
}

// the synchronous calls: css_run / css_run_pcm16 on a rate session's record
int run_rate(css_ctx* h, const float* pcm, const int16_t* const* planes, int64_t n_in, int32_t n_ch, const CssRunCfg* cfg,
             const CssSessionRate* rate, float* wav, int16_t* wav16, float* peaks, int64_t cap) {
    SessRate sr;
    CssPlan pl{};
    int rc = check_rate(h, n_in, n_ch, cfg, rate, cap, planes, &sr, &pl);
    if (rc != CSS_OK) return rc;
    css_ctx::QueuedSession q(pcm, planes, pl.n_samples, n_ch, *cfg, wav, wav16, peaks, cap, nullptr);
    session_rate_adopt(q, sr, pl.n_out);
    const CssRunCfg own = q.own_cfg();
    rc = run_impl(h, q.n, n_ch, &own, q.io(false));
    if (rc == CSS_OK) h->rate_sessions += 1;
    return rc;
}

int enqueue_rate(css_ctx* h, const float* pcm, const int16_t* const* planes, int64_t n_in, int32_t n_ch, const CssRunCfg* cfg,
                 const CssSessionRate* rate, float* wav, int16_t* wav16, float* peaks, int64_t cap) {
    SessRate sr;
    CssPlan pl{};
    const int rc = check_rate(h, n_in, n_ch, cfg, rate, cap, planes, &sr, &pl);
    if (rc != CSS_OK) return rc;
    return enqueue_impl(h, pcm, planes, pl.n_samples, n_ch, cfg, wav, wav16, peaks, cap, nullptr, &sr);
}
}  // namespace

void session_rate_adopt(css_ctx::QueuedSession& q, const SessRate& rate, int64_t n_out_model) {
    q.rate = rate;
    if (!rate.out_on) return;
    q.rate.wav = q.wav; q.rate.wav16 = q.wav16; q.rate.peaks = q.peaks; q.rate.cap = q.cap;
    q.wav = nullptr; q.wav16 = nullptr; q.peaks = nullptr; q.wav_mapped = nullptr;
    q.cap = n_out_model;
}

// rate_out: [S level words, 256 bytes | S rows of pad4(n_out) float32 | S rows of n_out int16 (PCM16 output)]
int session_rate_prepare(css_ctx* h, const SessRate& r) {
    if (!r.out_on) return CSS_OK;
    const size_t S = (size_t)h->d.num_spks;
    return ensure(h, h->rate_out, 256 + al256(S * (size_t)pad4(r.n_out) * sizeof(float)) + (r.wav16 ? S * (size_t)r.n_out * sizeof(int16_t) : 0));
}

size_t session_rate_capture_bytes(const SessRate& r, int n_ch, bool pcm16) {
    return (size_t)r.n_in * (size_t)n_ch * (pcm16 ? sizeof(int16_t) : sizeof(float));
}

// the recording as it was captured -> staging: the float piece [n_in][C] as it is, the PCM16 planes one behind the other
int session_rate_upload(css_ctx* h, const SessRate& r, const float* pcm, const int16_t* const* planes, int n_ch, void* staging, hipStream_t st) {
    if (!planes) {
        HIPCHK(h, hipMemcpyAsync(staging, pcm, session_rate_capture_bytes(r, n_ch, false), hipMemcpyHostToDevice, st));
        return CSS_OK;
    }
    for (int c = 0; c < n_ch; ++c)
        HIPCHK(h, hipMemcpyAsync((int16_t*)staging + (size_t)c * r.n_in, planes[c], (size_t)r.n_in * sizeof(int16_t), hipMemcpyHostToDevice, st));
    return CSS_OK;
}

SessionIngestJob session_rate_job(const SessRate& r, bool pcm16, int n_ch, const void* staging, float* dst, int64_t n_model, int64_t n_peak,
                                  unsigned int* level) {
    SessionIngestJob j{};
    j.r.src = staging; j.r.is_i16 = pcm16 ? 1 : 0; j.r.plane_ld = pcm16 ? r.n_in : 0; j.r.n = r.n_in;
    j.r.N0 = 0; j.r.m0 = 0; j.r.n_m = n_model;
    j.r.up = r.in.up; j.r.down = r.in.down; j.r.half = r.in.half; j.r.P = r.in.P; j.r.P_ld = r.in.P_ld; j.r.tab = r.in_tab;
    j.r.C = n_ch; j.r.dst = dst; j.r.dst_ld = 0;
    j.n_peak = n_peak; j.level = level;
    return j;
}

int session_rate_ingest(css_ctx* h, const SessionIngestJob* jobs, int n, hipStream_t st) {
    int launches = 0;
    const bool ok = launch_session_ingest_multi(jobs, n, st, &launches);
    h->rate_ingest_launches += launches;
    if (!ok) return fail(h, CSS_ERR_HIP, "the session ingest kernel's LDS could not be reserved");
    HIPCHK(h, hipGetLastError());
    return CSS_OK;
}

int session_output_on(css_ctx* h, const float* wav, int64_t wav_ld, const SessRate& r, hipStream_t st) {
    const int S = h->d.num_spks;
    const int64_t ld = pad4(r.n_out);
    const size_t rows_b = al256((size_t)S * (size_t)ld * sizeof(float));
    if (h->rate_out.cap < 256 + rows_b + (r.wav16 ? (size_t)S * (size_t)r.n_out * sizeof(int16_t) : 0))
        return fail(h, CSS_ERR_STATE, "internal: the session output was not prepared");
    unsigned int* pk = h->rate_out.as<unsigned int>();
    float* rows = (float*)((char*)h->rate_out.p + 256);
    int16_t* o16 = (int16_t*)((char*)h->rate_out.p + 256 + rows_b);
    HIPCHK(h, hipMemsetAsync(pk, 0, (size_t)S * sizeof(unsigned int), st));
    SessionOutputJob j{};
    j.src = wav; j.src_ld = wav_ld; j.n = h->plan.n_out; j.n_m = r.n_out;
    j.up = r.out.up; j.down = r.out.down; j.half = r.out.half; j.P = r.out.P; j.P_ld = r.out.P_ld; j.tab = r.out_tab;
    j.dst = rows; j.dst_ld = ld; j.peak = pk;
    {
        CSS_PROF(CSS_PROF_ENCODE, st);
        if (!launch_session_output(j, S, st)) return fail(h, CSS_ERR_HIP, "the session output kernel's LDS could not be reserved");
        h->rate_output_launches += 1;
        if (r.wav16) launch_encode_pcm16_with_peaks(rows, ld, S, r.n_out, pk, o16, r.n_out, st);
    }
    if (r.wav16) {
        HIPCHK(h, hipMemcpy2DAsync(r.wav16, (size_t)r.cap * sizeof(int16_t), o16, (size_t)r.n_out * sizeof(int16_t),
                                   (size_t)r.n_out * sizeof(int16_t), S, hipMemcpyDeviceToHost, st));
        if (r.peaks) HIPCHK(h, hipMemcpyAsync(r.peaks, pk, (size_t)S * sizeof(float), hipMemcpyDeviceToHost, st));
    } else if (int rc = waveforms_out(h, rows, ld, r.wav, r.cap, 0, r.n_out, st)) {
        return rc;
    }
    HIPCHK(h, hipGetLastError());
    return CSS_OK;
}

int css_session_rate_samples(const CssModelDesc* desc, const CssRunCfg* cfg, const CssSessionRate* rate, int64_t n_in,
                             int64_t* n_model, int64_t* n_out_model, int64_t* n_out) {
    if (!desc || !cfg || !rate || !n_model || !n_out_model || !n_out || n_in < 1 || n_in > RATE_N_MAX) return CSS_ERR_INVALID_ARG;
    bool in_on, out_on;
    ResampleRatio in{}, out{};
    if (!side_ratio(rate->in_up, rate->in_down, &in_on, &in) || !side_ratio(rate->out_up, rate->out_down, &out_on, &out))
        return CSS_ERR_INVALID_ARG;
    if (validate_desc(*desc)) return CSS_ERR_INVALID_ARG;
    const int64_t nm = in_on ? resample_count(in, n_in, true) : n_in;
    CssPlan pl{};
    CssRunCfg c = *cfg;
    c.w_first = c.w_mid = c.w_last = nullptr;   // (the plan's sizes do not depend on the windows)
    if (plan_impl(*desc, c, nm, &pl) != CSS_OK) return CSS_ERR_INVALID_ARG;
    *n_model = nm;
    *n_out_model = pl.n_out;
    *n_out = out_on ? resample_count(out, pl.n_out, true) : pl.n_out;
    return CSS_OK;
}

int css_run_rate(css_handle_t h, const float* pcm_host, int64_t n_in, int32_t n_ch, const CssRunCfg* cfg,
                 const CssSessionRate* rate, float* wav_host, int64_t cap) {
    if (!h || !pcm_host || !wav_host) return fail(h, CSS_ERR_INVALID_ARG, "null argument");
    return run_rate(h, pcm_host, nullptr, n_in, n_ch, cfg, rate, wav_host, nullptr, nullptr, cap);
}

int css_run_pcm16_rate(css_handle_t h, const int16_t* const* planes_host, int64_t n_in, int32_t n_ch, const CssRunCfg* cfg,
                       const CssSessionRate* rate, int16_t* wav_pcm16_host, int64_t cap, float* peaks_host) {
    if (!h || !planes_host || !wav_pcm16_host) return fail(h, CSS_ERR_INVALID_ARG, "null argument");
    return run_rate(h, nullptr, planes_host, n_in, n_ch, cfg, rate, nullptr, wav_pcm16_host, peaks_host, cap);
}

int css_run_enqueue_rate(css_handle_t h, const float* pcm_host, int64_t n_in, int32_t n_ch, const CssRunCfg* cfg,
                         const CssSessionRate* rate, float* wav_host, int64_t cap) {
    if (!h || !pcm_host || !wav_host) return fail(h, CSS_ERR_INVALID_ARG, "null argument");
    return enqueue_rate(h, pcm_host, nullptr, n_in, n_ch, cfg, rate, wav_host, nullptr, nullptr, cap);
}

int css_run_enqueue_pcm16_rate(css_handle_t h, const int16_t* const* planes_host, int64_t n_in, int32_t n_ch, const CssRunCfg* cfg,
                               const CssSessionRate* rate, int16_t* wav_pcm16_host, int64_t cap, float* peaks_host) {
    if (!h || !planes_host || !wav_pcm16_host) return fail(h, CSS_ERR_INVALID_ARG, "null argument");
    return enqueue_rate(h, nullptr, planes_host, n_in, n_ch, cfg, rate, nullptr, wav_pcm16_host, peaks_host, cap);
}

int css_session_rate_stats(css_handle_t h, int64_t* ingest_launches, int64_t* output_launches, int64_t* sessions) {
    if (!h || !ingest_launches || !output_launches || !sessions) return fail(h, CSS_ERR_INVALID_ARG, "null argument");
    *ingest_launches = h->rate_ingest_launches;
    *output_launches = h->rate_output_launches;
    *sessions = h->rate_sessions;
    return CSS_OK;
}
