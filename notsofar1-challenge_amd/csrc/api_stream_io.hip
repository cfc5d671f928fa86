// A stream with a rate ratio (css_stream_set_rate, include/css_mi355_rate.h) takes its pushes at the capture rate:
// a piece is copied as the caller laid it out into the stream's device staging and ONE launch per round (resample.hip) filters,
// decimates and de-interleaves the rate streams' pieces into their windows.  Everything behind the window is unchanged and
// counts model-rate samples; the call's checks are evaluated on the model-rate samples its inputs make computable.
// A stream with an output format (css_stream_set_output, include/css_mi355_stream_out.h) also writes the samples
// that became final at the playback rate, as float32 or PCM16, into the buffer bound to it: ONE table launch per round
// (resample.hip stream_output_kernel) between tail() and the downloads reads the round's final samples where tail() left them,
// and the converted samples go from the stream's device staging to the caller's memory.  The float download is skipped when
// the call's out_host is NULL.  Every stream keeps the running peak of its final samples: the kernel forms it for a stream with
// an output format, the host from the downloaded samples for every other one (no launch, no copy is added to that path).
#include "api_stream.hpp"

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

// The three ways piece [done, done + n_in) of a push's item reaches the window at `win` (n model-rate samples):
//   float32: the piece is transposed on the host into the stream's staging buffer and uploaded from there; the caller synchronises
//            once per round (*host_staging), because the next round reuses that buffer.
//   int16:   the piece is copied as it is from the caller's memory into the stream's device staging (one contiguous copy
//            for an interleaved piece, one 2-D copy for a planar one) and ONE table launch per round converts all streams'
//            pieces into their windows (`ing`; stream.hip stream_ingest_pcm16_kernel).  No host buffer is reused, the next round's
//            copy into the staging is ordered behind the launch on the stream: no synchronise but the one that ends the call.
//            (Nothing else leans on the per-round synchronise: the hand-off's page-locked staging is per round of a call, and
//            every device buffer the rounds share is written and read in stream order.)
//   a rate stream (either kind of call): the piece, cut in INPUT samples, is copied as it is into the stream's device staging
//            and ONE table launch per round resamples all rate streams' pieces into their windows (`rsj`; resample.hip
//            stream_ingest_resample_kernel); the rate-less items of the call take their own route above.  No host buffer,
//            no synchronise of its own.
int stage_piece(css_ctx* h, StreamState* s, const PushItem& p, bool pcm16, bool planar, int64_t done, int64_t n_in, int64_t n, float* win,
                std::vector<ResampleJob>* rsj, std::vector<StreamIngestPcm16>* ing, bool* host_staging) {
    const int C = s->n_ch;
    const size_t el = pcm16 ? sizeof(int16_t) : sizeof(float);
    // `cnt` samples per channel as the caller laid them out into a device staging whose planes, if planar, are plane_ld apart
    auto as_it_is = [&](void* stage, int64_t plane_ld, int64_t cnt) {
        const char* src = pcm16 ? (const char*)p.i16 : (const char*)p.f32;
        return planar ? hipMemcpy2DAsync(stage, (size_t)plane_ld * el, src + (size_t)done * el, (size_t)p.channel_stride * el, (size_t)cnt * el,
                                         (size_t)C, hipMemcpyHostToDevice, h->stream)
                      : hipMemcpyAsync(stage, src + (size_t)done * C * el, (size_t)cnt * C * el, hipMemcpyHostToDevice, h->stream);
    };
    if (RateStream* q = s->rate.get()) {
        HIPCHK(h, as_it_is(q->stage.p, q->max_in, n_in));
        rsj->push_back(rate_job(s, pcm16, planar, n_in, s->n_pushed + n, win, false));
    } else if (pcm16) {
        HIPCHK(h, as_it_is(s->pcm16_stage.p, s->piece, n));
        ing->push_back(StreamIngestPcm16{(const int16_t*)s->pcm16_stage.p, planar ? s->piece : 0, n, C, win, s->WS});
    } else {
        // samples -> the window, channel-major (a plain copy: the transform reads the same values css_run's does)
        *host_staging = true;
        const float* src = p.f32 + done * C;
        for (int ch = 0; ch < C; ++ch) {
            float* d = s->host_cm.data() + (size_t)ch * n;
            for (int64_t i = 0; i < n; ++i) d[i] = src[i * C + ch];
        }
        HIPCHK(h, hipMemcpy2DAsync(win, (size_t)s->WS * sizeof(float), s->host_cm.data(),
                                   (size_t)n * sizeof(float), (size_t)n * sizeof(float), (size_t)C, hipMemcpyHostToDevice, h->stream));
    }
    return CSS_OK;
}

// ---- output format ---------------------------------------------------------------------------------------------------------
// output samples written once `n_final` model-rate samples are final (finished: of the whole recording)
static int64_t output_count(const OutputStream* o, int64_t n_final, bool finished) {
    return o->unity ? n_final : resample_count(o->r, n_final, finished);
}
static size_t output_el(const OutputStream* o) { return o->cfg.pcm16 ? sizeof(int16_t) : sizeof(float); }
// a row of the staging that holds what `n` final samples can make in one round (the resampler's lag released at finish included)
static int64_t output_stage_ld(const OutputStream* o, int64_t n) {
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

// What a polyphase resampler of ratio r over `rows` rows keeps on the device: *H carried samples per row in two zeroed generations
// and the taps by phase.  Ends in a synchronise of the handle's stream (the zero fills; the host's table leaves scope); *e is the
// upload's error or the synchronise's, for the caller's message.
static int resampler_setup(css_ctx* h, const ResampleRatio& r, int rows, int* H, DevBuf hist[2], DevBuf& tab, hipError_t* e) {
    *H = (2 * r.half + r.up - 1) / r.up + 1;
    std::vector<float> taps((size_t)r.L), t((size_t)r.up * r.P_ld);
    resample_taps_f32(r, taps.data());
    resample_phase_table(r, taps.data(), t.data());
    int rc = CSS_OK;
    for (int b = 0; b < 2 && rc == CSS_OK; ++b) rc = ensure(h, hist[b], (size_t)rows * *H * sizeof(float), true);
    if (rc == CSS_OK) rc = ensure(h, tab, t.size() * sizeof(float));
    if (rc == CSS_OK) *e = hipMemcpyAsync(tab.p, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice, h->stream);
    const hipError_t es = hipStreamSynchronize(h->stream);
    if (*e == hipSuccess) *e = es;
    return rc;
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
    q->max_in = (s->piece * r.down + r.half) / r.up + 1;
    hipError_t e = hipSuccess;
    rc = ensure(h, q->stage, (size_t)s->n_ch * q->max_in * sizeof(float));
    if (rc == CSS_OK) rc = resampler_setup(h, r, s->n_ch, &q->H, q->hist, q->tab, &e);
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
        rc = resampler_setup(h, r, S, &o->H, o->hist, o->tab, &e);
    } else {
        const hipError_t es = hipStreamSynchronize(h->stream);   // (the zero fills)
        if (e == hipSuccess) e = es;
    }
    if (rc != CSS_OK) return rc;
    if (e != hipSuccess) return fail(h, CSS_ERR_HIP, std::string("output setup: ") + hipGetErrorString(e));
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
