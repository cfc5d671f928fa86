// include/css_mi355_nemo_chunk.h: a NeMo stream's frame history and the chunks written out of it (DESIGN.md 7b "NeMo chunks out of
// the frame history").  The ring is HandoffStream::ring with hist_frames (api_stream.hpp); the mel launch of a committed round fills
// it (api_stream_handoff.hip handoff_round_format, nemo_stream.hip nemo_mel_multi_kernel).  css_stream_nemo_chunks is
// css_stream_windows' shape: every item checked, then one table launch per NEMO_CHUNK_MULTI_MAX items (nemo_chunk_kernel) and one
// synchronise.  css_nemo_chunk_host is the same kernel on a caller's ring (the conventions of api_stream_kernels.hip).
#include <cmath>

#include "api_stream.hpp"
#include "api_kernel_stage.hpp"   // (Stager, arr_ok, stage_and_upload, download_all)

using namespace css;
using namespace css::kstage;

namespace {

static_assert(NEMO_CHUNK_MULTI_MAX == CSS_NEMO_CHUNK_TABLE && NEMO_CHUNK_MAX_WIDTH == CSS_NEMO_CHUNK_MAX_WIDTH, "the header states the table's size and the width");
static_assert(CSS_WINDOW_F32 == 0 && CSS_WINDOW_F16 == 1, "the header states the dtype values");
static_assert(sizeof(CssNemoChunkArray) == sizeof(CssKArray), "the stager's array descriptor");
CssKArray ka(const CssNemoChunkArray& a) { return CssKArray{a.p, a.elems}; }

// What is wrong with the fields a chunk request (CssStreamNemoChunk, CssNemoChunkJob) shares, for a history of `hist` frames that
// ends at frame J, or null.  out: the address the chunk's first element goes to (the kernel entry: its offset in bytes).
template <typename W>
const char* chunk_refusal(const W& w, int64_t hist, int64_t J, uintptr_t out) {
    if (w.dtype != CSS_WINDOW_F32 && w.dtype != CSS_WINDOW_F16) return "dtype is 0 (float32) or 1 (float16)";
    if (w.normalize != CSS_NEMO_CHUNK_RAW && w.normalize != CSS_NEMO_CHUNK_PER_FEATURE) return "normalize is CSS_NEMO_CHUNK_RAW or CSS_NEMO_CHUNK_PER_FEATURE";
    if (w.n_frames < 1 || w.width < w.n_frames || w.width > CSS_NEMO_CHUNK_MAX_WIDTH) return "1 <= n_frames <= width <= 3000";
    if (w.ld < w.width) return "ld < width";
    if (!std::isfinite(w.pad_value)) return "pad_value is not finite";
    if (w.first_frame < std::max<int64_t>(J - hist, 0) || w.first_frame > J - w.n_frames) return "frames outside the history (css_stream_nemo_history_range)";
    if (out % (w.dtype == CSS_WINDOW_F16 ? 2 : 4)) return "out_dev is not aligned to its element size";
    return nullptr;
}

template <typename W>
NemoChunkItem chunk_item(const W& w, const float* ring, int64_t hist, int n_mels, void* out, float* mean, float* stdv) {
    NemoChunkItem e{};
    e.ring = ring; e.out = out; e.mean = mean; e.stdv = stdv;
    e.hist = hist; e.ld = w.ld; e.first = w.first_frame;
    e.pad_value = w.pad_value;
    e.n_frames = w.n_frames; e.width = w.width; e.n_mels = n_mels; e.f16 = w.dtype == CSS_WINDOW_F16 ? 1 : 0; e.normalize = w.normalize;
    return e;
}

// the tables of a call, NEMO_CHUNK_MULTI_MAX items each
int launch_tables(const std::vector<NemoChunkItem>& w, hipStream_t st) {
    int launches = 0;
    for (size_t i0 = 0; i0 < w.size(); i0 += NEMO_CHUNK_MULTI_MAX, ++launches)
        launch_nemo_chunks(w.data() + i0, (int)std::min<size_t>(NEMO_CHUNK_MULTI_MAX, w.size() - i0), st);
    return launches;
}

}  // namespace

extern "C" {

int css_stream_nemo_history_open(css_handle_t h, int32_t id, int32_t history_frames) {
    StreamState* s = nullptr;
    int rc = check_stream_call(h, id, &s);
    if (rc != CSS_OK) return rc;
    if (history_frames < 32 || history_frames > (1 << 20)) return fail(h, CSS_ERR_INVALID_ARG, "history_frames is 32 .. 2^20");
    if (!s->ho) return fail(h, CSS_ERR_STATE, "the NeMo hand-off of this stream is off (css_stream_nemo_open)");
    if (!s->ho->nemo) return fail(h, CSS_ERR_STATE, "a Whisper hand-off stream has no NeMo history: its frame history is css_stream_window_open's");
    if (s->ho->hist_frames) return fail(h, CSS_ERR_STATE, "this stream has a frame history already");
    if (s->n_pushed > 0 || s->finished || (s->rate && s->rate->n_in > 0))
        return fail(h, CSS_ERR_STATE, "the frame history is switched on before the stream's first sample");
    HIPCHK(h, hipSetDevice(h->device));
    HandoffStream* o = s->ho.get();
    DevBuf ring;
    if ((rc = ensure(h, ring, (size_t)h->d.num_spks * o->cfg.n_mels * (size_t)history_frames * sizeof(float), true)) != CSS_OK) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    o->ring = std::move(ring);
    o->hist_frames = history_frames;
    return CSS_OK;
}

int css_stream_nemo_history_range(css_handle_t h, int32_t id, int64_t* first_frame, int64_t* end_frame) {
    if (!h) return CSS_ERR_INVALID_ARG;
    StreamState* s = get_stream(h, id);
    if (!s || !first_frame || !end_frame) return fail(h, CSS_ERR_INVALID_ARG, "no open stream with this id / null argument");
    if (!s->ho || !s->ho->nemo || !s->ho->hist_frames) return fail(h, CSS_ERR_STATE, "this stream has no NeMo frame history (css_stream_nemo_history_open)");
    for (int k = 0; k < h->d.num_spks; ++k) {
        const int64_t J = s->ho->m.J[(size_t)k];
        first_frame[k] = std::max<int64_t>(J - s->ho->hist_frames, 0);
        end_frame[k] = J;
    }
    return CSS_OK;
}

int css_stream_nemo_chunks(css_handle_t h, CssStreamNemoChunk* items, int32_t n_items, int32_t* launches) {
    if (!h) return CSS_ERR_INVALID_ARG;
    if (n_items < 0 || (n_items > 0 && !items)) return fail(h, CSS_ERR_INVALID_ARG, "bad argument");
    if (const char* q = queued_refusal(h)) return fail(h, CSS_ERR_STATE, q);
    std::vector<NemoChunkItem> w((size_t)n_items);
    std::vector<size_t> stats_at((size_t)n_items);
    size_t stats_floats = 0;
    for (int32_t i = 0; i < n_items; ++i) {
        const CssStreamNemoChunk& p = items[i];
        auto refuse = [&](const std::string& msg) { return refuse_item(h, CSS_ERR_INVALID_ARG, (size_t)i, p.id, msg); };
        const StreamState* s = get_stream(h, p.id);
        if (!s) return refuse("no open stream with this id");
        const HandoffStream* o = s->ho.get();
        if (!o || !o->nemo || !o->hist_frames) return refuse("the stream has no NeMo frame history (css_stream_nemo_history_open)");
        if (p.speaker < 0 || p.speaker >= h->d.num_spks) return refuse("speaker out of range");
        if (p.reserved != 0) return refuse("reserved must be 0");
        if (!p.out_dev) return refuse("out_dev is null");
        if (const char* bad = chunk_refusal(p, o->hist_frames, o->m.J[(size_t)p.speaker], (uintptr_t)p.out_dev)) return refuse(bad);
        const int64_t nm = o->cfg.n_mels;
        w[(size_t)i] = chunk_item(p, (const float*)o->ring.p + p.speaker * nm * o->hist_frames, o->hist_frames, (int)nm, p.out_dev, nullptr, nullptr);
        stats_at[(size_t)i] = stats_floats;
        stats_floats += 2 * (size_t)nm;
    }
    if (launches) *launches = 0;
    if (n_items == 0) return CSS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    HandoffCtx* c = h->handoff;   // (a stream with a frame history has the hand-off on)
    int rc;
    if ((rc = ensure(h, c->chunk_stats, stats_floats * sizeof(float))) != CSS_OK) return rc;
    if (c->chunk_pin.cap < stats_floats * sizeof(float)) HIPCHK(h, c->chunk_pin.alloc(stats_floats * sizeof(float)));
    for (int32_t i = 0; i < n_items; ++i) {
        w[(size_t)i].mean = (float*)c->chunk_stats.p + stats_at[(size_t)i];
        w[(size_t)i].stdv = w[(size_t)i].mean + w[(size_t)i].n_mels;
    }
    const int n_launch = launch_tables(w, h->stream);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(c->chunk_pin.p, c->chunk_stats.p, stats_floats * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int32_t i = 0; i < n_items; ++i) {
        const CssStreamNemoChunk& p = items[i];
        if (p.normalize != CSS_NEMO_CHUNK_PER_FEATURE) continue;
        const size_t nm = (size_t)w[(size_t)i].n_mels;
        const float* st = c->chunk_pin.as<float>() + stats_at[(size_t)i];
        if (p.mean_host) std::memcpy(p.mean_host, st, nm * sizeof(float));
        if (p.std_host) std::memcpy(p.std_host, st + nm, nm * sizeof(float));
    }
    if (launches) *launches = n_launch;
    return CSS_OK;
}

int css_nemo_chunk_host(css_handle_t h, CssNemoChunkJob* jobs, int32_t n_jobs) {
    CSS_DRAIN(h);
    if (!h) return CSS_ERR_INVALID_ARG;
    auto bad = [&](int i, const std::string& what) { return fail(h, CSS_ERR_INVALID_ARG, "css_nemo_chunk_host: job " + std::to_string(i) + ": " + what); };
    if (!jobs) return fail(h, CSS_ERR_INVALID_ARG, "css_nemo_chunk_host: null argument");
    if (n_jobs < 1 || n_jobs > CSS_STREAM_KERNEL_JOBS) return fail(h, CSS_ERR_INVALID_ARG, "css_nemo_chunk_host: 1 .. 64 jobs");
    for (int i = 0; i < n_jobs; ++i) {
        const CssNemoChunkJob& j = jobs[i];
        if (j.n_mels != 80 && j.n_mels != 128) return bad(i, "n_mels must be 80 or 128");
        if (j.hist < 1 || j.hist > HOST_CAP / j.n_mels) return bad(i, "hist must be 1 .. 2^28 / n_mels (the ring is staged whole)");
        if (j.end_frame < 0 || j.end_frame > ((int64_t)1 << 40)) return bad(i, "end_frame out of range");
        if (j.out_offset < 0 || j.out_offset > HOST_CAP) return bad(i, "out_offset out of range");
        if (j.ld < 0 || j.ld > HOST_CAP / j.n_mels) return bad(i, "ld must be 0 .. 2^28 / n_mels");
        if (const char* why = chunk_refusal(j, j.hist, j.end_frame, 0)) return bad(i, why);
        if (!arr_ok(ka(j.ring), (int64_t)j.n_mels * j.hist) || !arr_ok(ka(j.out), j.out_offset + (int64_t)(j.n_mels - 1) * j.ld + j.width) ||
            !arr_ok(ka(j.mean), j.n_mels) || !arr_ok(ka(j.std), j.n_mels) || !j.ring.p || !j.out.p || !j.mean.p || !j.std.p)
            return bad(i, "an array is null or shorter than its description");
    }
    Stager sg;
    struct At { size_t ring, out, mean, stdv; };
    std::vector<At> at((size_t)n_jobs);
    for (int i = 0; i < n_jobs; ++i) {
        const CssNemoChunkJob& j = jobs[i];
        at[(size_t)i] = At{sg.take(ka(j.ring), 4, false), sg.take(ka(j.out), j.dtype == CSS_WINDOW_F16 ? 2 : 4, true), sg.take(ka(j.mean), 4, true),
                           sg.take(ka(j.std), 4, true)};
    }
    char* base = nullptr;
    int rc;
    if ((rc = stage_and_upload(h, sg, &base)) != CSS_OK) return rc;
    std::vector<NemoChunkItem> w((size_t)n_jobs);
    for (int i = 0; i < n_jobs; ++i) {
        const CssNemoChunkJob& j = jobs[i];
        const At& a = at[(size_t)i];
        w[(size_t)i] = chunk_item(j, (const float*)(base + a.ring), j.hist, j.n_mels, base + a.out + (size_t)j.out_offset * (j.dtype == CSS_WINDOW_F16 ? 2 : 4),
                                  (float*)(base + a.mean), (float*)(base + a.stdv));
    }
    launch_tables(w, h->stream);
    return download_all(h, sg, base);
}

}  // extern "C"
