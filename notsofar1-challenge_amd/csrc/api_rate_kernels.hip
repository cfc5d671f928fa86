// include/css_mi355_rate_kernels.h: the table and session kernels of resample.hip on caller data, one entry per side (unit tests
// of the arithmetic; the companion of api_frontend.hip).  Every entry checks first, then stages in h->stage, makes the launch
// the path makes, downloads every allocation a launch could have written and synchronises.
#include <string>
#include <vector>

#include "api_ctx.hpp"
#include "api_kernel_stage.hpp"   // (Stager, stage_and_upload, download_all)
#include "../../include/css_mi355_rate_kernels.h"

using namespace css;
using namespace css::kstage;

namespace {

constexpr int64_t COUNT_MAX = (int64_t)1 << 40;  // sample counts and positions: their products with `down` stay far inside int64
constexpr int64_t N_M_MAX = (int64_t)1 << 24;    // outputs per job: the grids stay small

bool in_range(int64_t v) { return v >= 0 && v <= COUNT_MAX; }

// the phase table of a ratio on the host, as the handle builds it
std::vector<float> phase_table(const ResampleRatio& r) {
    std::vector<float> taps((size_t)r.L), tab((size_t)r.up * r.P_ld);
    resample_taps_f32(r, taps.data());
    resample_phase_table(r, taps.data(), tab.data());
    return tab;
}

}  // namespace

extern "C" {

int css_rate_ingest_host(css_handle_t h, int32_t form, CssRateIngestJob* jobs, int32_t n_jobs) {
    CSS_DRAIN(h);
    if (!h) return CSS_ERR_INVALID_ARG;
    auto bad = [&](const char* what) { return fail(h, CSS_ERR_INVALID_ARG, std::string("css_rate_ingest_host: ") + what); };
    if (!jobs) return bad("null argument");
    if (form < 0 || form > 1) return bad("form must be 0 (stream ingest) or 1 (session ingest)");
    if (n_jobs < 1 || n_jobs > CSS_RATE_KERNEL_JOBS) return bad("1 .. 64 jobs");
    std::vector<ResampleRatio> rr((size_t)n_jobs);
    for (int i = 0; i < n_jobs; ++i) {
        const CssRateIngestJob& j = jobs[i];
        if (j.C < 1 || j.C > 64) return bad("C must be 1 .. 64");
        if (!resample_ratio(j.up, j.down, &rr[(size_t)i])) return bad("a ratio the library refuses");
        if (!(form == 0 ? resample_fits(rr[(size_t)i], j.C) : session_ingest_fits(rr[(size_t)i], j.C)))
            return bad("the ratio's tile does not fit a workgroup's LDS");
        if (j.H < 0 || j.H > (1 << 20) || !in_range(j.n) || !in_range(j.n_m) || !in_range(j.m0) || !in_range(j.N0) || !in_range(j.n_peak))
            return bad("H, n, n_m, m0, N0, n_peak must lie in [0, 2^40] (H in [0, 2^20])");
        if (j.n_m > N_M_MAX) return bad("n_m above 2^24");
        if (j.src_offset < 0 || j.src_offset > 7) return bad("src_offset must be 0 .. 7 elements");
        if (j.plane_ld < 0 || (j.plane_ld > 0 && j.plane_ld < j.n)) return bad("plane_ld must be 0 (interleaved) or cover n");
        const int64_t src_need = j.n == 0 ? 0 : (j.plane_ld > 0 ? (int64_t)(j.C - 1) * j.plane_ld + j.n : j.n * j.C);
        if (j.src_elems < src_need || j.src_elems < 0 || j.src_elems > HOST_CAP) return bad("src is shorter than its description");
        if (j.src_elems > 0 && !j.src) return bad("null argument");
        const int64_t hist_need = (int64_t)j.C * j.H;
        if (j.hist_elems < hist_need || j.hist_elems > HOST_CAP) return bad("the history is shorter than its description");
        if (hist_need > 0 && !j.hist_in) return bad("null argument");
        if (!j.dst || j.dst_floats < 1 || j.dst_floats > HOST_CAP) return bad("dst: 1 .. 2^28 floats");
        if (form == 0) {
            if (j.has_hist_out < 0 || j.has_hist_out > 1) return bad("has_hist_out is 0 or 1");
            if (j.has_hist_out && (!j.hist_out || j.hist_out == j.hist_in)) return bad("hist_out must be another array than hist_in");
            if (j.dst_col < 0 || j.dst_col > 3) return bad("dst_col must be 0 .. 3 floats");
            if (j.dst_ld < j.dst_col + j.n_m || j.dst_ld > HOST_CAP) return bad("dst_ld must cover dst_col + n_m");
            if (j.dst_floats < j.dst_col + (int64_t)(j.C - 1) * j.dst_ld + j.n_m) return bad("dst is shorter than its description");
        } else {
            if (j.has_hist_out || j.dst_col || j.dst_ld) return bad("form 1: has_hist_out, dst_col and dst_ld must be 0");
            if (j.m0 + j.n_m > HOST_CAP || j.dst_floats < (j.m0 + j.n_m) * j.C) return bad("dst is shorter than its description");
        }
    }

    struct At { size_t tab, src, hin, hout, dst, level; };
    std::vector<At> at((size_t)n_jobs);
    std::vector<std::vector<float>> tabs((size_t)n_jobs);
    Stager sg;
    for (int i = 0; i < n_jobs; ++i) {
        CssRateIngestJob& j = jobs[i];
        At& a = at[(size_t)i];
        const size_t el = j.is_int16 ? sizeof(int16_t) : sizeof(float);
        float* const ho = j.has_hist_out ? j.hist_out : nullptr;
        tabs[(size_t)i] = phase_table(rr[(size_t)i]);
        // (regions, not arr(): a job's launch is handed every one of these, an empty history included)
        a.tab = sg.region(tabs[(size_t)i].size() * sizeof(float), tabs[(size_t)i].data(), nullptr);
        a.src = sg.region((size_t)j.src_elems * el, j.src, nullptr, (size_t)j.src_offset * el);
        a.hin = sg.region((size_t)j.hist_elems * sizeof(float), j.hist_in, nullptr);
        a.hout = sg.region((size_t)j.hist_elems * sizeof(float), ho, ho);
        a.dst = sg.region((size_t)j.dst_floats * sizeof(float), j.dst, j.dst);
        a.level = sg.region(sizeof(uint32_t), &j.level_before, &j.level_after);
    }
    char* base = nullptr;
    int rc;
    if ((rc = stage_and_upload(h, sg, &base)) != CSS_OK) return rc;
    hipStream_t st = h->stream;
    std::vector<ResampleJob> rj((size_t)n_jobs);
    std::vector<SessionIngestJob> sj((size_t)n_jobs);
    for (int i = 0; i < n_jobs; ++i) {
        const CssRateIngestJob& j = jobs[i];
        const At& a = at[(size_t)i];
        const ResampleRatio& r = rr[(size_t)i];
        const size_t el = j.is_int16 ? sizeof(int16_t) : sizeof(float);
        char* src_d = base + a.src + (size_t)j.src_offset * el;
        ResampleJob& e = rj[(size_t)i];
        e = ResampleJob{};
        e.src = src_d; e.is_i16 = j.is_int16 ? 1 : 0; e.plane_ld = j.plane_ld; e.n = j.n;
        e.hist_in = (const float*)(base + a.hin); e.hist_out = j.has_hist_out ? (float*)(base + a.hout) : nullptr; e.H = j.H;
        e.N0 = j.N0; e.m0 = j.m0; e.n_m = j.n_m;
        e.up = r.up; e.down = r.down; e.half = r.half; e.P = r.P; e.P_ld = r.P_ld; e.tab = (const float*)(base + a.tab);
        e.C = j.C; e.dst = (float*)(base + a.dst) + j.dst_col; e.dst_ld = j.dst_ld;
        sj[(size_t)i] = SessionIngestJob{e, j.n_peak, (unsigned int*)(base + a.level)};
    }
    const bool ok = form == 0 ? launch_stream_ingest_resample_multi(rj.data(), n_jobs, st)
                              : launch_session_ingest_multi(sj.data(), n_jobs, st, nullptr);
    if (!ok) {
        hipStreamSynchronize(st);
        return fail(h, CSS_ERR_HIP, "css_rate_ingest_host: the kernel's LDS could not be reserved");
    }
    return download_all(h, sg, base);
}

int css_rate_output_host(css_handle_t h, int32_t form, int32_t S, CssRateOutputJob* jobs, int32_t n_jobs) {
    CSS_DRAIN(h);
    if (!h) return CSS_ERR_INVALID_ARG;
    auto bad = [&](const char* what) { return fail(h, CSS_ERR_INVALID_ARG, std::string("css_rate_output_host: ") + what); };
    if (!jobs) return bad("null argument");
    if (form < 0 || form > 1) return bad("form must be 0 (stream output) or 1 (session output)");
    if (n_jobs < 1 || n_jobs > CSS_RATE_KERNEL_JOBS || (form == 1 && n_jobs != 1)) return bad("1 .. 64 jobs, one for form 1");
    if (S < 1 || S > 64) return bad("S must be 1 .. 64");
    std::vector<ResampleRatio> rr((size_t)n_jobs);
    for (int i = 0; i < n_jobs; ++i) {
        const CssRateOutputJob& j = jobs[i];
        ResampleRatio& r = rr[(size_t)i];
        const bool unity = form == 0 && j.up == 1 && j.down == 1;
        r = ResampleRatio{1, 1, 0, 0, 0, 0};
        if (!unity && !resample_ratio(j.up, j.down, &r)) return bad("a ratio the library refuses");
        if (!unity && !stream_output_fits(r)) return bad("the ratio's tile does not fit a workgroup's LDS");
        if (j.H < 0 || j.H > (1 << 20) || !in_range(j.n) || !in_range(j.n_m) || !in_range(j.m0) || !in_range(j.N0))
            return bad("H, n, n_m, m0, N0 must lie in [0, 2^40] (H in [0, 2^20])");
        if (j.n_m > N_M_MAX) return bad("n_m above 2^24");
        if (unity && j.n_m > j.n) return bad("1 / 1 copies: n_m <= n");
        if (form == 1 && (j.H || j.N0 || j.m0 || j.pcm16 || j.has_hist_out)) return bad("form 1: H, N0, m0, pcm16 and has_hist_out must be 0");
        if (j.pcm16 < 0 || j.pcm16 > 1 || j.has_hist_out < 0 || j.has_hist_out > 1) return bad("pcm16 and has_hist_out are 0 or 1");
        if (j.src_ld < j.n || j.src_ld > HOST_CAP) return bad("src_ld must cover n");
        if (!j.src || j.src_floats < 1 || j.src_floats > HOST_CAP || j.src_floats < (int64_t)(S - 1) * j.src_ld + j.n)
            return bad("src is shorter than its description");
        const int64_t hist_need = (int64_t)S * j.H;
        if (j.hist_elems < hist_need || j.hist_elems > HOST_CAP) return bad("the history is shorter than its description");
        if (hist_need > 0 && !j.hist_in) return bad("null argument");
        if (j.has_hist_out && (!j.hist_out || j.hist_out == j.hist_in)) return bad("hist_out must be another array than hist_in");
        const int64_t per16 = j.pcm16 ? 8 : 4;
        if (j.dst_ld < j.n_m || j.dst_ld % per16 || j.dst_ld > HOST_CAP) return bad("dst_ld must cover n_m and be a multiple of 16 bytes");
        if (!j.dst || j.dst_elems < 1 || j.dst_elems > HOST_CAP || j.dst_elems < (int64_t)(S - 1) * j.dst_ld + j.n_m)
            return bad("dst is shorter than its description");
        if (!j.peak || (form == 0 && !j.clipped)) return bad("null argument");
    }

    struct At { size_t tab, src, hin, hout, dst, peak, clip; };
    std::vector<At> at((size_t)n_jobs);
    std::vector<std::vector<float>> tabs((size_t)n_jobs);
    Stager sg;
    for (int i = 0; i < n_jobs; ++i) {
        const CssRateOutputJob& j = jobs[i];
        At& a = at[(size_t)i];
        float* const ho = j.has_hist_out ? j.hist_out : nullptr;
        uint64_t* const cl = form == 0 ? j.clipped : nullptr;
        if (rr[(size_t)i].L > 0) tabs[(size_t)i] = phase_table(rr[(size_t)i]);
        // (regions, not arr(): a job's launch is handed every one of these but an empty table)
        a.tab = sg.region(tabs[(size_t)i].size() * sizeof(float), tabs[(size_t)i].data(), nullptr);
        a.src = sg.region((size_t)j.src_floats * sizeof(float), j.src, nullptr);
        a.hin = sg.region((size_t)j.hist_elems * sizeof(float), j.hist_in, nullptr);
        a.hout = sg.region((size_t)j.hist_elems * sizeof(float), ho, ho);
        a.dst = sg.region((size_t)j.dst_elems * (j.pcm16 ? sizeof(int16_t) : sizeof(float)), j.dst, j.dst);
        a.peak = sg.region((size_t)S * sizeof(uint32_t), j.peak, j.peak);
        a.clip = sg.region((size_t)S * sizeof(uint64_t), cl, cl);
    }
    char* base = nullptr;
    int rc;
    if ((rc = stage_and_upload(h, sg, &base)) != CSS_OK) return rc;
    hipStream_t st = h->stream;
    std::vector<StreamOutputJob> oj((size_t)n_jobs);
    for (int i = 0; i < n_jobs; ++i) {
        const CssRateOutputJob& j = jobs[i];
        const At& a = at[(size_t)i];
        const ResampleRatio& r = rr[(size_t)i];
        StreamOutputJob& e = oj[(size_t)i];
        e = StreamOutputJob{};
        e.src = (const float*)(base + a.src); e.src_ld = j.src_ld; e.n = j.n;
        e.hist_in = (const float*)(base + a.hin); e.hist_out = j.has_hist_out ? (float*)(base + a.hout) : nullptr; e.H = j.H;
        e.N0 = j.N0; e.m0 = j.m0; e.n_m = j.n_m;
        e.up = r.up; e.down = r.down; e.half = r.half; e.P = r.P; e.P_ld = r.P_ld;
        e.tab = tabs[(size_t)i].empty() ? nullptr : (const float*)(base + a.tab);
        e.pcm16 = j.pcm16; e.gain = j.gain;
        e.dst = base + a.dst; e.dst_ld = j.dst_ld;
        e.peak = (unsigned int*)(base + a.peak); e.clipped = (unsigned long long*)(base + a.clip);
    }
    bool ok;
    if (form == 0) {
        ok = launch_stream_output_multi(oj.data(), n_jobs, S, st, nullptr);
    } else {
        const StreamOutputJob& o = oj[0];
        SessionOutputJob e{};
        e.src = o.src; e.src_ld = o.src_ld; e.n = o.n; e.n_m = o.n_m;
        e.up = o.up; e.down = o.down; e.half = o.half; e.P = o.P; e.P_ld = o.P_ld; e.tab = o.tab;
        e.dst = (float*)o.dst; e.dst_ld = o.dst_ld; e.peak = o.peak;
        ok = launch_session_output(e, S, st);
    }
    if (!ok) {
        hipStreamSynchronize(st);
        return fail(h, CSS_ERR_HIP, "css_rate_output_host: the kernel's LDS could not be reserved");
    }
    return download_all(h, sg, base);
}

}  // extern "C"
