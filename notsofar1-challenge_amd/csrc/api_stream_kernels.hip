// include/css_mi355_stream_kernels.h: the kernels of stream.hip and the streamed part of handoff.hip on caller data, one entry per
// launcher (unit tests of the kernels; the companion of api_rate_kernels.hip).  Every entry checks first, then stages in
// h->stage, makes the ONE launcher call the path makes, downloads every allocation a launch could have written and synchronises.
#include <algorithm>
#include <string>
#include <vector>

#include "api_ctx.hpp"
#include "api_kernel_stage.hpp"   // (Stager, arr_ok, stage_and_upload, download_all)
#include "stitch_common.hpp"   // (OLA_T: the gate kernel's block of frames)
#include "../../include/css_mi355_stream_kernels.h"
#include "../../include/css_mi355_stream_nemo.h"
#include "../../include/css_mi355_nemo_chunk.h"

using namespace css;
using namespace css::kstage;

namespace {

constexpr int64_t POS_MAX = (int64_t)1 << 40;    // frame and sample positions of a recording

bool pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }
bool pos_ok(int64_t v) { return v >= 0 && v <= POS_MAX; }
static_assert(sizeof(CssStreamNemoArray) == sizeof(CssKArray), "the stager's array descriptor");
CssKArray ka(const CssStreamNemoArray& a) { return CssKArray{a.p, a.elems}; }
static_assert(sizeof(CssNemoChunkArray) == sizeof(CssKArray), "the stager's array descriptor");
CssStreamNemoArray na(const CssNemoChunkArray& a) { return CssStreamNemoArray{a.p, a.elems}; }

// Both append entries: job i is job(i); nemo(i), where the call is css_stream_nemo_append_host, its NeMo part (else null).
template <class Job, class Nemo>
int append_host(css_ctx* h, const char* who, Job job, Nemo nemo, bool is_nemo, int32_t n_jobs, float* operand, int64_t operand_floats) {
    auto bad = [&](const char* what) { return fail(h, CSS_ERR_INVALID_ARG, std::string(who) + ": " + what); };
    if (!operand) return bad("null argument");
    if (n_jobs < 1 || n_jobs > CSS_STREAM_KERNEL_JOBS) return bad("1 .. 64 jobs");
    static_assert(sizeof(HandoffState) == 24, "the header states the state row");
    static_assert(NEMO_TAIL_LD == HANDOFF_TAIL_LD, "the headers state 512 floats for both tails");
    int64_t rows_total = 0;
    std::vector<int64_t> rows((size_t)n_jobs), row0((size_t)n_jobs);
    for (int i = 0; i < n_jobs; ++i) {
        const CssStreamAppendJob& j = job(i);
        if (j.S < 1 || j.S > 4 || j.S != job(0).S) return bad("S must be 1 .. 4, the same for all jobs");
        if (j.pad < 0 || j.pad > 4096) return bad("pad must be 0 .. 4096");
        if (j.drop < 0 || j.drop > 1 || j.closing < 0 || j.closing > 1 || j.preview < 0 || j.preview > 1) return bad("drop, closing and preview are 0 or 1");
        if (!pow2(j.gate_ld) || j.gate_ld > HOST_CAP) return bad("gate_ld must be a power of two");
        if (!pos_ok(j.t_g0) || !pos_ok(j.t_g1) || j.t_g1 < j.t_g0) return bad("t_g1 < t_g0 (or a negative frame count)");
        if (!pos_ok(j.D0) || !pos_ok(j.D1) || j.D1 < j.D0) return bad("D1 < D0 (or a negative sample count)");
        if (j.D0 % 256) return bad("D0 must be a multiple of 256");
        if (j.D1 - j.D0 > ((int64_t)1 << 24)) return bad("D1 - D0 above 2^24");
        if (!pos_ok(j.out_base) || j.out_ld < 0 || j.out_ld > HOST_CAP || j.carry_ld < 0 || j.carry_ld > HOST_CAP)
            return bad("out_base, out_ld and carry_ld must not be negative");
        const int64_t end = std::max(j.D1, 256 * j.t_g1);
        if (end > j.out_base && end - j.out_base > j.out_ld) return bad("out_ld does not reach the round's last sample");
        if (std::min(j.out_base, end) - j.D0 > j.carry_ld) return bad("out_base - D0 > carry_ld");
        if (256 * j.t_g1 - j.D1 > j.carry_ld) return bad("the undecided samples behind D1 do not fit carry_ld");
        if (!j.closing && j.drop && j.D1 > 256 * std::max<int64_t>(j.t_g1 - j.pad, 0)) return bad("an open round decides blocks whose frames are not gated-final");
        const int64_t look = j.drop ? std::min(j.t_g0, std::max<int64_t>(j.D0 / 256 - j.pad - 1, 0)) : j.t_g0;
        if (j.t_g1 - look > j.gate_ld) return bad("the ring is shorter than the frames the round reads");
        if (!arr_ok(j.gate, (int64_t)j.S * j.gate_ld) || !arr_ok(j.out, (int64_t)j.S * j.out_ld) || !arr_ok(j.carry_in, (int64_t)j.S * j.carry_ld) ||
            !arr_ok(j.carry_out, (int64_t)j.S * j.carry_ld) || !arr_ok(j.tail_in, (int64_t)j.S * HANDOFF_TAIL_LD) ||
            !arr_ok(j.tail_out, (int64_t)j.S * HANDOFF_TAIL_LD) || !arr_ok(j.st, j.S) || (j.preview && !arr_ok(j.st_out, j.S)) ||
            !arr_ok(j.act_out, (int64_t)j.S * (j.t_g1 - j.t_g0)) || !arr_ok(j.n_new, j.S) || !j.st.p || !j.n_new.p || (j.preview && !j.st_out.p))
            return bad("an array is null or shorter than its description");
        if (j.carry_out.p && j.carry_out.p == j.carry_in.p) return bad("carry_out must be another array than carry_in");
        if (j.tail_out.p == j.tail_in.p) return bad("tail_out must be another array than tail_in");
        const HandoffState* st = (const HandoffState*)j.st.p;
        for (int k = 0; k < j.S; ++k)
            if (st[k].A < 0 || st[k].A > POS_MAX ||
                st[k].J != (is_nemo ? (st[k].A >= 256 ? (st[k].A - 256) / 160 + 1 : 0) : (st[k].A >= 201 ? (st[k].A - 200) / 160 + 1 : 0)))
                return bad("a state row is not a state of an open stream");
        if (is_nemo) {
            const CssStreamNemoAppendJob& nj = *nemo(i);
            if (j.preview) return bad("a NeMo round is never a preview's");
            if (!std::isfinite(nj.preemphasis) || nj.preemphasis < 0.f || nj.preemphasis >= 1.f) return bad("preemphasis must be finite, at least 0 and below 1");
            if (!arr_ok(ka(nj.xlast_in), j.S) || !arr_ok(ka(nj.xlast_out), j.S) || !nj.xlast_in.p || !nj.xlast_out.p) return bad("an array is null or shorter than its description");
            if (nj.xlast_in.p == nj.xlast_out.p) return bad("xlast_out must be another array than xlast_in");
        }
        // handoff_rows / nemo_rows (api_stream_handoff.hip)
        rows[(size_t)i] = is_nemo ? (j.D1 - j.D0 + 256) / 160 + 2 + 4 : (j.D1 - j.D0 + 200) / 160 + 2 + 3;
        row0[(size_t)i] = rows_total;
        rows_total += rows[(size_t)i] * j.S;
    }
    if (operand_floats != rows_total * 160 + 1024) return bad("operand must hold (sum of S rows) 160 + 1024 floats");
    Stager sg;
    struct At { size_t gate, out, cin, cout, tin, tout, st, sto, act, nn, xin, xout; };
    std::vector<At> at((size_t)n_jobs);
    const size_t op_at = sg.take_raw(operand, (size_t)operand_floats * 4, true);
    for (int i = 0; i < n_jobs; ++i) {
        CssStreamAppendJob& j = job(i);
        At& a = at[(size_t)i];
        a.gate = sg.take(j.gate, 1, false); a.out = sg.take(j.out, 4, false); a.cin = sg.take(j.carry_in, 4, false);
        a.cout = sg.take(j.carry_out, 4, true); a.tin = sg.take(j.tail_in, 4, false); a.tout = sg.take(j.tail_out, 4, true);
        a.st = sg.take(j.st, sizeof(HandoffState), true);
        a.sto = j.preview ? sg.take(j.st_out, sizeof(HandoffState), true) : a.st;
        a.act = sg.take(j.act_out, 1, true); a.nn = sg.take(j.n_new, 4, true);
        if (is_nemo) { a.xin = sg.take(ka(nemo(i)->xlast_in), 4, false); a.xout = sg.take(ka(nemo(i)->xlast_out), 4, true); }
    }
    char* base = nullptr;
    int rc;
    if ((rc = stage_and_upload(h, sg, &base)) != CSS_OK) return rc;
    std::vector<HandoffAppend> ap((size_t)n_jobs);
    for (int i = 0; i < n_jobs; ++i) {
        CssStreamAppendJob& j = job(i);
        const At& a = at[(size_t)i];
        HandoffAppend& e = ap[(size_t)i];
        e = HandoffAppend{};
        e.gate = (const uint8_t*)(base + a.gate); e.gate_ld = j.gate_ld; e.gate_mask = j.gate_ld - 1;
        e.out = (const float*)(base + a.out); e.out_ld = j.out_ld; e.out_base = j.out_base;
        e.carry_in = (const float*)(base + a.cin); e.carry_out = (float*)(base + a.cout); e.carry_ld = j.carry_ld;
        e.tail_in = (const float*)(base + a.tin); e.tail_out = (float*)(base + a.tout);
        e.st = (const HandoffState*)(base + a.st); e.st_out = (HandoffState*)(base + a.sto);
        e.t_g0 = j.t_g0; e.t_g1 = j.t_g1; e.D0 = j.D0; e.D1 = j.D1;
        e.pad = j.pad; e.drop = j.drop; e.closing = j.closing; e.S = j.S;
        e.row0 = j.row0 = row0[(size_t)i]; e.rows = j.rows = rows[(size_t)i];
        e.act_out = (uint8_t*)(base + a.act); e.n_new = (int32_t*)(base + a.nn);
    }
    if (is_nemo) {
        std::vector<NemoAppend> nap((size_t)n_jobs);
        for (int i = 0; i < n_jobs; ++i)
            nap[(size_t)i] = NemoAppend{ap[(size_t)i], (const float*)(base + at[(size_t)i].xin), (float*)(base + at[(size_t)i].xout), nemo(i)->preemphasis, 0};
        launch_nemo_append_multi(nap.data(), n_jobs, (float*)(base + op_at), h->stream);
    } else {
        launch_handoff_append_multi(ap.data(), n_jobs, (float*)(base + op_at), h->stream);
    }
    return download_all(h, sg, base);
}

}  // namespace

extern "C" {

int css_stream_tail_host(css_handle_t h, int32_t form, CssStreamTailJob* jobs, int32_t n_jobs) {
    CSS_DRAIN(h);
    if (!h) return CSS_ERR_INVALID_ARG;
    auto bad = [&](const char* what) { return fail(h, CSS_ERR_INVALID_ARG, std::string("css_stream_tail_host: ") + what); };
    if (!jobs) return bad("null argument");
    if (form < 0 || form > 1) return bad("form must be 0 (activity) or 1 (gate and overlap-add)");
    if (n_jobs < 1 || n_jobs > CSS_STREAM_KERNEL_JOBS) return bad("1 .. 64 jobs");
    int max_erosion = 0;
    for (int i = 0; i < n_jobs; ++i) max_erosion = std::max(max_erosion, std::min(jobs[i].erosion, 4096));
    for (int i = 0; i < n_jobs; ++i) {
        const CssStreamTailJob& j = jobs[i];
        if (j.S < 1 || j.S > 4) return bad("S must be 1 .. 4");
        if (j.F < 1 || j.F > 1024 || j.T < 1 || j.T > 4096) return bad("F must be 1 .. 1024 and T 1 .. 4096");
        if (j.hop < 1 || j.hop > j.T) return bad("hop must be 1 .. T");
        if (j.S != jobs[0].S || j.F != jobs[0].F) return bad("the jobs of one call share S and F");
        if (form == 1 && (size_t)OLA_T * (2 * j.F + 1) * sizeof(float) + OLA_T + 2 * (size_t)max_erosion > 65536)
            return bad("the gate launch's LDS, 64 (2 F + 1) + 16 + 2 (the largest erosion) bytes, exceeds 64 KiB");
        if (j.KIp < 2 * j.F || j.KIp > 4096) return bad("KIp must cover 2 F (and be at most 4096)");
        if (j.dilation < 0 || j.dilation > 4096 || j.erosion < 0 || j.erosion > 4096) return bad("dilation and erosion must be 0 .. 4096");
        if (j.has_ring < 0 || j.has_ring > 1 || (j.has_ring && !pow2(j.gate_ld))) return bad("gate_ld must be a power of two");
        if (j.num_slots < 0 || j.num_slots > (1 << 20) || !pos_ok(j.seg_base) || !pos_ok(j.frame_base))
            return bad("num_slots, seg_base and frame_base must not be negative");
        if (j.num_segments_global < j.seg_base + j.num_slots) return bad("num_segments_global below seg_base + num_slots");
        if (j.mask_ld < j.num_slots * j.T || j.mask_ld > HOST_CAP) return bad("mask_ld must cover num_slots T");
        if (j.ld_frames < 1 || j.ld_frames > (1 << 24)) return bad("ld_frames must be 1 .. 2^24");
        if (j.t_lo < 0 || j.t_hi < j.t_lo || j.t_hi > j.ld_frames) return bad("the range must lie in [0, ld_frames]");
        if (j.T_long_global < j.frame_base || j.t_hi > j.T_long_global - j.frame_base) return bad("the range ends past T_long_global");
        if (!arr_ok(j.masks, (int64_t)j.S * j.F * j.mask_ld) || !arr_ok(j.sep, j.num_slots * j.S * j.F * j.T * 2) ||
            !arr_ok(j.perms, j.num_slots * j.S) || !arr_ok(j.w_first, j.T) || !arr_ok(j.w_mid, j.T) || !arr_ok(j.w_last, j.T) ||
            !arr_ok(j.act_b, (int64_t)j.S * j.ld_frames) || !arr_ok(j.Y, (int64_t)j.S * j.ld_frames * j.KIp) ||
            (j.has_ring && !arr_ok(j.ring, (int64_t)j.S * j.gate_ld)))
            return bad("an array is null or shorter than its description");
        const int32_t* perms = (const int32_t*)j.perms.p;
        for (int64_t q = 0; q < j.num_slots * j.S; ++q)
            if (perms[q] < 0 || perms[q] >= j.S) return bad("a permutation entry outside 0 .. S - 1");
        if (form == 1 && j.t_hi > j.t_lo) {
            const int64_t halo = (int64_t)j.erosion + j.dilation;
            const int64_t g_end = j.T_long_global - j.frame_base;
            const int64_t lo = std::max(j.t_lo - halo, -j.frame_base), hi = std::min(j.t_hi - 1 + halo, g_end - 1);
            if (lo < 0) return bad("the gate reads act_b below local frame 0 (t_lo < erosion + dilation with frame_base > 0)");
            if (hi >= j.ld_frames) return bad("the gate of the range's last frame reads act_b past ld_frames");
        }
    }
    Stager sg;
    struct At { size_t masks, sep, perms, w0, w1, w2, act, Y, ring; };
    std::vector<At> at((size_t)n_jobs);
    for (int i = 0; i < n_jobs; ++i) {
        CssStreamTailJob& j = jobs[i];
        At& a = at[(size_t)i];
        a.masks = sg.take(j.masks, 4, false); a.sep = sg.take(j.sep, 4, false); a.perms = sg.take(j.perms, 4, false);
        a.w0 = sg.take(j.w_first, 4, false); a.w1 = sg.take(j.w_mid, 4, false); a.w2 = sg.take(j.w_last, 4, false);
        a.act = sg.take(j.act_b, 1, true); a.Y = sg.take(j.Y, 4, true);
        a.ring = j.has_ring ? sg.take(j.ring, 1, true) : 0;
    }
    char* base = nullptr;
    int rc;
    if ((rc = stage_and_upload(h, sg, &base)) != CSS_OK) return rc;
    std::vector<StreamStitchArgs> sa((size_t)n_jobs);
    std::vector<StreamFrames> fr((size_t)n_jobs);
    for (int i = 0; i < n_jobs; ++i) {
        const CssStreamTailJob& j = jobs[i];
        const At& a = at[(size_t)i];
        StreamStitchArgs& e = sa[(size_t)i];
        e = StreamStitchArgs{};
        e.masks = (const float*)(base + a.masks); e.mask_ld = j.mask_ld;
        e.sep = (const float*)(base + a.sep); e.perms = (const int32_t*)(base + a.perms);
        e.S = j.S; e.F = j.F; e.T = j.T; e.hop = j.hop;
        e.num_slots = j.num_slots; e.seg_base = j.seg_base; e.frame_base = j.frame_base;
        e.num_segments_global = j.num_segments_global; e.T_long_global = j.T_long_global;
        e.w_first = (const float*)(base + a.w0); e.w_mid = (const float*)(base + a.w1); e.w_last = (const float*)(base + a.w2);
        e.act_b = (uint8_t*)(base + a.act); e.Y = (float*)(base + a.Y); e.KIp = j.KIp; e.ld_frames = j.ld_frames;
        e.activity_th = j.activity_th; e.dilation = j.dilation; e.erosion = j.erosion;
        if (j.has_ring) { e.gate_out = (uint8_t*)(base + a.ring); e.gate_ld = j.gate_ld; e.gate_mask = j.gate_ld - 1; }
        fr[(size_t)i] = StreamFrames{j.t_lo, j.t_hi};
    }
    if (form == 0) launch_stream_activity_multi(sa.data(), fr.data(), n_jobs, h->stream);
    else launch_stream_gate_ola_multi(sa.data(), fr.data(), n_jobs, h->stream);
    return download_all(h, sg, base);
}

int css_stream_scatter_host(css_handle_t h, const float* src, int64_t src_elems, int64_t src_ld, int32_t rows, CssStreamScatterJob* jobs,
                            int32_t n_jobs) {
    CSS_DRAIN(h);
    if (!h) return CSS_ERR_INVALID_ARG;
    auto bad = [&](const char* what) { return fail(h, CSS_ERR_INVALID_ARG, std::string("css_stream_scatter_host: ") + what); };
    if (!jobs || !src) return bad("null argument");
    if (n_jobs < 1 || n_jobs > CSS_STREAM_KERNEL_JOBS) return bad("1 .. 64 jobs");
    if (rows < 1 || rows > 65536) return bad("rows must be 1 .. 65536");
    if (src_ld < 1 || src_ld > HOST_CAP || src_elems > HOST_CAP || src_elems < (int64_t)rows * src_ld) return bad("src is shorter than [rows][src_ld]");
    for (int i = 0; i < n_jobs; ++i) {
        const CssStreamScatterJob& j = jobs[i];
        if (j.src_col < 0 || j.n_cols < 0 || j.src_col + j.n_cols > src_ld) return bad("the columns must lie in [0, src_ld]");
        if (j.dst_ld < j.n_cols || j.dst_ld > HOST_CAP) return bad("dst_ld must cover n_cols");
        if (j.dst_off < 0 || j.dst_off > 63) return bad("dst_off must be 0 .. 63");
        if (!arr_ok(j.dst, j.dst_off + (int64_t)(rows - 1) * j.dst_ld + j.n_cols) || !j.dst.p) return bad("dst is null or shorter than its description");
    }
    Stager sg;
    const size_t src_at = sg.take_raw((void*)src, (size_t)src_elems * 4, false);
    std::vector<size_t> at((size_t)n_jobs);
    for (int i = 0; i < n_jobs; ++i) at[(size_t)i] = sg.take(jobs[i].dst, 4, true);
    char* base = nullptr;
    int rc;
    if ((rc = stage_and_upload(h, sg, &base)) != CSS_OK) return rc;
    std::vector<MaskScatter> ms((size_t)n_jobs);
    for (int i = 0; i < n_jobs; ++i)
        ms[(size_t)i] = MaskScatter{(float*)(base + at[(size_t)i]) + jobs[i].dst_off, jobs[i].dst_ld, jobs[i].src_col, jobs[i].n_cols};
    launch_stream_scatter_masks((const float*)(base + src_at), src_ld, rows, ms.data(), n_jobs, h->stream);
    return download_all(h, sg, base);
}

int css_stream_ingest_host(css_handle_t h, CssStreamIngestJob* jobs, int32_t n_jobs) {
    CSS_DRAIN(h);
    if (!h) return CSS_ERR_INVALID_ARG;
    auto bad = [&](const char* what) { return fail(h, CSS_ERR_INVALID_ARG, std::string("css_stream_ingest_host: ") + what); };
    if (!jobs) return bad("null argument");
    if (n_jobs < 1 || n_jobs > CSS_STREAM_KERNEL_JOBS) return bad("1 .. 64 jobs");
    for (int i = 0; i < n_jobs; ++i) {
        const CssStreamIngestJob& j = jobs[i];
        if (j.C < 1 || j.C > 64) return bad("C must be 1 .. 64");
        if (j.C != jobs[0].C) return bad("the jobs of one call share C");
        if (j.n < 0 || j.n > ((int64_t)1 << 24)) return bad("n must be 0 .. 2^24");
        if (j.plane_ld < 0 || (j.plane_ld > 0 && j.plane_ld < j.n) || j.plane_ld > HOST_CAP) return bad("plane_ld must be 0 (interleaved) or cover n");
        if (j.dst_col < 0 || j.dst_col > 3) return bad("dst_col must be 0 .. 3");
        if (j.dst_ld < j.dst_col + j.n || j.dst_ld > HOST_CAP) return bad("dst_ld must cover dst_col + n");
        const int64_t src_need = j.n == 0 ? 0 : (j.plane_ld > 0 ? (int64_t)(j.C - 1) * j.plane_ld + j.n : j.n * j.C);
        if (!arr_ok(j.src, src_need)) return bad("src is null or shorter than its description");
        if (!arr_ok(j.dst, j.dst_col + (int64_t)(j.C - 1) * j.dst_ld + j.n) || !j.dst.p) return bad("dst is null or shorter than its description");
    }
    Stager sg;
    std::vector<size_t> src_at((size_t)n_jobs), dst_at((size_t)n_jobs);
    for (int i = 0; i < n_jobs; ++i) {
        src_at[(size_t)i] = sg.take(jobs[i].src, 2, false);
        dst_at[(size_t)i] = sg.take(jobs[i].dst, 4, true);
    }
    char* base = nullptr;
    int rc;
    if ((rc = stage_and_upload(h, sg, &base)) != CSS_OK) return rc;
    std::vector<StreamIngestPcm16> in((size_t)n_jobs);
    for (int i = 0; i < n_jobs; ++i) {
        const CssStreamIngestJob& j = jobs[i];
        in[(size_t)i] = StreamIngestPcm16{(const int16_t*)(base + src_at[(size_t)i]), j.plane_ld, j.n, j.C,
                                          (float*)(base + dst_at[(size_t)i]) + j.dst_col, j.dst_ld};
    }
    launch_stream_ingest_pcm16_multi(in.data(), n_jobs, h->stream);
    return download_all(h, sg, base);
}

int css_stream_append_host(css_handle_t h, CssStreamAppendJob* jobs, int32_t n_jobs, float* operand, int64_t operand_floats) {
    CSS_DRAIN(h);
    if (!h) return CSS_ERR_INVALID_ARG;
    if (!jobs) return fail(h, CSS_ERR_INVALID_ARG, "css_stream_append_host: null argument");
    return append_host(h, "css_stream_append_host", [&](int i) -> CssStreamAppendJob& { return jobs[i]; },
                       [](int) -> const CssStreamNemoAppendJob* { return nullptr; }, false, n_jobs, operand, operand_floats);
}

int css_stream_nemo_append_host(css_handle_t h, CssStreamNemoAppendJob* jobs, int32_t n_jobs, float* operand, int64_t operand_floats) {
    CSS_DRAIN(h);
    if (!h) return CSS_ERR_INVALID_ARG;
    if (!jobs) return fail(h, CSS_ERR_INVALID_ARG, "css_stream_nemo_append_host: null argument");
    if (n_jobs < 1 || n_jobs > CSS_STREAM_KERNEL_JOBS) return fail(h, CSS_ERR_INVALID_ARG, "css_stream_nemo_append_host: 1 .. 64 jobs");
    std::vector<CssStreamAppendJob> as((size_t)n_jobs);   // the Whisper entry's job of each: one set of checks, one staging
    for (int i = 0; i < n_jobs; ++i) {
        const CssStreamNemoAppendJob& j = jobs[i];
        as[(size_t)i] = CssStreamAppendJob{j.pad, j.drop, j.closing, j.S, 0, 0, j.gate_ld, j.out_ld, j.out_base, j.carry_ld, j.t_g0, j.t_g1, j.D0, j.D1,
                                           0, 0, ka(j.gate), ka(j.out), ka(j.carry_in), ka(j.carry_out), ka(j.tail_in), ka(j.tail_out), ka(j.st),
                                           CssKArray{nullptr, 0}, ka(j.act_out), ka(j.n_new)};
    }
    const int rc = append_host(h, "css_stream_nemo_append_host", [&](int i) -> CssStreamAppendJob& { return as[(size_t)i]; },
                               [&](int i) -> const CssStreamNemoAppendJob* { return &jobs[i]; }, true, n_jobs, operand, operand_floats);
    for (int i = 0; i < n_jobs; ++i) { jobs[i].row0 = as[(size_t)i].row0; jobs[i].rows = as[(size_t)i].rows; }
    return rc;
}

int css_stream_mel_host(css_handle_t h, int32_t S, const float* spec, int64_t spec_elems, int64_t ld, CssStreamMelJob* jobs, int32_t n_jobs) {
    CSS_DRAIN(h);
    if (!h) return CSS_ERR_INVALID_ARG;
    auto bad = [&](const char* what) { return fail(h, CSS_ERR_INVALID_ARG, std::string("css_stream_mel_host: ") + what); };
    if (!jobs || !spec) return bad("null argument");
    if (n_jobs < 1 || n_jobs > CSS_STREAM_KERNEL_JOBS) return bad("1 .. 64 jobs");
    if (S < 1 || S > 4) return bad("S must be 1 .. 4");
    if (ld < 1 || ld > HOST_CAP / 402 || spec_elems < 402 * ld || spec_elems > HOST_CAP) return bad("spec is shorter than [402][ld]");
    for (int i = 0; i < n_jobs; ++i) {
        const CssStreamMelJob& j = jobs[i];
        if (j.n_mels != 80 && j.n_mels != 128) return bad("n_mels must be 80 or 128");
        if (j.row0 < 0 || j.rows < 1 || j.rows > (1 << 20) || j.row0 + (int64_t)S * j.rows > ld) return bad("row0 + S rows must lie in [0, ld]");
        if (j.mel_ld < j.rows || j.mel_ld > HOST_CAP) return bad("mel_ld must cover rows");
        if (j.has_ring < 0 || j.has_ring > 1 || j.has_pvmax < 0 || j.has_pvmax > 1 || (j.has_ring && j.has_pvmax)) return bad("has_ring and has_pvmax are 0 or 1, not both");
        if (j.has_ring && (j.hist < 1 || j.hist > HOST_CAP)) return bad("hist must be at least 1");
        if (!arr_ok(j.n_new, S) || !arr_ok(j.st, S) || !arr_ok(j.mel, (int64_t)S * j.n_mels * j.mel_ld) || !j.n_new.p || !j.st.p || !j.mel.p ||
            (j.has_ring && (!arr_ok(j.ring, (int64_t)S * j.n_mels * j.hist) || !arr_ok(j.fmax, (int64_t)S * j.hist) || !j.ring.p || !j.fmax.p)) ||
            (j.has_pvmax && (!arr_ok(j.pvmax, (int64_t)S * j.rows) || !j.pvmax.p)))
            return bad("an array is null or shorter than its description");
        const int32_t* nn = (const int32_t*)j.n_new.p;
        const HandoffState* st = (const HandoffState*)j.st.p;
        for (int k = 0; k < S; ++k) {
            if (nn[k] < 0) return bad("n_new must not be negative");
            if (j.has_ring && st[k].J < nn[k]) return bad("a frame count J below n_new");
        }
    }
    std::vector<float> w80((size_t)80 * 201), w128((size_t)128 * 201);
    handoff_build_mel(w80.data(), 80);
    handoff_build_mel(w128.data(), 128);
    Stager sg;
    const size_t spec_at = sg.take_raw((void*)spec, (size_t)spec_elems * 4, false);
    const size_t w80_at = sg.take_raw(w80.data(), w80.size() * 4, false), w128_at = sg.take_raw(w128.data(), w128.size() * 4, false);
    struct At { size_t nn, st, mel, ring, fmax, pv; };
    std::vector<At> at((size_t)n_jobs);
    for (int i = 0; i < n_jobs; ++i) {
        CssStreamMelJob& j = jobs[i];
        At& a = at[(size_t)i];
        a.nn = sg.take(j.n_new, 4, false); a.st = sg.take(j.st, sizeof(HandoffState), true); a.mel = sg.take(j.mel, 4, true);
        a.ring = j.has_ring ? sg.take(j.ring, 4, true) : 0; a.fmax = j.has_ring ? sg.take(j.fmax, 4, true) : 0;
        a.pv = j.has_pvmax ? sg.take(j.pvmax, 4, true) : 0;
    }
    char* base = nullptr;
    int rc;
    if ((rc = stage_and_upload(h, sg, &base)) != CSS_OK) return rc;
    std::vector<HandoffMel> me((size_t)n_jobs);
    for (int i = 0; i < n_jobs; ++i) {
        const CssStreamMelJob& j = jobs[i];
        const At& a = at[(size_t)i];
        HandoffMel& e = me[(size_t)i];
        e = HandoffMel{};
        e.row0 = j.row0; e.rows = j.rows; e.n_new = (const int32_t*)(base + a.nn); e.st = (HandoffState*)(base + a.st);
        e.w = (const float*)(base + (j.n_mels == 80 ? w80_at : w128_at)); e.n_mels = j.n_mels;
        e.mel = (float*)(base + a.mel); e.mel_ld = j.mel_ld;
        if (j.has_ring) { e.ring = (float*)(base + a.ring); e.fmax = (float*)(base + a.fmax); e.hist = j.hist; }
        if (j.has_pvmax) e.pvmax = (float*)(base + a.pv);
    }
    launch_handoff_mel_multi(me.data(), n_jobs, S, (const float*)(base + spec_at), ld, h->stream);
    return download_all(h, sg, base);
}

// Both NeMo mel entries: job i's mel part is mj(i); hj, where the call is css_stream_nemo_mel_history_host, its jobs (else null: `jobs`).
static int nemo_mel_host(css_ctx* h, const char* who, int32_t S, const float* spec, int64_t spec_elems, int64_t ld, CssStreamNemoMelJob* jobs,
                         CssStreamNemoMelHistoryJob* hj, int32_t n_jobs) {
    auto bad = [&](const char* what) { return fail(h, CSS_ERR_INVALID_ARG, std::string(who) + ": " + what); };
    auto mj = [&](int i) {
        if (!hj) return jobs[i];
        const CssStreamNemoMelHistoryJob& q = hj[i];
        return CssStreamNemoMelJob{q.n_mels, q.reserved, q.row0, q.rows, q.mel_ld, na(q.n_new), na(q.mel)};
    };
    if ((!jobs && !hj) || !spec) return bad("null argument");
    if (n_jobs < 1 || n_jobs > CSS_STREAM_KERNEL_JOBS) return bad("1 .. 64 jobs");
    if (S < 1 || S > 4) return bad("S must be 1 .. 4");
    constexpr int64_t SPEC_ROWS = 2 * NEMO_BINS;
    if (ld < 1 || ld > HOST_CAP / SPEC_ROWS || spec_elems < SPEC_ROWS * ld || spec_elems > HOST_CAP) return bad("spec is shorter than [514][ld]");
    for (int i = 0; i < n_jobs; ++i) {
        const CssStreamNemoMelJob j = mj(i);
        if (j.n_mels != 80 && j.n_mels != 128) return bad("n_mels must be 80 or 128");
        if (j.row0 < 0 || j.rows < 1 || j.rows > (1 << 20) || j.row0 + (int64_t)S * j.rows > ld) return bad("row0 + S rows must lie in [0, ld]");
        if (j.mel_ld < j.rows || j.mel_ld > HOST_CAP) return bad("mel_ld must cover rows");
        if (!arr_ok(ka(j.n_new), S) || !arr_ok(ka(j.mel), (int64_t)S * j.n_mels * j.mel_ld) || !j.n_new.p || !j.mel.p) return bad("an array is null or shorter than its description");
        for (int k = 0; k < S; ++k)
            if (((const int32_t*)j.n_new.p)[k] < 0) return bad("n_new must not be negative");
        if (!hj) continue;
        const CssStreamNemoMelHistoryJob& q = hj[i];
        if (q.hist < 1 || q.hist > HOST_CAP / (S * j.n_mels)) return bad("hist must be 1 .. 2^28 / (S n_mels) (the ring is staged whole)");
        if (!arr_ok(ka(na(q.ring)), (int64_t)S * j.n_mels * q.hist) || !arr_ok(ka(na(q.frames_after)), S) || !q.ring.p || !q.frames_after.p)
            return bad("an array is null or shorter than its description");
        for (int k = 0; k < S; ++k) {
            const int64_t J = ((const int64_t*)q.frames_after.p)[k];
            if (J < ((const int32_t*)j.n_new.p)[k] || !pos_ok(J)) return bad("a frame count after the round below n_new");
        }
    }
    int rc;
    HIPCHK(h, hipSetDevice(h->device));
    if ((rc = nemo_ensure_tables(h)) != CSS_OK) return rc;
    Stager sg;
    const size_t spec_at = sg.take_raw((void*)spec, (size_t)spec_elems * 4, false);
    struct At { size_t nn, mel, ring, st; };
    std::vector<At> at((size_t)n_jobs);
    std::vector<std::vector<HandoffState>> st((size_t)n_jobs);   // the state rows the kernel reads the counts from
    for (int i = 0; i < n_jobs; ++i) {
        At& a = at[(size_t)i];
        a = At{sg.take(ka(mj(i).n_new), 4, false), sg.take(ka(mj(i).mel), 4, true), 0, 0};
        if (!hj) continue;
        st[(size_t)i].assign((size_t)S, HandoffState{});
        for (int k = 0; k < S; ++k) st[(size_t)i][(size_t)k].J = ((const int64_t*)hj[i].frames_after.p)[k];
        a.ring = sg.take(ka(na(hj[i].ring)), 4, true);
        a.st = sg.take_raw(st[(size_t)i].data(), (size_t)S * sizeof(HandoffState), false);
    }
    char* base = nullptr;
    if ((rc = stage_and_upload(h, sg, &base)) != CSS_OK) return rc;
    std::vector<NemoMel> me((size_t)n_jobs);
    for (int i = 0; i < n_jobs; ++i) {
        const CssStreamNemoMelJob j = mj(i);
        const At& a = at[(size_t)i];
        me[(size_t)i] = NemoMel{j.row0, j.rows, (const int32_t*)(base + a.nn), nemo_bank(h, j.n_mels), (float*)(base + a.mel), j.mel_ld, j.n_mels, 0};
        if (hj) { me[(size_t)i].ring = (float*)(base + a.ring); me[(size_t)i].hist = hj[i].hist; me[(size_t)i].st = (const HandoffState*)(base + a.st); }
    }
    launch_nemo_mel_multi(me.data(), n_jobs, S, (const float*)(base + spec_at), ld, h->stream);
    return download_all(h, sg, base);
}

int css_stream_nemo_mel_host(css_handle_t h, int32_t S, const float* spec, int64_t spec_elems, int64_t ld, CssStreamNemoMelJob* jobs,
                             int32_t n_jobs) {
    CSS_DRAIN(h);
    if (!h) return CSS_ERR_INVALID_ARG;
    return nemo_mel_host(h, "css_stream_nemo_mel_host", S, spec, spec_elems, ld, jobs, nullptr, n_jobs);
}

int css_stream_nemo_mel_history_host(css_handle_t h, int32_t S, const float* spec, int64_t spec_elems, int64_t ld,
                                     CssStreamNemoMelHistoryJob* jobs, int32_t n_jobs) {
    CSS_DRAIN(h);
    if (!h) return CSS_ERR_INVALID_ARG;
    return nemo_mel_host(h, "css_stream_nemo_mel_history_host", S, spec, spec_elems, ld, nullptr, jobs, n_jobs);
}

}  // extern "C"
