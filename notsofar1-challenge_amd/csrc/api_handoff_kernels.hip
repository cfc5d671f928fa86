// include/css_mi355_handoff_kernels.h: the window kernels and the queued sessions' hand-off kernels of handoff.hip on caller data,
// one entry per launcher (unit tests of the kernels; the companion of api_stream_kernels.hip).  Every entry checks first, then
// stages in h->stage, makes the launcher call(s) the path makes, downloads every allocation a launch could have written and
// synchronises.  An array with an element offset is staged whole at its 256-byte boundary; the kernel gets the address behind
// the offset.
#include <algorithm>
#include <string>
#include <vector>

#include "api_ctx.hpp"
#include "api_kernel_stage.hpp"
#include "../../include/css_mi355_handoff_kernels.h"

using namespace css;
using namespace css::kstage;

namespace {

constexpr int64_t POS_MAX = (int64_t)1 << 40;   // frame and sample positions of a recording

bool flag(int32_t v) { return v == 0 || v == 1; }
bool off_ok(int32_t v, int most) { return v >= 0 && v <= most; }
int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

}  // namespace

extern "C" {

int css_session_scan_host(css_handle_t h, CssSessionScanJob* job) {
    CSS_DRAIN(h);
    if (!h) return CSS_ERR_INVALID_ARG;
    auto bad = [&](const char* what) { return fail(h, CSS_ERR_INVALID_ARG, std::string("css_session_scan_host: ") + what); };
    if (!job) return bad("null argument");
    static_assert(sizeof(HandoffState) == 24, "the header states the state row");
    const CssSessionScanJob& j = *job;
    if (j.S < 1 || j.S > 4) return bad("S must be 1 .. 4");
    if (j.TL < 1 || j.TL > ((int64_t)1 << 24)) return bad("TL must be 1 .. 2^24");
    if (j.pad < 0 || j.pad > 4096) return bad("pad must be 0 .. 4096");
    if (!flag(j.drop)) return bad("drop is 0 or 1");
    if (j.cap_ranges < 1 || j.cap_ranges > (1 << 24)) return bad("cap_ranges must be at least 1");
    if (!off_ok(j.gate_off, 3)) return bad("gate_off must be 0 .. 3");
    const int64_t S = j.S, cap = j.cap_ranges;
    if (!arr_ok(j.gate, j.gate_off + S * j.TL) || !arr_ok(j.psum, S * (j.TL + 1)) || !arr_ok(j.regs, S * cap * 2) || !arr_ok(j.offs, S * cap) ||
        !arr_ok(j.st, S) || !arr_ok(j.n_new, S) || !arr_ok(j.n_ranges, S) || !arr_ok(j.ranges_out, S * cap * 2) ||
        !arr_ok(j.n_frames_out, S) || !arr_ok(j.n_ranges_out, S))
        return bad("an array is null or shorter than its description");
    Stager sg;
    const size_t gate = sg.take(j.gate, 1, false), psum = sg.take(j.psum, 4, true), regs = sg.take(j.regs, 8, true), offs = sg.take(j.offs, 8, true),
                 st = sg.take(j.st, sizeof(HandoffState), true), nn = sg.take(j.n_new, 4, true), nr = sg.take(j.n_ranges, 4, true),
                 ro = sg.take(j.ranges_out, 8, true), nfo = sg.take(j.n_frames_out, 8, true), nro = sg.take(j.n_ranges_out, 4, true);
    char* base = nullptr;
    int rc;
    if ((rc = stage_and_upload(h, sg, &base)) != CSS_OK) return rc;
    SessionHandoff e{};
    e.gate = (const uint8_t*)(base + gate) + j.gate_off; e.TL = j.TL;
    e.pad = j.pad; e.drop = j.drop; e.S = j.S; e.cap_ranges = j.cap_ranges;
    e.psum = (int32_t*)(base + psum); e.regs = (int64_t*)(base + regs); e.offs = (int64_t*)(base + offs);
    e.st = (HandoffState*)(base + st); e.n_new = (int32_t*)(base + nn); e.n_ranges = (int32_t*)(base + nr);
    e.ranges_out = (int64_t*)(base + ro); e.n_frames_out = (int64_t*)(base + nfo); e.n_ranges_out = (int32_t*)(base + nro);
    launch_session_keep_scan(e, h->stream);
    return download_all(h, sg, base);
}

int css_session_gather_host(css_handle_t h, CssSessionGatherJob* job) {
    CSS_DRAIN(h);
    if (!h) return CSS_ERR_INVALID_ARG;
    auto bad = [&](const char* what) { return fail(h, CSS_ERR_INVALID_ARG, std::string("css_session_gather_host: ") + what); };
    if (!job) return bad("null argument");
    const CssSessionGatherJob& j = *job;
    if (j.S < 1 || j.S > 4) return bad("S must be 1 .. 4");
    if (j.rows < 1 || j.rows > (1 << 20)) return bad("rows must be 1 .. 2^20");
    if (j.cap_ranges < 1 || j.cap_ranges > (1 << 24)) return bad("cap_ranges must be at least 1");
    if (!off_ok(j.wav_off, 3)) return bad("wav_off must be 0 .. 3");
    if (j.wav_ld < 1 || j.wav_ld > HOST_CAP) return bad("wav_ld must be at least 1");
    const int64_t S = j.S, cap = j.cap_ranges;
    if (!arr_ok(j.regs, S * cap * 2) || !arr_ok(j.offs, S * cap) || !arr_ok(j.st, S) || !arr_ok(j.n_ranges, S) ||
        !arr_ok(j.wav, j.wav_off + S * j.wav_ld))
        return bad("an array is null or shorter than its description");
    if (!j.operand.p || j.operand.elems != S * j.rows * 160 + 416) return bad("operand must hold S rows 160 + 416 floats");
    const HandoffState* stv = (const HandoffState*)j.st.p;
    const int32_t* nrv = (const int32_t*)j.n_ranges.p;
    for (int k = 0; k < j.S; ++k) {
        const int64_t A = stv[k].A;
        if (A < 0 || A > POS_MAX) return bad("a sample count A below 0");
        if (nrv[k] < 0) return bad("a run count below 0");
        const int64_t nr = std::min<int64_t>(nrv[k], cap);
        if (A == 0 || nr == 0) continue;
        const int64_t* reg = (const int64_t*)j.regs.p + (int64_t)k * cap * 2;
        const int64_t* off = (const int64_t*)j.offs.p + (int64_t)k * cap;
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
    Stager sg;
    const size_t regs = sg.take(j.regs, 8, false), offs = sg.take(j.offs, 8, false), st = sg.take(j.st, sizeof(HandoffState), false),
                 nr = sg.take(j.n_ranges, 4, false), wav = sg.take(j.wav, 4, false), op = sg.take(j.operand, 4, true);
    char* base = nullptr;
    int rc;
    if ((rc = stage_and_upload(h, sg, &base)) != CSS_OK) return rc;
    SessionHandoff e{};
    e.S = j.S; e.cap_ranges = j.cap_ranges;
    e.regs = (int64_t*)(base + regs); e.offs = (int64_t*)(base + offs); e.st = (HandoffState*)(base + st); e.n_ranges = (int32_t*)(base + nr);
    launch_session_gather(e, (const float*)(base + wav) + j.wav_off, j.wav_ld, (float*)(base + op), j.rows, h->stream);
    return download_all(h, sg, base);
}

int css_session_norm_host(css_handle_t h, CssSessionNormJob* job) {
    CSS_DRAIN(h);
    if (!h) return CSS_ERR_INVALID_ARG;
    auto bad = [&](const char* what) { return fail(h, CSS_ERR_INVALID_ARG, std::string("css_session_norm_host: ") + what); };
    if (!job) return bad("null argument");
    const CssSessionNormJob& j = *job;
    if (j.S < 1 || j.S > 4) return bad("S must be 1 .. 4");
    if (j.n_mels < 1 || j.n_mels > 128) return bad("n_mels must be 1 .. 128");
    if (j.rows > (1 << 24)) return bad("rows must be at most 2^24");
    if (j.mel_ld < 0 || j.mel_ld > HOST_CAP || j.mel_ld < j.rows) return bad("mel_ld must cover rows");
    if (j.out_ld < 0 || j.out_ld > HOST_CAP) return bad("out_ld must not be negative");
    const int64_t SM = (int64_t)j.S * j.n_mels;
    if (!arr_ok(j.st, j.S) || !j.st.p || !arr_ok(j.mel, SM * j.mel_ld) || !arr_ok(j.out, SM * j.out_ld))
        return bad("an array is null or shorter than its description");
    const HandoffState* stv = (const HandoffState*)j.st.p;
    for (int k = 0; k < j.S; ++k)
        if (stv[k].J < 0 || stv[k].J > std::max<int64_t>(j.rows, 0)) return bad("a frame count J outside 0 .. rows");
    Stager sg;
    const size_t st = sg.take(j.st, sizeof(HandoffState), false), mel = sg.take(j.mel, 4, false), out = sg.take(j.out, 4, true);
    char* base = nullptr;
    int rc;
    if ((rc = stage_and_upload(h, sg, &base)) != CSS_OK) return rc;
    SessionHandoff e{};
    e.S = j.S; e.st = (HandoffState*)(base + st);
    launch_session_norm(e, (const float*)(base + mel), j.mel_ld, j.n_mels, (float*)(base + out), j.out_ld, j.rows, h->stream);
    return download_all(h, sg, base);
}

int css_session_windows_host(css_handle_t h, CssSessionWindowsJob* job) {
    CSS_DRAIN(h);
    if (!h) return CSS_ERR_INVALID_ARG;
    auto bad = [&](const char* what) { return fail(h, CSS_ERR_INVALID_ARG, std::string("css_session_windows_host: ") + what); };
    if (!job) return bad("null argument");
    CssSessionWindowsJob& j = *job;
    if (j.S < 1 || j.S > 4) return bad("S must be 1 .. 4");
    if (j.n_mels < 1 || j.n_mels > 128) return bad("n_mels must be 1 .. 128");
    if (j.width < 1 || j.width > (1 << 20) || j.stride < 1 || j.stride > (1 << 20)) return bad("width and stride must be at least 1");
    if (!flag(j.f16) || !flag(j.has_win) || !flag(j.has_whole)) return bad("f16, has_win and has_whole are 0 or 1");
    if (!off_ok(j.win_off, 7) || !off_ok(j.whole_off, 7) || !off_ok(j.mel_off, 3)) return bad("win_off and whole_off are 0 .. 7, mel_off 0 .. 3");
    if (j.mel_ld < 0 || j.mel_ld > HOST_CAP || j.max_frames < 0 || j.max_frames > j.mel_ld) return bad("max_frames must lie in 0 .. mel_ld");
    const int64_t n_win = ceil_div(j.max_frames, j.stride);
    if (j.has_win && (j.ld < j.width || j.ld > HOST_CAP)) return bad("ld must cover width");
    if (j.has_win && (j.cap_windows < n_win || j.cap_windows > HOST_CAP)) return bad("cap_windows below ceil(max_frames / stride)");
    if (j.has_whole && (j.whole_ld < 1 || j.whole_ld > HOST_CAP)) return bad("whole_ld must be at least 1");
    const int64_t SM = (int64_t)j.S * j.n_mels;
    const size_t el = j.f16 ? 2 : 4;
    if (!arr_ok(j.st, j.S) || !j.st.p || !arr_ok(j.mel, j.mel_off + SM * j.mel_ld) || !arr_ok(j.n_windows_out, j.S) || !j.n_windows_out.p ||
        !arr_ok(j.window_max_out, j.S) || !j.window_max_out.p ||
        (j.has_win && (j.cap_windows > HOST_CAP / (SM * j.ld) || !arr_ok(j.win, j.win_off + SM * j.cap_windows * j.ld) || !j.win.p)) ||
        (j.has_whole && (!arr_ok(j.whole, j.whole_off + SM * j.whole_ld) || !j.whole.p)))
        return bad("an array is null or shorter than its description");
    const HandoffState* stv = (const HandoffState*)j.st.p;
    for (int k = 0; k < j.S; ++k)
        if (stv[k].J < 0) return bad("a frame count J below 0");
    Stager sg;
    const size_t st = sg.take(j.st, sizeof(HandoffState), false), mel = sg.take(j.mel, 4, false), nw = sg.take(j.n_windows_out, 4, true),
                 wm = sg.take(j.window_max_out, 4, true);
    const size_t win = j.has_win ? sg.take(j.win, el, true) : 0, whole = j.has_whole ? sg.take(j.whole, el, true) : 0;
    char* base = nullptr;
    int rc;
    if ((rc = stage_and_upload(h, sg, &base)) != CSS_OK) return rc;
    SessionWindows sw{};   // as session_handoff_on fills it (api_session_handoff.hip)
    sw.st = (const HandoffState*)(base + st); sw.mel = (const float*)(base + mel) + j.mel_off; sw.mel_ld = j.mel_ld; sw.max_frames = j.max_frames;
    sw.S = j.S; sw.n_mels = j.n_mels; sw.width = j.width; sw.stride = j.stride; sw.f16 = j.f16;
    sw.win = j.has_win ? (void*)(base + win + (size_t)j.win_off * el) : nullptr; sw.ld = j.ld; sw.cap_windows = j.cap_windows;
    sw.n_win_jobs = j.n_win_jobs = j.has_win ? n_win : 0;
    sw.whole = j.has_whole ? (void*)(base + whole + (size_t)j.whole_off * el) : nullptr; sw.whole_ld = j.whole_ld;
    sw.n_whole_jobs = j.n_whole_jobs = j.has_whole ? ceil_div(j.whole_ld, SESSION_WINDOW_CHUNK) : 0;
    sw.n_windows_out = (int32_t*)(base + nw); sw.window_max_out = (float*)(base + wm);
    launch_session_windows(sw, h->stream);
    return download_all(h, sg, base);
}

int css_stream_windows_host(css_handle_t h, CssStreamWindowJob* items, int32_t n_items, void* res, int64_t res_rows) {
    CSS_DRAIN(h);
    if (!h) return CSS_ERR_INVALID_ARG;
    auto bad = [&](const char* what) { return fail(h, CSS_ERR_INVALID_ARG, std::string("css_stream_windows_host: ") + what); };
    if (!items || !res) return bad("null argument");
    static_assert(sizeof(WindowOut) == 24, "the header states the result row");
    static_assert(CSS_WINDOW_KERNEL_ITEMS == 2 * WINDOW_MULTI_MAX, "two full launches per call");
    if (n_items < 1 || n_items > CSS_WINDOW_KERNEL_ITEMS) return bad("1 .. 64 items");
    if (res_rows < n_items || res_rows > (1 << 20)) return bad("res must hold a row per item");
    for (int i = 0; i < n_items; ++i) {
        const CssStreamWindowJob& j = items[i];
        if (j.width < 1 || j.width > 3000) return bad("width must be 1 .. 3000");
        if (j.n_frames < 1 || j.n_frames > j.width) return bad("n_frames must be 1 .. width");
        if (j.n_mels < 1 || j.n_mels > 128) return bad("n_mels must be 1 .. 128");
        if (!flag(j.f16) || !flag(j.has_pv)) return bad("f16 and has_pv are 0 or 1");
        if (j.ld < j.width || j.ld > HOST_CAP) return bad("ld must cover width");
        if (j.hist < 1 || j.hist > HOST_CAP) return bad("hist must be at least 1");
        if (j.J < 0 || j.J > ((int64_t)1 << 60)) return bad("J must not be negative");
        if (!off_ok(j.ring_off, 3) || !off_ok(j.pv_off, 3) || !off_ok(j.out_off, 7)) return bad("ring_off and pv_off are 0 .. 3, out_off 0 .. 7");
        if (!arr_ok(j.ring, j.ring_off + (int64_t)j.n_mels * j.hist) || !j.ring.p || !arr_ok(j.fmax, j.hist) || !j.fmax.p ||
            !arr_ok(j.out, j.out_off + (int64_t)j.n_mels * j.ld) || !j.out.p)
            return bad("an array is null or shorter than its description");
        if (j.has_pv) {
            if (j.pv_ld < 1 || j.pv_ld > HOST_CAP) return bad("pv_ld must be at least 1");
            if (!arr_ok(j.pv, j.pv_off + (int64_t)j.n_mels * j.pv_ld) || !j.pv.p || !arr_ok(j.pvmax, j.pv_ld) || !j.pvmax.p ||
                !arr_ok(j.n_new, 1) || !j.n_new.p)
                return bad("an array is null or shorter than its description");
            if (*(const int32_t*)j.n_new.p < 0) return bad("n_new must not be negative");
        } else if (j.n_frames > std::min(j.J, j.hist)) {
            return bad("a window out of the history alone asks for more frames than min(J, hist)");
        }
    }
    Stager sg;
    struct At { size_t ring, fmax, pv, pvmax, nn, out; };
    std::vector<At> at((size_t)n_items);
    const size_t res_at = sg.take_raw(res, (size_t)res_rows * sizeof(WindowOut), true);
    for (int i = 0; i < n_items; ++i) {
        const CssStreamWindowJob& j = items[i];
        At& a = at[(size_t)i];
        a.ring = sg.take(j.ring, 4, false); a.fmax = sg.take(j.fmax, 4, false);
        a.pv = j.has_pv ? sg.take(j.pv, 4, false) : 0; a.pvmax = j.has_pv ? sg.take(j.pvmax, 4, false) : 0;
        a.nn = j.has_pv ? sg.take(j.n_new, 4, false) : 0;
        a.out = sg.take(j.out, j.f16 ? 2 : 4, true);
    }
    char* base = nullptr;
    int rc;
    if ((rc = stage_and_upload(h, sg, &base)) != CSS_OK) return rc;
    std::vector<WindowItem> w((size_t)n_items);
    for (int i = 0; i < n_items; ++i) {
        const CssStreamWindowJob& j = items[i];
        const At& a = at[(size_t)i];
        WindowItem& e = w[(size_t)i];
        e = WindowItem{};
        e.ring = (const float*)(base + a.ring) + j.ring_off; e.fmax = (const float*)(base + a.fmax);
        if (j.has_pv) {
            e.pv = (const float*)(base + a.pv) + j.pv_off; e.pvmax = (const float*)(base + a.pvmax);
            e.n_new = (const int32_t*)(base + a.nn); e.pv_ld = j.pv_ld;
        }
        e.out = (void*)(base + a.out + (size_t)j.out_off * (j.f16 ? 2 : 4)); e.res = (WindowOut*)(base + res_at) + i;
        e.hist = j.hist; e.ld = j.ld; e.J = j.J;
        e.n_frames = j.n_frames; e.width = j.width; e.n_mels = j.n_mels; e.f16 = j.f16;
    }
    for (size_t i0 = 0; i0 < w.size(); i0 += WINDOW_MULTI_MAX)   // (launch_windows, api_stream_handoff.hip)
        launch_stream_windows(w.data() + i0, (int)std::min<size_t>(WINDOW_MULTI_MAX, w.size() - i0), h->stream);
    return download_all(h, sg, base);
}

}  // extern "C"
