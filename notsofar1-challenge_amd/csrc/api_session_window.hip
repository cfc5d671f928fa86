// libcss_mi355.so: Whisper encoder windows of whole sessions (include/css_mi355_session_window.h) -- the session
// hand-off of api_session_handoff.hip with one more launch behind its mel kernel: session_window_kernel (handoff.hip) cuts the
// windows, and optionally the whole padded log-mel, out of the raw rows in sh_work straight into the caller's device memory, as
// float32 or float16, at the session's own maximum.  The frame counts and the maximum stay on the device; this unit only checks
// the caller's description against the host-side bounds and hands it to the hand-off's own entry points.  It owns no memory.
#include "api_ctx.hpp"
#include "../../include/css_mi355_session_window.h"

static_assert(CSS_WINDOW_MAX_WIDTH == 3000 && CSS_WINDOW_F32 == 0 && CSS_WINDOW_F16 == 1, "the header's rule is stated with these");

namespace {
// what needs no plan: the description itself
const char* window_shape_error(const CssSessionWindows* w) {
    if (!w || !w->n_windows || !w->window_max) return "null argument (win, n_windows, window_max)";
    if (!w->windows_dev && !w->mel_dev) return "windows_dev and mel_dev are both NULL";
    if (w->width < 1 || w->width > CSS_WINDOW_MAX_WIDTH) return "width must be in [1, 3000]";
    if (w->stride < 1 || w->stride > w->width) return "stride must be in [1, width]";
    if (w->dtype != CSS_WINDOW_F32 && w->dtype != CSS_WINDOW_F16) return "dtype must be CSS_WINDOW_F32 or CSS_WINDOW_F16";
    if (w->windows_dev && w->ld < w->width) return "ld is below width";
    return nullptr;
}

// device memory of the handle's device from p to p + bytes, p aligned to `el`
bool device_span_ok(const css_ctx* h, const void* p, size_t bytes, size_t el) {
    if ((uintptr_t)p % el) return false;
    const void* ends[2] = {p, (const char*)p + (bytes ? bytes - 1 : 0)};
    for (const void* q : ends) {
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, q) != hipSuccess) { (void)hipGetLastError(); return false; }
        if (at.type != hipMemoryTypeDevice || at.device != h->device) return false;
    }
    return true;
}

// the description against the session's frame bound; on CSS_OK `req` is filled but for the addresses of the two count arrays
int check_windows(css_ctx* h, const CssSessionWindows* w, int64_t frames, int n_mels, SessWindowReq* req) {
    if (const char* e = window_shape_error(w)) return fail(h, CSS_ERR_INVALID_ARG, e);
    const int S = h->d.num_spks;
    const int64_t windows = (frames + w->stride - 1) / w->stride;
    const size_t el = w->dtype == CSS_WINDOW_F16 ? 2 : 4;
    if (w->windows_dev) {
        if (w->cap_windows < windows) return fail(h, CSS_ERR_INVALID_ARG, "cap_windows below css_session_window_bounds: need " + std::to_string(windows));
        // the last element the kernel may write: row n_mels - 1 of window cap_windows - 1 of speaker S - 1, column width - 1
        const size_t span = ((((size_t)S * w->cap_windows) * n_mels - 1) * (size_t)w->ld + w->width) * el;
        if (!device_span_ok(h, w->windows_dev, span, el))
            return fail(h, CSS_ERR_INVALID_ARG, "windows_dev is not device memory of the handle's device, or not aligned to its element size");
    }
    if (w->mel_dev) {
        if (w->mel_ld < std::max<int64_t>(frames, 1)) return fail(h, CSS_ERR_INVALID_ARG, "mel_ld below css_session_window_bounds: need " + std::to_string(frames));
        if (!device_span_ok(h, w->mel_dev, (size_t)S * n_mels * (size_t)w->mel_ld * el, el))
            return fail(h, CSS_ERR_INVALID_ARG, "mel_dev is not device memory of the handle's device, or not aligned to its element size");
    }
    req->on = true;
    req->width = w->width; req->stride = w->stride; req->f16 = w->dtype == CSS_WINDOW_F16;
    req->windows = w->windows_dev; req->ld = w->ld; req->cap_windows = w->cap_windows;
    req->whole = w->mel_dev; req->whole_ld = w->mel_ld;
    return CSS_OK;
}

// the checks of a queued window session, in the order: the hand-off's own (its codes), the description, the count arrays
int check_enqueue_windows(css_ctx* h, int64_t n_samples, int32_t n_ch, const CssRunCfg* cfg, const CssStreamHandoffCfg* hcfg,
                          const CssSessionHandoffOut* out, const CssSessionWindows* win, SessHandoffReq* req, int64_t* n_out) {
    if (const char* e = window_shape_error(win)) return fail(h, CSS_ERR_INVALID_ARG, e);
    int64_t frames = 0;
    int rc = session_handoff_enqueue_check(h, n_samples, n_ch, cfg, hcfg, out, true, req, n_out, &frames);
    if (rc != CSS_OK) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    if ((rc = check_windows(h, win, frames, hcfg->n_mels, &req->win)) != CSS_OK) return rc;
    req->win.n_windows = (int32_t*)mapped_host(win->n_windows);
    req->win.window_max = (float*)mapped_host(win->window_max);
    if (!req->win.n_windows || !req->win.window_max)
        return fail(h, CSS_ERR_INVALID_ARG, "n_windows and window_max of a queued session must be page-locked (css_host_alloc)");
    return CSS_OK;
}
}  // namespace

int css_session_window_bounds(const CssModelDesc* desc, const CssRunCfg* cfg, const CssStreamHandoffCfg* hcfg, int32_t width,
                              int32_t stride, int64_t n_samples, int64_t* frames, int32_t* ranges, int64_t* windows) {
    if (!frames || !ranges || !windows || width < 1 || width > CSS_WINDOW_MAX_WIDTH || stride < 1 || stride > width) return CSS_ERR_INVALID_ARG;
    int64_t f = 0;
    int32_t r = 0;
    const int rc = css_session_handoff_bounds(desc, cfg, hcfg, n_samples, &f, &r);
    if (rc != CSS_OK) return rc;
    *frames = f; *ranges = r; *windows = (f + stride - 1) / stride;
    return CSS_OK;
}

int css_handoff_windows_all(css_handle_t h, const float* wav_dev, int64_t wav_ld, const CssStreamHandoffCfg* hcfg,
                            CssSessionHandoffOut* out, CssSessionWindows* win) {
    if (!h) return CSS_ERR_INVALID_ARG;
    if (const char* e = window_shape_error(win)) return fail(h, CSS_ERR_INVALID_ARG, e);
    int64_t frames = 0;
    int rc = session_handoff_all_check(h, wav_dev, wav_ld, hcfg, out, true, &frames);
    if (rc != CSS_OK) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    SessWindowReq req;
    if ((rc = check_windows(h, win, frames, hcfg->n_mels, &req)) != CSS_OK) return rc;
    req.n_windows = win->n_windows;     // (host addresses: session_handoff_all_run maps or stages them)
    req.window_max = win->window_max;
    if ((rc = session_handoff_all_run(h, wav_dev, wav_ld, hcfg, out, &req)) != CSS_OK) return rc;
    h->window_sessions += 1;
    return CSS_OK;
}

int css_run_enqueue_windows(css_handle_t h, const float* pcm_host, int64_t n_samples, int32_t n_ch, const CssRunCfg* cfg,
                            float* wav_host, int64_t cap, const CssStreamHandoffCfg* hcfg, CssSessionHandoffOut* out,
                            CssSessionWindows* win) {
    if (!h || !pcm_host) return fail(h, CSS_ERR_INVALID_ARG, "null argument");
    SessHandoffReq req;
    int64_t n_out = 0;
    int rc = check_enqueue_windows(h, n_samples, n_ch, cfg, hcfg, out, win, &req, &n_out);
    if (rc != CSS_OK) return rc;
    if ((rc = enqueue_impl(h, pcm_host, nullptr, n_samples, n_ch, cfg, wav_host, nullptr, nullptr, wav_host ? cap : n_out, &req)) != CSS_OK) return rc;
    h->window_sessions += 1;
    return CSS_OK;
}

int css_run_enqueue_pcm16_windows(css_handle_t h, const int16_t* const* planes_host, int64_t n_samples, int32_t n_ch,
                                  const CssRunCfg* cfg, int16_t* wav_pcm16_host, int64_t cap, float* peaks_host,
                                  const CssStreamHandoffCfg* hcfg, CssSessionHandoffOut* out, CssSessionWindows* win) {
    if (!h || !planes_host || !wav_pcm16_host || n_samples < 1 || n_ch < 1) return fail(h, CSS_ERR_INVALID_ARG, "bad argument");
    SessHandoffReq req;
    int64_t n_out = 0;
    int rc = check_enqueue_windows(h, n_samples, n_ch, cfg, hcfg, out, win, &req, &n_out);
    if (rc != CSS_OK) return rc;
    if ((rc = enqueue_impl(h, nullptr, planes_host, n_samples, n_ch, cfg, nullptr, wav_pcm16_host, peaks_host, cap, &req)) != CSS_OK) return rc;
    h->window_sessions += 1;
    return CSS_OK;
}

int css_session_window_stats(css_handle_t h, int64_t* launches, int64_t* sessions) {
    if (!h) return CSS_ERR_INVALID_ARG;
    if (launches) *launches = h->window_launches;
    if (sessions) *sessions = h->window_sessions;
    return CSS_OK;
}
