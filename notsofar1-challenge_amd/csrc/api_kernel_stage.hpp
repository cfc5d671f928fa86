// Staging of caller arrays for the kernel entries (api_stream_kernels.hip, api_handoff_kernels.hip): every array in h->stage at a
// 256-byte boundary with 256 bytes of room on both sides, uploaded whole, the outputs downloaded whole.
#pragma once
#include <vector>

#include "api_ctx.hpp"
#include "../../include/css_mi355_stream_kernels.h"   // (CssKArray)

namespace css {
namespace kstage {

constexpr int64_t HOST_CAP = (int64_t)1 << 28;   // elements per array

// Byte offsets into h->stage: every region starts on 256 bytes and has 256 bytes of room on both sides.  Arrays are registered
// before the allocation, then uploaded whole; those marked `out` come back whole.
struct Stager {
    struct Slot { size_t at, bytes; void* host; bool out; };
    size_t bytes = 256;
    std::vector<Slot> slots;
    size_t take(const CssKArray& a, size_t el, bool out) {
        const size_t n = (size_t)a.elems * el, at = bytes;
        bytes += (n + 255) / 256 * 256 + 256;
        slots.push_back(Slot{at, n, a.p, out});
        return at;
    }
    size_t take_raw(void* host, size_t n, bool out) { return take(CssKArray{host, (int64_t)n}, 1, out); }
    hipError_t upload(char* base, hipStream_t st) const {
        for (const Slot& s : slots)
            if (s.bytes > 0)
                if (hipError_t e = hipMemcpyAsync(base + s.at, s.host, s.bytes, hipMemcpyHostToDevice, st)) return e;
        return hipStreamSynchronize(st);   // (the sources are pageable host memory of this call)
    }
    hipError_t download(char* base, hipStream_t st) const {
        for (const Slot& s : slots)
            if (s.out && s.bytes > 0)
                if (hipError_t e = hipMemcpyAsync(s.host, base + s.at, s.bytes, hipMemcpyDeviceToHost, st)) return e;
        return hipStreamSynchronize(st);
    }
};

inline bool arr_ok(const CssKArray& a, int64_t need) { return a.elems >= need && a.elems >= 0 && a.elems <= HOST_CAP && (a.elems == 0 || a.p); }

inline int stage_and_upload(css_ctx* h, const Stager& sg, char** base) {
    HIPCHK(h, hipSetDevice(h->device));
    int rc;
    if ((rc = ensure(h, h->stage, sg.bytes)) != CSS_OK) return rc;
    *base = (char*)h->stage.p;
    HIPCHK(h, sg.upload(*base, h->stream));
    return CSS_OK;
}
inline int download_all(css_ctx* h, const Stager& sg, char* base) {
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, sg.download(base, h->stream));
    HIPCHK(h, hipGetLastError());
    return CSS_OK;
}

}  // namespace kstage
}  // namespace css
