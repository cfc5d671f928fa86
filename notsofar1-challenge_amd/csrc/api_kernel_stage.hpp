// Staging of caller arrays for every kernel entry (api_gemm_kernels.hip, api_encoder.hip, api_frontend.hip, api_backend.hip,
// api_rate_kernels.hip, api_stream_kernels.hip, api_handoff_kernels.hip): every array in h->stage at a 256-byte boundary with
// 256 bytes of room on both sides, uploaded whole, the outputs downloaded whole.
#pragma once
#include <vector>

#include "api_ctx.hpp"
#include "../../include/css_mi355_stream_kernels.h"   // (CssKArray)

namespace css {
namespace kstage {

constexpr int64_t HOST_CAP = (int64_t)1 << 28;   // elements per array: far below the kernels' 32-bit offsets and grids

enum : unsigned { UP = 1, DOWN = 2 };   // the copies of a caller array: before the launch, after it

// Byte offsets into h->stage: every region starts on 256 bytes and has 256 bytes of room on both sides, so no region has
// offset 0, which stands for an absent array (dev() makes a null pointer of it).  Regions are registered before the allocation;
// upload() copies those with a host source whole and fills those with a fill word, download() brings those with a host
// destination back whole.  The size, the place and both copies of a region come from its one slot.
struct Stager {
    struct Slot { size_t at, bytes; const void* up; void* down; bool fill; uint32_t word; };
    size_t bytes = 256;
    std::vector<Slot> slots;
    // `lead + n` bytes, of which the n behind `lead` (a source offset, in bytes) are copied: from `up` and to `down`, where they
    // are not null.  The host side may be a local of the entry (a level word, a table built for the call) or a descriptor
    // field: upload() and download() synchronise before they return.
    size_t region(size_t n, const void* up, void* down, size_t lead = 0) {
        const size_t at = bytes;
        bytes += (lead + n + 255) / 256 * 256 + 256;
        slots.push_back(Slot{at + lead, n, up, down, false, 0});
        return at;
    }
    size_t take(const CssKArray& a, size_t el, bool out) { return region((size_t)a.elems * el, a.p, out ? a.p : nullptr); }
    size_t take_raw(void* host, size_t n, bool out) { return region(n, host, out ? host : nullptr); }
    // a caller array by pointer, absent when the pointer is null
    size_t arr(const void* p, int64_t elems, size_t el, unsigned dir) {
        return p ? region((size_t)elems * el, dir & UP ? p : nullptr, dir & DOWN ? const_cast<void*>(p) : nullptr) : 0;
    }
    // device only: what the launch leaves there between its kernels
    size_t scratch(int64_t elems, size_t el) { return region((size_t)elems * el, nullptr, nullptr); }
    // `words` 32-bit words filled with `word`, not uploaded; downloaded to `down` where it is not null
    size_t filled(int64_t words, uint32_t word, void* down) {
        const size_t at = region((size_t)words * 4, nullptr, down);
        slots.back().fill = true; slots.back().word = word;
        return at;
    }
    template <class T> static T* dev(char* base, size_t at) { return at ? reinterpret_cast<T*>(base + at) : nullptr; }

    hipError_t upload(char* base, hipStream_t st) const {
        for (const Slot& s : slots) {
            if (s.up && s.bytes > 0)
                if (hipError_t e = hipMemcpyAsync(base + s.at, s.up, s.bytes, hipMemcpyHostToDevice, st)) return e;
            if (s.fill && s.bytes > 0)
                if (hipError_t e = hipMemsetD32Async((hipDeviceptr_t)(base + s.at), (int)s.word, s.bytes / 4, st)) return e;
        }
        return hipStreamSynchronize(st);   // (the sources are pageable host memory of this call)
    }
    hipError_t download(char* base, hipStream_t st) const {
        for (const Slot& s : slots)
            if (s.down && s.bytes > 0)
                if (hipError_t e = hipMemcpyAsync(s.down, base + s.at, s.bytes, hipMemcpyDeviceToHost, st)) return e;
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
