// The element stores of the kernels that write rows into a caller's float32 or float16 device memory (handoff.hip: encoder
// windows; nemo_stream.hip: NeMo chunks): one element, and 16 bytes of them at a 16-byte boundary.  float16 is the float32 value
// rounded to nearest-even.
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

namespace css {

template <typename T> struct WindowVec;
template <> struct WindowVec<float> {
    static constexpr int V = 4;
    static __device__ __forceinline__ void store(float* p, float v) { *p = v; }
    static __device__ __forceinline__ void store16(float* p, const float* v) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    }
};
template <> struct WindowVec<__half> {
    static constexpr int V = 8;
    static __device__ __forceinline__ void store(__half* p, float v) { *p = __float2half_rn(v); }
    static __device__ __forceinline__ void store16(__half* p, const float* v) {
        auto two = [&](int i) {
            return (uint32_t)__half_as_ushort(__float2half_rn(v[i])) | ((uint32_t)__half_as_ushort(__float2half_rn(v[i + 1])) << 16);
        };
        *reinterpret_cast<uint4*>(p) = make_uint4(two(0), two(2), two(4), two(6));
    }
};

}  // namespace css
