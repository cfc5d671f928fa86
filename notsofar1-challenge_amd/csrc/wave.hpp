// Reductions over the 64 lanes of a wave; every lane gets the result.  Two kinds, and a kernel keeps the kind it has: they
// add in different orders, so their sums differ in the last bits.
//   wave_sum_dpp       four DPP steps inside each row of 16 lanes (quad swaps, then the 8- and 16-lane mirrors), then the four
//                      row totals through scalar registers.  No LDS.
//   wave_sum_shfl /    the __shfl_xor butterfly.  __shfl_xor compiles to ds_bpermute: six dependent LDS round trips
//   wave_max_shfl      (~100 cycles each) per value.
#pragma once
#include <hip/hip_runtime.h>

namespace css {

// v + the value of the partner lane under DPP control CTRL
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
// the partner lane's value under DPP control CTRL
template <int CTRL>
__device__ __forceinline__ double dpp_get(double v) {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    return __hiloint2double(__builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, false),
                            __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, false));
}
template <int CTRL>
__device__ __forceinline__ double dpp_add(double v) { return v + dpp_get<CTRL>(v); }

// sum over the 16 lanes of a DPP row; every lane of the row ends up with the row's total
template <typename T>
__device__ __forceinline__ T row16_sum(T v) {
    v = dpp_add<0xB1>(v);    // quad_perm [1,0,3,2]
    v = dpp_add<0x4E>(v);    // quad_perm [2,3,0,1]
    v = dpp_add<0x141>(v);   // row_half_mirror: lane i <-> 7 - i
    v = dpp_add<0x140>(v);   // row_mirror:      lane i <-> 15 - i
    return v;
}

__device__ __forceinline__ float wave_sum_dpp(float v) {
    v = row16_sum(v);
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return (r0 + r1) + (r2 + r3);
}
__device__ __forceinline__ double wave_sum_dpp(double v) {
    v = row16_sum(v);
    const int lo = __double2loint(v), hi = __double2hiint(v);
    double r[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = __hiloint2double(__builtin_amdgcn_readlane(hi, 16 * i), __builtin_amdgcn_readlane(lo, 16 * i));
    return (r[0] + r[1]) + (r[2] + r[3]);
}

template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce_shfl(T v, Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o));
    return v;
}
template <typename T>   // float, double or an integer count
__device__ __forceinline__ T wave_sum_shfl(T v) { return wave_reduce_shfl(v, [](T a, T b) { return a + b; }); }
__device__ __forceinline__ float wave_max_shfl(float v) { return wave_reduce_shfl(v, [](float a, float b) { return fmaxf(a, b); }); }

}  // namespace css
