// The stitching arithmetic that the offline kernels (stitch.hip: StitchArgs, a whole recording) and the stream kernels
// (stream.hip: StreamStitchArgs, a window of segment slots) have in common: which segments cover a frame and with what weight,
// the weighted overlap-add of one mask or spectrum value over them, and the mean over frequency behind the activity gate.
// Both units call THESE functions, so a streamed frame is the offline frame by construction.  The float32 operation order is
// the reference's `zeros += w * x` (css.py:254-299): multiply, add in ascending segment order starting from zero, divide -- and
// the contraction-free helpers of kernels.hpp are the only arithmetic here, so no FMA changes a bit.
// (The walk is the general one, for any number of covering segments; stitch.hip keeps tuned forms for up to two and four.)
#pragma once
#include "kernels.hpp"

namespace css {

// block shape of the overlap-add kernels: 16 frames (lanes run over time) x 16 frequency groups (a 60 s meeting is only 3749
// frames: 64-frame blocks gave 177 blocks for 256 CUs)
constexpr int OLA_T = 16, OLA_FG = 16;

// ---- a segment's weight at its local frame tl (css.py:258,290: first / last by the segment's place in the recording)
__device__ __forceinline__ float seg_weight(const StitchArgs& a, int64_t seg, int tl) {
    const float* w = seg == 0 ? a.w_first : (seg == a.num_segments - 1 ? a.w_last : a.w_mid);
    return w[tl];
}
__device__ __forceinline__ float seg_weight(const StreamStitchArgs& a, int64_t seg, int tl) {
    const int64_t g = a.seg_base + seg;   // slot `seg` of the window is segment g of the recording
    const float* w = g == 0 ? a.w_first : (g == a.num_segments_global - 1 ? a.w_last : a.w_mid);
    return w[tl];
}

// ---- the segments covering frame t, ascending: [*s0, *s1] (segments of the recording / slots of the window)
__device__ __forceinline__ void covering(const StitchArgs& a, int64_t t, int64_t* s0, int64_t* s1) {
    const int64_t lo = t - a.T + 1;
    *s0 = lo <= 0 ? 0 : (lo + a.hop - 1) / a.hop;
    const int64_t hi = t / a.hop;
    *s1 = hi < a.num_segments ? hi : a.num_segments - 1;
}
__device__ __forceinline__ void covering(const StreamStitchArgs& a, int64_t t, int64_t* s0, int64_t* s1) {
    const int64_t lo = t - a.T + 1;
    *s0 = lo <= 0 ? 0 : (lo + a.hop - 1) / a.hop;
    const int64_t hi = t / a.hop;
    *s1 = hi < a.num_slots ? hi : a.num_slots - 1;
}

// ---- the walk over [s0, s1], A = StitchArgs or StreamStitchArgs
template <class A>
__device__ __forceinline__ float ola_weight_sum(const A& a, int64_t t, int64_t s0, int64_t s1) {
    float ws = 0.f;
    for (int64_t seg = s0; seg <= s1; ++seg) ws = css_add_rn(ws, seg_weight(a, seg, (int)(t - seg * a.hop)));
    return ws;
}
// stitched mask of (stream s, bin f, frame t); ws = ola_weight_sum
template <class A>
__device__ __forceinline__ float ola_mask_value(const A& a, int s, int f, int64_t t, int64_t s0, int64_t s1, float ws) {
    float v = 0.f;
    for (int64_t seg = s0; seg <= s1; ++seg) {
        const int tl = (int)(t - seg * a.hop);
        const float m = a.masks[((int64_t)a.perms[seg * a.S + s] * a.F + f) * a.mask_ld + seg * a.T + tl];
        v = css_add_rn(v, css_mul_rn(seg_weight(a, seg, tl), m));
    }
    return css_div_rn(v, ws);
}
// stitched and gated spectrum value (Re, Im) of (stream s, bin f, frame t); a frame nothing covers stays zero
template <class A>
__device__ __forceinline__ float2 ola_spec_value(const A& a, int s, int f, int64_t t, int64_t s0, int64_t s1, float ws, float gate) {
    const float2* sep = reinterpret_cast<const float2*>(a.sep);
    float re = 0.f, im = 0.f;
    for (int64_t seg = s0; seg <= s1; ++seg) {
        const int tl = (int)(t - seg * a.hop);
        const float w = seg_weight(a, seg, tl);
        const float2 v = sep[((seg * a.S + a.perms[seg * a.S + s]) * (int64_t)a.F + f) * a.T + tl];
        re = css_add_rn(re, css_mul_rn(w, v.x));
        im = css_add_rn(im, css_mul_rn(w, v.y));
    }
    if (s1 >= s0) {
        re = css_mul_rn(css_div_rn(re, ws), gate);
        im = css_mul_rn(css_div_rn(im, ws), gate);
    }
    return make_float2(re, im);
}

// ---- activity of the block's frames (css.py:303-304): the mean over frequency of the stitched mask, against the threshold.
// Every thread of the block calls it with the float64 sum of its frequency group (fg) at its frame (lane); the 16 groups are
// added in a fixed order; out(activity, activity >= th) runs in the thread that owns the frame, if the frame is `active`.
template <class Out>
__device__ __forceinline__ void ola_activity(double sum, int fg, int lane, bool active, int F, float th, Out&& out) {
    __shared__ double red[OLA_FG][OLA_T];
    red[fg][lane] = sum;
    __syncthreads();
    if (fg == 0 && active) {
        double tot = 0.0;
#pragma unroll
        for (int g = 0; g < OLA_FG; ++g) tot += red[g][lane];
        const float act = (float)(tot / (double)F);
        out(act, (uint8_t)(act >= th ? 1 : 0));
    }
}

}  // namespace css
