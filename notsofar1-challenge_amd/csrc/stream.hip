// The stitching tail of a streamed session (css_stream_*, api_stream.hip): the frames that became final in one push, over a
// bounded window of segment slots.  The offline kernels (stitch.hip) pick the first / last segment window from the local
// segment index and the session's segment count, and gate over the whole recording; a stream knows neither its length
// nor keeps its past.  These two kernels take a window base (global segment index of slot 0) and the global segment
// count (INT64_MAX while the stream is open: no segment is the last one yet), and reproduce the float32 operation order of
// ola_masks_kernel / morph_kernel / ola_stft_kernel exactly, so that every frame they produce is the offline frame bit for bit.
//   stream_activity_kernel   weighted overlap-add of the permuted masks, mean over frequency, threshold -> act_b
//   stream_gate_ola_kernel   dilate / erode of act_b (left halo from earlier pushes), weighted overlap-add of the permuted
//                            spectra, gating -> synthesis rows Y
#include <climits>

#include "kernels.hpp"

namespace css {

__device__ __forceinline__ float stream_seg_weight(const StreamStitchArgs& a, int64_t seg, int tl) {
    const int64_t g = a.seg_base + seg;   // css.py:258,290: first / last by the segment's place in the recording
    const float* w = g == 0 ? a.w_first : (g == a.num_segments_global - 1 ? a.w_last : a.w_mid);
    return w[tl];
}
// the segments of the window covering local frame t, ascending (as first_seg / last_seg of stitch.hip)
__device__ __forceinline__ void stream_cover(const StreamStitchArgs& a, int64_t t, int64_t* s0, int64_t* s1) {
    const int64_t lo = t - a.T + 1;
    *s0 = lo <= 0 ? 0 : (lo + a.hop - 1) / a.hop;
    const int64_t hi = t / a.hop;
    *s1 = hi < a.num_slots ? hi : a.num_slots - 1;
}

// ola_masks_kernel's block shape and reduction order: 16 frames x 16 frequency groups, float64 partial sums per group,
// the 16 groups added in a fixed order
constexpr int SA_T = 16, SA_FG = 16;
__global__ __launch_bounds__(256) void stream_activity_kernel(StreamStitchArgs a, int64_t t_lo, int64_t t_hi) {
    __shared__ double red[SA_FG][SA_T];
    const int s = blockIdx.y;
    const int lane = threadIdx.x & (SA_T - 1), fg = threadIdx.x / SA_T;
    const int64_t t = t_lo + (int64_t)blockIdx.x * SA_T + lane;
    const bool active = t < t_hi;
    double sum = 0.0;
    if (active) {
        int64_t s0, s1;
        stream_cover(a, t, &s0, &s1);
        float ws = 0.f;
        for (int64_t seg = s0; seg <= s1; ++seg) ws = __fadd_rn(ws, stream_seg_weight(a, seg, (int)(t - seg * a.hop)));
        for (int f = fg; f < a.F; f += SA_FG) {
            float v = 0.f;
            for (int64_t seg = s0; seg <= s1; ++seg) {
                const int tl = (int)(t - seg * a.hop);
                const float m = a.masks[((int64_t)a.perms[seg * a.S + s] * a.F + f) * a.mask_ld + seg * a.T + tl];
                v = __fadd_rn(v, __fmul_rn(stream_seg_weight(a, seg, tl), m));
            }
            sum += (double)__fdiv_rn(v, ws);
        }
    }
    red[fg][lane] = sum;
    __syncthreads();
    if (fg == 0 && active) {
        double tot = 0.0;
#pragma unroll
        for (int g = 0; g < SA_FG; ++g) tot += red[g][lane];
        const float act = (float)(tot / (double)a.F);
        a.act_b[(int64_t)s * a.ld_frames + t] = act >= a.activity_th ? 1 : 0;
    }
}

// morph_kernel twice (dilate with zeros outside the recording, erode with ones outside it), then ola_stft_kernel's
// overlap-add, division and gate, written as float32 synthesis rows.  Block = 16 frames of one stream.
constexpr int SG_T = 16;
__global__ __launch_bounds__(256) void stream_gate_ola_kernel(StreamStitchArgs a, int64_t t_lo, int64_t t_hi) {
    extern __shared__ __attribute__((aligned(16))) float tile[];   // [SG_T][2F + 1], then the dilated bits
    const int TS = 2 * a.F + 1;
    uint8_t* dil = reinterpret_cast<uint8_t*>(tile + SG_T * TS);   // [SG_T + 2 E]
    const int s = blockIdx.y;
    const int64_t t0 = t_lo + (int64_t)blockIdx.x * SG_T;
    const int tx = threadIdx.x & (SG_T - 1), fy = threadIdx.x >> 4;
    const int64_t t = t0 + tx;
    const bool active = t < t_hi;
    const uint8_t* row = a.act_b + (int64_t)s * a.ld_frames;
    const int64_t g_end = a.T_long_global - a.frame_base;   // local end of the recording (huge while the stream is open)
    const int nd = SG_T + 2 * a.erosion;
    for (int i = threadIdx.x; i < nd; i += blockDim.x) {
        const int64_t u = t0 - a.erosion + i;
        uint8_t v = 0;
        if (u + a.frame_base >= 0 && u < g_end)
            for (int64_t w = u - a.dilation; w <= u + a.dilation; ++w) {
                const uint8_t x = (w + a.frame_base < 0 || w >= g_end) ? 0 : row[w];
                v = v | x;
            }
        dil[i] = v;
    }
    __syncthreads();
    uint8_t keep = 1;
    if (active)
        for (int i = tx; i <= tx + 2 * a.erosion; ++i) {
            const int64_t u = t0 - a.erosion + i;
            const uint8_t x = (u + a.frame_base < 0 || u >= g_end) ? 1 : dil[i];
            keep = keep & x;
        }
    const float gate = active && keep ? 1.f : 0.f;
    const float2* sep = reinterpret_cast<const float2*>(a.sep);
    int64_t gs0 = 0, gs1 = -1;
    float wsum = 0.f;
    if (active) {
        stream_cover(a, t, &gs0, &gs1);
        for (int64_t seg = gs0; seg <= gs1; ++seg) wsum = __fadd_rn(wsum, stream_seg_weight(a, seg, (int)(t - seg * a.hop)));
    }
    for (int f = fy; f < a.F; f += 16) {
        float re = 0.f, im = 0.f;
        if (active) {
            for (int64_t seg = gs0; seg <= gs1; ++seg) {
                const int tl = (int)(t - seg * a.hop);
                const float w = stream_seg_weight(a, seg, tl);
                const float2 v = sep[((seg * a.S + a.perms[seg * a.S + s]) * (int64_t)a.F + f) * a.T + tl];
                re = __fadd_rn(re, __fmul_rn(w, v.x));
                im = __fadd_rn(im, __fmul_rn(w, v.y));
            }
            if (gs1 >= gs0) {
                re = __fmul_rn(__fdiv_rn(re, wsum), gate);
                im = __fmul_rn(__fdiv_rn(im, wsum), gate);
            }
        }
        tile[tx * TS + f] = re;
        tile[tx * TS + a.F + f] = im;
    }
    __syncthreads();
    for (int r = 0; r < SG_T; ++r) {
        if (t0 + r >= t_hi) break;
        float* out = a.Y + ((int64_t)s * a.ld_frames + t0 + r) * a.KIp;
        for (int j = threadIdx.x; j < a.KIp; j += 256) out[j] = j < 2 * a.F ? tile[r * TS + j] : 0.f;
    }
}

void launch_stream_activity(const StreamStitchArgs& a, int64_t t_lo, int64_t t_hi, hipStream_t s) {
    if (t_hi <= t_lo) return;
    hipLaunchKernelGGL(stream_activity_kernel, dim3((unsigned)((t_hi - t_lo + SA_T - 1) / SA_T), a.S), dim3(SA_T * SA_FG), 0, s,
                       a, t_lo, t_hi);
}

void launch_stream_gate_ola(const StreamStitchArgs& a, int64_t t_lo, int64_t t_hi, hipStream_t s) {
    if (t_hi <= t_lo) return;
    const size_t lds = (size_t)SG_T * (2 * a.F + 1) * sizeof(float) + (size_t)SG_T + 2 * (size_t)a.erosion;
    hipLaunchKernelGGL(stream_gate_ola_kernel, dim3((unsigned)((t_hi - t_lo + SG_T - 1) / SG_T), a.S), dim3(256), lds, s,
                       a, t_lo, t_hi);
}

}  // namespace css
