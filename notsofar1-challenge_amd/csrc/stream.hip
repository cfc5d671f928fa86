// The stitching tail of a streamed session (css_stream_*, api_stream.hip): the frames that became final in one push, over a
// bounded window of segment slots.  The offline kernels (stitch.hip) pick the first / last segment window from the local
// segment index and the session's segment count, and gate over the whole recording; a stream knows neither its length
// nor keeps its past.  These two kernels take a window base (global segment index of slot 0) and the global segment
// count (INT64_MAX while the stream is open: no segment is the last one yet).  Covering segments, weights, the overlap-add
// walk and the frequency mean are the functions of stitch_common.hpp that ola_masks_kernel<0> / ola_stft_kernel<0> call, and
// the gate reproduces morph_kernel, so that every frame they produce is the offline frame bit for bit.
//   stream_activity_kernel   weighted overlap-add of the permuted masks, mean over frequency, threshold -> act_b
//   stream_gate_ola_kernel   dilate / erode of act_b (left halo from earlier pushes), weighted overlap-add of the permuted
//                            spectra, gating -> synthesis rows Y (and, for a stream with the hand-off on, the gate bytes)
// Both are table launches (table.hpp): up to STREAM_MULTI_MAX streams' windows and frame ranges
// by value, blockIdx.z selects the entry, blocks past an entry's range return at once.  One stream is a table of one entry,
// so there is one copy of each body and one kernel for css_stream_push, css_stream_push_many and css_stream_finish.
//   stream_scatter_masks_kernel   the mask columns of an estimator batch shared by several streams -> each stream's window
//   stream_ingest_pcm16_kernel    the int16 pieces of a round, interleaved or planar -> float32 rows of each stream's window
#include <algorithm>
#include <climits>

#include "kernels.hpp"
#include "stitch_common.hpp"
#include "table.hpp"

namespace css {

struct StreamEntry { StreamStitchArgs a; StreamFrames r; };
struct StreamMulti : Table<StreamEntry, STREAM_MULTI_MAX> {};

// ola_masks_kernel<0> without the stitched masks themselves: only the activity bits leave
__device__ __forceinline__ void stream_activity_body(const StreamStitchArgs& a, int64_t t_lo, int64_t t_hi) {
    const int s = blockIdx.y;
    const int lane = threadIdx.x & (OLA_T - 1), fg = threadIdx.x / OLA_T;
    const int64_t t = t_lo + (int64_t)blockIdx.x * OLA_T + lane;
    const bool active = t < t_hi;
    double sum = 0.0;
    if (active) {
        int64_t s0, s1;
        covering(a, t, &s0, &s1);
        const float ws = ola_weight_sum(a, t, s0, s1);
        for (int f = fg; f < a.F; f += OLA_FG) sum += (double)ola_mask_value(a, s, f, t, s0, s1, ws);
    }
    ola_activity(sum, fg, lane, active, a.F, a.activity_th, [&](float, uint8_t on) { a.act_b[(int64_t)s * a.ld_frames + t] = on; });
}

__global__ __launch_bounds__(256) void stream_activity_kernel(StreamMulti m) {
    const StreamFrames r = m.e[blockIdx.z].r;
    if (r.t_lo + (int64_t)blockIdx.x * OLA_T >= r.t_hi) return;
    stream_activity_body(m.e[blockIdx.z].a, r.t_lo, r.t_hi);
}

// morph_kernel twice (dilate with zeros outside the recording, erode with ones outside it), then ola_stft_kernel<0>'s
// overlap-add, division and gate, written as float32 synthesis rows.  Block = OLA_T frames of one stream.
__device__ __forceinline__ void stream_gate_ola_body(const StreamStitchArgs& a, int64_t t_lo, int64_t t_hi) {
    extern __shared__ __attribute__((aligned(16))) float tile[];   // [OLA_T][2F + 1], then the dilated bits
    const int TS = 2 * a.F + 1;
    uint8_t* dil = reinterpret_cast<uint8_t*>(tile + OLA_T * TS);   // [OLA_T + 2 E]
    const int s = blockIdx.y;
    const int64_t t0 = t_lo + (int64_t)blockIdx.x * OLA_T;
    const int tx = threadIdx.x & (OLA_T - 1), fy = threadIdx.x >> 4;
    const int64_t t = t0 + tx;
    const bool active = t < t_hi;
    const uint8_t* row = a.act_b + (int64_t)s * a.ld_frames;
    const int64_t g_end = a.T_long_global - a.frame_base;   // local end of the recording (huge while the stream is open)
    const int nd = OLA_T + 2 * a.erosion;
    for (int i = threadIdx.x; i < nd; i += blockDim.x) {
        const int64_t u = t0 - a.erosion + i;
        uint8_t v = 0;
        if (u + a.frame_base >= 0 && u < g_end)
            for (int64_t w = u - a.dilation; w <= u + a.dilation; ++w) {
                // (w >= ld_frames: only lanes at or above t_hi get there -- the block dilates whole -- and the row ends at ld_frames)
                const uint8_t x = (w + a.frame_base < 0 || w >= g_end || w >= a.ld_frames) ? 0 : row[w];
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
    if (a.gate_out && active && fy == 0) a.gate_out[(int64_t)s * a.gate_ld + ((t + a.frame_base) & a.gate_mask)] = keep;
    int64_t gs0 = 0, gs1 = -1;
    float wsum = 0.f;
    if (active) {
        covering(a, t, &gs0, &gs1);
        wsum = ola_weight_sum(a, t, gs0, gs1);
    }
    for (int f = fy; f < a.F; f += 16) {
        const float2 v = active ? ola_spec_value(a, s, f, t, gs0, gs1, wsum, gate) : make_float2(0.f, 0.f);
        tile[tx * TS + f] = v.x;
        tile[tx * TS + a.F + f] = v.y;
    }
    __syncthreads();
    for (int r = 0; r < OLA_T; ++r) {
        if (t0 + r >= t_hi) break;
        float* out = a.Y + ((int64_t)s * a.ld_frames + t0 + r) * a.KIp;
        for (int j = threadIdx.x; j < a.KIp; j += 256) out[j] = j < 2 * a.F ? tile[r * TS + j] : 0.f;
    }
}

__global__ __launch_bounds__(256) void stream_gate_ola_kernel(StreamMulti m) {
    const StreamFrames r = m.e[blockIdx.z].r;
    if (r.t_lo + (int64_t)blockIdx.x * OLA_T >= r.t_hi) return;
    stream_gate_ola_body(m.e[blockIdx.z].a, r.t_lo, r.t_hi);
}

// The mask head of a shared batch writes ONE matrix [rows][src_ld] (time fastest, batch segment c at column c T); stream e's
// segments are n_cols consecutive columns of it and belong at a column of that stream's own window matrix.  Rows are runs of
// T floats (186: not a multiple of 4) whose source and destination columns differ mod 4, so neither side can be 16-byte
// aligned for more than one row in four: a wave copies one row with dword loads and stores, 64 consecutive floats per
// access (256 contiguous bytes on both sides).  It is 0.77 MB per segment behind an estimator pass of milliseconds.
constexpr int SC_ENTRIES = 16, SC_ROWS = 4;
struct MaskScatterTable : Table<MaskScatter, SC_ENTRIES> {};
__global__ __launch_bounds__(64 * SC_ROWS) void stream_scatter_masks_kernel(const float* __restrict__ src, int64_t src_ld, int rows,
                                                                            MaskScatterTable tab) {
    const MaskScatter e = tab.e[blockIdx.y];
    const int row = blockIdx.x * SC_ROWS + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* __restrict__ in = src + (int64_t)row * src_ld + e.src_col;
    float* __restrict__ out = e.dst + (int64_t)row * e.dst_ld;
    for (int64_t c = lane; c < e.n_cols; c += 64) out[c] = in[c];
}

// The PCM16 pieces of a round (css_stream_push_many_pcm16): int16 in device staging -> float32 rows of each stream's sample
// window, the scaling of pcm16_to_cm_kernel ((float)q * 2^-15, exact).  A table launch: blockIdx.y = entry, a block takes
// `tile` samples of all channels, blocks past an entry's n return at once.  A planar entry (and one channel) needs no LDS:
// lane i converts sample i of a channel, a wave reads 128 contiguous bytes and writes 64 consecutive dwords.  An interleaved
// row is 2 C bytes (14 for 7 channels), so the block copies its contiguous span of tile * C values into LDS with 16-byte
// loads (tile is a multiple of 8 and the staging 16-byte aligned, so every span starts aligned; the last values of the last
// span go one by one) and then writes channel after channel from there.  The destination column is arbitrary mod 4 (any
// number of samples was pushed before), so the stores are dwords, 64 consecutive ones per wave, as in
// stream_scatter_masks_kernel.
constexpr int IN_THREADS = 256, IN_TILE_MAX = 1024, IN_LDS_MAX = 32768;
struct StreamIngestTable : Table<StreamIngestPcm16, STREAM_MULTI_MAX> {};
__global__ __launch_bounds__(IN_THREADS) void stream_ingest_pcm16_kernel(StreamIngestTable tab, int tile) {
    extern __shared__ __attribute__((aligned(16))) int16_t span[];   // [tile][C] of an interleaved entry
    const StreamIngestPcm16 e = tab.e[blockIdx.y];
    const int64_t i0 = (int64_t)blockIdx.x * tile;
    if (i0 >= e.n) return;
    const int nt = (int)(e.n - i0 < tile ? e.n - i0 : tile);
    const float scale = 1.0f / 32768.0f;
    float* __restrict__ out = e.dst + i0;
    if (e.plane_ld > 0 || e.C == 1) {
        for (int c = 0; c < e.C; ++c) {
            const int16_t* __restrict__ in = e.src + (int64_t)c * e.plane_ld + i0;
            float* __restrict__ o = out + (int64_t)c * e.dst_ld;
            for (int i = threadIdx.x; i < nt; i += IN_THREADS) o[i] = __fmul_rn((float)in[i], scale);
        }
        return;
    }
    const int total = nt * e.C;
    const int16_t* __restrict__ in = e.src + i0 * e.C;
    const uint4* __restrict__ in16 = reinterpret_cast<const uint4*>(in);
    uint4* span16 = reinterpret_cast<uint4*>(span);
    for (int v = threadIdx.x; v < total / 8; v += IN_THREADS) span16[v] = in16[v];
    for (int j = (total & ~7) + threadIdx.x; j < total; j += IN_THREADS) span[j] = in[j];
    __syncthreads();
    for (int c = 0; c < e.C; ++c) {
        float* __restrict__ o = out + (int64_t)c * e.dst_ld;
        for (int i = threadIdx.x; i < nt; i += IN_THREADS) o[i] = __fmul_rn((float)span[i * e.C + c], scale);
    }
}

void launch_stream_ingest_pcm16_multi(const StreamIngestPcm16* e, int n, hipStream_t s) {
    for_each_table<StreamIngestTable>(e, n, [&](const StreamIngestTable& tab, int cnt) {
        const int64_t most = table_max(tab, cnt, (int64_t)0, [](const StreamIngestPcm16& p) { return p.n; });
        const int C = table_max(tab, cnt, 1, [](const StreamIngestPcm16& p) { return p.C; });
        // the largest multiple of 64 samples whose interleaved span fits IN_LDS_MAX (at least 64: C is 1 or 7 here)
        const int tile = std::max(64, std::min(IN_TILE_MAX, IN_LDS_MAX / (2 * C) / 64 * 64));
        if (most > 0)
            hipLaunchKernelGGL(stream_ingest_pcm16_kernel, dim3((unsigned)((most + tile - 1) / tile), cnt), dim3(IN_THREADS),
                               (size_t)tile * C * sizeof(int16_t), s, tab, tile);
        return true;
    });
}

static int64_t most_frames(const StreamMulti& m, int cnt) {
    return table_max(m, cnt, (int64_t)0, [](const StreamEntry& e) { return e.r.t_hi - e.r.t_lo; });
}

void launch_stream_activity_multi(const StreamStitchArgs* a, const StreamFrames* r, int n, hipStream_t s) {
    for_each_table<StreamMulti>(n, [&](int i) { return StreamEntry{a[i], r[i]}; }, [&](const StreamMulti& m, int cnt) {
        const int64_t most = most_frames(m, cnt);
        if (most > 0)
            hipLaunchKernelGGL(stream_activity_kernel, dim3((unsigned)((most + OLA_T - 1) / OLA_T), m.e[0].a.S, cnt), dim3(OLA_T * OLA_FG), 0, s, m);
        return true;
    });
}

void launch_stream_gate_ola_multi(const StreamStitchArgs* a, const StreamFrames* r, int n, hipStream_t s) {
    for_each_table<StreamMulti>(n, [&](int i) { return StreamEntry{a[i], r[i]}; }, [&](const StreamMulti& m, int cnt) {
        const int64_t most = most_frames(m, cnt);
        // the dynamic LDS of the launch is the largest entry's
        const int erosion = table_max(m, cnt, 0, [](const StreamEntry& e) { return e.a.erosion; });
        const size_t lds = (size_t)OLA_T * (2 * m.e[0].a.F + 1) * sizeof(float) + (size_t)OLA_T + 2 * (size_t)erosion;
        if (most > 0)
            hipLaunchKernelGGL(stream_gate_ola_kernel, dim3((unsigned)((most + OLA_T - 1) / OLA_T), m.e[0].a.S, cnt), dim3(256), lds, s, m);
        return true;
    });
}

void launch_stream_activity(const StreamStitchArgs& a, int64_t t_lo, int64_t t_hi, hipStream_t s) {
    const StreamFrames r{t_lo, t_hi};
    launch_stream_activity_multi(&a, &r, 1, s);
}
void launch_stream_gate_ola(const StreamStitchArgs& a, int64_t t_lo, int64_t t_hi, hipStream_t s) {
    const StreamFrames r{t_lo, t_hi};
    launch_stream_gate_ola_multi(&a, &r, 1, s);
}

void launch_stream_scatter_masks(const float* src, int64_t src_ld, int rows, const MaskScatter* e, int n, hipStream_t s) {
    for_each_table<MaskScatterTable>(e, n, [&](const MaskScatterTable& tab, int cnt) {
        hipLaunchKernelGGL(stream_scatter_masks_kernel, dim3((unsigned)((rows + SC_ROWS - 1) / SC_ROWS), cnt), dim3(64 * SC_ROWS), 0, s,
                           src, src_ld, rows, tab);
        return true;
    });
}

}  // namespace css
