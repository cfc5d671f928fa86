// The NeMo hand-off of STREAMED sessions (include/css_mi355_stream_nemo.h; DESIGN.md 7b "The NeMo hand-off of a stream"): the
// append kernel and the multi-owner mel kernel of a round (kernels.hpp NemoAppend, NemoMel).  The product between them is
// launch_gemm on the offline path's [514][512] analysis matrix; the tile is the offline path's (nemo_tile.hpp).  The mel kernel
// also keeps a stream's frame history, and nemo_chunk_kernel turns spans of it into a consumer's chunks
// (include/css_mi355_nemo_chunk.h; DESIGN.md 7b "NeMo chunks out of the frame history").
#include "kernels.hpp"
#include "nemo_tile.hpp"
#include "table.hpp"
#include "window_vec.hpp"

namespace css {

struct NemoAppendTable : Table<NemoAppend, HANDOFF_MULTI_MAX> {};
struct NemoMelTable : Table<NemoMel, HANDOFF_MULTI_MAX> {};

// One block per (stream, speaker); handoff_append_kernel's round for NeMo's operand.  The block-membership test and the
// compaction of the kept blocks of [D0, D1) behind sample A0 are that kernel's.  A sample is pre-emphasised as it is compacted:
// its predecessor is the sample before it in its block, for a block's first sample the last sample of the kept block before it
// in this round (a kept block with a successor is whole: only the round's last block can be cut, by a closing D1), for the
// round's first kept sample the speaker's carried x_last, and concatenation sample 0 has none.  Operand column x is
// y[160 J0 - 256 + x]: the carried tail, the new samples, zeros before the recording's start and from y[A1] on.
__global__ __launch_bounds__(256) void nemo_append_kernel(NemoAppendTable tab, float* __restrict__ operand) {
    const NemoAppend& ne = tab.e[blockIdx.z];
    const HandoffAppend& e = ne.a;
    const int k = blockIdx.y, tid = threadIdx.x;
    constexpr int HOP = 256;
    __shared__ int len[256], off[256];
    __shared__ int64_t prev[256];   // the round's last kept block before block c0 + b, or -1
    __shared__ int total;
    __shared__ int64_t last_kept;   // the round's last kept block so far, or -1 (thread 0's)
    const int64_t A0 = e.st[k].A, J0 = e.st[k].J;
    const int64_t base = (int64_t)NEMO_HOP * J0 - NEMO_NFFT / 2;   // the concatenation index of operand column 0 (and of tail_in[0])
    float* __restrict__ op = operand + (e.row0 + (int64_t)k * e.rows) * NEMO_HOP;
    const int64_t op_n = e.rows * NEMO_HOP;
    const uint8_t* __restrict__ gate = e.gate + (int64_t)k * e.gate_ld;
    const float* __restrict__ out = e.out + (int64_t)k * e.out_ld;
    const float* __restrict__ carry = e.carry_in + (int64_t)k * e.carry_ld;
    const float* __restrict__ tail_in = e.tail_in + (int64_t)k * NEMO_TAIL_LD;
    const float p = ne.preemph;
    auto sample = [&](int64_t n) { return n >= e.out_base ? out[n - e.out_base] : carry[n - e.D0]; };
    if (tid == 0) last_kept = -1;
    // ---- the kept blocks of [D0, D1), pre-emphasised and compacted behind sample A0 of the concatenation
    int64_t A1 = A0;
    const int64_t q_lo = e.D0 / HOP, q_hi = (e.D1 + HOP - 1) / HOP;
    for (int64_t c0 = q_lo; c0 < q_hi; c0 += 256) {
        const int64_t q = c0 + tid;
        int n = 0;
        if (q < q_hi) {
            bool keep = !e.drop;
            if (e.drop) {
                const int64_t t_lo = q - e.pad - 1 < 0 ? 0 : q - e.pad - 1, t_hi = q + e.pad < e.t_g1 - 1 ? q + e.pad : e.t_g1 - 1;
                for (int64_t t = t_lo; t <= t_hi; ++t) keep = keep || gate[t & e.gate_mask] != 0;
            }
            if (keep) n = (int)(((q + 1) * HOP < e.D1 ? (q + 1) * HOP : e.D1) - q * HOP);
        }
        len[tid] = n;
        __syncthreads();
        if (tid == 0) {
            int acc = 0;
            int64_t lk = last_kept;
            for (int i = 0; i < 256; ++i) {
                off[i] = acc; prev[i] = lk;
                if (len[i] > 0) lk = c0 + i;
                acc += len[i];
            }
            total = acc;
            last_kept = lk;
        }
        __syncthreads();
        for (int i = tid; i < 256 * HOP; i += 256) {
            const int b = i >> 8, r = i & (HOP - 1);
            if (r < len[b]) {
                const int64_t c = A1 + off[b] + r, n_src = (c0 + b) * HOP + r;
                float v = sample(n_src);
                if (p != 0.f && c > 0) {
                    const float before = r > 0 ? sample(n_src - 1) : prev[b] >= 0 ? sample((prev[b] + 1) * HOP - 1) : ne.xlast_in[k];
                    v = css_add_rn(v, -css_mul_rn(p, before));
                }
                const int64_t x = c - base;
                if (x < op_n) op[x] = v;
            }
        }
        A1 += total;
        __syncthreads();
    }
    // ---- frames complete now; the rest of the operand: what the tail carried, zeros
    const int64_t J1 = e.closing ? A1 / NEMO_HOP : (A1 >= NEMO_NFFT / 2 ? (A1 - NEMO_NFFT / 2) / NEMO_HOP + 1 : 0);
    for (int64_t x = tid; x < op_n; x += 256) {
        const int64_t c = base + x;
        if (c >= A0 && c < A1) continue;   // a new sample in its own place, written above
        op[x] = c >= 0 && c < A0 && x < NEMO_TAIL_LD ? tail_in[x] : 0.f;
    }
    __syncthreads();
    const int64_t tail1 = (int64_t)NEMO_HOP * J1 - NEMO_NFFT / 2;
    float* __restrict__ tail_out = e.tail_out + (int64_t)k * NEMO_TAIL_LD;
    for (int64_t i = tid; tail1 + i < A1 && i < NEMO_TAIL_LD; i += 256) {
        const int64_t x = tail1 + i - base;   // (J1 >= J0 for every state of a stream: not negative)
        tail_out[i] = tail1 + i < 0 || x < 0 || x >= op_n ? 0.f : op[x];
    }
    // ---- the samples still undecided, for the next round; the gate bytes of the round; the last kept sample; the counts
    const int64_t end = e.t_g1 * HOP;
    float* __restrict__ carry_out = e.carry_out + (int64_t)k * e.carry_ld;
    for (int64_t n = e.D1 + tid; n < end; n += 256) carry_out[n - e.D1] = sample(n);
    uint8_t* __restrict__ act = e.act_out + (int64_t)k * (e.t_g1 - e.t_g0);
    for (int64_t t = e.t_g0 + tid; t < e.t_g1; t += 256) act[t - e.t_g0] = gate[t & e.gate_mask];
    if (tid == 0) {
        const int64_t lk = last_kept;
        ne.xlast_out[k] = lk >= 0 ? sample(((lk + 1) * HOP < e.D1 ? (lk + 1) * HOP : e.D1) - 1) : ne.xlast_in[k];
        e.st_out[k].A = A1;
        e.st_out[k].J = J1;
        e.n_new[k] = (int)(J1 - J0);
    }
}

// nemo_mel_kernel for the owners of a round: frame counts from device memory, tiles past a count return at once
__global__ __launch_bounds__(256) void nemo_mel_multi_kernel(NemoMelTable tab, const float* __restrict__ spec, int64_t ld) {
    const NemoMel& e = tab.e[blockIdx.z];
    const int k = blockIdx.y;
    const int64_t nfr = e.n_new[k] < e.rows ? e.n_new[k] : e.rows, j0 = (int64_t)blockIdx.x * NEMO_TILE_FRAMES;
    if (j0 >= nfr) return;
    __shared__ NemoTilePw pw;
    nemo_mel_tile(pw, spec, ld, e.row0 + (int64_t)k * e.rows, j0, nfr, e.w, e.n_mels, e.mel + (int64_t)k * e.n_mels * e.mel_ld, e.mel_ld);
    if (!e.ring) return;   // (uniform over the block: an entry without a history pays nothing more)
    // The frame history: the tile's frames are copied out of the rows the block has just written, so the tile itself -- and with it
    // the offline kernel that shares it -- stays as it is.  The round's frame j is frame J - n_new + j of the concatenation, J the
    // count after the round; frames j and j + hist share a slot, so only the round's last `hist` frames are written and no two
    // threads of a launch write one slot.
    __syncthreads();
    const int tj = threadIdx.x & (NEMO_TILE_FRAMES - 1), ty = threadIdx.x >> 5;
    const int64_t j = j0 + tj, n_new = e.n_new[k];
    if (j >= nfr || j < n_new - e.hist) return;
    const int64_t slot = (e.st[k].J - n_new + j) % e.hist;
    const float* __restrict__ mel = e.mel + (int64_t)k * e.n_mels * e.mel_ld + j;
    float* __restrict__ ring = e.ring + (int64_t)k * e.n_mels * e.hist + slot;
    for (int m = ty; m < e.n_mels; m += NEMO_TILE_ROWS) ring[(int64_t)m * e.hist] = mel[(int64_t)m * e.mel_ld];
}

// ---- NeMo chunks out of the frame history (kernels.hpp NemoChunkItem) ---------------------------------------------------------
struct NemoChunkTable : Table<NemoChunkItem, NEMO_CHUNK_MULTI_MAX> {};

// float64 sum and product that stay ONE rounding each (kernels.hpp css_add_rn: an operation compiled with contraction off cannot
// become half of an FMA)
__device__ __forceinline__ double nemo_dadd(double x, double y) {
#pragma clang fp contract(off)
    return x + y;
}
__device__ __forceinline__ double nemo_dmul(double x, double y) {
#pragma clang fp contract(off)
    return x * y;
}
// x[l] += x[l + s] for s = 32 .. 1 over the wave's lanes; every lane gets x[0].  (A lane at or above s adds a value the tree does
// not use: nothing below s reads it.)
__device__ __forceinline__ double nemo_wave_tree(double x) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) x = nemo_dadd(x, __shfl_down(x, s));
    return __shfl(x, 0);
}

// `len` floats from src (global) to dst (LDS), consecutive lanes on consecutive floats: scalar loads up to src's first 16-byte
// boundary, 16-byte loads from there, scalar loads behind the last whole one
__device__ __forceinline__ void nemo_chunk_load(const float* __restrict__ src, float* dst, int len, int lane) {
    const int head = min((int)((4 - (((uintptr_t)src >> 2) & 3)) & 3), len);
    const int nvec = (len - head) / 4, tail = head + nvec * 4;
    for (int c = lane; c < head; c += 64) dst[c] = src[c];
    for (int c = tail + lane; c < len; c += 64) dst[c] = src[c];
    for (int g = lane; g < nvec; g += 64) {
        const int c = head + g * 4;
        const float4 q = *reinterpret_cast<const float4*>(src + c);
        dst[c] = q.x; dst[c + 1] = q.y; dst[c + 2] = q.z; dst[c + 3] = q.w;
    }
}

// One row of a chunk out of the wave's LDS copy `rw` of its n frames: column c < n is rw[c], normalised with `norm`; the columns
// behind them are pad.  Written as handoff.hip's window_row writes a row: scalar stores up to dst's first 16-byte boundary, 16-byte
// stores from there, scalar stores behind the last whole one.
template <typename T>
__device__ __forceinline__ void nemo_chunk_row(const float* rw, int n, int width, bool norm, float mean, float denom, float pad,
                                               T* __restrict__ dst, int lane) {
    constexpr int V = WindowVec<T>::V;
    auto one = [&](int c) {
        if (c >= n) return pad;
        const float v = rw[c];
        return norm ? css_div_rn(css_add_rn(v, -mean), denom) : v;
    };
    const int head = min((int)(((16 - ((uintptr_t)dst & 15)) & 15) / sizeof(T)), width);
    const int nvec = (width - head) / V, tail = head + nvec * V;
    for (int c = lane; c < head; c += 64) WindowVec<T>::store(dst + c, one(c));
    for (int c = tail + lane; c < width; c += 64) WindowVec<T>::store(dst + c, one(c));
    for (int g = lane; g < nvec; g += 64) {
        const int c = head + g * V;
        float v[V];
#pragma unroll
        for (int i = 0; i < V; ++i) v[i] = one(c + i);
        WindowVec<T>::store16(dst + c, v);
    }
}

// A block has one chunk and NEMO_CHUNK_ROWS bands; a wave has one band row at a time.  The row's span is at most two contiguous
// pieces of the ring -- slots [slot0, min(slot0 + n, hist)) and, behind a wrap, [0, ...) -- which the wave copies into its LDS
// row once; both float64 passes and the write pass read the frames from there in span order, so nothing below depends on the slot
// the span starts in or on a wrap inside it.
__global__ __launch_bounds__(256) void nemo_chunk_kernel(NemoChunkTable tab) {
    const NemoChunkItem& e = tab.e[blockIdx.z];
    const int m0 = blockIdx.x * NEMO_CHUNK_ROWS;
    if (m0 >= e.n_mels) return;
    __shared__ float rows[4][NEMO_CHUNK_MAX_WIDTH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = e.n_frames;
    const int64_t slot0 = e.first % e.hist;
    const int n_a = (int)(slot0 + n <= e.hist ? n : e.hist - slot0);
    float* rw = rows[wave];
    for (int r = 0; r < NEMO_CHUNK_ROWS; r += 4) {
        const int m = m0 + r + wave;
        const bool live = m < e.n_mels;
        if (live) {
            const float* __restrict__ ring = e.ring + (int64_t)m * e.hist;
            nemo_chunk_load(ring + slot0, rw, n_a, lane);
            if (n_a < n) nemo_chunk_load(ring, rw + n_a, n - n_a, lane);
        }
        __syncthreads();
        if (live) {
            float mean_f = 0.f, denom = 1.f;
            if (e.normalize) {
                double s = 0.0;
                for (int c = lane; c < n; c += 64) s = nemo_dadd(s, (double)rw[c]);
                const double mean = nemo_wave_tree(s) / (double)n;
                double q = 0.0;
                for (int c = lane; c < n; c += 64) {
                    const double d = nemo_dadd((double)rw[c], -mean);
                    q = nemo_dadd(q, nemo_dmul(d, d));
                }
                const double ss = nemo_wave_tree(q);
                mean_f = (float)mean;
                const float std_f = n > 1 ? (float)sqrt(ss / (double)(n - 1)) : 0.f;
                denom = css_add_rn(std_f, NEMO_STD_EPS);
                if (lane == 0) { e.mean[m] = mean_f; e.stdv[m] = std_f; }
            }
            if (e.f16) nemo_chunk_row<__half>(rw, n, e.width, e.normalize != 0, mean_f, denom, e.pad_value, (__half*)e.out + (int64_t)m * e.ld, lane);
            else nemo_chunk_row<float>(rw, n, e.width, e.normalize != 0, mean_f, denom, e.pad_value, (float*)e.out + (int64_t)m * e.ld, lane);
        }
        __syncthreads();   // (the row is free for the wave's next band)
    }
}

void launch_nemo_chunks(const NemoChunkItem* e, int n, hipStream_t s) {
    // (the caller chunks and counts the launches: more than one table here would be a launch it does not report)
    for_each_table<NemoChunkTable>(e, std::min(n, NEMO_CHUNK_MULTI_MAX), [&](const NemoChunkTable& tab, int cnt) {
        const int most = table_max(tab, cnt, 1, [](const NemoChunkItem& w) { return (int)w.n_mels; });
        hipLaunchKernelGGL(nemo_chunk_kernel, dim3((unsigned)((most + NEMO_CHUNK_ROWS - 1) / NEMO_CHUNK_ROWS), 1, cnt), dim3(256), 0, s, tab);
        return true;
    });
}

void launch_nemo_append_multi(const NemoAppend* e, int n, float* operand, hipStream_t s) {
    for_each_table<NemoAppendTable>(e, n, [&](const NemoAppendTable& tab, int cnt) {
        hipLaunchKernelGGL(nemo_append_kernel, dim3(1, tab.e[0].a.S, cnt), dim3(256), 0, s, tab, operand);
        return true;
    });
}
void launch_nemo_mel_multi(const NemoMel* e, int n, int S, const float* spec, int64_t ld, hipStream_t s) {
    for_each_table<NemoMelTable>(e, n, [&](const NemoMelTable& tab, int cnt) {
        const int64_t most = table_max(tab, cnt, (int64_t)1, [](const NemoMel& m) { return m.rows; });
        hipLaunchKernelGGL(nemo_mel_multi_kernel, dim3((unsigned)((most + NEMO_TILE_FRAMES - 1) / NEMO_TILE_FRAMES), S, cnt), dim3(256), 0, s, tab,
                           spec, ld);
        return true;
    });
}

}  // namespace css
