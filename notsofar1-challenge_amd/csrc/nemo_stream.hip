// The NeMo hand-off of STREAMED sessions (include/css_mi355_stream_nemo.h; DESIGN.md 7b "The NeMo hand-off of a stream"): the
// append kernel and the multi-owner mel kernel of a round (kernels.hpp NemoAppend, NemoMel).  The product between them is
// launch_gemm on the offline path's [514][512] analysis matrix; the tile is the offline path's (nemo_tile.hpp).
#include "kernels.hpp"
#include "nemo_tile.hpp"
#include "table.hpp"

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
