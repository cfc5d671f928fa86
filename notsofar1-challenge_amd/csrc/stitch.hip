// Stitching of the separated segments (css/css.py:254-312): permutation alignment of adjacent
// segments (training/losses.py PitWrapper), weighted overlap-add, activity gating with
// dilate/erode (utils/numpy_utils.py), and the hand-off layout for the inverse transform.
//
// All kernels are in gather form: an output frame t collects the segments i with i*hop <= t < i*hop + T
// (two with the shipped configuration; bit-exact segment indexing st = i * hop, css.py:183,287), so
// nothing is accumulated with atomics and a frame range can be produced by any rank that holds the
// segments covering it.
#include <algorithm>

#include "kernels.hpp"
#include "lsap.hpp"
#include "split_f16.hpp"
#include "stitch_common.hpp"
#include "table.hpp"
#include "wave.hpp"

namespace css {

// ------------------------------------------------------------------------------------------------
// Raw PIT cost of boundary b (segments b | b+1):  cost[a][c] = mean_{F, overlap} loss(L_a - R_c)
// with L = last `overlap` frames of segment b, R = first `overlap` frames of segment b+1, both in
// their RAW channel order (losses.py:50-71; css.py:267-276).  The cost of an already-permuted left
// segment is a row permutation of this matrix, so all boundaries are computed in parallel and the
// sequential dependence of css.py:266-285 is confined to the tiny scan below.
//   input 0: masks   input 1: |separated spectrum|     loss 0: L1   loss 1: squared error
// ------------------------------------------------------------------------------------------------
// frequency chunks per boundary: 39 boundaries alone would occupy 39 of 256 CUs; with 48 a thread takes two (bin, frame)
// elements, all of whose loads are in flight at once (16 chunks: six dependent rounds of loads per thread).  The chunk sums
// are added in a fixed order and a cost must be the same bit pattern wherever it is computed -- by any call, any rank, and a
// streamed session (api_stream.hip), which does not know how many segments its recording will have.  So the count is ONE
// constant for every meeting length.  (It used to drop to 16 from 129 segments on: 1 208 boundaries of a 30-min meeting
// took 305 us with 16 chunks against 383 us with 48 -- 78 us of a 30-min pass; the costs of such meetings moved in their last
// float64 bits with the change, the suite's long-meeting tests hold the results.)
constexpr int PIT_CH = 48;   // (scratch layout)
__host__ __device__ inline int pit_chunks(int64_t) { return PIT_CH; }

// One block per (boundary, frequency chunk) -> partial[b][chunk][16]; a second kernel adds the chunks in a fixed
// order, so the cost is the same bit pattern whatever boundary range or GPU computes it.
__device__ __forceinline__ void pit_cost_body(const StitchArgs& a, int loss, int input, const int64_t b, const int ch, const int nch,
                                              double* __restrict__ partial) {
    __shared__ double red[4][SMAX * SMAX];
    const int S = a.S, F = a.F, T = a.T, ov = a.T - a.hop;
    const int f_lo = (int)((int64_t)F * ch / nch), f_hi = (int)((int64_t)F * (ch + 1) / nch);
    double acc[SMAX * SMAX];
#pragma unroll
    for (int i = 0; i < SMAX * SMAX; ++i) acc[i] = 0.0;
    for (int idx = threadIdx.x; idx < (f_hi - f_lo) * ov; idx += 256) {
        const int f = f_lo + idx / ov, t = idx % ov;
        float l[SMAX], r[SMAX];
#pragma unroll
        for (int k = 0; k < SMAX; ++k) {
            if (k < S) {
                if (input == 0) {
                    l[k] = a.masks[((int64_t)k * F + f) * a.mask_ld + b * T + (T - ov) + t];
                    r[k] = a.masks[((int64_t)k * F + f) * a.mask_ld + (b + 1) * T + t];
                } else {
                    const float2 lv = reinterpret_cast<const float2*>(a.sep)[((b * S + k) * (int64_t)F + f) * T + (T - ov) + t];
                    const float2 rv = reinterpret_cast<const float2*>(a.sep)[(((b + 1) * S + k) * (int64_t)F + f) * T + t];
                    l[k] = sqrtf(lv.x * lv.x + lv.y * lv.y);
                    r[k] = sqrtf(rv.x * rv.x + rv.y * rv.y);
                }
            } else { l[k] = 0.f; r[k] = 0.f; }
        }
#pragma unroll
        for (int i = 0; i < SMAX; ++i)
#pragma unroll
            for (int j = 0; j < SMAX; ++j) {
                const float d = l[i] - r[j];
                acc[i * SMAX + j] += loss == 0 ? (double)fabsf(d) : (double)(d * d);
            }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < SMAX * SMAX; ++i) {
        const double v = wave_sum_dpp(acc[i]);
        if (lane == 0) red[wave][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < SMAX * SMAX) {
        const int q = threadIdx.x;
        partial[(b * PIT_CH + ch) * (SMAX * SMAX) + q] = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
    }
}

__global__ __launch_bounds__(256) void pit_cost_kernel(StitchArgs a, int loss, int input, int64_t b_lo,
                                                       double* __restrict__ partial) {
    pit_cost_body(a, loss, input, b_lo + blockIdx.x, blockIdx.y, (int)gridDim.y, partial);
}

__device__ __forceinline__ void pit_cost_final_body(const double* __restrict__ partial, int S, int F, int ov, int64_t b_lo, int64_t b_hi,
                                                    double* __restrict__ costs, int nch, const int64_t i) {
    const int ss = S * S;
    if (i >= (b_hi - b_lo) * ss) return;
    const int64_t b = b_lo + i / ss;
    const int e = (int)(i % ss), q = (e / S) * SMAX + e % S;
    // (all loads first, over the compile-time maximum: a loop over the run-time count is 48 dependent round trips, 18 us)
    double part[PIT_CH];
#pragma unroll
    for (int ch = 0; ch < PIT_CH; ++ch) part[ch] = ch < nch ? partial[(b * PIT_CH + ch) * (SMAX * SMAX) + q] : 0.0;
    double v = 0.0;
#pragma unroll
    for (int ch = 0; ch < PIT_CH; ++ch) v += part[ch];   // (the unused chunks add + 0.0 to a non-negative sum: the same bits)
    costs[b * ss + e] = v / ((double)F * ov);
}

__global__ __launch_bounds__(64) void pit_cost_final_kernel(const double* __restrict__ partial, int S, int F, int ov,
                                                            int64_t b_lo, int64_t b_hi, double* __restrict__ costs, int nch) {
    pit_cost_final_body(partial, S, F, ov, b_lo, b_hi, costs, nch, (int64_t)blockIdx.x * 64 + threadIdx.x);
}

// All boundaries of the sessions of a queue group in one pair of launches (a table launch, blockIdx.z / .y = session); every
// session keeps its own chunk count, scratch and cost matrix, so each cost is the bit pattern the per-session launch gives.
// (The per-session launch below keeps kernels of its own: as a table of one entry it made the grouped stream pushes, which
// compute every stream's newest boundary with it, 0.4 ms per round of 16 streams slower -- profiles/r22_shared_device_code.json.)
struct PitEntry { StitchArgs a; double* partial; double* costs; int loss, input; };
struct PitMulti : Table<PitEntry, PIT_MULTI_MAX> {};
__global__ __launch_bounds__(256) void pit_cost_multi_kernel(PitMulti m) {
    const PitEntry& e = m.e[blockIdx.z];
    const int nch = pit_chunks(e.a.num_segments);
    if ((int64_t)blockIdx.x >= e.a.num_segments - 1 || (int)blockIdx.y >= nch) return;
    pit_cost_body(e.a, e.loss, e.input, blockIdx.x, blockIdx.y, nch, e.partial);
}
__global__ __launch_bounds__(64) void pit_cost_final_multi_kernel(PitMulti m) {
    const PitEntry& e = m.e[blockIdx.y];
    pit_cost_final_body(e.partial, e.a.S, e.a.F, e.a.T - e.a.hop, 0, e.a.num_segments - 1, e.costs, pit_chunks(e.a.num_segments),
                        (int64_t)blockIdx.x * 64 + threadIdx.x);
}
void launch_pit_costs_multi(const StitchArgs* a, double* const* scratch, double* const* costs, int n, int loss, int input, hipStream_t s) {
    for_each_table<PitMulti>(n, [&](int i) { return PitEntry{a[i], scratch[i], costs[i], loss, input}; }, [&](const PitMulti& m, int cnt) {
        const int64_t nb = table_max(m, cnt, (int64_t)0, [](const PitEntry& e) { return e.a.num_segments - 1; });
        const int nch = table_max(m, cnt, 0, [](const PitEntry& e) { return pit_chunks(e.a.num_segments); });
        if (nb <= 0) return true;
        hipLaunchKernelGGL(pit_cost_multi_kernel, dim3((unsigned)nb, nch, cnt), dim3(256), 0, s, m);
        hipLaunchKernelGGL(pit_cost_final_multi_kernel, dim3((unsigned)((nb * m.e[0].a.S * m.e[0].a.S + 63) / 64), cnt), dim3(64), 0, s, m);
        return true;
    });
}

size_t pit_cost_scratch_bytes(int64_t n_boundaries) { return (size_t)std::max<int64_t>(n_boundaries, 1) * PIT_CH * SMAX * SMAX * sizeof(double); }

void launch_pit_costs(const StitchArgs& a, int loss, int input, int64_t b_lo, int64_t b_hi, double* scratch, double* costs,
                      hipStream_t s) {
    if (b_hi <= b_lo) return;
    const int nch = pit_chunks(a.num_segments);
    hipLaunchKernelGGL(pit_cost_kernel, dim3((unsigned)(b_hi - b_lo), nch), dim3(256), 0, s, a, loss, input, b_lo, scratch);
    const int64_t n = (b_hi - b_lo) * a.S * a.S;
    hipLaunchKernelGGL(pit_cost_final_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, scratch, a.S, a.F, a.T - a.hop, b_lo,
                       b_hi, costs, nch);
}

// ------------------------------------------------------------------------------------------------
// Sequential permutation scan (css.py:266-285 with losses.py:32-48): perm[0] = identity;
// perm[i+1] = linear_sum_assignment(cost_i with its rows in the order perm[i]).
// The reference minimises with scipy.optimize.linear_sum_assignment (losses.py:43; scipy 1.11.4): the shortest-
// augmenting-path algorithm of scipy's rectangular_lsap (Crouse 2016).  Any exact method finds the same optimum; WHICH
// optimum on exact ties is decided by that algorithm's scan order (columns in descending order, an unassigned column
// wins among equally cheap ones, later ones otherwise) -- and exact ties are the normal case where two speakers are
// silent through a whole overlap (every cost between them is 0: scipy swaps them, a lexicographic search would not).
// So the algorithm is restated step by step, for S <= 4, shared by host and device; tests/test_cabi.py holds it to
// scipy itself on tie-laden matrices.  c[a][b] = cost of assigning row a to column b; out: col4row.
// ------------------------------------------------------------------------------------------------
__host__ __device__ inline void pit_scan_impl(const double* costs, int64_t n_boundaries, int S, int32_t* perms) {
    for (int a = 0; a < S; ++a) perms[a] = a;
    for (int64_t b = 0; b < n_boundaries; ++b) {
        const double* c = costs + b * S * S;
        const int32_t* lp = perms + b * S;
        int32_t* rp = perms + (b + 1) * S;
        V4<V4<double>> m;
        for (int a = 0; a < SMAX; ++a) {
            V4<double> row;
            row.fill(0.0);
            for (int k = 0; k < S; ++k)
                if (a < S) row.set(k, c[lp[a] * S + k]);   // the left segment's channels in their stitched order
            m.set(a, row);
        }
        V4<int> sig;
        lsap_small(m, S, sig);
        for (int a = 0; a < S; ++a) rp[a] = sig.get(a);
    }
}

// Device form of the scan.  A permutation is a state (its lexicographic index, S! <= 24 states), and
// boundary b is a transition table next[b][state_in] -> state_out that depends only on the raw cost
// matrix of b.  All tables are built in parallel (one thread per (boundary, incoming state), in LDS);
// what remains sequential is one LDS lookup per boundary by a single lane, instead of a chain of
// dependent global-memory reads (180 us for 39 boundaries became a few us; 1208 boundaries of a 30-min
// meeting stay under 0.1 ms).  Chunked so that any meeting length fits the LDS.
constexpr int SCAN_CHUNK = 4096;
constexpr int NPMAX = 24;

__device__ __forceinline__ V4<int> perm_from_index(int idx, int S) {
    // idx-th permutation of 0..S-1 in lexicographic order (factorial number system)
    V4<int> avail{0, 1, 2, 3}, p;
    p.fill(0);
    int f = 1;
    for (int i = 2; i < S; ++i) f *= i;  // (S-1)!
    int n = S;
    for (int a = 0; a < S; ++a) {
        const int d = idx / f;
        idx -= d * f;
        p.set(a, avail.get(d));
        for (int i = 0; i < SMAX - 1; ++i)
            if (i >= d) avail.set(i, avail.get(i + 1));
        --n;
        if (n > 1) f /= (n);
    }
    return p;
}
// lexicographic index of a permutation of 0..S-1 (its Lehmer code in the factorial number system)
__device__ __forceinline__ int index_of_perm(const V4<int>& p, int S) {
    int idx = 0;
#pragma unroll
    for (int a = 0; a < SMAX; ++a) {
        int smaller = 0, fact = 1;
#pragma unroll
        for (int b = a + 1; b < SMAX; ++b) {
            if (b < S && a < S && p.get(b) < p.get(a)) ++smaller;
            if (b < S) fact *= (b - a);     // (S - 1 - a)!
        }
        idx += smaller * fact;
    }
    return idx;
}
__device__ __forceinline__ V4<int> unpack_perm(unsigned v) { return V4<int>{(int)(v & 15u), (int)((v >> 4) & 15u), (int)((v >> 8) & 15u), (int)((v >> 12) & 15u)}; }

__global__ __launch_bounds__(256) void pit_scan_kernel(const double* __restrict__ costs, int64_t b_lo, int64_t n_boundaries, int S,
                                                       int32_t* __restrict__ perms) {
    __shared__ uint8_t next[SCAN_CHUNK * NPMAX];
    __shared__ uint8_t state_of[SCAN_CHUNK];
    __shared__ unsigned short ptab[NPMAX];   // the S! permutations in lexicographic order, four bits per entry
    __shared__ int carry;
    int np = 1;
    for (int i = 2; i <= S; ++i) np *= i;
    if ((int)threadIdx.x < np) {
        const V4<int> p = perm_from_index((int)threadIdx.x, S);
        ptab[threadIdx.x] = (unsigned short)(p.a | (p.b << 4) | (p.c << 8) | (p.d << 12));
    }
    if (threadIdx.x == 0) {
        carry = 0;  // identity = lexicographic index 0
        if (b_lo > 0) {   // resume: the lexicographic index of the permutation segment b_lo already has
            V4<int> want;
            want.fill(0);
            for (int a = 0; a < S; ++a) want.set(a, perms[b_lo * S + a]);
            carry = index_of_perm(want, S);
        }
    }
    if (b_lo == 0 && threadIdx.x < S) perms[threadIdx.x] = threadIdx.x;
    __syncthreads();
    for (int64_t b0 = b_lo; b0 < n_boundaries; b0 += SCAN_CHUNK) {
        const int nb = (int)(n_boundaries - b0 < SCAN_CHUNK ? n_boundaries - b0 : SCAN_CHUNK);
        for (int e = threadIdx.x; e < nb * np; e += blockDim.x) {
            const int b = e / np, pin = e - b * np;
            const double* c = costs + (b0 + b) * S * S;
            const V4<int> lp = unpack_perm(ptab[pin]);
            V4<V4<double>> m;
            for (int a = 0; a < SMAX; ++a) {
                V4<double> row;
                row.fill(0.0);
                for (int k = 0; k < SMAX; ++k)
                    if (a < S && k < S) row.set(k, c[lp.get(a) * S + k]);
                m.set(a, row);
            }
            V4<int> sig;
            lsap_small(m, S, sig);
            next[b * np + pin] = (uint8_t)index_of_perm(sig, S);   // the state (lexicographic index) of the assignment found
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int st = carry;
            for (int b = 0; b < nb; ++b) {
                st = next[b * np + st];
                state_of[b] = (uint8_t)st;
            }
            carry = st;
        }
        __syncthreads();
        for (int b = threadIdx.x; b < nb; b += blockDim.x) {
            const V4<int> p = unpack_perm(ptab[state_of[b]]);
            for (int a = 0; a < S; ++a) perms[(b0 + b + 1) * S + a] = p.get(a);
        }
        __syncthreads();
    }
}

void launch_pit_scan(const double* costs, int64_t b_lo, int64_t b_hi, int S, int32_t* perms, hipStream_t s) {
    hipLaunchKernelGGL(pit_scan_kernel, dim3(1), dim3(256), 0, s, costs, b_lo, b_hi, S, perms);
}

void pit_scan_host(const double* costs, int64_t n_boundaries, int S, int32_t* perms) {
    pit_scan_impl(costs, n_boundaries, S, perms);
}

// ------------------------------------------------------------------------------------------------
// helpers shared by the two overlap-add kernels
// ------------------------------------------------------------------------------------------------
// The segments covering frame t, in ascending segment order.  NC = ceil(T / hop) of them at most: two with the shipped
// 3 s / 1.5 s configuration, up to four take the same code (the kernels are instantiated for NC = 2 and 4: slot i is
// ALWAYS segment t / hop - (NC - 1) + i, present or not, so every index is a compile-time constant and nothing lives in
// private scratch); denser segmentations (any hop >= 1 the reference accepts, css.py:144-171) take the NC = 0
// instantiation: the general walk of stitch_common.hpp, which the stream kernels share.  The sums start from zero exactly as the reference's
// `zeros += w * x` does (css.py:254-295): 0 + w x is w x, so the float32 operation order is the reference's.
constexpr int MAXC = 4;
__host__ __device__ inline int contributor_class(int T, int hop) {
    const int nc = (T + hop - 1) / hop;
    return nc <= 2 ? 2 : (nc <= MAXC ? MAXC : 0);
}
template <int NC>
struct Covering {
    int64_t seg[NC];
    int tl[NC];
    float w[NC];      // 0 for an absent slot
    bool on[NC];
    __device__ __forceinline__ void build(const StitchArgs& a, int64_t t) {
        const int64_t i1 = t / a.hop;
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const int64_t sg = i1 - (NC - 1) + i;
            const int64_t l = t - sg * a.hop;
            on[i] = sg >= 0 && sg < a.num_segments && l >= 0 && l < a.T;
            seg[i] = on[i] ? sg : 0;
            tl[i] = on[i] ? (int)l : 0;
            w[i] = on[i] ? seg_weight(a, sg, (int)l) : 0.f;
        }
    }
    __device__ __forceinline__ float weight_sum() const {
        float ws = 0.f;
#pragma unroll
        for (int i = 0; i < NC; ++i)
            if (on[i]) ws = css_add_rn(ws, w[i]);
        return ws;
    }
};

// ------------------------------------------------------------------------------------------------
// Weighted overlap-add of the (permuted) masks + mean over frequency (css.py:254-299, 303-304):
//   mask_st[s][f][t] = (sum_i w_i[t - st_i] * mask_i[perm_i[s]][f][t - st_i]) / (sum_i w_i[t - st_i])
//   activity[s][t]   = mean_f mask_st[s][f][t];   act_b = activity >= th
// The float32 operation order of the reference (multiply, add in ascending segment order, divide) is
// reproduced with operations compiled with contraction off (kernels.hpp css_mul_rn / css_add_rn / css_div_rn), so no FMA
// changes a bit.
// Block = OLA_T frames x OLA_FG frequency groups; lanes run over time (contiguous mask reads); the frequency mean is
// accumulated in float64 and the 16 partial sums are added in a fixed order (stitch_common.hpp ola_activity).
// ------------------------------------------------------------------------------------------------
template <int NC>
__global__ __launch_bounds__(256) void ola_masks_kernel(StitchArgs a, int64_t t_lo, int64_t t_hi) {
    const int s = blockIdx.y;
    const int lane = threadIdx.x & (OLA_T - 1), fg = threadIdx.x / OLA_T;
    const int64_t t = t_lo + (int64_t)blockIdx.x * OLA_T + lane;
    const bool active = t < t_hi;
    double sum = 0.0;
    if constexpr (NC == 0) {
        if (active) {
            int64_t s0, s1;
            covering(a, t, &s0, &s1);
            const float ws = ola_weight_sum(a, t, s0, s1);
            float* out = a.mask_st + (int64_t)s * a.F * a.T_long + t;
            for (int f = fg; f < a.F; f += OLA_FG) {
                const float v = ola_mask_value(a, s, f, t, s0, s1, ws);
                out[(int64_t)f * a.T_long] = v;
                sum += (double)v;
            }
        }
    } else {
        if (active) {
            Covering<NC> c;
            c.build(a, t);
            const float wsum = c.weight_sum();
            const float* mp[NC];
#pragma unroll
            for (int i = 0; i < NC; ++i)
                mp[i] = a.masks + (int64_t)(c.on[i] ? a.perms[c.seg[i] * a.S + s] : 0) * a.F * a.mask_ld + c.seg[i] * a.T + c.tl[i];
            float* out = a.mask_st + (int64_t)s * a.F * a.T_long + t;
            for (int f = fg; f < a.F; f += OLA_FG) {
                float v = 0.f;
#pragma unroll
                for (int i = 0; i < NC; ++i)
                    if (c.on[i]) v = css_add_rn(v, css_mul_rn(c.w[i], mp[i][(int64_t)f * a.mask_ld]));
                v = css_div_rn(v, wsum);
                out[(int64_t)f * a.T_long] = v;
                sum += (double)v;
            }
        }
    }
    ola_activity(sum, fg, lane, active, a.F, a.activity_th, [&](float act, uint8_t on) {
        a.activity[(int64_t)s * a.T_long + t] = act;
        a.act_b[(int64_t)s * a.T_long + t] = on;
    });
}

void launch_ola_masks(const StitchArgs& a, int64_t t_lo, int64_t t_hi, hipStream_t s) {
    if (t_hi <= t_lo) return;
    const dim3 grid((unsigned)((t_hi - t_lo + OLA_T - 1) / OLA_T), a.S), block(OLA_T * OLA_FG);
    switch (contributor_class(a.T, a.hop)) {
        case 2: hipLaunchKernelGGL(ola_masks_kernel<2>, grid, block, 0, s, a, t_lo, t_hi); break;
        case 4: hipLaunchKernelGGL(ola_masks_kernel<4>, grid, block, 0, s, a, t_lo, t_hi); break;
        default: hipLaunchKernelGGL(ola_masks_kernel<0>, grid, block, 0, s, a, t_lo, t_hi); break;
    }
}

// ------------------------------------------------------------------------------------------------
// dilate (zero padding) then erode (one padding) of the per-speaker activity (css.py:305-308,
// numpy_utils.py:4-13).  act_final over [t_lo, t_hi) needs act_b over [t_lo - E - Dl, t_hi + E + Dl).
// ------------------------------------------------------------------------------------------------
__global__ void morph_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int64_t T_long, int radius,
                             int erode, int64_t t_lo, int64_t t_hi) {
    const int s = blockIdx.y;
    const int64_t t = t_lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= t_hi) return;
    const uint8_t* row = in + (int64_t)s * T_long;
    uint8_t v = erode ? 1 : 0;
    for (int64_t u = t - radius; u <= t + radius; ++u) {
        const uint8_t x = (u < 0 || u >= T_long) ? (erode ? 1 : 0) : row[u];
        v = erode ? (v & x) : (v | x);
    }
    out[(int64_t)s * T_long + t] = v;
}

void launch_morphology(const StitchArgs& a, int64_t t_lo, int64_t t_hi, hipStream_t s) {
    if (t_hi <= t_lo) return;
    const int64_t d_lo = t_lo - a.erosion < 0 ? 0 : t_lo - a.erosion;
    const int64_t d_hi = t_hi + a.erosion > a.T_long ? a.T_long : t_hi + a.erosion;
    hipLaunchKernelGGL(morph_kernel, dim3((unsigned)((d_hi - d_lo + 255) / 256), a.S), dim3(256), 0, s, a.act_b,
                       a.act_tmp, a.T_long, a.dilation, 0, d_lo, d_hi);
    hipLaunchKernelGGL(morph_kernel, dim3((unsigned)((t_hi - t_lo + 255) / 256), a.S), dim3(256), 0, s, a.act_tmp,
                       a.act_final, a.T_long, a.erosion, 1, t_lo, t_hi);
}

// ------------------------------------------------------------------------------------------------
// Weighted overlap-add of the (permuted) separated spectra, activity gating (css.py:294,298,312) and
// the hand-off layout of the synthesis GEMM: Y[s][t][0..F) = Re, [F..2F) = Im, zero padding to KIp.
// Block = OLA_T frames of one stream; reads run over time (128-byte runs of float2), the tile is turned
// through LDS so the writes run over the frequency axis.
// ------------------------------------------------------------------------------------------------
template <int NC>
__global__ __launch_bounds__(256) void ola_stft_kernel(StitchArgs a, int64_t t_lo, int64_t t_hi) {
    extern __shared__ __attribute__((aligned(16))) float tile[];  // [OLA_T][2F + 1] (odd stride: no bank conflicts)
    const int TS = 2 * a.F + 1;
    const int s = blockIdx.y;
    const int64_t t0 = t_lo + (int64_t)blockIdx.x * OLA_T;
    const int tx = threadIdx.x & (OLA_T - 1), fy = threadIdx.x >> 4;  // 16 frames x 16 bins per pass
    const int64_t t = t0 + tx;
    const bool active = t < t_hi;
    const float2* sep = reinterpret_cast<const float2*>(a.sep);
    const float gate = active && a.act_final[(int64_t)s * a.T_long + t] ? 1.f : 0.f;
    if constexpr (NC == 0) {
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
    } else {
        Covering<NC> c;
        const float2* pp[NC];
        float wsum = 1.f;
        bool any = false;
        if (active) {
            c.build(a, t);
            wsum = c.weight_sum();
#pragma unroll
            for (int i = 0; i < NC; ++i) {
                any |= c.on[i];
                pp[i] = sep + (c.seg[i] * a.S + (c.on[i] ? a.perms[c.seg[i] * a.S + s] : 0)) * (int64_t)a.F * a.T + c.tl[i];
            }
        }
        for (int f = fy; f < a.F; f += 16) {
            float re = 0.f, im = 0.f;
            if (active && any) {
#pragma unroll
                for (int i = 0; i < NC; ++i)
                    if (c.on[i]) {
                        const float2 v = pp[i][(int64_t)f * a.T];
                        re = css_add_rn(re, css_mul_rn(c.w[i], v.x));
                        im = css_add_rn(im, css_mul_rn(c.w[i], v.y));
                    }
                re = css_mul_rn(css_div_rn(re, wsum), gate);
                im = css_mul_rn(css_div_rn(im, wsum), gate);
            }
            tile[tx * TS + f] = re;
            tile[tx * TS + a.F + f] = im;
        }
    }
    __syncthreads();
    const float lvl = a.y_split ? level_gain(a.level) : 1.f;
    for (int r = 0; r < OLA_T; ++r) {
        if (t0 + r >= t_hi) break;
        float* out = a.Y + ((int64_t)s * a.T_long + t0 + r) * a.KIp;
        for (int j = threadIdx.x; j < a.KIp; j += 256) {
            const float v = j < 2 * a.F ? tile[r * TS + j] : 0.f;  // zero K padding
            // operand rows of the synthesis GEMM.  (+ 0.f: a gated frame holds -0 where the sum was negative, and whether the halves
            // of -0 leave as -0 or +0 is otherwise the compiler's choice -- product and conversion fuse into an FMA with a +0 addend
            // or they do not; +0 either way now, the bits the fused form has always written)
            if (a.y_split) split_store(reinterpret_cast<_Float16*>(out), j, v * lvl + 0.f);
            else out[j] = v;
        }
    }
}

void launch_ola_stft(const StitchArgs& a, int64_t t_lo, int64_t t_hi, hipStream_t s) {
    if (t_hi <= t_lo) return;
    const size_t lds = (size_t)OLA_T * (2 * a.F + 1) * sizeof(float);
    const dim3 grid((unsigned)((t_hi - t_lo + OLA_T - 1) / OLA_T), a.S), block(256);
    switch (contributor_class(a.T, a.hop)) {
        case 2: hipLaunchKernelGGL(ola_stft_kernel<2>, grid, block, lds, s, a, t_lo, t_hi); break;
        case 4: hipLaunchKernelGGL(ola_stft_kernel<4>, grid, block, lds, s, a, t_lo, t_hi); break;
        default: hipLaunchKernelGGL(ola_stft_kernel<0>, grid, block, lds, s, a, t_lo, t_hi); break;
    }
}

}  // namespace css
