// Rate conversion at a stream's ingest (css_stream_set_rate) and of a whole recording (css_resample_host): input at the capture
// rate -> the model's 16 kHz, by the polyphase filter of scipy.signal.resample_poly(x, up, down, padtype='constant') with its
// default taps.  (DESIGN.md 7b "Pushes at the capture rate": the definition, the counts, what is refused.)
//
//   half = 10 max(up, down), L = 2 half + 1, h = up * firwin(L, 1 / max(up, down), window=('kaiser', 5.0))   (float64 -> float32 once)
//   y[m] = sum_i x[i] h[half + m down - i up]   over 0 <= half + m down - i up <= 2 half,   x[i] = 0 outside [0, n_in)
//
// One output sample is ONE float32 fmaf chain from 0.0f over its inputs in ascending i (resample_sample below, inlined by both
// kernels), so its bits depend on nothing but the recording: not on how pushes, pieces or tiles were cut, not on which of the
// two kernels made it.  With i_hi = floor((m down + half) / up) the chain runs over the P = ceil(L / up) inputs i_hi - P + 1 ..
// i_hi; the taps are laid out per phase ((m down + half) mod up), P per phase in the chain's order, so a phase that has only
// P - 1 taps starts with a 0.0f tap: fmaf(x, 0, +0) = +0, the chain's value is untouched.
//
//   stream_ingest_resample_kernel   a table launch (blockIdx.z = entry) for the rate streams of a round: [carried | piece] ->
//                                   the streams' sample windows, and the inputs the next round still reads -> the other
//                                   generation of the carried history
//   resample_kernel                 a whole recording -> [n_out][C] (css_resample_host)
//   session_ingest_resample_kernel  a table launch for the rate sessions of a queue group: recordings -> [n_model][C] and their
//                                   levels (css_run*_rate); session_output_kernel: a session's waveforms -> the output rate
//   stream_output_kernel            a table launch for the streams of a round that have an output format: [carried | the round's
//                                   final samples] -> float32 or PCM16 at the playback rate (css_stream_set_output), the carried
//                                   samples' other generation, the running peak and the clipped counts
#include "api_ctx.hpp"
#include "table.hpp"
#include "wave.hpp"
#include "../../include/css_mi355_rate.h"
#include "../../include/css_mi355_stream_out.h"

#include <numeric>
#include <type_traits>

namespace css {

bool resample_ratio(int up, int down, ResampleRatio* r) {
    if (up <= 0 || down <= 0 || up == down || std::gcd(up, down) != 1) return false;
    const int64_t mx = std::max(up, down), L = 20 * mx + 1;
    if (L > 16384) return false;
    const int64_t P = (L + up - 1) / up;
    if (P > RS_P_MAX) return false;
    *r = ResampleRatio{up, down, (int)(10 * mx), (int)L, (int)P, (int)(P | 1)};
    return true;
}

// I0 by its power series sum_k ((x / 2)^k / k!)^2: the terms fall below 2^-53 of the sum after some 25 of them at x = 5
static double bessel_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < sum * 1e-18) break;
    }
    return sum;
}

void resample_taps_f32(const ResampleRatio& r, float* taps) {
    const double pi = 3.14159265358979323846, beta = 5.0, cut = 1.0 / (double)std::max(r.up, r.down), alpha = (double)r.half;
    std::vector<double> h((size_t)r.L);
    const double i0b = bessel_i0(beta);
    double sum = 0.0;
    for (int n = 0; n < r.L; ++n) {
        const double m = (double)n - alpha, x = cut * m;
        const double sinc = x == 0.0 ? 1.0 : std::sin(pi * x) / (pi * x);
        const double t = m / alpha;
        h[(size_t)n] = cut * sinc * (bessel_i0(beta * std::sqrt(1.0 - t * t)) / i0b);
        sum += h[(size_t)n];
    }
    for (int n = 0; n < r.L; ++n) taps[n] = (float)(h[(size_t)n] / sum * (double)r.up);
}

// tab[phase][j], j < P: the tap of input i_hi - P + 1 + j, h[phase + (P - 1 - j) up] (0 where that is past the last tap)
void resample_phase_table(const ResampleRatio& r, const float* taps, float* tab) {
    for (int ph = 0; ph < r.up; ++ph)
        for (int j = 0; j < r.P_ld; ++j) {
            const int64_t k = ph + (int64_t)(r.P - 1 - j) * r.up;
            tab[(size_t)ph * r.P_ld + j] = (j < r.P && k < r.L) ? taps[k] : 0.0f;
        }
}

int64_t resample_count(const ResampleRatio& r, int64_t n_in, bool finished) {
    const int64_t num = n_in * r.up - (finished ? 0 : r.half);
    return num <= 0 ? 0 : (num + r.down - 1) / r.down;
}

namespace {

// LDS position of input p of a row: one dword of padding per 32, so that the lanes' read stride of `down` dwords (2 and 6 fold
// two lanes onto one of the 32 banks) spreads over the banks
__device__ __forceinline__ int swz(int p) { return p + (p >> 5); }

// THE output sample: inputs a .. a + P - 1 of a row of the staged span, taps of the sample's phase in the same order
__device__ __forceinline__ float resample_sample(const float* __restrict__ row, int a, const float* __restrict__ tp, int P) {
    float acc = 0.0f;
#pragma unroll 4
    for (int j = 0; j < P; ++j) acc = __fmaf_rn(row[swz(a + j)], tp[j], acc);
    return acc;
}

__device__ __forceinline__ float to_float(int16_t q) { return __fmul_rn((float)q, 1.0f / 32768.0f); }
__device__ __forceinline__ float to_float(float v) { return v; }

// A contiguous run of cnt elements at g -> put(element index, value): 16-byte loads over the aligned middle of the run
template <typename T, typename Put>
__device__ __forceinline__ void run_to_lds(const T* __restrict__ g, int cnt, Put put) {
    constexpr int V = 16 / (int)sizeof(T);
    const int tid = threadIdx.x, nth = blockDim.x;
    int head = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(g) & 15u)) & 15u) / sizeof(T));
    head = head < cnt ? head : cnt;
    for (int e = tid; e < head; e += nth) put(e, 1, to_float(g[e]));
    const int nv = (cnt - head) / V;
    const uint4* __restrict__ g16 = reinterpret_cast<const uint4*>(g + head);
    for (int v = tid; v < nv; v += nth) {
        const uint4 q = g16[v];
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
        float f[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            if constexpr (sizeof(T) == 2) f[k] = to_float((int16_t)(unsigned short)(w[k >> 1] >> (16 * (k & 1))));
            else f[k] = __uint_as_float(w[k]);
        }
        put(head + v * V, V, f);
    }
    for (int e = head + nv * V + tid; e < cnt; e += nth) put(e, 1, to_float(g[e]));
}

// element e of an entry's piece as float (the history block and nothing else reads single elements)
__device__ __forceinline__ float piece_at(const ResampleJob& e, int64_t j, int c) {
    const int64_t at = e.plane_ld > 0 ? (int64_t)c * e.plane_ld + j : j * e.C + c;
    return e.is_i16 ? to_float(static_cast<const int16_t*>(e.src)[at]) : static_cast<const float*>(e.src)[at];
}

template <typename T>
__device__ __forceinline__ void piece_to_lds(const ResampleJob& e, int64_t j0, int cnt, int p0, float* xs, int row_ld) {
    const T* src = static_cast<const T*>(e.src);
    const int C = e.C;
    if (e.plane_ld > 0 || C == 1) {
        for (int c = 0; c < C; ++c) {
            float* row = xs + c * row_ld;
            run_to_lds(src + (int64_t)c * e.plane_ld + j0, cnt, [&](int at, int n, auto v) {
                if constexpr (std::is_same<decltype(v), float>::value) row[swz(p0 + at)] = v;
                else
                    for (int k = 0; k < n; ++k) row[swz(p0 + at + k)] = v[k];
            });
        }
        return;
    }
    run_to_lds(src + j0 * C, cnt * C, [&](int at, int n, auto v) {
        int j = at / C, c = at - j * C;
        if constexpr (std::is_same<decltype(v), float>::value) xs[c * row_ld + swz(p0 + j)] = v;
        else
            for (int k = 0; k < n; ++k) {
                xs[c * row_ld + swz(p0 + j)] = v[k];
                if (++c == C) { c = 0; ++j; }
            }
    });
}

// Outputs [m0 + t0, m0 + t0 + RS_TILE) of entry e, all channels: the taps and the span of inputs they read into LDS (float,
// channel-major), then 64 consecutive outputs per wave and channel.  STREAM: dst[c * dst_ld + (m - m0)]; else dst[m * C + c].
// PEAK: returns the thread's max |y| over its outputs m < n_peak, all channels (0 otherwise).
template <bool STREAM, bool PEAK = false>
__device__ __forceinline__ float resample_tile(const ResampleJob& e, int64_t t0, float* lds, int64_t n_peak = 0) {
    const int C = e.C, P = e.P, up = e.up, down = e.down;
    const int nt = (int)(e.n_m - t0 < RS_TILE ? e.n_m - t0 : RS_TILE);
    const int span_max = (RS_TILE * down + up - 1) / up + P + 1;
    const int row_ld = swz(span_max - 1) + 1;
    float* tab = lds;
    float* xs = lds + up * e.P_ld;
    for (int v = threadIdx.x; v < up * e.P_ld; v += blockDim.x) tab[v] = e.tab[v];
    // the tile's first output: i_hi = num / up, phase = num % up; output t of the tile adds t * down to num
    const int64_t num = (e.m0 + t0) * down + e.half;
    const int64_t ihi0 = num / up;
    const int rem0 = (int)(num - ihi0 * up);
    const int64_t i_first = ihi0 - (P - 1);
    const int span = (rem0 + (nt - 1) * down) / up + P;
    // input i is element s = i - (N0 - H) of [carried history (H) | piece (n)]; zero before and behind
    const int64_t s0 = i_first - (e.N0 - e.H);
    const int pz = (int)(s0 < 0 ? (-s0 < span ? -s0 : span) : 0);                          // [0, pz): zeros
    const int64_t h_end = (int64_t)e.H - s0;                                                // position of piece element 0
    const int ph = (int)(h_end < pz ? pz : (h_end < span ? h_end : span));                 // [pz, ph): history
    const int64_t p_end = h_end + e.n;
    const int pp = (int)(p_end < ph ? ph : (p_end < span ? p_end : span));                 // [ph, pp): piece, [pp, span): zeros
    for (int c = 0; c < C; ++c) {
        float* row = xs + c * row_ld;
        for (int p = threadIdx.x; p < pz; p += blockDim.x) row[swz(p)] = 0.0f;
        for (int p = pz + threadIdx.x; p < ph; p += blockDim.x) row[swz(p)] = e.hist_in[(int64_t)c * e.H + (s0 + p)];
        for (int p = pp + threadIdx.x; p < span; p += blockDim.x) row[swz(p)] = 0.0f;
    }
    if (pp > ph) {
        const int64_t j0 = s0 + ph - e.H;
        if (e.is_i16) piece_to_lds<int16_t>(e, j0, pp - ph, ph, xs, row_ld);
        else piece_to_lds<float>(e, j0, pp - ph, ph, xs, row_ld);
    }
    __syncthreads();
    const int t = threadIdx.x;
    float pk = 0.0f;
    if (t >= nt) return pk;
    const int nu = rem0 + t * down;
    const int a = nu / up;
    const float* tp = tab + (nu - a * up) * e.P_ld;
    const bool scanned = PEAK && e.m0 + t0 + t < n_peak;
    for (int c = 0; c < C; ++c) {
        const float y = resample_sample(xs + c * row_ld, a, tp, P);
        if (STREAM) e.dst[(int64_t)c * e.dst_ld + t0 + t] = y;
        else e.dst[(e.m0 + t0 + t) * C + c] = y;
        if (scanned) pk = fmaxf(pk, fabsf(y));
    }
    return pk;
}

struct ResampleTable : Table<ResampleJob, STREAM_MULTI_MAX> {};

__global__ __launch_bounds__(RS_TILE) void stream_ingest_resample_kernel(ResampleTable tab) {
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];
    const ResampleJob e = tab.e[blockIdx.z];
    const int64_t tiles = (e.n_m + RS_TILE - 1) / RS_TILE;
    if ((int64_t)blockIdx.x < tiles) {
        resample_tile<true>(e, (int64_t)blockIdx.x * RS_TILE, rs_lds);
        return;
    }
    // one more block per entry: the last H inputs of [carried | piece] become the next round's carried history
    if ((int64_t)blockIdx.x != tiles || !e.hist_out) return;
    for (int v = threadIdx.x; v < e.C * e.H; v += blockDim.x) {
        const int c = v / e.H, k = v - c * e.H;
        const int64_t s = e.n + k;
        e.hist_out[v] = s < e.H ? e.hist_in[(int64_t)c * e.H + s] : piece_at(e, s - e.H, c);
    }
}

__global__ __launch_bounds__(RS_TILE) void resample_kernel(ResampleJob e) {
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];
    resample_tile<false>(e, (int64_t)blockIdx.x * RS_TILE, rs_lds);
}

// ---- the output side of a stream (include/css_mi355_stream_out.h; DESIGN.md 7b "Final samples at the playback rate") ----------
// The twin of stream_ingest_resample_kernel: a table launch, blockIdx.z = entry (a stream), blockIdx.y = separated stream,
// blockIdx.x = tile of SO_TILE output samples; block `tiles` of an entry writes the next generation of the carried samples and
// blocks past it return at once.  A tile stages the taps and the span [carried | the round's final samples] of its speaker,
// runs resample_sample per output sample (lane l of a pass takes output 256 pass + l), converts, and leaves through an output
// tile in LDS so that the stores are 16 bytes per lane.
// LDS banks (ds_read_b32: 32 banks, conflicts within a 32-lane half): consecutive lanes' first taps lie down / up of a sample
// apart.  At the playback rates above the model's (3 / 1, 441 / 160, 2 / 1) that is less than one dword: a half reads at most
// 32 down / up + 1 consecutive dwords, equal addresses broadcast, no conflict, and swz's padding dword only shifts them.  Below
// it (1 / 2: a stride of 2 dwords folds lanes l and l + 16 onto one bank) swz moves the upper 16 lanes by one dword, as on the
// input side.  The taps of a phase start at phase * P_ld: 3 rows at 3 / 1 (banks 0, 21, 10); at 441 / 160 the lanes' phases step
// by 160 = 5 * 32, so whatever P_ld is the half's 32 lanes meet on the ~12 banks their wraps past 441 select (about 3 lanes per
// bank, on one of the two reads per fmaf).
struct StreamOutputTable : Table<StreamOutputJob, STREAM_MULTI_MAX> {};

// floats of LDS before the output tile: the taps by phase and the span's row (nothing at 1 / 1), rounded to 16 bytes
__host__ __device__ __forceinline__ int so_tile_at(int up, int down, int P, int P_ld) {
    if (up == down) return 0;
    const int span_max = (SO_TILE * down + up - 1) / up + P + 1;
    return (up * P_ld + (span_max - 1 + ((span_max - 1) >> 5) + 1) + 3) & ~3;
}

__global__ __launch_bounds__(RS_TILE) void stream_output_kernel(StreamOutputTable tab) {
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];
    __shared__ float w_peak[RS_TILE / 64];
    __shared__ unsigned int w_clip[RS_TILE / 64];
    const StreamOutputJob e = tab.e[blockIdx.z];
    const int64_t tiles = (e.n_m + SO_TILE - 1) / SO_TILE;
    const int64_t b = blockIdx.x;
    if (b > tiles) return;
    const int k = blockIdx.y, tid = threadIdx.x;
    const float* __restrict__ src = e.src + (int64_t)k * e.src_ld;
    // the running peak: the entry's tiles + 1 blocks of this speaker share the round's n samples
    const int64_t per = (e.n + tiles) / (tiles + 1);
    const int64_t lo = b * per < e.n ? b * per : e.n, hi = lo + per < e.n ? lo + per : e.n;
    float m = 0.f;
    for (int64_t i = lo + tid; i < hi; i += RS_TILE) m = fmaxf(m, fabsf(src[i]));
    unsigned int clip = 0;
    if (b == tiles) {
        // the last H inputs of [carried | the round's samples] become the next round's carried history
        if (e.hist_out)
            for (int v = tid; v < e.H; v += RS_TILE) {
                const int64_t s = e.n + v;
                e.hist_out[(int64_t)k * e.H + v] = s < e.H ? e.hist_in[(int64_t)k * e.H + s] : src[s - e.H];
            }
    } else {
        const bool unity = e.up == e.down;
        const int up = e.up, down = e.down, P = e.P;
        const int64_t t0 = b * SO_TILE;
        const int nt = (int)(e.n_m - t0 < SO_TILE ? e.n_m - t0 : SO_TILE);
        float* otile = rs_lds + so_tile_at(up, down, P, e.P_ld);
        float* taps = rs_lds;
        float* row = rs_lds + up * e.P_ld;
        int rem0 = 0;
        if (!unity) {
            for (int v = tid; v < up * e.P_ld; v += RS_TILE) taps[v] = e.tab[v];
            // the tile's first output: i_hi = num / up, phase = num % up; output t of the tile adds t * down to num
            const int64_t num = (e.m0 + t0) * down + e.half;
            const int64_t ihi0 = num / up;
            rem0 = (int)(num - ihi0 * up);
            const int span = (rem0 + (nt - 1) * down) / up + P;
            // input i is element s = i - (N0 - H) of [carried (H) | the round's samples (n)]; zero before and behind
            const int64_t s0 = ihi0 - (P - 1) - (e.N0 - e.H);
            for (int p = tid; p < span; p += RS_TILE) {
                const int64_t s = s0 + p;
                float x = 0.f;
                if (s >= 0 && s < e.H) x = e.hist_in[(int64_t)k * e.H + s];
                else if (s >= e.H && s - e.H < e.n) x = src[s - e.H];
                row[swz(p)] = x;
            }
            __syncthreads();
        }
        for (int t = tid; t < nt; t += RS_TILE) {
            float y;
            if (unity) {
                y = src[t0 + t];
            } else {
                const int nu = rem0 + t * down;
                const int a = nu / up;
                y = resample_sample(row, a, taps + (nu - a * up) * e.P_ld, P);
            }
            if (e.pcm16) {
                const double r = rint((double)__fmul_rn(y, e.gain) * 32767.0);
                const double c = fmin(fmax(r, -32768.0), 32767.0);
                clip += c != r ? 1u : 0u;
                reinterpret_cast<int16_t*>(otile)[t] = (int16_t)c;
            } else {
                otile[t] = y;
            }
        }
        __syncthreads();
        // dst rows and tile starts are multiples of 16 bytes: whole vectors, then the tile's last elements one by one
        if (e.pcm16) {
            int16_t* d = static_cast<int16_t*>(e.dst) + (int64_t)k * e.dst_ld + t0;
            const int nv = nt / 8;
            for (int v = tid; v < nv; v += RS_TILE) reinterpret_cast<uint4*>(d)[v] = reinterpret_cast<const uint4*>(otile)[v];
            for (int t = nv * 8 + tid; t < nt; t += RS_TILE) d[t] = reinterpret_cast<const int16_t*>(otile)[t];
        } else {
            float* d = static_cast<float*>(e.dst) + (int64_t)k * e.dst_ld + t0;
            const int nv = nt / 4;
            for (int v = tid; v < nv; v += RS_TILE) reinterpret_cast<uint4*>(d)[v] = reinterpret_cast<const uint4*>(otile)[v];
            for (int t = nv * 4 + tid; t < nt; t += RS_TILE) d[t] = otile[t];
        }
    }
    // one atomic of each kind per block, and only when it changes the word
    m = wave_max_shfl(m);
    clip = wave_sum_shfl(clip);
    if ((tid & 63) == 0) { w_peak[tid >> 6] = m; w_clip[tid >> 6] = clip; }
    __syncthreads();
    if (tid == 0) {
        float bm = w_peak[0];
        unsigned int bc = w_clip[0];
        for (int w = 1; w < RS_TILE / 64; ++w) { bm = fmaxf(bm, w_peak[w]); bc += w_clip[w]; }
        if (bm > __uint_as_float(__hip_atomic_load(e.peak + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) atomicMax(e.peak + k, __float_as_uint(bm));
        if (bc) atomicAdd(e.clipped + k, (unsigned long long)bc);
    }
}

// ---- whole sessions at the capture rate (include/css_mi355_session_rate.h; DESIGN.md 7 "N1 / N2 at the capture rate") ---------------------------------------
// The ingest edge: resample_kernel as a table launch, blockIdx.z = a rate session of the queue group, blockIdx.x = tile of RS_TILE
// model-rate samples of all channels; blocks past a session's last tile return at once.  The tile's outputs also give the
// recording's level: the block's max |y| over the samples launch_pcm_peak_f32 would scan, one atomicMax per block and only when
// it raises the word -- a maximum, so the word does not depend on the order.
struct SessionIngestTable : Table<SessionIngestJob, SESSION_RATE_TABLE> {};

// the block's maximum of m into *word (float bits of a non-negative value), by thread 0; w [RS_TILE / 64] is LDS
__device__ __forceinline__ void block_peak_to(float m, float* w, unsigned int* word) {
    const int tid = threadIdx.x;
    m = wave_max_shfl(m);
    if ((tid & 63) == 0) w[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        float bm = w[0];
        for (int i = 1; i < RS_TILE / 64; ++i) bm = fmaxf(bm, w[i]);
        if (bm > __uint_as_float(__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) atomicMax(word, __float_as_uint(bm));
    }
}

__global__ __launch_bounds__(RS_TILE) void session_ingest_resample_kernel(SessionIngestTable tab) {
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];
    __shared__ float w_peak[RS_TILE / 64];
    const SessionIngestJob e = tab.e[blockIdx.z];
    const int64_t t0 = (int64_t)blockIdx.x * RS_TILE;
    if (t0 >= e.r.n_m) return;
    const float m = resample_tile<false, true>(e.r, t0, rs_lds, e.n_peak);
    block_peak_to(m, w_peak, e.level);
}

// The output edge of ONE session: blockIdx.y = separated stream, blockIdx.x = tile of SO_TILE output samples.  stream_output_kernel
// without the carried history, the sample formats and the clip counts: a tile stages the taps and its span of waveform row k
// (zeros before sample 0 and behind sample n - 1), lane l of a pass takes output 256 pass + l, and the tile leaves through LDS so
// that the stores are 16 bytes per lane.  The LDS bank argument is stream_output_kernel's (same layout, same swz).  The peak is
// that of the OUTPUT samples (write_wav normalises what it writes), one atomicMax per block.
__global__ __launch_bounds__(RS_TILE) void session_output_kernel(SessionOutputJob e) {
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];
    __shared__ float w_peak[RS_TILE / 64];
    const int k = blockIdx.y, tid = threadIdx.x;
    const int up = e.up, down = e.down, P = e.P;
    const int64_t t0 = (int64_t)blockIdx.x * SO_TILE;
    if (t0 >= e.n_m) return;
    const int nt = (int)(e.n_m - t0 < SO_TILE ? e.n_m - t0 : SO_TILE);
    const float* __restrict__ src = e.src + (int64_t)k * e.src_ld;
    float* taps = rs_lds;
    float* row = rs_lds + up * e.P_ld;
    float* otile = rs_lds + so_tile_at(up, down, P, e.P_ld);
    for (int v = tid; v < up * e.P_ld; v += RS_TILE) taps[v] = e.tab[v];
    // the tile's first output: i_hi = num / up, phase = num % up; output t of the tile adds t * down to num
    const int64_t num = t0 * down + e.half;
    const int64_t ihi0 = num / up;
    const int rem0 = (int)(num - ihi0 * up);
    const int span = (rem0 + (nt - 1) * down) / up + P;
    const int64_t s0 = ihi0 - (P - 1);
    for (int p = tid; p < span; p += RS_TILE) {
        const int64_t s = s0 + p;
        row[swz(p)] = (s >= 0 && s < e.n) ? src[s] : 0.f;
    }
    __syncthreads();
    float m = 0.f;
    for (int t = tid; t < nt; t += RS_TILE) {
        const int nu = rem0 + t * down;
        const int a = nu / up;
        const float y = resample_sample(row, a, taps + (nu - a * up) * e.P_ld, P);
        otile[t] = y;
        m = fmaxf(m, fabsf(y));
    }
    __syncthreads();
    // dst rows and tile starts are multiples of 16 bytes: whole vectors, then the tile's last elements one by one
    float* d = e.dst + (int64_t)k * e.dst_ld + t0;
    const int nv = nt / 4;
    for (int v = tid; v < nv; v += RS_TILE) reinterpret_cast<uint4*>(d)[v] = reinterpret_cast<const uint4*>(otile)[v];
    for (int t = nv * 4 + tid; t < nt; t += RS_TILE) d[t] = otile[t];
    block_peak_to(m, w_peak, e.peak + k);
}

size_t so_lds_bytes(int up, int down, int P, int P_ld) { return ((size_t)so_tile_at(up, down, P, P_ld) + SO_TILE) * sizeof(float); }

size_t lds_bytes(const ResampleJob& e) {
    const int span_max = (RS_TILE * e.down + e.up - 1) / e.up + e.P + 1;
    const int row_ld = span_max - 1 + ((span_max - 1) >> 5) + 1;
    return ((size_t)e.up * e.P_ld + (size_t)e.C * row_ld) * sizeof(float);
}

constexpr size_t RS_LDS_MAX = 160 * 1024;

}  // namespace

bool resample_fits(const ResampleRatio& r, int C) {
    ResampleJob e{};
    e.up = r.up; e.down = r.down; e.P = r.P; e.P_ld = r.P_ld; e.C = C;
    return lds_bytes(e) <= RS_LDS_MAX;
}

bool launch_stream_ingest_resample_multi(const ResampleJob* e, int n, hipStream_t s) {
    return for_each_table<ResampleTable>(e, n, [&](const ResampleTable& tab, int cnt) {
        const int64_t most = table_max(tab, cnt, (int64_t)0, [](const ResampleJob& j) { return (j.n_m + RS_TILE - 1) / RS_TILE + 1; });
        const size_t lds = table_max(tab, cnt, (size_t)0, [](const ResampleJob& j) { return lds_bytes(j); });
        if (lds > RS_LDS_MAX) return false;
        if (lds > 65536 && hipFuncSetAttribute(reinterpret_cast<const void*>(stream_ingest_resample_kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return false;
        hipLaunchKernelGGL(stream_ingest_resample_kernel, dim3((unsigned)most, 1, cnt), dim3(RS_TILE), lds, s, tab);
        return true;
    });
}

bool stream_output_fits(const ResampleRatio& r) { return so_lds_bytes(r.up, r.down, r.P, r.P_ld) <= RS_LDS_MAX; }

bool launch_stream_output_multi(const StreamOutputJob* e, int n, int S, hipStream_t s, int* launches) {
    return for_each_table<StreamOutputTable>(e, n, [&](const StreamOutputTable& tab, int cnt) {
        const int64_t most = table_max(tab, cnt, (int64_t)0, [](const StreamOutputJob& j) { return (j.n_m + SO_TILE - 1) / SO_TILE + 1; });
        const size_t lds = table_max(tab, cnt, (size_t)0, [](const StreamOutputJob& j) { return so_lds_bytes(j.up, j.down, j.P, j.P_ld); });
        if (lds > RS_LDS_MAX) return false;
        if (lds > 65536 && hipFuncSetAttribute(reinterpret_cast<const void*>(stream_output_kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return false;
        hipLaunchKernelGGL(stream_output_kernel, dim3((unsigned)most, (unsigned)S, cnt), dim3(RS_TILE), lds, s, tab);
        if (launches) ++*launches;
        return true;
    });
}

// (both session kernels keep a few static LDS words beside the dynamic tile)
constexpr size_t SESSION_LDS_STATIC = 64;

bool session_ingest_fits(const ResampleRatio& r, int C) {
    ResampleJob e{};
    e.up = r.up; e.down = r.down; e.P = r.P; e.P_ld = r.P_ld; e.C = C;
    return lds_bytes(e) + SESSION_LDS_STATIC <= RS_LDS_MAX;
}

bool launch_session_ingest_multi(const SessionIngestJob* e, int n, hipStream_t s, int* launches) {
    return for_each_table<SessionIngestTable>(e, n, [&](const SessionIngestTable& tab, int cnt) {
        const int64_t most = table_max(tab, cnt, (int64_t)1, [](const SessionIngestJob& j) { return (j.r.n_m + RS_TILE - 1) / RS_TILE; });
        const size_t lds = table_max(tab, cnt, (size_t)0, [](const SessionIngestJob& j) { return lds_bytes(j.r); });
        if (lds + SESSION_LDS_STATIC > RS_LDS_MAX) return false;
        if (lds > 65536 - SESSION_LDS_STATIC &&
            hipFuncSetAttribute(reinterpret_cast<const void*>(session_ingest_resample_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds) != hipSuccess)
            return false;
        hipLaunchKernelGGL(session_ingest_resample_kernel, dim3((unsigned)most, 1, cnt), dim3(RS_TILE), lds, s, tab);
        if (launches) ++*launches;
        return true;
    });
}

bool launch_session_output(const SessionOutputJob& e, int S, hipStream_t s) {
    const size_t lds = so_lds_bytes(e.up, e.down, e.P, e.P_ld);
    if (lds + SESSION_LDS_STATIC > RS_LDS_MAX) return false;
    if (lds > 65536 - SESSION_LDS_STATIC &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(session_output_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
            hipSuccess)
        return false;
    if (e.n_m > 0)
        hipLaunchKernelGGL(session_output_kernel, dim3((unsigned)((e.n_m + SO_TILE - 1) / SO_TILE), (unsigned)S), dim3(RS_TILE), lds, s, e);
    return true;
}

bool launch_resample(const ResampleJob& e, hipStream_t s) {
    const size_t lds = lds_bytes(e);
    if (lds > RS_LDS_MAX) return false;
    if (lds > 65536 && hipFuncSetAttribute(reinterpret_cast<const void*>(resample_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)lds) != hipSuccess)
        return false;
    if (e.n_m > 0)
        hipLaunchKernelGGL(resample_kernel, dim3((unsigned)((e.n_m + RS_TILE - 1) / RS_TILE)), dim3(RS_TILE), lds, s, e);
    return true;
}

}  // namespace css

// ---- entry points that need no stream (include/css_mi355_rate.h) --------------------------------------------------------------
int css_stream_rate_samples(int32_t up, int32_t down, int64_t n_in, int32_t finished, int64_t* n_model) {
    ResampleRatio r;
    if (!n_model || n_in < 0 || !resample_ratio(up, down, &r) || n_in > INT64_MAX / r.up) return CSS_ERR_INVALID_ARG;
    *n_model = resample_count(r, n_in, finished != 0);
    return CSS_OK;
}

// (include/css_mi355_stream_out.h)
int css_stream_output_samples(const CssStreamOutputCfg* cfg, int64_t n_final_model, int32_t finished, int64_t* n) {
    if (!cfg || !n || n_final_model < 0) return CSS_ERR_INVALID_ARG;
    if (cfg->up == 1 && cfg->down == 1) { *n = n_final_model; return CSS_OK; }
    return css_stream_rate_samples(cfg->up, cfg->down, n_final_model, finished, n);
}

int css_resample_taps(int32_t up, int32_t down, float* taps, int32_t cap, int32_t* n_taps) {
    ResampleRatio r;
    if (!n_taps || !resample_ratio(up, down, &r)) return CSS_ERR_INVALID_ARG;
    *n_taps = r.L;
    if (!taps || cap < r.L) return CSS_ERR_INVALID_ARG;
    resample_taps_f32(r, taps);
    return CSS_OK;
}

int css_resample_host(css_handle_t h, const void* src, int32_t is_int16, int64_t n_in, int32_t n_ch, int64_t sample_stride,
                      int64_t channel_stride, int32_t up, int32_t down, float* out_host, int64_t cap, int64_t* n_out) {
    if (!h) return CSS_ERR_INVALID_ARG;
    ResampleRatio r;
    if (!n_out || n_in < 0 || (n_in > 0 && !src) || n_ch < 1 || n_ch > 64) return fail(h, CSS_ERR_INVALID_ARG, "bad argument");
    if (!resample_ratio(up, down, &r) || !resample_fits(r, n_ch) || n_in > ((int64_t)1 << 40))
        return fail(h, CSS_ERR_INVALID_ARG, "rate ratio: up != down in lowest terms, at most 128 taps per output sample and 16384 taps");
    const bool inter = (sample_stride == n_ch && channel_stride == 1) || (n_ch == 1 && sample_stride == 1);
    const bool planar = !inter && sample_stride == 1 && channel_stride >= n_in;
    if (n_in > 0 && !inter && !planar)
        return fail(h, CSS_ERR_INVALID_ARG, "strides: interleaved (sample_stride = channels, channel_stride = 1) or planar "
                                            "(sample_stride = 1, channel_stride >= n_in)");
    const int64_t m = resample_count(r, n_in, true);
    if (m > 0 && (!out_host || cap < m)) return fail(h, CSS_ERR_INVALID_ARG, "output capacity below ceil(n_in * up / down)");
    *n_out = m;
    if (m == 0) return CSS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const size_t el = is_int16 ? sizeof(int16_t) : sizeof(float);
    std::vector<float> taps((size_t)r.L), tab((size_t)r.up * r.P_ld);
    resample_taps_f32(r, taps.data());
    resample_phase_table(r, taps.data(), tab.data());
    DevBuf d_src, d_tab, d_out;   // released when the call returns, behind the synchronise below
    hipError_t e = dev_alloc(d_src, (size_t)n_in * n_ch * el);
    if (e == hipSuccess) e = dev_alloc(d_tab, tab.size() * sizeof(float));
    if (e == hipSuccess) e = dev_alloc(d_out, (size_t)m * n_ch * sizeof(float));
    if (e == hipSuccess) e = hipMemcpyAsync(d_tab.p, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess)
        e = planar ? hipMemcpy2DAsync(d_src.p, (size_t)n_in * el, src, (size_t)channel_stride * el, (size_t)n_in * el, (size_t)n_ch,
                                      hipMemcpyHostToDevice, h->stream)
                   : hipMemcpyAsync(d_src.p, src, (size_t)n_in * n_ch * el, hipMemcpyHostToDevice, h->stream);
    bool launched = true;
    if (e == hipSuccess) {
        ResampleJob j{};
        j.src = d_src.p; j.is_i16 = is_int16 ? 1 : 0; j.plane_ld = planar ? n_in : 0; j.n = n_in;
        j.N0 = 0; j.m0 = 0; j.n_m = m;
        j.up = r.up; j.down = r.down; j.half = r.half; j.P = r.P; j.P_ld = r.P_ld; j.tab = d_tab.as();
        j.C = n_ch; j.dst = d_out.as(); j.dst_ld = 0;
        launched = launch_resample(j, h->stream);
        if (launched) e = hipGetLastError();
    }
    if (e == hipSuccess && launched) e = hipMemcpyAsync(out_host, d_out.p, (size_t)m * n_ch * sizeof(float), hipMemcpyDeviceToHost, h->stream);
    const hipError_t es = hipStreamSynchronize(h->stream);
    if (!launched) return fail(h, CSS_ERR_HIP, "the resampling kernel's LDS could not be reserved");
    if (e != hipSuccess || es != hipSuccess)
        return fail(h, CSS_ERR_HIP, std::string("css_resample_host: ") + hipGetErrorString(e != hipSuccess ? e : es));
    return CSS_OK;
}
