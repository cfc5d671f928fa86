// Device hand-off of the separated streams to the ASR front end.
//
// The reference writes the streams to wav files and Whisper reads them back (asr/asr.py:58,73-74); it notes itself that
// the silent parts could be dropped to save ASR compute (css/css.py:313).  Here a stream stays in HBM: the frames the
// activity gate kept (css.py:303-312, plus a margin) are cut out and concatenated -- the region table is the time map
// back -- and turned into Whisper's input features on the device: reflect-padded 400-point Hann STFT at hop 160, power
// spectrum, slaney mel filterbank (80 or 128 bands), log10 with the 1e-10 floor, the max - 8 clamp, (x + 4) / 4
// (whisper/audio.py log_mel_spectrogram -- a dependency that is not under the reference tree and not installed here:
// its published algorithm is restated; tests compare with the oracle's numpy restatement, which is held to
// transformers.WhisperFeatureExtractor in tests/test_oracle_whisper_pin.py).
#include <algorithm>
#include <cmath>
#include <vector>

#include <hip/hip_fp16.h>

#include "kernels.hpp"
#include "table.hpp"
#include "wave.hpp"
#include "window_vec.hpp"

namespace css {

constexpr int MEL_TILE_FRAMES = 32, MEL_TILE_ROWS = 8;   // a mel tile: thread t has frame t % 32 and bands t / 32, t / 32 + 8, ...
constexpr int MEL_NFFT = 400, MEL_BINS = 201, MEL_K = 416;   // hop 160 (the row stride of the frame operand);   // K padded to the GEMM's 32

// ---- host: tables ---------------------------------------------------------------------------------------------------
// analysis matrix [2 * 201][416]: rows f = cos, 201 + f = -sin of 2 pi f n / 400, times the periodic Hann window
void handoff_build_dft(float* m) {
    for (int f = 0; f < MEL_BINS; ++f)
        for (int n = 0; n < MEL_K; ++n) {
            double c = 0.0, s = 0.0;
            if (n < MEL_NFFT) {
                const double w = (double)(float)(0.5 - 0.5 * std::cos(2.0 * M_PI * n / MEL_NFFT));
                const double a = 2.0 * M_PI * (double)((int64_t)f * n % MEL_NFFT) / MEL_NFFT;
                c = std::cos(a) * w;
                s = -std::sin(a) * w;
            }
            m[(size_t)f * MEL_K + n] = (float)c;
            m[(size_t)(MEL_BINS + f) * MEL_K + n] = (float)s;
        }
}

static double hz_to_mel(double f) {
    const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
    return f >= min_log_hz ? min_log_mel + std::log(f / min_log_hz) / logstep : f / f_sp;
}
static double mel_to_hz(double m) {
    const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
    return m >= min_log_mel ? min_log_hz * std::exp(logstep * (m - min_log_mel)) : f_sp * m;
}
// librosa.filters.mel(sr=16000, n_fft=2 (bins - 1), n_mels) (slaney scale and normalisation), float32 [n_mels][bins]: 201 bins
// for Whisper's 400-point transform, 257 for the 512-point one of nemo.hip
void handoff_build_mel(float* w, int n_mels, int bins) {
    const double sr = 16000.0;
    std::vector<double> mel_f(n_mels + 2);
    const double lo = hz_to_mel(0.0), hi = hz_to_mel(sr / 2);
    for (int i = 0; i < n_mels + 2; ++i) mel_f[i] = mel_to_hz(lo + (hi - lo) * i / (n_mels + 1));
    for (int i = 0; i < n_mels; ++i) {
        const double enorm = 2.0 / (mel_f[i + 2] - mel_f[i]);
        for (int f = 0; f < bins; ++f) {
            const double hz = sr / 2 * f / (bins - 1);
            const double lower = (hz - mel_f[i]) / (mel_f[i + 1] - mel_f[i]);
            const double upper = (mel_f[i + 2] - hz) / (mel_f[i + 2] - mel_f[i + 1]);
            w[(size_t)i * bins + f] = (float)(std::fmax(0.0, std::fmin(lower, upper)) * enorm);
        }
    }
}

// ---- device ---------------------------------------------------------------------------------------------------------
// out[i] = concatenation of the regions of `wav`, reflect-padded by 200 samples at both ends (torch.stft center=True),
// i in [0, n_act + 400); zeros up to `total`.  regions: [nr][2] sample ranges, offs[r] = samples before region r.
__global__ void handoff_gather_kernel(const float* __restrict__ wav, const int64_t* __restrict__ regions,
                                      const int64_t* __restrict__ offs, int nr, int64_t n_act, float* __restrict__ out,
                                      int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    float v = 0.f;
    if (i < n_act + MEL_NFFT && n_act > 0) {
        int64_t j = i - MEL_NFFT / 2;
        if (j < 0) j = -j;                                   // reflect (no edge repeat)
        if (j >= n_act) j = 2 * (n_act - 1) - j;
        j = j < 0 ? 0 : j;
        int lo = 0, hi = nr - 1;
        while (lo < hi) {                                    // last region with offs[r] <= j
            const int mid = (lo + hi + 1) >> 1;
            if (offs[mid] <= j) lo = mid; else hi = mid - 1;
        }
        v = wav[regions[2 * lo] + (j - offs[lo])];
    }
    out[i] = v;
}

// One tile of 32 frames, shared by the offline kernel and the streamed one so that both round alike (re * re + im * im is
// open to contraction: one copy of the expression, one rounding).  spec [402][ld] (rows f: Re, 201 + f: Im; time fastest),
// the tile's frames are columns col0 + j0 .. of it -> mel[m * mel_ld + j] = log10(max(sum_f w[m][f] |X|^2, 1e-10)) for the
// frames j < nfr, and the maximum of what was written into *gmax (as an order-preserving integer).  pw: the block's LDS for the
// tile's power spectra, the caller's (free again once every thread has returned)
using MelTilePw = float[MEL_BINS][MEL_TILE_FRAMES + 1];
__device__ __forceinline__ void handoff_mel_tile(MelTilePw& pw, const float* __restrict__ spec, int64_t ld, int64_t col0, int64_t j0, int64_t nfr,
                                                 const float* __restrict__ w, int n_mels, float* __restrict__ mel, int64_t mel_ld,
                                                 int* __restrict__ gmax) {
    static_assert(MEL_TILE_FRAMES == 32 && MEL_TILE_ROWS == 8, "256 threads: the low five bits are the frame");
    const int tj = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int f = ty; f < MEL_BINS; f += MEL_TILE_ROWS) {
        const int64_t j = j0 + tj;
        float p = 0.f;
        if (j < nfr) {
            const float re = spec[(int64_t)f * ld + col0 + j], im = spec[(int64_t)(MEL_BINS + f) * ld + col0 + j];
            p = re * re + im * im;
        }
        pw[f][tj] = p;
    }
    __syncthreads();
    float best = -INFINITY;
    for (int m = ty; m < n_mels; m += MEL_TILE_ROWS) {
        float acc = 0.f;
        const float* wm = w + (size_t)m * MEL_BINS;
        for (int f = 0; f < MEL_BINS; ++f) acc = fmaf(wm[f], pw[f][tj], acc);
        // At the floor the value is -10.0f itself: the device library's log10f(1e-10f) lies one ulp below it, and Whisper's
        // features of silence are -1.5, the value the encoder windows pad with.  (A NaN sum compares false: the floor, as fmaxf gave.)
        const float v = acc > 1e-10f ? log10f(acc) : -10.0f;
        if (j0 + tj < nfr) {
            mel[(int64_t)m * mel_ld + j0 + tj] = v;
            best = fmaxf(best, v);
        }
    }
    best = wave_max_shfl(best);
    if ((threadIdx.x & 63) == 0 && best > -INFINITY) {
        const int b = __float_as_int(best);
        atomicMax(gmax, b >= 0 ? b : b ^ 0x7fffffff);       // monotone map float -> int
    }
}

__global__ __launch_bounds__(256) void handoff_mel_kernel(const float* __restrict__ spec, int64_t ld, int64_t nfr,
                                                          const float* __restrict__ w, int n_mels, float* __restrict__ mel,
                                                          int* __restrict__ gmax) {
    __shared__ MelTilePw pw;
    handoff_mel_tile(pw, spec, ld, 0, (int64_t)blockIdx.x * MEL_TILE_FRAMES, nfr, w, n_mels, mel, nfr, gmax);
}

__global__ void handoff_norm_kernel(float* __restrict__ mel, int64_t count, const int* __restrict__ gmax) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int b = *gmax;
    const float mx = __int_as_float(b >= 0 ? b : b ^ 0x7fffffff);
    mel[i] = (fmaxf(mel[i], mx - 8.0f) + 4.0f) * 0.25f;
}

void launch_handoff_gather(const float* wav, const int64_t* regions, const int64_t* offs, int nr, int64_t n_act, float* out,
                           int64_t total, hipStream_t s) {
    if (total <= 0) return;
    hipLaunchKernelGGL(handoff_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, wav, regions, offs, nr, n_act, out, total);
}
void launch_handoff_mel(const float* spec, int64_t ld, int64_t nfr, const float* w, int n_mels, float* mel, int* gmax, hipStream_t s) {
    if (nfr <= 0) return;
    hipMemsetAsync(gmax, 0x80, sizeof(int), s);             // 0x80808080: below every mapped finite value
    hipLaunchKernelGGL(handoff_mel_kernel, dim3((unsigned)((nfr + MEL_TILE_FRAMES - 1) / MEL_TILE_FRAMES)), dim3(256), 0, s, spec, ld, nfr, w, n_mels, mel, gmax);
    const int64_t count = nfr * n_mels;
    hipLaunchKernelGGL(handoff_norm_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, mel, count, gmax);
}

// ---- streamed sessions ----------------------------------------------------------------------------------------------
struct HandoffAppendTable : Table<HandoffAppend, HANDOFF_MULTI_MAX> {};
struct HandoffMelTable : Table<HandoffMel, HANDOFF_MULTI_MAX> {};

// One block per (stream, speaker).  Block q of 256 samples is kept iff an active frame t has t - pad <= q <= t + pad + 1
// (frame t spans blocks t and t + 1); every frame that can keep a block below D1 is gated-final.  The kept samples of
// [D0, D1) go behind the A samples already in the concatenation; with J frames emitted, frame j is the 400 samples from
// 160 j of the concatenation reflect-padded by 200, so operand column x of this speaker's rows is padded sample 160 J + x.
__global__ __launch_bounds__(256) void handoff_append_kernel(HandoffAppendTable tab, float* __restrict__ operand) {
    const HandoffAppend& e = tab.e[blockIdx.z];
    const int k = blockIdx.y, tid = threadIdx.x;
    constexpr int HOP = 256;
    __shared__ int len[256], off[256];
    __shared__ int total;
    const int64_t A0 = e.st[k].A, J0 = e.st[k].J;
    const int64_t tail0 = J0 > 0 ? 160 * J0 - 200 : 0;
    float* __restrict__ op = operand + (e.row0 + (int64_t)k * e.rows) * 160;
    const int64_t op_n = e.rows * 160;
    const uint8_t* __restrict__ gate = e.gate + (int64_t)k * e.gate_ld;
    const float* __restrict__ out = e.out + (int64_t)k * e.out_ld;
    const float* __restrict__ carry = e.carry_in + (int64_t)k * e.carry_ld;
    const float* __restrict__ tail_in = e.tail_in + (int64_t)k * HANDOFF_TAIL_LD;
    auto sample = [&](int64_t n) { return n >= e.out_base ? out[n - e.out_base] : carry[n - e.D0]; };
    // ---- the kept blocks of [D0, D1), compacted behind sample A0 of the concatenation
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
            for (int i = 0; i < 256; ++i) { off[i] = acc; acc += len[i]; }
            total = acc;
        }
        __syncthreads();
        for (int i = tid; i < 256 * HOP; i += 256) {
            const int b = i >> 8, r = i & (HOP - 1);
            if (r < len[b]) {
                const int64_t x = A1 + off[b] + r + 200 - 160 * J0;
                if (x < op_n) op[x] = sample((c0 + b) * HOP + r);
            }
        }
        A1 += total;
        __syncthreads();
    }
    // ---- frames complete now; the rest of the operand: what the tail carried, the reflections, zeros
    const int64_t J1 = e.closing ? A1 / 160 : (A1 >= 201 ? (A1 - 200) / 160 + 1 : 0);
    auto concat = [&](int64_t c) { return c < A0 ? tail_in[c - tail0] : op[c + 200 - 160 * J0]; };
    for (int64_t x = tid; x < op_n; x += 256) {
        const int64_t i = 160 * J0 + x;
        int64_t j = i - 200;
        bool mirrored = j < 0, own = false;   // own: a new sample in its own place, written above
        if (mirrored) j = -j;
        float v = 0.f;
        if (e.closing ? (A1 > 0 && i < A1 + 400) : j < A1) {
            if (j >= A1) { j = 2 * (A1 - 1) - j; mirrored = true; }   // (the gather kernel's reflection, clamp included)
            j = j < 0 ? 0 : j;
            own = !mirrored && j >= A0;
            if (!own) v = concat(j);
        }
        if (!own) op[x] = v;
    }
    __syncthreads();
    const int64_t tail1 = J1 > 0 ? 160 * J1 - 200 : 0;
    float* __restrict__ tail_out = e.tail_out + (int64_t)k * HANDOFF_TAIL_LD;
    // (J1 == 1: tail1 is -40 and the first 40 floats stand for samples before the concatenation: nothing reads them, and there is
    //  nothing to read for them -- with J0 == 0 concat(c < 0) would be tail_in[-40 ..], below the speaker's row)
    for (int64_t c = tail1 + tid; c < A1 && c - tail1 < HANDOFF_TAIL_LD; c += 256) tail_out[c - tail1] = c < 0 ? 0.f : concat(c);
    // ---- the samples still undecided, for the next round; the gate bytes of the round; the counts
    const int64_t end = e.t_g1 * HOP;
    float* __restrict__ carry_out = e.carry_out + (int64_t)k * e.carry_ld;
    for (int64_t n = e.D1 + tid; n < end; n += 256) carry_out[n - e.D1] = sample(n);
    uint8_t* __restrict__ act = e.act_out + (int64_t)k * (e.t_g1 - e.t_g0);
    for (int64_t t = e.t_g0 + tid; t < e.t_g1; t += 256) act[t - e.t_g0] = gate[t & e.gate_mask];
    if (tid == 0) {
        if (e.st_out != e.st) e.st_out[k].gmax = e.st[k].gmax;   // (a preview: the mel kernel folds into the scratch row)
        e.st_out[k].A = A1;
        e.st_out[k].J = J1;
        e.n_new[k] = (int)(J1 - J0);
    }
}

// A frame's maximum over the bands, for the tile's frame of this thread's column: every thread reads back the values it stored
// itself (the tile's own float32 results: MEL_TILE_FRAMES / MEL_TILE_ROWS are the tile's mapping of threads to outputs, so no
// thread reads another's store), hands each to keep(m, v) and folds them; the row groups of a column gather in the tile's LDS once
// every thread is done with it.  take: whether this thread's frame takes part.  The maximum is row 0's (ty == 0) result.
template <typename Keep>
__device__ __forceinline__ float handoff_frame_max(MelTilePw& pw, bool take, const float* __restrict__ mel, int64_t mel_ld, int n_mels, Keep keep) {
    float (*fm)[MEL_TILE_FRAMES] = reinterpret_cast<float (*)[MEL_TILE_FRAMES]>(&pw[0][0]);   // [MEL_TILE_ROWS][MEL_TILE_FRAMES]
    const int tj = threadIdx.x & (MEL_TILE_FRAMES - 1), ty = threadIdx.x / MEL_TILE_FRAMES;
    float best = -INFINITY;
    if (take)
        for (int m = ty; m < n_mels; m += MEL_TILE_ROWS) {
            const float v = mel[(int64_t)m * mel_ld];
            keep(m, v);
            best = fmaxf(best, v);
        }
    __syncthreads();   // (the tile's last reads of pw)
    fm[ty][tj] = best;
    __syncthreads();
    if (ty == 0) {
#pragma unroll
        for (int i = 1; i < MEL_TILE_ROWS; ++i) best = fmaxf(best, fm[i][tj]);
    }
    return best;
}

// PVMAX: the launch of a preview's round that has an entry with HandoffMel::pvmax (windows up to the present); every other launch
// is the <false> instance, which has no code for it.
template <bool PVMAX>
__global__ __launch_bounds__(256) void handoff_mel_multi_kernel(HandoffMelTable tab, const float* __restrict__ spec, int64_t ld) {
    const HandoffMel& e = tab.e[blockIdx.z];
    const int k = blockIdx.y;
    const int64_t nfr = e.n_new[k] < e.rows ? e.n_new[k] : e.rows, j0 = (int64_t)blockIdx.x * MEL_TILE_FRAMES;
    if (j0 >= nfr) return;
    __shared__ MelTilePw pw;
    handoff_mel_tile(pw, spec, ld, e.row0 + (int64_t)k * e.rows, j0, nfr, e.w, e.n_mels, e.mel + (int64_t)k * e.n_mels * e.mel_ld, e.mel_ld,
                     &e.st[k].gmax);
    const int64_t j = j0 + (threadIdx.x & (MEL_TILE_FRAMES - 1));
    const bool row0 = threadIdx.x < MEL_TILE_FRAMES;
    const float* mel = e.mel + (int64_t)k * e.n_mels * e.mel_ld + j;
    if constexpr (PVMAX) {
        // The provisional frames stay where the tile wrote them; each frame's maximum over the bands goes next to them.
        if (e.pvmax) {
            const float best = handoff_frame_max(pw, j < nfr, mel, e.mel_ld, e.n_mels, [](int, float) {});
            if (row0 && j < nfr) e.pvmax[(int64_t)k * e.rows + j] = best;
            return;
        }
    }
    if (!e.ring) return;
    // The frame history: the frames go into the ring with their maxima over the bands (a kernel without a history pays no LDS and
    // no barrier for this).  The append kernel has moved st.J to the count after the round, so the round's frame j is frame
    // J - n_new + j of the concatenation; only the last `hist` frames of a round are kept, so no two blocks of a launch write one slot.
    const bool keep = j < nfr && j >= nfr - e.hist;
    const int64_t slot = keep ? (e.st[k].J - e.n_new[k] + j) % e.hist : 0;
    float* ring = e.ring + (int64_t)k * e.n_mels * e.hist + slot;
    const float best = handoff_frame_max(pw, keep, mel, e.mel_ld, e.n_mels, [&](int m, float v) { ring[(int64_t)m * e.hist] = v; });
    if (row0 && keep) e.fmax[(int64_t)k * e.hist + slot] = best;
}

// ---- encoder windows: a span of the frame history, then a preview's provisional frames where the window reaches the present ----
struct WindowTable : Table<WindowItem, WINDOW_MULTI_MAX> {};

// Frames s .. s + V - 1 of one band's row of `len` floats (the caller has s + V <= len) through 16-byte loads: as they are at a
// 16-byte boundary; off it, the aligned pieces around them where those lie inside the row (selects on constant positions: no
// scratch).  false: neither fits, nothing was loaded.
template <int V>
__device__ __forceinline__ bool window_load16(const float* __restrict__ row, int64_t s, int64_t len, float (&v)[V]) {
    const int d = (int)(((uintptr_t)(row + s) >> 2) & 3);   // floats past a 16-byte boundary
    if (d == 0) {
#pragma unroll
        for (int i = 0; i < V; i += 4) {
            const float4 q = *reinterpret_cast<const float4*>(row + s + i);
            v[i] = q.x; v[i + 1] = q.y; v[i + 2] = q.z; v[i + 3] = q.w;
        }
        return true;
    }
    if (s >= d && s - d + V + 4 <= len) {
        float b[V + 4];
#pragma unroll
        for (int i = 0; i < V + 4; i += 4) {
            const float4 q = *reinterpret_cast<const float4*>(row + s - d + i);
            b[i] = q.x; b[i + 1] = q.y; b[i + 2] = q.z; b[i + 3] = q.w;
        }
#pragma unroll
        for (int i = 0; i < V; ++i) v[i] = d == 1 ? b[i + 1] : d == 2 ? b[i + 2] : b[i + 3];
        return true;
    }
    return false;
}

// The span as the block resolved it: columns [0, n_ring) are the ring's slots slot0 .. (wrapping at hist), columns
// [n_ring, used) the provisional frames p0 .., the rest padding.
struct WindowSpan { int64_t slot0; int n_ring, used, p0; };

// One wave per band: consecutive lanes on consecutive columns.  The destination row is written with scalar stores up to its
// first 16-byte boundary, 16-byte stores from there, scalar stores behind the last whole one.  A 16-byte group that lies in one
// stretch of the ring, or wholly in the provisional frames, is read with 16-byte loads inside that source; the ring's wrap, the
// seam between the sources and the last frames before the padding are taken frame by frame.  (A window out of the history alone
// has n_ring == used: no column is provisional.)
template <typename T>
__device__ __forceinline__ void window_row(const WindowItem& e, const WindowSpan& sp, const float* __restrict__ ring,
                                           const float* __restrict__ pv, T* __restrict__ dst, float lo, float fill, int lane) {
    constexpr int V = WindowVec<T>::V;
    auto norm = [&](float raw) { return (fmaxf(raw, lo) + 4.0f) * 0.25f; };
    auto one = [&](int c) {
        if (c >= sp.used) return fill;
        if (c >= sp.n_ring) return norm(pv[sp.p0 + (c - sp.n_ring)]);
        int64_t s = sp.slot0 + c;
        if (s >= e.hist) s -= e.hist;
        return norm(ring[s]);
    };
    const int head = min((int)(((16 - ((uintptr_t)dst & 15)) & 15) / sizeof(T)), e.width);
    const int nvec = (e.width - head) / V, tail = head + nvec * V;
    for (int c = lane; c < head; c += 64) WindowVec<T>::store(dst + c, one(c));
    for (int c = tail + lane; c < e.width; c += 64) WindowVec<T>::store(dst + c, one(c));
    for (int g = lane; g < nvec; g += 64) {
        const int c = head + g * V;
        float v[V];
        bool done = false;
        if (c + V <= sp.n_ring) {
            int64_t s = sp.slot0 + c;
            if (s >= e.hist) s -= e.hist;
            if (s + V <= e.hist) done = window_load16<V>(ring, s, e.hist, v);
        } else if (c >= sp.n_ring && c + V <= sp.used) {
            done = window_load16<V>(pv, sp.p0 + (c - sp.n_ring), e.pv_ld, v);
        }
        if (done) {
#pragma unroll
            for (int i = 0; i < V; ++i) v[i] = norm(v[i]);
        } else {
#pragma unroll
            for (int i = 0; i < V; ++i) v[i] = one(c + i);
        }
        WindowVec<T>::store16(dst + c, v);
    }
}

__global__ __launch_bounds__(256) void stream_window_kernel(WindowTable tab) {
    const WindowItem& e = tab.e[blockIdx.z];
    const int m0 = blockIdx.x * WINDOW_ROWS;
    if (m0 >= e.n_mels) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the span: P provisional frames behind the J final ones, of which the ring holds [R, J)
    const int64_t n_new = e.n_new ? *e.n_new : 0;
    const int64_t P = n_new < e.pv_ld ? n_new : e.pv_ld;
    const int64_t E = e.J + P, R = e.J > e.hist ? e.J - e.hist : 0, a = E - e.n_frames > R ? E - e.n_frames : R;
    WindowSpan sp;
    sp.used = (int)(E - a);
    const int n_prov = sp.used < P ? sp.used : (int)P;
    sp.n_ring = sp.used - n_prov;
    sp.p0 = (int)P - n_prov;
    sp.slot0 = a % e.hist;
    if (blockIdx.x == 0 && tid == 0) {
        e.res->first_frame = a;
        e.res->n_used = sp.used;
        e.res->n_provisional = n_prov;
    }
    if (sp.used == 0) return;
    // the window's maximum: over the per-frame maxima of its frames (a maximum is exact in any order)
    __shared__ float wm[4];
    float M = -INFINITY;
    for (int c = tid; c < sp.used; c += 256) {
        if (c >= sp.n_ring) {
            M = fmaxf(M, e.pvmax[sp.p0 + (c - sp.n_ring)]);
        } else {
            int64_t s = sp.slot0 + c;
            if (s >= e.hist) s -= e.hist;
            M = fmaxf(M, e.fmax[s]);
        }
    }
    M = wave_max_shfl(M);
    if (lane == 0) wm[wave] = M;
    __syncthreads();
    M = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
    if (blockIdx.x == 0 && tid == 0) e.res->window_max = M;
    const float lo = M - 8.0f, fill = (fmaxf(-10.0f, lo) + 4.0f) * 0.25f;
    for (int m = m0 + wave; m < e.n_mels && m < m0 + WINDOW_ROWS; m += 4) {
        const float* ring = e.ring + (int64_t)m * e.hist;
        const float* pv = e.pv + (int64_t)m * e.pv_ld;
        if (e.f16) window_row<__half>(e, sp, ring, pv, (__half*)e.out + (int64_t)m * e.ld, lo, fill, lane);
        else window_row<float>(e, sp, ring, pv, (float*)e.out + (int64_t)m * e.ld, lo, fill, lane);
    }
}

void launch_stream_windows(const WindowItem* e, int n, hipStream_t s) {
    // (the caller chunks and counts the launches: more than one table here would be a launch it does not report)
    for_each_table<WindowTable>(e, std::min(n, WINDOW_MULTI_MAX), [&](const WindowTable& tab, int cnt) {
        const int most = table_max(tab, cnt, 1, [](const WindowItem& w) { return (int)w.n_mels; });
        hipLaunchKernelGGL(stream_window_kernel, dim3((unsigned)((most + WINDOW_ROWS - 1) / WINDOW_ROWS), 1, cnt), dim3(256), 0, s, tab);
        return true;
    });
}

void launch_handoff_append_multi(const HandoffAppend* e, int n, float* operand, hipStream_t s) {
    for_each_table<HandoffAppendTable>(e, n, [&](const HandoffAppendTable& tab, int cnt) {
        hipLaunchKernelGGL(handoff_append_kernel, dim3(1, tab.e[0].S, cnt), dim3(256), 0, s, tab, operand);
        return true;
    });
}
void launch_handoff_mel_multi(const HandoffMel* e, int n, int S, const float* spec, int64_t ld, hipStream_t s) {
    for_each_table<HandoffMelTable>(e, n, [&](const HandoffMelTable& tab, int cnt) {
        const int64_t most = table_max(tab, cnt, (int64_t)1, [](const HandoffMel& m) { return m.rows; });
        const dim3 grid((unsigned)((most + MEL_TILE_FRAMES - 1) / MEL_TILE_FRAMES), S, cnt);
        if (table_max(tab, cnt, 0, [](const HandoffMel& m) { return m.pvmax ? 1 : 0; }))   // any entry with provisional maxima
            hipLaunchKernelGGL(handoff_mel_multi_kernel<true>, grid, dim3(256), 0, s, tab, spec, ld);
        else hipLaunchKernelGGL(handoff_mel_multi_kernel<false>, grid, dim3(256), 0, s, tab, spec, ld);
        return true;
    });
}

// ---- queued sessions: ranges and counts found on the device ---------------------------------------------------------------------
constexpr int SCAN_PER_THREAD = SESSION_SCAN_CHUNK / 256;
static_assert(SCAN_PER_THREAD == 4, "a thread of the keep-scan owns one 32-bit word of gate bytes / four sample blocks");

// Exclusive prefix sums of v over the block's 256 threads (x and y apiece), and the block's sums: a shuffle scan inside each
// wave, the four waves' sums through LDS.  Every thread of the block calls it; sh is free again when it returns.
__device__ __forceinline__ int2 session_block_scan(int2 v, int2 (&sh)[4], int2& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int2 x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int ax = __shfl_up(x.x, o), ay = __shfl_up(x.y, o);
        if (lane >= o) { x.x += ax; x.y += ay; }
    }
    if (lane == 63) sh[wave] = x;
    __syncthreads();
    int2 before = make_int2(0, 0);
    total = make_int2(0, 0);
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < wave) { before.x += sh[w].x; before.y += sh[w].y; }
        total.x += sh[w].x; total.y += sh[w].y;
    }
    __syncthreads();
    return make_int2(before.x + x.x - v.x, before.y + x.y - v.y);
}

// One block per speaker of the session.  Pass 1: psum[t] = active frames below t, for t = 0 .. TL, in chunks of
// SESSION_SCAN_CHUNK frames with a carry; the chunks are laid over the 32-bit words of the gate row (a speaker's row starts at
// k TL: any alignment), a thread takes one word as a whole where it lies inside the row and byte by byte at the row's two ends.
// Pass 2: block q is kept iff psum says that a frame of [q - pad - 1, q + pad] is active; a prefix sum over the kept blocks and
// over the run starts, again chunk by chunk, gives every run its index -- so the run table comes out in ascending order -- and
// the samples kept before it.  A run's start and its end are written by the threads that own those blocks.
__global__ __launch_bounds__(256) void session_keep_scan_kernel(SessionHandoff e) {
    const int k = blockIdx.x, tid = threadIdx.x;
    __shared__ int2 sh[4];
    const int64_t TL = e.TL;
    const uint8_t* __restrict__ gate = e.gate + (int64_t)k * TL;
    int32_t* __restrict__ psum = e.psum + (int64_t)k * (TL + 1);
    int2 total;
    if (e.drop) {
        const int64_t a = (int64_t)((uintptr_t)gate & 3);   // bytes between the word boundary below the row and the row
        int carry = 0;
        if (tid == 0) psum[0] = 0;
        for (int64_t c0 = 0; c0 < a + TL; c0 += SESSION_SCAN_CHUNK) {
            const int64_t u = c0 + (int64_t)tid * SCAN_PER_THREAD;   // this thread's word: row frames [u - a, u - a + 4)
            int b[SCAN_PER_THREAD];
            if (u >= a && u + SCAN_PER_THREAD <= a + TL) {
                const uint32_t w = *reinterpret_cast<const uint32_t*>(gate + (u - a));
#pragma unroll
                for (int i = 0; i < SCAN_PER_THREAD; ++i) b[i] = ((w >> (8 * i)) & 0xffu) != 0;
            } else {
#pragma unroll
                for (int i = 0; i < SCAN_PER_THREAD; ++i) {
                    const int64_t t = u + i - a;
                    b[i] = (t >= 0 && t < TL) ? gate[t] != 0 : 0;
                }
            }
            const int2 ex = session_block_scan(make_int2(b[0] + b[1] + b[2] + b[3], 0), sh, total);
            int run = carry + ex.x;
#pragma unroll
            for (int i = 0; i < SCAN_PER_THREAD; ++i) {
                const int64_t t = u + i - a;
                run += b[i];
                if (t >= 0 && t < TL) psum[t + 1] = run;
            }
            carry += total.x;
        }
        __syncthreads();   // pass 2 reads what other threads of this block stored
    }
    const int64_t pad = e.pad;
    auto kept = [&](int64_t q) -> int {   // blocks 0 .. TL; outside: not kept
        if (q < 0 || q > TL) return 0;
        if (!e.drop) return 1;
        const int64_t lo = q - pad - 1 < 0 ? 0 : q - pad - 1, hi = q + pad < TL - 1 ? q + pad : TL - 1;
        return psum[hi + 1] - psum[lo] > 0;
    };
    int64_t* __restrict__ regs = e.regs + (int64_t)k * e.cap_ranges * 2;
    int64_t* __restrict__ offs = e.offs + (int64_t)k * e.cap_ranges;
    int64_t* __restrict__ ranges_out = e.ranges_out + (int64_t)k * e.cap_ranges * 2;
    int64_t blocks_before = 0;
    int runs_before = 0;
    for (int64_t c0 = 0; c0 <= TL; c0 += SESSION_SCAN_CHUNK) {
        const int64_t q0 = c0 + (int64_t)tid * SCAN_PER_THREAD;
        int f[SCAN_PER_THREAD + 2];   // kept flags of blocks q0 - 1 .. q0 + 4
#pragma unroll
        for (int i = 0; i < SCAN_PER_THREAD + 2; ++i) f[i] = kept(q0 - 1 + i);
        int nk = 0, ns = 0;
#pragma unroll
        for (int i = 1; i <= SCAN_PER_THREAD; ++i) { nk += f[i]; ns += f[i] && !f[i - 1]; }
        const int2 ex = session_block_scan(make_int2(nk, ns), sh, total);
        int64_t blk = blocks_before + ex.x;
        int r = runs_before + ex.y;   // runs that start below the block at hand
#pragma unroll
        for (int i = 1; i <= SCAN_PER_THREAD; ++i) {
            const int64_t q = q0 + i - 1;
            if (f[i] && !f[i - 1]) {
                if (r < e.cap_ranges) { regs[2 * r] = q * 256; offs[r] = blk * 256; ranges_out[2 * r] = q * 256; }
                ++r;
            }
            if (f[i] && !f[i + 1] && r - 1 < e.cap_ranges) { regs[2 * (r - 1) + 1] = (q + 1) * 256; ranges_out[2 * (r - 1) + 1] = (q + 1) * 256; }
            blk += f[i];
        }
        blocks_before += total.x;
        runs_before += total.y;
    }
    if (tid == 0) {
        const int64_t n_act = blocks_before * 256, nfr = n_act / 160;   // whisper: 1 + n // hop frames, the last one dropped
        e.st[k].A = n_act;
        e.st[k].J = nfr;
        e.st[k].gmax = (int)0x80808080;   // below every mapped finite value (launch_handoff_mel's reset)
        e.n_new[k] = (int32_t)nfr;
        e.n_ranges[k] = runs_before;
        e.n_frames_out[k] = nfr;
        e.n_ranges_out[k] = runs_before;
    }
}

// handoff_gather_kernel's body for all speakers, the run count and the sample count read from what the keep-scan wrote:
// operand floats [k per, (k + 1) per) are speaker k's; behind the last speaker's, 416 zeros (the product's last rows read them)
__global__ __launch_bounds__(256) void session_gather_kernel(SessionHandoff e, const float* __restrict__ wavs, int64_t wav_ld,
                                                             float* __restrict__ operand, int64_t per) {
    const int k = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= per + (k == e.S - 1 ? MEL_K : 0)) return;
    const int64_t n_act = e.st[k].A;
    const int nr = e.n_ranges[k] < e.cap_ranges ? e.n_ranges[k] : e.cap_ranges;
    const int64_t* __restrict__ regions = e.regs + (int64_t)k * e.cap_ranges * 2;
    const int64_t* __restrict__ offs = e.offs + (int64_t)k * e.cap_ranges;
    const float* __restrict__ wav = wavs + (int64_t)k * wav_ld;
    float v = 0.f;
    if (i < n_act + MEL_NFFT && n_act > 0 && nr > 0) {
        int64_t j = i - MEL_NFFT / 2;
        if (j < 0) j = -j;                                   // reflect (no edge repeat)
        if (j >= n_act) j = 2 * (n_act - 1) - j;
        j = j < 0 ? 0 : j;
        int lo = 0, hi = nr - 1;
        while (lo < hi) {                                    // last region with offs[r] <= j
            const int mid = (lo + hi + 1) >> 1;
            if (offs[mid] <= j) lo = mid; else hi = mid - 1;
        }
        v = wav[regions[2 * lo] + (j - offs[lo])];
    }
    operand[(int64_t)k * per + i] = v;
}

// handoff_norm_kernel's expression per speaker, over the columns below the speaker's frame count only
__global__ __launch_bounds__(256) void session_norm_kernel(SessionHandoff e, const float* __restrict__ mel, int64_t mel_ld, int n_mels,
                                                           float* __restrict__ out, int64_t out_ld) {
    const int k = blockIdx.z, m = blockIdx.y;
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= e.st[k].J || j >= out_ld) return;
    const int b = e.st[k].gmax;
    const float mx = __int_as_float(b >= 0 ? b : b ^ 0x7fffffff);
    const int64_t row = (int64_t)k * n_mels + m;
    out[row * out_ld + j] = (fmaxf(mel[row * mel_ld + j], mx - 8.0f) + 4.0f) * 0.25f;
}

// One row of one job of the window kernel below: dst[c] for c < wd is the normalised raw frame row[s0 + c] where c < n and `fill`
// behind.  Written as window_row writes a row: scalar stores up to dst's first 16-byte boundary, 16-byte stores from there, scalar
// stores behind the last whole one.  A 16-byte group wholly below n is read through window_load16 (a window starts at any frame,
// so the source has any alignment); the group that holds frame n - 1 and a source at the row's two ends are taken frame by frame.
template <typename T>
__device__ __forceinline__ void session_window_row(const float* __restrict__ row, int64_t row_len, int64_t s0, int64_t n, int64_t wd,
                                                   T* __restrict__ dst, float lo, float fill, int lane) {
    constexpr int V = WindowVec<T>::V;
    auto norm = [&](float raw) { return (fmaxf(raw, lo) + 4.0f) * 0.25f; };   // session_norm_kernel's expression
    auto one = [&](int64_t c) { return c < n ? norm(row[s0 + c]) : fill; };
    const int64_t to_boundary = (int64_t)(((16 - ((uintptr_t)dst & 15)) & 15) / sizeof(T));
    const int64_t head = to_boundary < wd ? to_boundary : wd;
    const int64_t nvec = (wd - head) / V, tail = head + nvec * V;
    for (int64_t c = lane; c < head; c += 64) WindowVec<T>::store(dst + c, one(c));
    for (int64_t c = tail + lane; c < wd; c += 64) WindowVec<T>::store(dst + c, one(c));
    for (int64_t g = lane; g < nvec; g += 64) {
        const int64_t c = head + g * V;
        float v[V];
        if (c + V <= n && window_load16<V>(row, s0 + c, row_len, v)) {
#pragma unroll
            for (int i = 0; i < V; ++i) v[i] = norm(v[i]);
        } else {
#pragma unroll
            for (int i = 0; i < V; ++i) v[i] = one(c + i);
        }
        WindowVec<T>::store16(dst + c, v);
    }
}

// The encoder windows and the whole log-mel of a queued session (kernels.hpp SessionWindows): a block has one job of one speaker,
// a wave one band of it.  The frame count and the maximum are the keep-scan's and the mel kernel's words in device memory; the
// grid covers the host's bounds, and what lies beyond the counts leaves at once.  No LDS, no barrier.
__global__ __launch_bounds__(256) void session_window_kernel(SessionWindows e) {
    const int k = blockIdx.z, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = blockIdx.y * SESSION_WINDOW_ROWS + wave;
    const int64_t job = blockIdx.x;
    const int64_t J = e.st[k].J < e.max_frames ? e.st[k].J : e.max_frames;
    const int b = e.st[k].gmax;
    const float mx = __int_as_float(b >= 0 ? b : b ^ 0x7fffffff);
    if (job == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        e.n_windows_out[k] = (int32_t)((J + e.stride - 1) / e.stride);
        e.window_max_out[k] = mx;
    }
    if (J <= 0 || m >= e.n_mels) return;
    const float lo = mx - 8.0f, fill = (fmaxf(-10.0f, lo) + 4.0f) * 0.25f;
    const float* __restrict__ row = e.mel + ((int64_t)k * e.n_mels + m) * e.mel_ld;
    int64_t s0, n, wd, at;   // the job's first frame, frames, columns, and its first element in the output
    if (job < e.n_win_jobs) {
        s0 = job * e.stride;
        n = J - s0 < e.width ? J - s0 : e.width;
        if (n < 1) return;
        wd = e.width;
        at = (((int64_t)k * e.cap_windows + job) * e.n_mels + m) * e.ld;
    } else {
        s0 = (job - e.n_win_jobs) * SESSION_WINDOW_CHUNK;
        wd = e.whole_ld - s0 < SESSION_WINDOW_CHUNK ? e.whole_ld - s0 : SESSION_WINDOW_CHUNK;
        n = J - s0 < wd ? J - s0 : wd;
        n = n < 0 ? 0 : n;
        at = ((int64_t)k * e.n_mels + m) * e.whole_ld + s0;
    }
    void* out = job < e.n_win_jobs ? e.win : e.whole;
    if (e.f16) session_window_row<__half>(row, e.mel_ld, s0, n, wd, (__half*)out + at, lo, fill, lane);
    else session_window_row<float>(row, e.mel_ld, s0, n, wd, (float*)out + at, lo, fill, lane);
}

void launch_session_keep_scan(const SessionHandoff& e, hipStream_t s) {
    hipLaunchKernelGGL(session_keep_scan_kernel, dim3(e.S), dim3(256), 0, s, e);
}
void launch_session_gather(const SessionHandoff& e, const float* wav, int64_t wav_ld, float* operand, int64_t rows, hipStream_t s) {
    const int64_t per = rows * 160;
    hipLaunchKernelGGL(session_gather_kernel, dim3((unsigned)((per + MEL_K + 255) / 256), e.S), dim3(256), 0, s, e, wav, wav_ld, operand, per);
}
void launch_session_norm(const SessionHandoff& e, const float* mel, int64_t mel_ld, int n_mels, float* out, int64_t out_ld, int64_t rows,
                         hipStream_t s) {
    if (rows <= 0) return;
    hipLaunchKernelGGL(session_norm_kernel, dim3((unsigned)((rows + 255) / 256), n_mels, e.S), dim3(256), 0, s, e, mel, mel_ld, n_mels, out, out_ld);
}
void launch_session_windows(const SessionWindows& e, hipStream_t s) {
    static_assert(SESSION_WINDOW_ROWS == 4 && SESSION_WINDOW_CHUNK % 8 == 0, "a wave per band; chunks of whole 16-byte groups");
    const int64_t jobs = e.n_win_jobs + e.n_whole_jobs;
    if (jobs < 1) return;
    hipLaunchKernelGGL(session_window_kernel, dim3((unsigned)jobs, (unsigned)((e.n_mels + SESSION_WINDOW_ROWS - 1) / SESSION_WINDOW_ROWS), e.S),
                       dim3(256), 0, s, e);
}

}  // namespace css
