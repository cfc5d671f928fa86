// Device hand-off of the separated streams to NeMo-family consumers (include/css_mi355_nemo_handoff.h; DESIGN.md 7 "N4 for NeMo
// hosts"): the features of NeMo's AudioToMelSpectrogramPreprocessor, whose arithmetic transformers publishes as
// ParakeetFeatureExtractor (models/parakeet/feature_extraction_parakeet.py) -- pre-emphasis over the concatenation of the kept
// ranges, 256 zeros on both sides, a symmetric 400-point Hann window centred in a 512-point transform at hop 160, power
// spectrum, slaney mel bank at 257 bins (80 or 128 bands), ln(x + 2^-24), and per band (x - mean) / (std + 1e-5) with the
// unbiased std over the stream's n // 160 valid frames.  The ranges, the counts and the run table are the session hand-off's
// keep-scan's (handoff.hip); the spectra are one exact float32 product (launch_gemm) over the frame operand the gather lays out.
#include <cmath>
#include <vector>

#include "kernels.hpp"
#include "nemo_tile.hpp"

namespace css {

// ---- host: tables ---------------------------------------------------------------------------------------------------
// analysis matrix [2 * 257][512]: rows f = cos, 257 + f = -sin of 2 pi f n / 512, times the window: zero on [0, 56) and
// [456, 512), the symmetric Hann 0.5 - 0.5 cos(2 pi i / 399) (as a float32 value, torch.hann_window(400, periodic=False)'s
// format) at n = 56 + i
void nemo_build_dft(float* m) {
    for (int f = 0; f < NEMO_BINS; ++f)
        for (int n = 0; n < NEMO_NFFT; ++n) {
            double c = 0.0, s = 0.0;
            if (n >= NEMO_WIN_OFF && n < NEMO_WIN_OFF + NEMO_WIN) {
                const double w = (double)(float)(0.5 - 0.5 * std::cos(2.0 * M_PI * (n - NEMO_WIN_OFF) / (NEMO_WIN - 1)));
                const double a = 2.0 * M_PI * (double)((int64_t)f * n % NEMO_NFFT) / NEMO_NFFT;
                c = std::cos(a) * w;
                s = -std::sin(a) * w;
            }
            m[(size_t)f * NEMO_NFFT + n] = (float)c;
            m[(size_t)(NEMO_BINS + f) * NEMO_NFFT + n] = (float)s;
        }
}

// ---- device ---------------------------------------------------------------------------------------------------------
// The frame operand of all speakers in one launch: operand floats [k per, (k + 1) per) are speaker k's padded signal -- 256
// zeros, the pre-emphasised concatenation y[c] = x[c] - p x[c - 1] (y[0] = x[0]; the product and the difference rounded apart,
// as torch computes them; p == 0: y = x), zeros behind it -- so that frame j is the 512 floats from 160 j; behind the last
// speaker's, 512 zeros (the product's last rows read them).  x[c] is the run table's: the last run r with offs[r] <= c holds it
// at wav[regs[r][0] + c - offs[r]]; across a seam x[c - 1] is the last sample of the run before.  Counts from device memory.
__global__ __launch_bounds__(256) void nemo_gather_kernel(SessionHandoff e, const float* __restrict__ wavs, int64_t wav_ld,
                                                          float* __restrict__ operand, int64_t per, float preemph) {
    const int k = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= per + (k == e.S - 1 ? NEMO_NFFT : 0)) return;
    const int64_t n_act = e.st[k].A;
    const int nr = e.n_ranges[k] < e.cap_ranges ? e.n_ranges[k] : e.cap_ranges;
    const int64_t* __restrict__ regions = e.regs + (int64_t)k * e.cap_ranges * 2;
    const int64_t* __restrict__ offs = e.offs + (int64_t)k * e.cap_ranges;
    const float* __restrict__ wav = wavs + (int64_t)k * wav_ld;
    const int64_t c = i - NEMO_NFFT / 2;
    float v = 0.f;
    if (c >= 0 && c < n_act && nr > 0) {
        auto run_of = [&](int64_t j) {                           // last run with offs[r] <= j
            int lo = 0, hi = nr - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (offs[mid] <= j) lo = mid; else hi = mid - 1;
            }
            return lo;
        };
        const int r = run_of(c);
        v = wav[regions[2 * r] + (c - offs[r])];
        if (preemph != 0.f && c > 0) {
            const int rp = c - 1 >= offs[r] ? r : run_of(c - 1);
            const float before = wav[regions[2 * rp] + (c - 1 - offs[rp])];
            v = css_add_rn(v, -css_mul_rn(preemph, before));
        }
    }
    operand[(int64_t)k * per + i] = v;
}

__global__ __launch_bounds__(256) void nemo_mel_kernel(NemoFeatures e, const float* __restrict__ spec, int64_t ld) {
    const int k = blockIdx.y;
    const int64_t J = e.st[k].J, nfr = J < e.rows - 4 ? J : e.rows - 4, j0 = (int64_t)blockIdx.x * NEMO_TILE_FRAMES;
    if (j0 >= nfr) return;
    __shared__ NemoTilePw pw;
    nemo_mel_tile(pw, spec, ld, (int64_t)k * e.rows, j0, nfr, e.w, e.n_mels, e.raw + (int64_t)k * e.n_mels * e.raw_ld, e.raw_ld);
}

// The sum of v over the block's 256 threads in a fixed order: a tree over LDS.  Every thread calls it; sh is free on return.
__device__ __forceinline__ double nemo_block_sum(double v, double (&sh)[256]) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
#pragma unroll
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) sh[tid] += sh[tid + o];
        __syncthreads();
    }
    const double total = sh[0];
    __syncthreads();
    return total;
}

// One block per (band, speaker): mean = sum / L and std = sqrt(sum (v - mean)^2 / (L - 1)) over the speaker's L valid frames of
// the raw row, both sums in float64 in a fixed order (thread t takes frames t, t + 256, ...; then the tree), each result rounded
// to float32 once.  L == 1: std = 0 (the definition's NaN, which NeMo replaces by 0 too).  L == 0: nothing is written.  The
// values depend on the row and on L alone: not on the grid, the speaker's place or the session's place in a queue group.
__global__ __launch_bounds__(256) void nemo_stats_kernel(NemoFeatures e) {
    const int m = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
    const int64_t J = e.st[k].J, L = J < e.rows - 4 ? J : e.rows - 4;
    if (L <= 0) return;
    __shared__ double sh[256];
    const float* __restrict__ row = e.raw + ((int64_t)k * e.n_mels + m) * e.raw_ld;
    double s = 0.0;
    for (int64_t j = tid; j < L; j += 256) s += (double)row[j];
    const double mean = nemo_block_sum(s, sh) / (double)L;
    double q = 0.0;
    for (int64_t j = tid; j < L; j += 256) {
        const double d = (double)row[j] - mean;
        q += d * d;
    }
    const double ss = nemo_block_sum(q, sh);
    if (tid == 0) {
        const float mean_f = (float)mean, std_f = L > 1 ? (float)sqrt(ss / (double)(L - 1)) : 0.f;
        const int64_t at = (int64_t)k * e.n_mels + m;
        e.mean[at] = mean_f;
        e.stdv[at] = std_f;
        if (e.mean_out) e.mean_out[at] = mean_f;
        if (e.std_out) e.std_out[at] = std_f;
    }
}

// out[(k n_mels + m) out_ld + j] for the frames j below the speaker's count only: (raw - mean) / (std + 1e-5) in float32, each
// step rounded once, or (normalize == 0) the raw value
__global__ __launch_bounds__(256) void nemo_norm_kernel(NemoFeatures e) {
    const int k = blockIdx.z, m = blockIdx.y;
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= e.st[k].J || j >= e.rows - 4 || j >= e.out_ld) return;
    const int64_t row = (int64_t)k * e.n_mels + m;
    float v = e.raw[row * e.raw_ld + j];
    if (e.normalize) v = css_div_rn(css_add_rn(v, -e.mean[row]), css_add_rn(e.stdv[row], NEMO_STD_EPS));
    e.out[row * e.out_ld + j] = v;
}

void launch_nemo_gather(const SessionHandoff& e, const float* wav, int64_t wav_ld, float* operand, int64_t rows, float preemph, hipStream_t s) {
    const int64_t per = rows * NEMO_HOP;
    hipLaunchKernelGGL(nemo_gather_kernel, dim3((unsigned)((per + NEMO_NFFT + 255) / 256), e.S), dim3(256), 0, s, e, wav, wav_ld, operand, per,
                       preemph);
}
void launch_nemo_mel(const NemoFeatures& e, const float* spec, int64_t ld, hipStream_t s) {
    if (e.rows - 4 <= 0) return;
    hipLaunchKernelGGL(nemo_mel_kernel, dim3((unsigned)((e.rows - 4 + NEMO_TILE_FRAMES - 1) / NEMO_TILE_FRAMES), e.S), dim3(256), 0, s, e, spec, ld);
}
void launch_nemo_stats(const NemoFeatures& e, hipStream_t s) {
    hipLaunchKernelGGL(nemo_stats_kernel, dim3(e.n_mels, e.S), dim3(256), 0, s, e);
}
void launch_nemo_norm(const NemoFeatures& e, hipStream_t s) {
    if (e.rows - 4 <= 0 || !e.out) return;
    hipLaunchKernelGGL(nemo_norm_kernel, dim3((unsigned)((e.rows - 4 + 255) / 256), e.n_mels, e.S), dim3(256), 0, s, e);
}

}  // namespace css
