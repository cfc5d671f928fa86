// The mel tile of the NeMo features, shared by the offline kernel (nemo.hip) and the streamed one (nemo_stream.hip) so that both
// round alike: ONE copy of re * re + im * im.
#pragma once
#include "kernels.hpp"

namespace css {

constexpr int NEMO_TILE_FRAMES = 32, NEMO_TILE_ROWS = 8;   // a mel tile: thread t has frame t % 32 and bands t / 32, t / 32 + 8, ...
static_assert(NEMO_NFFT == 512 && NEMO_BINS == 257, "the power tile below is [257][33] floats of static LDS");

// One tile of 32 frames of one speaker: spec [514][ld] (rows f: Re, 257 + f: Im; time fastest), the speaker's frames are the
// columns col0 .. of it -> raw[m * raw_ld + j] = logf(sum_f w[m][f] |X|^2 + 2^-24) for the frames j < nfr.  The ONE place of
// re * re + im * im (open to contraction: one copy of the expression, one rounding) for every path that makes these features.
using NemoTilePw = float[NEMO_BINS][NEMO_TILE_FRAMES + 1];
__device__ __forceinline__ void nemo_mel_tile(NemoTilePw& pw, const float* __restrict__ spec, int64_t ld, int64_t col0, int64_t j0, int64_t nfr,
                                              const float* __restrict__ w, int n_mels, float* __restrict__ raw, int64_t raw_ld) {
    static_assert(NEMO_TILE_FRAMES == 32 && NEMO_TILE_ROWS == 8, "256 threads: the low five bits are the frame");
    const int tj = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t j = j0 + tj;
    for (int f = ty; f < NEMO_BINS; f += NEMO_TILE_ROWS) {
        float p = 0.f;
        if (j < nfr) {
            const float re = spec[(int64_t)f * ld + col0 + j], im = spec[(int64_t)(NEMO_BINS + f) * ld + col0 + j];
            p = re * re + im * im;
        }
        pw[f][tj] = p;
    }
    __syncthreads();
    for (int m = ty; m < n_mels; m += NEMO_TILE_ROWS) {
        float acc = 0.f;
        const float* wm = w + (size_t)m * NEMO_BINS;
        for (int f = 0; f < NEMO_BINS; ++f) acc = fmaf(wm[f], pw[f][tj], acc);
        if (j < nfr) raw[(int64_t)m * raw_ld + j] = logf(acc + NEMO_LOG_GUARD);
    }
}

}  // namespace css
