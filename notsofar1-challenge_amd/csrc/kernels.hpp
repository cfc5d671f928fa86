// Internal launch interface of the gfx950 kernels (one declaration per kernel family).
// Everything here is device-pointer based and asynchronous on the given stream.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace css {

// ------------------------------------------------------------------------------------------------
// gemm.hip -- fp32 MFMA GEMM  C[m][n] = epilogue( sum_k A[m*lda + k] * B[n*ldb + k] )
// Both operands are K-contiguous ("NT"): A is an activation / DFT matrix, B a weight [out][in] or a
// strided view of frames.  K must be a multiple of 32; M, N arbitrary.
// ------------------------------------------------------------------------------------------------
enum GemmAct : int { ACT_NONE = 0, ACT_RELU = 1, ACT_SIGMOID = 2 };

struct GemmArgs {
    const float* A; int64_t lda; int64_t strideA;   // batch stride (0 = shared)
    const float* B; int64_t ldb; int64_t strideB;
    float* C; int64_t ldc; int64_t strideC;
    int M, N, K, batch;
    const float* bias;      // nullptr or [N] (bias_along_m == 0) / [M] (bias_along_m == 1)
    int bias_along_m;
    int act;                // GemmAct
    const float* residual;  // nullptr or [M][ldr]: C = residual + alpha * (acc + bias)
    int64_t ldr;
    float alpha;            // only with residual
    // split-f16 operands (split_f16.hpp): A and B are split matrices addressed as float matrices (lda / ldb = their
    // padded K); three f16 MFMAs per product, float32 accumulation.  split_out = n > 0: columns [0, n) of C are
    // written in the split format for the next consumer (n % 32 == 0), the remaining columns as float32.
    int split_in;
    int split_out;
    // b_tiled (with split_in): B is a weight matrix in the tile-major split layout of gemm_split_wd.hip
    // (launch_split_convert_tiled); batch must be 1 and N % 32 == 0.
    int b_tiled;
    // b_frag32 (exact float32, gemm_f32.hip): B is a weight in float32 FRAGMENT order (launch_f32_fragments); batch 1, N % 32 == 0
    int b_frag32;
    const float* B_rows;   // with b_frag32: the same weight row-major (ld = ldb), for the launches gemm_f32.hip does not take
                           // (an operand of 2 GiB and more, a misaligned A): launch_gemm then runs gemm.hip's kernel on it
    // hint: other kernels run beside this launch (two-lane mask estimator): prefer 4-wave 64-row tiles, two of which
    // -- from different launches -- share a CU, over one 8-wave 128-row tile per CU
    int concurrent;
    int nt_store;   // epilogue stores bypass the caches (nontemporal)
    // weights-direct kernel only: columns n < 2 * frag_D (the q and k projections of the attention, D = heads * 64) leave
    // in the attention kernel's operand order instead of row-major C (encoder.hip qk fragment layout); rows are tokens
    // of segments of frag_T frames, frag_invT = 1.0f / frag_T
    float* frag_out;
    int frag_D, frag_T, frag_heads;
    float frag_invT;
    int tile_rows;         // weights-direct kernel: 0 = choose, else 32 / 64 / 96 / 128 (8 waves) / 4 (128 rows, 4 waves) / 65 (64 rows, 64-bit global loads)
    int narrow_epilogue;   // tools: keep the 4-byte-per-lane epilogue of the weights-direct kernel (A/B timing)
    // split kernels: *range_flag |= 1 when a finished accumulator is not finite -- an operand left the split-f16 range
    // (split_f16.hpp: nothing is clamped); checked here, in the consumer, because a ReLU downstream would launder a NaN
    unsigned int* range_flag;
    int layout;            // LDS-staged kernels (gemm.hip, gemm_split.hip): 0 = choose, else 8 / 4 (128-row tiles, 8 / 4 waves) / 64;
                           // exact float32 only: 1 = gemm_f32.hip with its balanced plan (what 0 chooses), 11 .. 14 = gemm_f32.hip with
                           // every tile 32 / 64 / 96 / 128 rows, 2 = gemm.hip's kernel with its own choice among 8 / 4 / 64
    // LDS-staged kernels: an XCD's consecutive tiles walk the ROW tiles of one column panel (they share the B panel) instead
    // of the column tiles of one row panel: for launches whose B operand is the large one.  Same tiles, same bits.
    int m_fastest;
    // weights-direct kernel: the result leaves transposed, C^T[n][m] at C + n * ldc + m (column bias and activation only;
    // no residual, no split output)
    int c_transposed;
};
void launch_gemm(const GemmArgs& g, hipStream_t s);        // dispatches on g.split_in
// gemm_f32.hip: the exact float32 product on four independent 4-wave blocks per CU with balanced tile heights (same bits as
// gemm.hip's kernel); forced_tm = 1..4: every tile 32 * forced_tm rows, 0: the balanced plan.  false: not launched (an
// operand beyond the 32-bit buffer offsets, K % 16): the caller takes gemm.hip's kernel
bool launch_gemm_f32(const GemmArgs& g, hipStream_t s, int forced_tm);
// float32 W [N][K] (row stride ld_src; N % 32 == 0, K % 8 == 0) -> the fragment order GemmArgs::b_frag32 names, N * K floats
void launch_f32_fragments(const float* src, int64_t ld_src, float* dst, int N, int K, hipStream_t s);
void launch_gemm_split(const GemmArgs& g, hipStream_t s);  // gemm_split.hip
void launch_gemm_split_wd(const GemmArgs& g, hipStream_t s);  // gemm_split_wd.hip (g.b_tiled)
// float32 W [N][K] (row stride ld_src, K % 32 == 0) -> tile-major split-f16 weights, (N rounded up to 32) * K floats
void launch_split_convert_tiled(const float* src, int64_t ld_src, float* dst, int N, int K, hipStream_t s);
// float32 [rows][K] (row stride ld_src) -> split-f16 [rows][Kp] (Kp % 32 == 0, zero padded past K)
void launch_split_convert(const float* src, int64_t ld_src, float* dst, int64_t rows, int K, int Kp, hipStream_t s);

// ------------------------------------------------------------------------------------------------
// encoder.hip -- the non-GEMM pieces of the Conformer
// ------------------------------------------------------------------------------------------------
// y = LN(x) * w + b over rows of length D (D % 256 == 0, D <= 1024); optional ReLU.  y (float32) and y_split
// (the same rows as a split-f16 GEMM operand, split_f16.hpp) are each optional.
void launch_layernorm(const float* x, float* y, float* y_split, const float* w, const float* b, int rows, int D,
                      int relu, hipStream_t s);
// y = LN(x; w1, b1) (float32, may alias x), then z / z_split = LN(y; w2, b2) (each optional), one pass over the rows
void launch_layernorm2(const float* x, float* y, const float* w1, const float* b1, float* z, float* z_split,
                       const float* w2, const float* b2, int rows, int D, hipStream_t s);
// conv-module front half: u = LN(x); z = (pw[0]*u + pw[1]) * sigmoid(pw[2]*u + pw[3])
void launch_ln_glu(const float* x, float* z, const float* w, const float* b, const float* pw, int rows, int D,
                   hipStream_t s);
// conv-module back half: depthwise conv over time inside each segment (zero padded), eval-BatchNorm,
// ReLU, scalar pointwise conv, residual:  h += pw[4] * relu((conv(z) + dw_b) * alpha + beta) + pw[5]
void launch_dwconv(const float* z, float* h, const float* dw_wt, const float* dw_b, const float* bn_alpha,
                   const float* bn_beta, const float* pw, int nseg, int T, int D, int taps, hipStream_t s);
// the whole conv module in one kernel: x_out = x_in + conv_module(x_in); x_out must not alias x_in.  Returns false when
// (D, taps) is not covered and nothing was launched (use launch_ln_glu + launch_dwconv).  z / z_split (either may be
// null) = LayerNorm(x_out; ln2_w, ln2_b) as float32 / split-f16 rows: the LayerNorm of the module that follows.
bool launch_conv_module(const float* x_in, float* x_out, const float* ln_w, const float* ln_b, const float* pw,
                        const float* dw_wt, const float* dw_b, const float* bn_alpha, const float* bn_beta,
                        const float* ln2_w, const float* ln2_b, float* z, float* z_split, int nseg, int T,
                        int D, int taps, hipStream_t s);
// relative-position multi-head attention: qkv [tokens][3D] -> ctx [tokens][D] (float32, or split-f16 rows).
// qk_split: the q and k columns of qkv and the position rows are split-f16 (scores on the f16 matrix cores with
// float32-grade accuracy); v is float32 either way.  pe_frag: the relative-position table rearranged for this T by
// launch_pe_fragments from the row-major table of the same arithmetic (float32 or split-f16 rows of d_k = 64):
// pe_fragment_tiles(T) tiles of 32 rows x 64, 2048 floats each.
inline int pe_fragment_tiles(int T) { return 2 * ((T + 31) / 32); }
void launch_pe_fragments(const float* pe, float* frag, int T, int maxlen, int split, hipStream_t s);
// qk_frag (split mode only, may be null): q and k in operand order, written by the QKV GEMM (GemmArgs::frag_out):
// float4 index ((((seg * H + head) * ceil(T / 32) + tile) * 2 + which) * 8 + chunk) * 64 + lane, which = 0 q / 1 k;
// qk_fragment_floats(nseg, T, H) floats.  The q and k columns of qkv are then not read.
inline int64_t qk_fragment_floats(int64_t nseg, int T, int H) { return nseg * H * ((T + 31) / 32) * 2 * 8 * 64 * 4; }
void launch_relpos_attention(const float* qkv, const float* qk_frag, const float* pe_frag, float* ctx, int nseg, int T, int D,
                             int H, int maxlen, int qk_split, int split_out, hipStream_t s);
// segments beyond 512 frames (encoder.hip relpos_attn_long_kernel): qkv = float32 rows [token][3 D], pe = the float32
// table [2 maxlen][64]; false: the head width is not 64 or one query's rows do not fit the LDS
bool launch_relpos_attention_long(const float* qkv, const float* pe, float* ctx, int nseg, int T, int D, int H, int maxlen,
                                  int split_out, hipStream_t s);

// ------------------------------------------------------------------------------------------------
// stft.hip -- the analysis transform as an LDS-staged FFT (frame_len 512, hop 256, 257 bins)
// ------------------------------------------------------------------------------------------------
size_t stft_table_floats();
void stft_build_tables(float* host, int window = 0);   // window (0: hann, 1: sqrt_hann / 16) | radix-4 twiddles | real-spectrum twiddles
// frames 0 .. nf-1 of C channels (channel c's first sample at x + c * x_stride, frame t at sample 256 t) -> planes
// out[(c * 514 + r) * row_ld + t], r = f (Re) / 257 + f (Im).  false: the kernel's LDS could not be reserved.
// phase != nullptr: also the PHASE planes phase[(c * 257 + f) * row_ld + t] = css_phase_of(Re, Im) -- the angle the IPD
// features are made of (feature.py:214-221), formed once per frame here instead of once per segment and microphone pair in
// the feature kernel (a frame lies in two segments, microphone 0 in six pairs: 18 atan2 per feature element became 6 + 7/2).
// PRECONDITION: x_stride is even and x 8-byte aligned (samples are read as float2); t_lo >= 0.  The spectrum leaves as float4
// stores when row_ld % 4 == 0 and `out` is 16-byte aligned -- the decision looks at `out` ALONE, and the phase planes leave
// through the same kind of store: `phase` must have the alignment of `out` modulo 16 bytes (every caller gives both the same).
bool launch_stft_fft(const float* x, int64_t x_stride, int C, int64_t t_lo, int64_t t_hi, const float* tables, float* out,
                     int64_t row_ld, hipStream_t s, float* phase = nullptr);

// XCD-aware work order: workgroup L of a 1-D grid runs on XCD L % 8 (round robin), and each XCD has its own L2.  Work items
// that read the same operands should therefore be neighbours IN ONE XCD: every XCD takes a contiguous range of the n items,
// consecutive workgroups of an XCD consecutive items of its range.  (A bijection of [0, n) for every n.)
__device__ __forceinline__ int css_xcd_item(int L, int n) {
    const int q = n >> 3, rem = n & 7, xcd = L & 7;
    return xcd * q + (xcd < rem ? xcd : rem) + (L >> 3);
}

// Phase of a spectrum value as the reference reaches it.  An exactly real negative bin (DC / Nyquist have Im == +0 by
// construction of the transform) goes through polar() -> angle() in the reference (conformer_wrapper.py:124,94), which
// maps it to the float32 value just inside -pi; the side of the atan2 branch cut of the IPD feature depends on that
// (DESIGN.md "Numerical hazards").  CSS_PHASE_NEG_REAL is that value.
#define CSS_PHASE_NEG_REAL (-3.14159250259399414f) /* 0xC0490FDA */
__device__ __forceinline__ float css_phase_of(float re, float im) {
    return (im == 0.f && re < 0.f) ? CSS_PHASE_NEG_REAL : atan2f(im, re);
}

// float32 product, sum and quotient that stay ONE rounding each, whatever follows them.  __fmul_rn / __fadd_rn / __fdiv_rn are a
// plain * + / in this toolchain (__clang_hip_math.h without OCML_BASIC_ROUNDED_OPERATIONS) and carry the contraction of the
// code around them: `__fadd_rn(v, __fmul_rn(w, m))` compiled to one FMA in the overlap-add kernels, whose sums then were not the
// reference's `zeros += w * x` from the second contributor on.  An operation compiled with contraction off
// cannot become half of an FMA.
__device__ __forceinline__ float css_mul_rn(float x, float y) {
#pragma clang fp contract(off)
    return x * y;
}
__device__ __forceinline__ float css_add_rn(float x, float y) {
#pragma clang fp contract(off)
    return x + y;
}
__device__ __forceinline__ float css_div_rn(float x, float y) {
#pragma clang fp contract(off)
    return x / y;
}

// ------------------------------------------------------------------------------------------------
// frontend.hip -- PCM layout, features, inverse-transform overlap-add
// ------------------------------------------------------------------------------------------------
// samples [i_lo, i_hi) of every channel: pcm [n][C] -> pcm_cm [C][n_pad] (zeros past n)
// (split_out: channel rows as split-f16 GEMM operands, n_pad % 32 == 0)
void launch_deinterleave(const float* pcm, float* pcm_cm, int64_t n, int C, int64_t n_pad, int64_t i_lo, int64_t i_hi,
                         int split_out, hipStream_t s);
// *peak = max(*peak, max |x|) as float bits (int16 samples scaled by 2^-15): the recording's level (split_f16.hpp level_gain)
void launch_pcm_peak_f32(const float* x, int64_t count, unsigned int* peak, hipStream_t s);
void launch_pcm_peak_i16(const int16_t* x, int64_t count, unsigned int* peak, hipStream_t s);
// wav edges on the device: C mono PCM16 planes [C][n] -> sample-major float32 [n][C]; and peak-normalised PCM16
// encoding of the S output streams (peak_bits: S words of scratch, holds max|x| as float bits afterwards)
void launch_pcm16_to_float(const int16_t* planes, float* pcm, int64_t n, int C, hipStream_t s);
void launch_pcm16_to_channel_major(const int16_t* planes, float* pcm_cm, int64_t n, int C, int64_t n_pad, int64_t i_lo,
                                   int64_t i_hi, hipStream_t s);
void launch_encode_pcm16(const float* wav, int S, int64_t n, unsigned int* peak_bits, int16_t* out, int64_t out_ld,
                         hipStream_t s);
// the second of its two steps alone: rows wav [S][wav_ld] with their peaks already in peak_bits (the session output kernel's)
void launch_encode_pcm16_with_peaks(const float* wav, int64_t wav_ld, int S, int64_t n, const unsigned int* peak_bits, int16_t* out,
                                    int64_t out_ld, hipStream_t s);
// features for segments [seg_lo, seg_lo + nseg): X planes -> feat [nseg*T][Kp] (bias/scale folded); float32 rows
// or split-f16 rows (split_f16.hpp; the padding columns are never written and must be zero)
// Segments beyond 512 frames (8 s) take kernels written for any length (features_long_kernel, relpos_attn_long_kernel,
// scm_long_kernel).  CSS_FORCE_LONG_PATH=1 in the environment sends EVERY segment length through them: the tests hold
// them to the fixtures of the fast kernels that way.
bool css_force_long_path();

struct FeatOpts {   // CssFeatureCfg in kernel-argument form
    int log_mag, mvn, ipd_norm, ipd_version, ipd_cos, num_pairs;
    unsigned char pair_l[16], pair_r[16];
};
// PH: the phase planes launch_stft_fft wrote beside X (same T_ld), or nullptr: the kernel forms the phases itself (same
// function on the same values: the features are the same bits either way)
void launch_features(const float* X, int64_t T_ld, int64_t stft_frames, int C, int F, float* feat, int Kp,
                     const float* in_bias, const float* in_scale, int64_t seg_lo, int nseg, int T, int hop,
                     int split_out, const FeatOpts& opts, hipStream_t s, const float* PH = nullptr);
// out[b][hop*(q - out_q0) + r] = G[b][q][r] + G[b][q-1][hop + r] for output blocks q in [q_lo, q_hi), taking
// only frames in [f_lo, f_hi) (frame_len == 2*hop); out has row stride out_ld
// level (may be null): the samples are multiplied by 1 / level_gain(level) (undoes the scaling of the split spectra rows)
void launch_wave_ola(const float* G, float* out, int B, int64_t T_frames, int hop, int frame_len, int64_t q_lo, int64_t q_hi,
                     int64_t f_lo, int64_t f_hi, int64_t out_ld, int64_t out_q0, const unsigned int* level, hipStream_t s);
// gathered [world][S][ld] waveform shards (rank r: output blocks t_lo[r] .. t_hi[r]) -> out [S][out_ld] (world <= 64)
void launch_join_shards(const float* gathered, int64_t ld, const int64_t* t_lo, const int64_t* t_hi, int world, int S, int hop,
                        int64_t n_out, float* out, int64_t out_ld, hipStream_t s);
// [B][2F][T] planes -> [B][T][KIp] rows for the inverse GEMM
void launch_planes_to_rows(const float* planes, float* rows, int B, int F2, int64_t T, int KIp, hipStream_t s);

// ------------------------------------------------------------------------------------------------
// handoff.hip -- active regions of a separated stream -> Whisper log-mel features on the device
// ------------------------------------------------------------------------------------------------
void handoff_build_dft(float* m);                 // [402][416]
void handoff_build_mel(float* w, int n_mels, int bins = 201);   // [n_mels][bins]: the slaney bank over bins - 1 equal steps up to 8 kHz
void launch_handoff_gather(const float* wav, const int64_t* regions, const int64_t* offs, int nr, int64_t n_act, float* out,
                           int64_t total, hipStream_t s);
void launch_handoff_mel(const float* spec, int64_t ld, int64_t nfr, const float* w, int n_mels, float* mel, int* gmax, hipStream_t s);

// The hand-off of STREAMED sessions (api_stream_handoff.hip): per round of a push, the samples whose membership in the concatenation
// became decided are appended, the Whisper frames they complete are laid out as rows of ONE frame operand for all streams and
// speakers of the round (one DFT product), and their raw log-mel values (no max - 8 clamp: that needs a maximum over a span
// the consumer chooses) are written with the running maximum.  Table launches: blockIdx.z = entry (a stream), blockIdx.y =
// speaker.  What is carried between rounds lives in per-stream buffers of two generations (read one, write the other).
constexpr int HANDOFF_TAIL_LD = 512;          // floats per speaker of the concatenation tail (< 400 are used)
constexpr int HANDOFF_GMAX_NONE = (int)0x807fffff;   // -inf in the order-preserving integer form of the running maximum
struct HandoffState { int64_t A; int64_t J; int gmax; int pad_; };   // per (stream, speaker): samples appended, frames emitted, max
struct HandoffAppend {
    const uint8_t* gate; int64_t gate_ld, gate_mask;   // the gate ring (StreamStitchArgs::gate_out)
    const float* out; int64_t out_ld, out_base;         // the round's output samples [S][out_ld]; column 0 is sample out_base
    const float* carry_in; float* carry_out; int64_t carry_ld;   // undecided samples [D0, out_base) -> [D1, the round's end)
    const float* tail_in; float* tail_out;              // [S][HANDOFF_TAIL_LD]: concatenated samples not yet behind a frame
    const HandoffState* st;                             // [S]: the counts and the maximum before the round
    HandoffState* st_out;                               // [S]: after it.  A push: st itself; a preview: scratch rows (gmax is copied across)
    int64_t t_g0, t_g1, D0, D1;                         // gated-final frames and decided samples before / after the round
    int pad, drop, closing, S;
    int64_t row0, rows;                                 // speaker k owns operand rows [row0 + k rows, row0 + (k + 1) rows)
    uint8_t* act_out; int32_t* n_new;                   // out: gate bytes [S][t_g1 - t_g0], frames completed [S]
};
struct HandoffMel {
    int64_t row0, rows;                                 // as above: the entry's columns of the spectra
    const int32_t* n_new; HandoffState* st;             // [S] each (st: the append entry's st_out)
    const float* w; int n_mels;                         // the entry's filterbank [n_mels][201]
    float* mel; int64_t mel_ld;                         // out [S][n_mels][mel_ld]
    // the stream's frame history (css_stream_window_open), null without one and in a preview's round: frame j of speaker k's
    // concatenation at ring[(k n_mels + m) hist + j mod hist], its maximum over the bands at fmax[k hist + j mod hist]
    float* ring; float* fmax; int64_t hist;
    // a preview's round whose stream is asked for windows up to the present (css_stream_present_windows), null otherwise: the
    // maximum over the bands of provisional frame j of speaker k at pvmax[k rows + j]
    float* pvmax;
};
constexpr int HANDOFF_MULTI_MAX = 16;
void launch_handoff_append_multi(const HandoffAppend* e, int n, float* operand, hipStream_t s);
void launch_handoff_mel_multi(const HandoffMel* e, int n, int S, const float* spec, int64_t ld, hipStream_t s);

// The hand-off of QUEUED sessions (include/css_mi355_session_handoff.h, api_session_handoff.hip): all S streams of a finished
// session, with no host decision between the steps.  The keep-scan kernel turns the gate bytes into the run table and the counts
// in device memory (512 / 256 frames: block q of 256 samples is kept iff a frame of [q - pad - 1, q + pad] is active); the gather
// and the normalisation read their counts from there and are launched over the host-known bounds; the product and the mel
// kernel in between are the streams' (launch_gemm, launch_handoff_mel_multi with n_new = the frame counts).
constexpr int SESSION_SCAN_CHUNK = 1024;      // gate frames / sample blocks per step of the keep-scan's prefix sums
struct SessionHandoff {
    const uint8_t* gate; int64_t TL;                    // the gate bytes [S][TL] (act_final)
    int32_t pad, drop, S, cap_ranges;
    int32_t* psum;                                      // scratch [S][TL + 1]: active frames below t
    int64_t* regs; int64_t* offs;                       // out: run table [S][cap_ranges][2] sample ranges, [S][cap_ranges] samples before
    HandoffState* st;                                   // out [S]: A = kept samples, J = frames, gmax = the reset maximum
    int32_t* n_new; int32_t* n_ranges;                  // out [S] each: frames again (HandoffMel::n_new), runs
    int64_t* ranges_out; int64_t* n_frames_out; int32_t* n_ranges_out;   // the caller's [S][cap_ranges][2], [S], [S] (device addresses)
};
void launch_session_keep_scan(const SessionHandoff& e, hipStream_t s);          // one block per speaker
// operand rows [k rows, (k + 1) rows) of 160 floats: speaker k's kept samples, reflect-padded; zeros up to the operand's end + 416
void launch_session_gather(const SessionHandoff& e, const float* wav, int64_t wav_ld, float* operand, int64_t rows, hipStream_t s);
// out[(k n_mels + m) out_ld + j] = Whisper's normalisation of mel[(k n_mels + m) mel_ld + j], j < the speaker's frame count only
void launch_session_norm(const SessionHandoff& e, const float* mel, int64_t mel_ld, int n_mels, float* out, int64_t out_ld, int64_t rows,
                         hipStream_t s);

// Encoder windows of a QUEUED session (include/css_mi355_session_window.h, api_session_window.hip): one launch behind the mel
// kernel, reading the raw rows mel [S][n_mels][mel_ld] and the counts st[k].J / st[k].gmax from device memory.  A block has one
// JOB of one speaker and SESSION_WINDOW_ROWS bands (one wave per band).  Jobs 0 .. n_win_jobs - 1 are windows: window w holds the
// frames from w stride, n = min(width, J - w stride) of them, and leaves at once when n < 1.  The jobs behind them are chunks of
// SESSION_WINDOW_CHUNK columns of the whole log-mel row (`whole`, every column below whole_ld: the frames, then the fill); they
// leave when J == 0.  Session normalisation: clamp at gmax - 8, (x + 4) / 4, fill = what -10 takes under it.
constexpr int SESSION_WINDOW_ROWS = 4;
constexpr int SESSION_WINDOW_CHUNK = 4096;              // (a multiple of the 16-byte store: chunks keep the row's alignment)
struct SessionWindows {
    const HandoffState* st; const float* mel; int64_t mel_ld, max_frames;   // J is taken as at most max_frames (the host's bound)
    int32_t S, n_mels, width, stride, f16;
    int64_t n_win_jobs, n_whole_jobs;                   // the grid's jobs: ceil(max_frames / stride) or 0; ceil(whole_ld / CHUNK) or 0
    void* win; int64_t ld, cap_windows;                 // [S][cap_windows][n_mels][ld] of the dtype, or null
    void* whole; int64_t whole_ld;                      // [S][n_mels][whole_ld] of the dtype, or null
    int32_t* n_windows_out; float* window_max_out;      // the caller's [S] each (device addresses)
};
void launch_session_windows(const SessionWindows& e, hipStream_t s);

// Whisper encoder windows (include/css_mi355_window.h, css_mi355_present_window.h): at most n_frames frames of one speaker counted
// back from the end of a preview's provisional frames -- the ring's frames [a, J), then the last provisional ones -- clamped at their
// own maximum - 8, (x + 4) / 4, padded to `width` columns with the value a frame of digital zeros takes, as float32 or float16 into
// the caller's device memory.  How many frames the preview made (P = *n_new, at most pv_ld) is known on the device only, so the
// kernel resolves the span itself: E = J + P, a = max(E - n_frames, max(J - hist, 0)), used = E - a, of which min(used, P) are
// provisional; it leaves them in *res.  A table launch: blockIdx.z = window.
// n_new == nullptr: no provisional frames (P = 0; pv and pvmax are never read, pv_ld is 0), a window out of the history alone:
// frames [first, first + n_frames) with J := first + n_frames.  The host has checked max(J' - hist, 0) <= first and J <= J' for the
// speaker's count J', so n_frames <= hist and J - hist <= first: a = max(J - n_frames, max(J - hist, 0)) = first, used = n_frames.
struct WindowOut { int64_t first_frame; int32_t n_used, n_provisional; float window_max; int32_t pad_; };
struct WindowItem {
    const float* ring; const float* fmax;               // the speaker's rows of the history: [n_mels][hist], [hist]
    const float* pv; const float* pvmax;                // the speaker's provisional frames [n_mels][pv_ld] and their maxima [pv_ld]
    const int32_t* n_new;                               // the speaker's count of the preview's round (HandoffAppend::n_new + k)
    void* out; WindowOut* res;                          // out [n_mels][ld] of the dtype; the span (window_max only where used > 0)
    int64_t hist, ld, J, pv_ld;                         // J: frames the pushes returned for the speaker
    int32_t n_frames, width, n_mels, f16;
};
constexpr int WINDOW_MULTI_MAX = 32;                    // (CSS_WINDOW_TABLE of the header)
constexpr int WINDOW_ROWS = 8;                          // mel bands per block
void launch_stream_windows(const WindowItem* e, int n, hipStream_t s);   // one launch; n <= WINDOW_MULTI_MAX

// ------------------------------------------------------------------------------------------------
// nemo.hip -- the kept ranges of the separated streams -> NeMo's log-mel features on the device (DESIGN.md 7 "N4 for NeMo hosts")
// ------------------------------------------------------------------------------------------------
// Behind the keep-scan of a queued session (launch_session_keep_scan: run table, offsets, st[k].A kept samples, st[k].J = A / 160
// frames), with no host decision between the steps: gather (all speakers, pre-emphasis across the seams, zero pads), the product
// (launch_gemm on the [514][512] analysis matrix, exact float32), mel (raw ln rows), statistics, normalisation.  A speaker owns
// `rows` operand rows of 160 floats -- frame j is the 512 floats from row j -- and rows - 4 is the bound of its frame count.
constexpr int NEMO_NFFT = 512, NEMO_BINS = 257, NEMO_WIN = 400, NEMO_WIN_OFF = 56, NEMO_HOP = 160;
constexpr float NEMO_LOG_GUARD = 5.9604644775390625e-8f;   // 2^-24
constexpr float NEMO_STD_EPS = 1e-5f;
void nemo_build_dft(float* m);                    // [514][512], window folded in
struct NemoFeatures {
    const HandoffState* st; int32_t S, n_mels, normalize, pad_;
    int64_t rows;                                       // operand rows per speaker; the frame count is taken as at most rows - 4
    const float* w;                                     // the bank [n_mels][257]
    float* raw; int64_t raw_ld;                         // [S][n_mels][raw_ld]: ln(mel + 2^-24), frames below the count
    float* mean; float* stdv;                           // [S][n_mels] each, written where the count is at least 1
    float* mean_out; float* std_out;                    // the caller's [S][n_mels] (device addresses), or null
    float* out; int64_t out_ld;                         // the caller's [S][n_mels][out_ld] (device address): frames below the count only
};
// operand rows [k rows, (k + 1) rows) of 160 floats: 256 zeros, speaker k's pre-emphasised kept samples, zeros; zeros up to the operand's end + 512
void launch_nemo_gather(const SessionHandoff& e, const float* wav, int64_t wav_ld, float* operand, int64_t rows, float preemph, hipStream_t s);
void launch_nemo_mel(const NemoFeatures& e, const float* spec, int64_t ld, hipStream_t s);   // spec [514][ld], speaker k's frames at columns k rows ..
void launch_nemo_stats(const NemoFeatures& e, hipStream_t s);                                // one block per (band, speaker)
void launch_nemo_norm(const NemoFeatures& e, hipStream_t s);

// The NeMo hand-off of STREAMED sessions (include/css_mi355_stream_nemo.h, api_stream_handoff.hip; DESIGN.md 7b "The NeMo hand-off
// of a stream"): the Whisper stream hand-off's round -- append, ONE product, mel -- with NeMo's operand.  The append entry is the
// Whisper one (same gate ring, decided samples, carry, counts, gate bytes) with three differences: the samples are pre-emphasised
// while they are compacted (the predecessor of a sample is the kept sample before it, across seams and across rounds: x_last is
// carried per speaker), the tail is y[160 J - 256, A) at its own leading dimension, and what lies outside [0, A) is zero instead
// of a reflection.  Operand column x of a speaker's rows is y[160 J0 - 256 + x]; frame j is complete once A >= 160 j + 256, so
// every emitted row is the offline gather's row (nemo_gather_kernel), float for float.  a.st_out[k].gmax is left alone.
constexpr int NEMO_TAIL_LD = 512;                       // floats per speaker of the tail (A - (160 J - 256) < 512 are used)
struct NemoAppend {
    HandoffAppend a;                                    // tail_in / tail_out: [S][NEMO_TAIL_LD]
    const float* xlast_in; float* xlast_out;            // [S]: the last kept sample x[A - 1] before / after the round (unread while A == 0)
    float preemph; int32_t pad_;
};
struct NemoMel {
    int64_t row0, rows;                                 // the entry's columns of the spectra (NemoAppend::a.row0, rows)
    const int32_t* n_new;                               // [S]: frames the append completed
    const float* w;                                     // the bank [n_mels][257]
    float* mel; int64_t mel_ld;                         // out [S][n_mels][mel_ld]: ln(mel + 2^-24)
    int32_t n_mels, pad_;
    // the frame history (include/css_mi355_nemo_chunk.h), null for an entry without one: [S][n_mels][hist], frame j of speaker k's
    // concatenation in slot j mod hist.  st[k].J is k's frame count AFTER the round (the append kernel's st_out), so the round's
    // frame j is frame J - n_new + j; only the round's last `hist` frames are written: frames j and j + hist share a slot.
    float* ring; int64_t hist; const HandoffState* st;
};
void launch_nemo_append_multi(const NemoAppend* e, int n, float* operand, hipStream_t s);   // tables of HANDOFF_MULTI_MAX
void launch_nemo_mel_multi(const NemoMel* e, int n, int S, const float* spec, int64_t ld, hipStream_t s);

// NeMo chunks out of the frame history (include/css_mi355_nemo_chunk.h; DESIGN.md 7b "NeMo chunks out of the frame history"):
// frames [first, first + n_frames) of one speaker's ring, raw or normalised per band over the span -- (raw - mean) / (std + 1e-5),
// nemo_norm_kernel's expression, with the span's own mean and unbiased std -- padded with pad_value to `width` columns, as float32
// or float16 into the caller's device memory.  The sums are float64 in ONE order: lane l of 64 adds frames l, l + 64, ... in
// increasing order, then x[l] += x[l + s] for s = 32 .. 1; d * d and the addition of the second pass are rounded apart.  The host
// has checked max(J - hist, 0) <= first and first + n_frames <= J for the speaker's count J.  A table launch: blockIdx.z = chunk.
struct NemoChunkItem {
    const float* ring;                                  // the speaker's rows of the history: [n_mels][hist]
    void* out; float* mean; float* stdv;                // out [n_mels][ld] of the dtype; the span's statistics [n_mels] each (written with `normalize`)
    int64_t hist, ld, first;
    float pad_value;
    int32_t n_frames, width, n_mels, f16, normalize;
};
constexpr int NEMO_CHUNK_MULTI_MAX = 32;                // (CSS_NEMO_CHUNK_TABLE of the header)
constexpr int NEMO_CHUNK_ROWS = 8;                      // mel bands per block
constexpr int NEMO_CHUNK_MAX_WIDTH = 3000;              // (CSS_NEMO_CHUNK_MAX_WIDTH; a wave keeps its row's frames in LDS)
void launch_nemo_chunks(const NemoChunkItem* e, int n, hipStream_t s);   // one launch; n <= NEMO_CHUNK_MULTI_MAX

// ------------------------------------------------------------------------------------------------
// loss.hip -- validation loss of the training loop (train.py:411 _calc_loss): S x S base-loss sums + the noise term
// ------------------------------------------------------------------------------------------------
int val_loss_chunks(int F);
// partial: B * val_loss_chunks(F) * 16 doubles (entries a * 3 + s and [15 -> 9]: see loss.hip)
void launch_val_loss(const float* X, const float* masks, const float* G, int B, int T, int F, int S, int loss_name, int base,
                     int clip, double* partial, hipStream_t s);

// ------------------------------------------------------------------------------------------------
// mvdr.hip -- WTA masks, spatial covariance, MVDR solve, beamform + mask
// ------------------------------------------------------------------------------------------------
struct MvdrArgs {
    const float* X; int64_t T_ld; int64_t stft_frames; int C; int F;
    const float* masks; int64_t mask_ld;   // [(S+1)F][mask_ld]; column = segment*T + t
    int S; int T; int hop;
    int64_t seg_lo; int nseg;
    const uint8_t* wta_override;           // nullptr or [segments][F][T]
    double* scm;                           // [segments][S+1][F][C C]: packed Hermitian, C real diagonal entries, then (Re, Im) of (c, d), c < d, row by row
    double* bfw;                           // [segments][S][F][C][2]
    float* sep;                            // [segments][S][F][T][2]
    float mask_floor;
    int use_mvdr;
};
// PRECONDITIONS of the launches below (the paths guarantee them; css_mvdr_host, include/css_mi355_backend.h, refuses the rest):
//   2 <= C <= 8 for launch_scm, both solves and the MVDR beamformer (one instantiation per C of the packed C x C layout; the sets
//   of a multi-session solve share one C); use_mvdr == 0 reads microphone 0 alone
//   1 <= S <= 3: scm_kernel sorts the frames of the S + 1 mask rows into FOUR lists, one per group of 16 lanes
//   mask_ld >= (seg_lo + nseg) T; T_ld covers the last valid frame min(stft_frames, (seg_lo + nseg - 1) hop + T): frames from
//   stft_frames on are never read
//   an override byte is a winner index below S + 1, or 16 | bits with at least one of the bits 0 .. S set (a frame no mask wins
//   would count towards no list and no plain sum)
bool launch_scm(const MvdrArgs& a, hipStream_t s);   // false: the LDS of a long-segment launch could not be reserved
void launch_mvdr_solve(const MvdrArgs& a, hipStream_t s);
// the same for n sessions' argument sets in one launch (a queue group's sessions; each result is the per-session launch's)
constexpr int MVDR_MULTI_MAX = 8;
void launch_mvdr_solve_multi(const MvdrArgs* a, int n, hipStream_t s);
void launch_beamform(const MvdrArgs& a, hipStream_t s);
// optional power normalisation (css.py:233-247): scales sep of each segment in place by the float64 gain, each value rounded to
// float32 once.  A segment without a valid frame, or whose reference microphone and stream sum are both silent, has the gain
// 0 / 0 of the reference's own formula: every value of it becomes NaN (the paths' segments all hold valid frames)
void launch_segment_power_norm(const MvdrArgs& a, double* scratch, hipStream_t s);

// ------------------------------------------------------------------------------------------------
// stitch.hip -- PIT costs, permutation scan, weighted overlap-add, activity gate
// ------------------------------------------------------------------------------------------------
struct StitchArgs {
    const float* masks; int64_t mask_ld;
    const float* sep;
    int S; int F; int T; int hop;
    int64_t num_segments; int64_t T_long;
    const float* w_first; const float* w_mid; const float* w_last;  // device [T]
    const int32_t* perms;      // [segments][S]
    float* mask_st;            // [S][F][T_long]
    float* activity;           // [S][T_long]
    uint8_t* act_b; uint8_t* act_tmp; uint8_t* act_final;  // [S][T_long]
    float activity_th; int dilation; int erosion;
    float* Y; int KIp;         // [S][T_long][KIp]
    int y_split;               // Y rows as split-f16 GEMM operands (split_f16.hpp) instead of float32
    const unsigned int* level; // with y_split: the rows are scaled by level_gain(level) (split_f16.hpp); null = 1
};
// PRECONDITIONS of the launches below (css_stitch_host, include/css_mi355_backend.h, refuses the rest): 1 <= S <= 4 (SMAX);
// 1 <= hop <= T, and hop < T for the costs (their mean divides by F (T - hop)); mask_ld >= num_segments T; every row of perms
// that a launch reads is a permutation of 0 .. S - 1 (it indexes mask rows and spectra); T_long <= (num_segments - 1) hop + T:
// every frame is covered by a segment (a frame none covers would be 0 / 0 in the masks); KIp >= 2 F, KIp % 32 == 0 with y_split;
// launch_ola_stft's tile is 16 (2 F + 1) floats of dynamic LDS: F <= 511 without raising the kernel's limit.
// scratch: pit_cost_scratch_bytes(total boundaries) bytes, indexed by absolute boundary
size_t pit_cost_scratch_bytes(int64_t n_boundaries);
void launch_pit_costs(const StitchArgs& a, int loss, int input, int64_t b_lo, int64_t b_hi, double* scratch, double* costs,
                      hipStream_t s);
// every boundary of n sessions (a queue group: same S) in one pair of launches; scratch[i] / costs[i] as above per session
constexpr int PIT_MULTI_MAX = 8;
void launch_pit_costs_multi(const StitchArgs* a, double* const* scratch, double* const* costs, int n, int loss, int input, hipStream_t s);
// permutations of segments b_lo + 1 .. b_hi from the raw costs of boundaries [b_lo, b_hi), continuing from the
// permutation of segment b_lo already in perms (b_lo == 0: the identity, written here)
void launch_pit_scan(const double* costs, int64_t b_lo, int64_t b_hi, int S, int32_t* perms, hipStream_t s);
void pit_scan_host(const double* costs, int64_t n_boundaries, int S, int32_t* perms);
void launch_ola_masks(const StitchArgs& a, int64_t t_lo, int64_t t_hi, hipStream_t s);
void launch_morphology(const StitchArgs& a, int64_t t_lo, int64_t t_hi, hipStream_t s);
void launch_ola_stft(const StitchArgs& a, int64_t t_lo, int64_t t_hi, hipStream_t s);

// stream.hip: the stitching tail of a streamed session over a window of segment slots (api_stream.hip).  Local segment j of
// the window is segment seg_base + j of the recording and starts at local frame j * hop; local frame 0 is frame frame_base.
struct StreamStitchArgs {
    const float* masks; int64_t mask_ld;   // [(S+1)F][mask_ld], slot j at column j*T
    const float* sep;                      // [slots][S][F][T][2]
    const int32_t* perms;                  // [slots][S]
    int S; int F; int T; int hop;
    int64_t num_slots;                     // slots holding segments
    int64_t seg_base, frame_base;
    int64_t num_segments_global;           // INT64_MAX while the stream is open
    int64_t T_long_global;                 // INT64_MAX while the stream is open
    const float* w_first; const float* w_mid; const float* w_last;
    uint8_t* act_b;                        // [S][ld_frames]
    float* Y; int KIp;                     // [S][ld_frames][KIp]
    int64_t ld_frames;
    float activity_th; int dilation; int erosion;
    // hand-off (handoff.hip): nullptr, or the ring [S][gate_ld] that receives the gate byte of every frame the gate kernel
    // finalises, frame t of the recording at column t & gate_mask
    uint8_t* gate_out; int64_t gate_ld, gate_mask;
};
void launch_stream_activity(const StreamStitchArgs& a, int64_t t_lo, int64_t t_hi, hipStream_t s);
void launch_stream_gate_ola(const StreamStitchArgs& a, int64_t t_lo, int64_t t_hi, hipStream_t s);
// the same for n streams' windows (a grouped push: same S and F), each with its own local frame range, in launches of up to
// STREAM_MULTI_MAX entries; every frame written is the single launch's (which IS this launch with one entry)
constexpr int STREAM_MULTI_MAX = 16;
struct StreamFrames { int64_t t_lo, t_hi; };
void launch_stream_activity_multi(const StreamStitchArgs* a, const StreamFrames* r, int n, hipStream_t s);
void launch_stream_gate_ola_multi(const StreamStitchArgs* a, const StreamFrames* r, int n, hipStream_t s);
// mask columns of a shared estimator batch -> the streams' windows: for entry e, rows 0 .. rows - 1, columns [src_col, src_col +
// n_cols) of src (leading dimension src_ld) to dst[row * dst_ld + c], c < n_cols.  A pure copy, any number of entries.
struct MaskScatter { float* dst; int64_t dst_ld; int64_t src_col; int64_t n_cols; };
void launch_stream_scatter_masks(const float* src, int64_t src_ld, int rows, const MaskScatter* e, int n, hipStream_t s);
// PCM16 pieces of a round (css_stream_push_many_pcm16) -> the streams' sample windows: dst[c * dst_ld + i] = (float)q[i][c] * 2^-15
// for i < n, c < C.  src is device staging, 16-byte aligned: interleaved [n][C] (plane_ld = 0), or planar with channel c at
// src + c * plane_ld (one channel is planar with any plane_ld).  One launch per STREAM_MULTI_MAX entries; all entries of a
// call have the handle's channel count.
struct StreamIngestPcm16 { const int16_t* src; int64_t plane_ld; int64_t n; int C; float* dst; int64_t dst_ld; };
void launch_stream_ingest_pcm16_multi(const StreamIngestPcm16* e, int n, hipStream_t s);

// ---- resample.hip: rate conversion at a stream's ingest and of whole recordings (scipy.signal.resample_poly's default filter)
// up / down in lowest terms; half = 10 max(up, down), L = 2 half + 1 taps, P = ceil(L / up) taps per output sample; P_ld = P | 1
// is the pitch of a phase's taps in the table (odd: the per-lane gather of up > 1 spreads over the LDS banks)
constexpr int RS_TILE = 256, RS_P_MAX = 128;
struct ResampleRatio { int up, down, half, L, P, P_ld; };
bool resample_ratio(int up, int down, ResampleRatio* r);                       // false: a ratio the library refuses
void resample_taps_f32(const ResampleRatio& r, float* taps);                   // the L float32 taps (float64 on the host, rounded once)
void resample_phase_table(const ResampleRatio& r, const float* taps, float* tab);   // [up][P_ld], a phase's taps in the chain's order
int64_t resample_count(const ResampleRatio& r, int64_t n_in, bool finished);   // outputs computable after n_in inputs / of a recording of n_in
bool resample_fits(const ResampleRatio& r, int C);                             // the tile's LDS (taps + C rows of the span) fits a workgroup
// Outputs [m0, m0 + n_m) of a recording whose inputs [N0 - H, N0) are hist_in [C][H] (float) and [N0, N0 + n) the piece at src
// (device memory; int16 or float32; interleaved [n][C] with plane_ld = 0, or planar with channel c at src + c * plane_ld);
// every other input is zero.  The stream launch writes dst[c * dst_ld + (m - m0)] and, with hist_out, the last H inputs of
// [hist_in | piece] to hist_out [C][H] (another buffer than hist_in); launch_resample writes dst[m * C + c].
struct ResampleJob {
    const void* src; int is_i16; int64_t plane_ld, n;
    const float* hist_in; float* hist_out; int H;
    int64_t N0, m0, n_m;
    int up, down, half, P, P_ld; const float* tab;
    int C; float* dst; int64_t dst_ld;
};
bool launch_stream_ingest_resample_multi(const ResampleJob* e, int n, hipStream_t s);   // false: the LDS could not be reserved
bool launch_resample(const ResampleJob& e, hipStream_t s);
// The output side of a stream (include/css_mi355_stream_out.h): the n final samples per separated stream a round made,
// src [S][src_ld] (the recording's samples [N0, N0 + n)), -> outputs [m0, m0 + n_m) at the rate up / down, as float32 or as
// int16 (__fmul_rn by gain, rint(double * 32767), clamp) at dst[k * dst_ld + (m - m0)] (rows 16-byte aligned).  Inputs
// [N0 - H, N0) are hist_in [S][H]; every other input is zero.  With hist_out the last H inputs of [hist_in | src] go to
// hist_out [S][H] (another buffer than hist_in).  up == down == 1: a copy / conversion, no taps, no span, no history.  Also
// peak[k] = max(peak[k], max |src[k][:]| as float bits) and clipped[k] += samples of the round the clamp changed.
constexpr int SO_TILE = 1024;   // output samples per block
struct StreamOutputJob {
    const float* src; int64_t src_ld, n;
    const float* hist_in; float* hist_out; int H;
    int64_t N0, m0, n_m;
    int up, down, half, P, P_ld; const float* tab;
    int pcm16; float gain;
    void* dst; int64_t dst_ld;
    unsigned int* peak; unsigned long long* clipped;
};
bool stream_output_fits(const ResampleRatio& r);   // the tile's LDS (taps, span, output tile) fits a workgroup
// one launch per STREAM_MULTI_MAX entries (S separated streams each); false: the LDS could not be reserved
bool launch_stream_output_multi(const StreamOutputJob* e, int n, int S, hipStream_t s, int* launches);
// The two wav edges of whole sessions at the capture rate (include/css_mi355_session_rate.h).
// Ingest: a table launch over the rate sessions of a queue group -- entry r is launch_resample's job (the whole recording ->
// dst [n_m][C], the session's slot of the sample buffer), and *level = max(*level, max |dst[m][:]| over m < n_peak) as float
// bits: the word launch_pcm_peak_f32 makes of those samples.
constexpr int SESSION_RATE_TABLE = 8;   // css_ctx::MAX_GROUP
struct SessionIngestJob { ResampleJob r; int64_t n_peak; unsigned int* level; };
bool session_ingest_fits(const ResampleRatio& r, int C);
bool launch_session_ingest_multi(const SessionIngestJob* e, int n, hipStream_t s, int* launches);   // false: the LDS could not be reserved
// Output: rows src [S][src_ld] of n model-rate samples -> dst [S][dst_ld] float32, n_m samples per row at up / down (dst and
// dst_ld multiples of 16 bytes), and peak[k] = max(peak[k], max |dst[k][:]|) as float bits.
struct SessionOutputJob {
    const float* src; int64_t src_ld, n, n_m;
    int up, down, half, P, P_ld; const float* tab;
    float* dst; int64_t dst_ld;
    unsigned int* peak;
};
bool launch_session_output(const SessionOutputJob& e, int S, hipStream_t s);   // false: the LDS could not be reserved

}  // namespace css
