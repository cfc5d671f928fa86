// Exact float32 MFMA GEMM for gfx950, second form (round 5):  C[m][n] = epilogue( sum_k A[m][k] * B[n][k] ).
//
// Same arithmetic as gemm.hip (v_mfma_f32_32x32x2_f32 is a k-ordered fmaf chain; the same K permutation inside each
// group of 8 k), so every output is bit for bit what gemm_kernel writes -- what changes is how the matrix pipe is fed:
//
//   * FOUR independent 4-wave blocks per CU instead of one 8-wave block.  The round-4 kernel needs 169 registers, i.e.
//     two waves per SIMD, both from ONE block: they run the same 32 MFMAs between the same barriers, and the pipe idles
//     while both store the next slab, meet and wait for their first operand reads (a slab takes 2 680 cycles for 2 048 of
//     MFMA issue with one wave per SIMD, tools/gemm_f32_bench.hip).  Here a wave owns 32 COLUMNS of the block's tile and all
//     of its rows (TM row tiles of 32: at most 64 accumulator registers), the slab is 16 deep (short tiles: deeper, below) and
//     double buffered (2 x (128 + 128) rows x 20 floats = 40 960 B: exactly a quarter of the CU's 160 KB), and the kernel is held to
//     128 registers (__launch_bounds__(256, 4)) -- four waves per SIMD from four blocks that fill each other's bubbles.
//     The kernels of the fast epilogue -- every Linear layer's -- fit that without spilling (hipcc -Rpass-analysis=
//     kernel-resource-usage: no scratch; tests/test_gemm_f32_registers.py) because the host picks the epilogue kind: the
//     general epilogue's state, which made the one-body kernel spill, exists only in the kernels that need it.
//   * PERSISTENT blocks over a balanced cut of the work.  The launch is 1 024 blocks (4 x 256 CUs); the output is
//     counted in UNITS of 32 rows x 128 columns, the units of a launch are a line (batch entry, column panel, row unit --
//     row unit fastest), every "virtual CU" takes an equal contiguous piece of that line and each of its four blocks a
//     quarter of the piece, walked in tiles of 1..4 units.  A block's time is proportional to its units, so every CU is
//     busy for ceil(units / 256) unit times whatever M is: M = 22 320 x N = 512 is 2 792 units = 10.9 per CU, where 700
//     tiles of 128 rows leave a quarter of the CUs with 12 units and the rest with 8.
//   * The four blocks of a CU are kept OUT OF PHASE: their first tiles have different heights, so their tile ends --
//     the epilogue's residual reads and result writes, the next tile's cold first slab -- fall into the other blocks'
//     K loops instead of all CUs leaving the matrix pipe idle together (one round of equal tiles: 25 us of a 116 us
//     launch was prologue + epilogue, fitted over K).
//   * The SLAB DEPTH belongs to the tile (round 10): what a wave pays per slab -- the wait for the next slab's loads, the LDS
//     store, the block barrier, the first operand read behind it -- is the same for every tile height, the MFMAs it buys are
//     8 per row unit and 16 k.  With the weights as register fragments and the fast epilogue (every Linear layer) a 32-row tile
//     takes slabs 64 deep and a 64- or 96-row tile 32 deep (f32_max_depth; the deepest that divides K), 32 MFMAs per wave and
//     barrier like the 128-row tile (48 at 96 rows); the A loads of a thread are whole 16-byte pieces of 256- / 128-byte row
//     runs, the weight fragments a ring of one register set: each chunk's but the last's is requested a slab ahead, behind the
//     last MFMA that read its registers, the last chunk's at the top of its own slab (f32_tile says why).  Same order of the
//     MFMAs over k, same bits (tests/test_hip_gemm_f32_slab_depth.py).
//   * Operands arrive by buffer loads (rows past M / N read zeros: no clamped row pointers, one offset register per
//     operand); the epilogue requests a tile's residual values one 32 x 32 tile ahead (the first under the last slab's
//     MFMAs) and writes 16-byte row pieces after a turn through a wave-private LDS patch.
#include <algorithm>
#include <type_traits>

#include "gemm_common.hpp"

namespace css {

namespace {

constexpr int F_BK = 16;                     // slab depth of the tallest tile (and of every tile whose B operand goes through LDS)
constexpr int F_LD = 20;                     // its LDS row stride in floats (depth + 4: see f32_tile)
constexpr int F_BUF = (128 + BN) * F_LD;     // floats per slab buffer (A region sized for the tallest tile)
constexpr int F_PATCH_LD = 36;

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float epi_value(float acc, float bn, float bm, int act, bool has_res, float rv, float alpha) {
    float v = acc + bn + bm;
    if (act == ACT_RELU) v = fmaxf(v, 0.f);
    else if (act == ACT_SIGMOID) v = sigmoidf_(v);
    if (has_res) v = rv + alpha * v;
    return v;
}

#ifndef F32_DMA
#define F32_DMA 0   // 1: global -> LDS by the DMA path (buffer_load ... lds), unpadded 64-byte LDS rows with an XOR swizzle
#endif
#ifndef F32_SPREAD
#define F32_SPREAD 1   // the next slab's global loads one per two MFMA groups of this slab instead of as a burst in front of it
#endif
#ifndef F32_DEEP
#define F32_DEEP 1   // 0 (tools, A/B): every tile with 16-deep slabs, as before round 10
#endif
#ifndef F32_DEEP_TM1
#define F32_DEEP_TM1 64   // slab depth of the 32-row tiles (tools: 16, 32)
#endif
#ifndef F32_DEEP_TM2
#define F32_DEEP_TM2 32   // of the 64-row tiles (tools: 16)
#endif
#ifndef F32_DEEP_TM3
#define F32_DEEP_TM3 32   // of the 96-row tiles (tools: 16)
#endif
// The deepest slab a tile of TM units may take (round 10).  What a wave pays per slab -- the wait for the global loads, the LDS
// store, the block barrier, the first operand read -- does not depend on the tile's height, but the MFMAs it buys do: 8 TM per
// 16 k.  So the short tiles take deeper slabs, 32 MFMAs per wave and barrier like the 128-row tile: 64 k for 32 rows, 32 k for
// 64 rows -- and 32 k for 96 rows too (48 MFMAs: spill-free, and faster in tools/gemm_f32_bench.hip and in the pipeline,
// profiles/r10_gemm_f32_slab_depth.md).  Only the kernels with the weights as register fragments (BD) can: their slab buffers' B
// half is free.  A deep A slab of 32 x 68 or 64 x 36 floats fits the 128 x 20 floats of a buffer's A half; the 96 x 36 = 3 456
// floats of the 96-row tile run on into the unused B half (f32_tile's static_assert holds a BD slab to the whole buffer).  The order
// of the MFMAs over k does not change, so no bit does.  (The DMA path of the tools keeps its unpadded 16-float rows, and a deep
// slab's weight ring needs the spread loads: depth 16 only for F32_DMA and for F32_SPREAD = 0.)
constexpr int f32_max_depth(int tm, bool bd) {
    return (!bd || !F32_DEEP || !F32_SPREAD || F32_DMA) ? 16 : tm == 1 ? F32_DEEP_TM1 : tm == 2 ? F32_DEEP_TM2 : tm == 3 ? F32_DEEP_TM3 : 16;
}

// BD: the B operand is a static weight in FRAGMENT order (launch_f32_fragments: float4 index ((j K/8 + kc) 64 + lane) holds
// W[32 j + (lane & 31)][8 kc + 4 (lane >> 5) .. + 3], i.e. what lane `lane` feeds to the four MFMAs of chunk kc for column
// tile j): it goes global -> registers as one coalesced 1 KiB load per wave and chunk -- no LDS store, no LDS read, half the
// slab buffer -- because every memory instruction of this loop costs matrix issue time.
// FAST: the fast epilogue (below), chosen on the host (f32_fast_epilogue): its launches run a kernel with no general-epilogue code.
// DK: the slab depth (16, 32, 64; a divisor of K -- f32_tile_any picks it per launch).  LDS rows are DK + 4 floats: DK / 4 + 1 is
// odd, and the 16 lanes a ds_read_b128 serves together hold rows of 16 different residues mod 16, so they read 16 different
// bank quads (as 20 = 16 + 4 did); a staging store's 8 lanes hold 8 consecutive pieces of one row for DK >= 32.
template <int TM, bool BD, bool FAST, int DK>
__device__ __forceinline__ void f32_tile(const GemmArgs& g, const float* __restrict__ A, const float* __restrict__ B,
                                         float* __restrict__ C, const int m0, const int n0, float* __restrict__ lds) {
    // (the thread's index behind a compiler barrier: what every tile form derives from it -- staging rows, LDS addresses -- is
    // otherwise formed once in front of the tile walk, for all forms, and held in registers the K loops do not have)
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
    const int M = g.M, N = g.N;
    int gK = g.K;
    int64_t glda = g.lda;
    if constexpr (FAST) asm volatile("" : "+s"(gK), "+s"(glda));   // (as ldc and ldr below: slab counts, extents and pass strides per tile)
    constexpr int BM = 32 * TM;
    constexpr int LD = DK + 4;               // LDS row stride in floats
    constexpr int PPR = DK / 4;              // 16-byte pieces of a row's part of the slab: consecutive threads, one row piece each
    constexpr int RPP = 256 / PPR;           // rows per staging pass
    constexpr int NPA = (BM + RPP - 1) / RPP;   // staging passes over the A tile
    constexpr int NCH = DK / 8;              // 8-k chunks (four MFMAs per row tile each) of a slab
    static_assert(DK == 16 || (BD && (DK == 32 || DK == 64)), "deep slabs: the weights-as-fragments kernels only");
    static_assert(BM * LD <= (BD ? F_BUF : 128 * F_LD), "the A slab must fit its buffer");
    static_assert(!F32_DMA || DK == 16, "the DMA path stages 16-float rows");
    // ---- staging: thread -> (row srow + RPP i, floats sk .. sk + 3) of the slab
    const int srow = tid / PPR, sk = (tid % PPR) * 4;
    // (rows may overlap -- the analysis transform of an arbitrary frame size hands the recording's frames over as rows with
    // stride hop < K: the extent is the last row's end, not rows x stride)
    const int64_t extA = (int64_t)(M - 1) * glda + (glda > gK ? glda : gK), extB = (int64_t)(N - 1) * g.ldb + (g.ldb > gK ? g.ldb : gK);
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(A), 0, (int)(extA * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(B), 0, (int)((BD ? (int64_t)((N + 31) / 32 * 32) * gK : extB) * 4), 0x00020000);
    const int voA = (int)(((int64_t)(m0 + srow) * glda + sk) * 4), voB = (int)(((int64_t)(n0 + srow) * g.ldb + sk) * 4);
    const int passA = (int)(RPP * glda * 4), passB = (int)(64 * g.ldb * 4);   // (B through LDS: DK = 16, 64 rows per pass)
    const bool a1_on = (BM % RPP == 0) || srow < BM % RPP;   // the last A pass may cover fewer rows (DK = 16: 32 of 64 for an odd TM)
#ifndef F32_TOOLS
#define F32_TOOLS 0   // tools/gemm_f32_bench.hip only (-DF32_TOOLS=1): the block census below (GemmArgs::narrow_epilogue == 77 turns
                      // GemmArgs::range_flag into a census buffer).  The library never compiles that path: range_flag there is ONE word.
#endif
#ifndef F32_PROBE
#define F32_PROBE 0   // tools: wave 0 of every block adds up where its slabs' clocks go (issue of the 32 MFMAs incl. operand reads | LDS stores incl. the wait for the global loads | barrier) into the census buffer
#endif
#ifndef F32_FAST_EPILOGUE
#define F32_FAST_EPILOGUE 1   // 0: the general epilogue for every launch (A/B, tools)
#endif
#ifndef F32_TRANSPOSED
#define F32_TRANSPOSED 0   // 1: the MFMA operands swapped (weights first): the accumulators hold the tile TRANSPOSED -- lane = token row,
                           // a register group = four consecutive output features -- and the fast epilogue stores 16-byte pieces
                           // straight from the registers, no turn through the LDS patch (same products, same bits)
#endif
#ifndef F32_STORE_GUARD
#define F32_STORE_GUARD 1   // 0 (tools): without the wait state behind the fast epilogue's 16-byte stores
#endif
// A buffer store of more than 64 bits reads its data registers AFTER it has issued: a VALU result written to one of them in the
// very next slot is what gets stored.  LLVM pads that slot unless the store's soffset is an SGPR (GCNHazardRecognizer::
// createsVALUHazard) -- and the fast epilogue's stores carry their row offset exactly there.  gfx950 does corrupt such a pair
// inside this kernel (seen twice: F32_TRANSPOSED=1, and the shipped epilogue as `-O1 -g` schedules it -- DESIGN.md 3.1c), so the
// wait state is put there by construction: the asm reads the stored registers, so nothing may redefine them in front of it, and
// it is itself one slot.  (tests/test_store_hazard_scan.py scans every unit's ISA for the pair.)
#if F32_STORE_GUARD
#define F32_AFTER_STORE(o) asm volatile("s_nop 0" : : "v"(o));
#else
#define F32_AFTER_STORE(o)
#endif
#if F32_DMA
    // LDS row r (16 floats = four 16-byte slots) holds its k segment s in slot s ^ ((r >> 2) & 3): the 16 lanes of a
    // ds_read_b128 group then hit 16 distinct bank quads.  The DMA writes lane l's 16 bytes at base + 16 l, so lane l
    // (row l >> 2 of its wave's 16 rows, slot l & 3) FETCHES segment (l & 3) ^ ((row >> 2) & 3).
    constexpr int D_BUF = (128 + BN) * 16;
    f32x4 wc[NCH] = {}, wn[NCH] = {};   // (never loaded: launch_gemm_f32 refuses fragment-ordered weights in a DMA build)
    const int vw = 0;
    const int dseg = ((tid & 3) ^ ((tid >> 4) & 3)) * 4;
    const int dvoA = (int)(((int64_t)(m0 + srow) * glda + dseg) * 4), dvoB = (int)(((int64_t)(n0 + srow) * g.ldb + dseg) * 4);
    const bool a1_wave = (BM % 64 == 0) || w < (BM % 64) / 16;   // (wave-uniform: a wave covers 16 rows of a pass)
    typedef __attribute__((address_space(3))) void lds_void;
#define F32_GLOAD(k0, buf)                                                                                       \
    _Pragma("unroll") for (int i = 0; i < NPA; ++i) {                                                            \
        if (i + 1 < NPA || a1_wave)                                                                              \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_void*)(lds + (buf) * D_BUF + (i * 64 + 16 * w) * 16), 16, dvoA, (k0) * 4 + i * passA, 0, 0); \
    }                                                                                                            \
    _Pragma("unroll") for (int i = 0; i < 2; ++i)                                                                \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_void*)(lds + (buf) * D_BUF + (128 + i * 64 + 16 * w) * 16), 16, dvoB, (k0) * 4 + i * passB, 0, 0);
#define F32_LSTORE(buf) __builtin_amdgcn_s_waitcnt(0x0F70);   /* vmcnt(0): this wave's pieces of the next slab have landed */
#define F32_GLOAD1(k0, j)
#undef F32_SPREAD
#define F32_SPREAD 0
#else
    f32x4 ra[NPA], rb[2];
    // BD: this slab's / the next slab's weight fragments (NCH chunks of 8 k each).  A deep slab keeps ONE set, wc, as a ring:
    // chunk ch's fragment of the next slab is requested into wc[ch] behind the chunk's last MFMA, a whole slab ahead of its use
    // -- no second set (64 registers at depth 64) and no copies.  The LAST chunk's fragment is requested at the top of its own
    // slab instead (4 NCH - 4 MFMA groups ahead of its use): a load behind the slab's last MFMA is a load the compiler may place
    // in front of that MFMA -- nothing in the block uses the MFMA's result --, and then the fragment needs other registers than
    // the ones the MFMA still reads: the ring turns into a shift with copies and a vmcnt(0) at every slab's head (seen in the
    // depth-64 body).  So wc[NCH - 1] is not carried from slab to slab at all.
    f32x4 wc[NCH], wn[DK == 16 ? NCH : 1];
    const int vw = (int)((((int64_t)(n0 / 32 + w) * (gK / 8)) * 64 + lane) * 16);
#define F32_GLOAD(k0, buf)                                                                                       \
    _Pragma("unroll") for (int i = 0; i < NPA; ++i) {                                                            \
        if (i + 1 < NPA || a1_on) ra[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsA, voA, (k0) * 4 + i * passA, 0)); \
    }                                                                                                            \
    if constexpr (!BD) {                                                                                         \
        _Pragma("unroll") for (int i = 0; i < 2; ++i)                                                            \
            rb[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsB, voB, (k0) * 4 + i * passB, 0)); \
    } else {                                                                                                     \
        _Pragma("unroll") for (int i = 0; i < (DK == 16 ? NCH : NCH - 1); ++i) {   /* (deep: the last chunk's at its slab's top) */ \
            const f32x4 w_ = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsB, vw, ((k0) / 8 + i) * 1024, 0)); \
            if constexpr (DK == 16) wn[i] = w_; else wc[i] = w_;                                                 \
        }                                                                                                        \
    }
    // load j of the next slab (A passes first, then the B / weight pieces): F32_SPREAD issues them one per two MFMA groups (deep
    // slabs: the A passes one per group from the slab's first, each weight piece behind its chunk)
#define F32_GLOAD1(k0, j)                                                                                        \
    {                                                                                                            \
        if ((j) < NPA) {                                                                                         \
            if ((j) + 1 < NPA || a1_on) ra[(j) < NPA ? (j) : 0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsA, voA, (k0) * 4 + (j) * passA, 0)); \
        } else if ((j) < NPA + (BD ? NCH : 2)) {                                                                 \
            if constexpr (!BD) rb[((j) - NPA) & 1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsB, voB, (k0) * 4 + ((j) - NPA) * passB, 0)); \
            else wn[DK == 16 ? ((j) - NPA) & 1 : 0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsB, vw, ((k0) / 8 + (j) - NPA) * 1024, 0)); \
        }                                                                                                        \
    }
#define F32_LSTORE(buf)                                                                                          \
    {                                                                                                            \
        float* as_ = lds + (buf) * F_BUF + srow * LD + sk;                                                       \
        _Pragma("unroll") for (int i = 0; i < NPA; ++i) {                                                        \
            if (i + 1 < NPA || a1_on) *reinterpret_cast<f32x4*>(as_ + i * RPP * LD) = ra[i];                     \
        }                                                                                                        \
        if constexpr (!BD) {                                                                                     \
            _Pragma("unroll") for (int i = 0; i < 2; ++i) *reinterpret_cast<f32x4*>(as_ + (128 + i * 64) * LD) = rb[i]; \
        }                                                                                                        \
    }
#endif
    f32x16 acc[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) acc[i] = f32x16{0};
    const int nk = gK / DK;
#if F32_PROBE
    const unsigned long long t_in_ = (w == 0) ? __builtin_readcyclecounter() : 0;
#endif
    F32_GLOAD(0, 0)
    F32_LSTORE(0)
    if constexpr (BD && DK == 16) { wc[0] = wn[0]; wc[1] = wn[1]; }
    __syncthreads();
#if F32_DMA
    constexpr int S_BUF = D_BUF, S_LD = 16;
    const int sw4 = ((c >> 2) & 3) * 4;
    const int aoff = c * 16, boff = (128 + 32 * w + c) * 16;
#define F32_SLOT(ch) (((8 * (ch) + 4 * h)) ^ sw4)
#else
    constexpr int S_BUF = F_BUF, S_LD = LD;
    const int aoff = c * LD + 4 * h, boff = (128 + 32 * w + c) * LD + 4 * h;
#define F32_SLOT(ch) (8 * (ch))
#endif
    // epilogue operands: lane -> rows (lane >> 3) + 8 j of each 32 x 32 tile, columns n .. n + 3
    const float* __restrict__ bias = g.bias;
    const float* __restrict__ res = g.residual;
    const int act = g.act;
    const bool bias_m = bias && g.bias_along_m, bias_n = bias && !g.bias_along_m, has_res = res != nullptr;
    int64_t ldc = g.ldc, ldr = g.ldr;
    // (behind a compiler barrier: otherwise every row multiple of ldc and ldr that the epilogues of all tile forms use is formed in
    // front of the tile walk and held in scalar registers through it -- with the deep forms' bodies more than there are)
    if constexpr (FAST) asm volatile("" : "+s"(ldc), "+s"(ldr));
    const float alpha = g.alpha;
    // (the general epilogue's 16-byte pieces; the fast one always has them)
    const bool wide = FAST || ((ldc % 4 == 0) && (N % 4 == 0) && ((reinterpret_cast<uintptr_t>(C) & 15) == 0) &&
                               (!has_res || ((ldr % 4 == 0) && ((reinterpret_cast<uintptr_t>(res) & 15) == 0))));
    // The fast form of the epilogue (round 5): a wave in its epilogue shares its SIMD with three waves issuing MFMAs back to
    // back, and EVERY instruction it issues waits for a slot between them -- the slab-clock probe (tools, F32_PROBE) put the
    // last slab + epilogue at 15 k clocks of a K = 512 tile's 100 k and at 37 k of 162 k for the QKV tiles, ~220 vector-ALU
    // instructions per 32 x 32 tile (64-bit row addresses, row / column bound compares, exec masks, the bias_m select).  With
    // the rows addressed through buffer descriptors -- one per-lane offset per tile, the row piece as a SCALAR offset, rows
    // past M dropped (stores) or read as zero (residual) by the bounds check -- a row piece costs its arithmetic and nothing
    // else.  (The scalar offset takes part in the bounds check on gfx950: tools/buffer_bounds_probe.hip, loads and stores.)
    // Conditions (f32_fast_epilogue, on the host): 16-byte pieces, whole 128-column panels, column bias or none, no sigmoid,
    // operands below 2 GiB.
    constexpr bool fast = FAST;
    const __amdgpu_buffer_rsrc_t rsC = __builtin_amdgcn_make_buffer_rsrc(C, 0, fast ? (int)((int64_t)M * ldc * 4) : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsR = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(res), 0, (fast && has_res) ? (int)((int64_t)M * ldr * 4) : 0, 0x00020000);
    f32x4 rv[2][4];   // residual pieces of the tile being written and of the next one
#if F32_TRANSPOSED
    // (accumulator layout: lane (c, h) = token row m0 + 32 i + c, registers 4 q .. 4 q + 3 = features n0 + 32 w + 8 q + 4 h .. + 3)
    auto prefetch_fast = [&](int i, int slot, int lane_) {
        const int vo_ = (int)((((int64_t)m0 + (lane_ & 31)) * ldr + n0 + 32 * w + 4 * (lane_ >> 5)) * 4);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            rv[slot][q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsR, vo_, (int)((32 * i * ldr + 8 * q) * 4), 0));
    };
#else
    // (32-bit unsigned offsets: M ldr 4 < 2^31 (f32_fast_epilogue), and the rows of a tail tile past M stay below 2^32)
    auto prefetch_fast = [&](int i, int slot, int lane_) {
        const int vo_ = (int)(((unsigned)(m0 + (lane_ >> 3)) * (unsigned)ldr + n0 + 32 * w + (lane_ & 7) * 4) * 4u);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            rv[slot][j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsR, vo_, (int)((unsigned)(32 * i + 8 * j) * (unsigned)ldr * 4u), 0));
    };
#endif
    // (lane_ is `lane` behind a compiler barrier at the call sites below: the 64-bit row addresses of the epilogue must
    // not be formed before the K loop and carried through it -- the loop has no registers to spare)
    auto prefetch = [&](int i, int slot, int lane_) {
        const int n_ = n0 + 32 * w + (lane_ & 7) * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = m0 + 32 * i + (lane_ >> 3) + 8 * j;
            const int mc = m < M ? m : M - 1;
            rv[slot][j] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (has_res && n_ < N) {
                if (wide) {
                    rv[slot][j] = *reinterpret_cast<const f32x4*>(res + (int64_t)mc * ldr + n_);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) rv[slot][j][e] = res[(int64_t)mc * ldr + (n_ + e < N ? n_ + e : N - 1)];
                }
            }
        }
    };
#ifndef F32_ABLATE
#define F32_ABLATE 0   // tools: timing probes (wrong results): 1 no slab barrier, 2 no global loads / LDS stores, 4 no LDS operand reads; 8 (right results): accumulators in AGPRs
#endif
    f32x4 abl_a = {1.f, 2.f, 3.f, (float)lane}, abl_b = {0.5f, 0.25f, (float)w, 1.f};
#define F32_MFMA(i, av, bv)                                                                                      \
    {                                                                                                            \
        if (F32_ABLATE & 8) asm volatile("v_mfma_f32_32x32x2_f32 %0, %1, %2, %0" : "+a"(acc[i]) : "v"(av), "v"(bv)); \
        else if (F32_TRANSPOSED) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(bv, av, acc[i], 0, 0, 0);         \
        else acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[i], 0, 0, 0);                             \
    }
    // A deep slab (DK > 16, weights in registers) reads chunk ch + 1's A fragments in front of chunk ch's MFMAs: the slab's
    // NCH operand reads cost one exposed LDS latency, the first, instead of one each.
#define F32_COMPUTE(buf)                                                                                         \
    {                                                                                                            \
        const float* as = lds + (buf) * S_BUF + aoff;                                                            \
        const float* bs = lds + (buf) * S_BUF + boff;                                                            \
        if constexpr (DK == 16) {                                                                                \
            _Pragma("unroll") for (int ch = 0; ch < 2; ++ch) {                                                   \
                f32x4 b = abl_b;                                                                                 \
                if constexpr (BD) b = wc[ch];                                                                    \
                else if (!(F32_ABLATE & 4)) b = *reinterpret_cast<const f32x4*>(bs + F32_SLOT(ch));              \
                f32x4 a[TM];                                                                                     \
                _Pragma("unroll") for (int i = 0; i < TM; ++i) {                                                 \
                    a[i] = abl_a;                                                                                \
                    if (!(F32_ABLATE & 4)) a[i] = *reinterpret_cast<const f32x4*>(as + i * 32 * S_LD + F32_SLOT(ch)); \
                }                                                                                                \
                __builtin_amdgcn_sched_barrier(0);                                                               \
                _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                  \
                    if (F32_SPREAD && spread_k0 >= 0 && !(e & 1)) { F32_GLOAD1(spread_k0, ch * 2 + (e >> 1)) __builtin_amdgcn_sched_barrier(0); } \
                    _Pragma("unroll") for (int i = 0; i < TM; ++i) F32_MFMA(i, a[i][e], b[e])                    \
                    if (F32_SPREAD && spread_k0 >= 0) __builtin_amdgcn_sched_barrier(0);                         \
                }                                                                                                \
                __builtin_amdgcn_sched_barrier(0);                                                               \
            }                                                                                                    \
        } else {                                                                                                 \
            wc[NCH - 1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsB, vw, (cur_k0 / 8 + NCH - 1) * 1024, 0)); \
            f32x4 a[2][TM];                                                                                      \
            _Pragma("unroll") for (int i = 0; i < TM; ++i) {                                                     \
                a[0][i] = abl_a;                                                                                 \
                if (!(F32_ABLATE & 4)) a[0][i] = *reinterpret_cast<const f32x4*>(as + i * 32 * S_LD);            \
            }                                                                                                    \
            _Pragma("unroll") for (int ch = 0; ch < NCH; ++ch) {                                                 \
                if (ch + 1 < NCH) {                                                                              \
                    _Pragma("unroll") for (int i = 0; i < TM; ++i) {                                             \
                        a[(ch + 1) & 1][i] = abl_a;                                                              \
                        if (!(F32_ABLATE & 4)) a[(ch + 1) & 1][i] = *reinterpret_cast<const f32x4*>(as + i * 32 * S_LD + 8 * (ch + 1)); \
                    }                                                                                            \
                }                                                                                                \
                __builtin_amdgcn_sched_barrier(0);                                                               \
                _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                  \
                    if (spread_k0 >= 0 && ch * 4 + e < NPA) { F32_GLOAD1(spread_k0, ch * 4 + e) __builtin_amdgcn_sched_barrier(0); } \
                    _Pragma("unroll") for (int i = 0; i < TM; ++i) F32_MFMA(i, a[ch & 1][i][e], wc[ch][e])       \
                    if (spread_k0 >= 0) __builtin_amdgcn_sched_barrier(0);                                       \
                }                                                                                                \
                if (spread_k0 >= 0 && ch + 1 < NCH) {                                                            \
                    wc[ch] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsB, vw, (spread_k0 / 8 + ch) * 1024, 0)); \
                }                                                                                                \
                __builtin_amdgcn_sched_barrier(0);                                                               \
            }                                                                                                    \
        }                                                                                                        \
    }
    // slabs 0 .. nk - 2: the next slab travels global -> registers under this slab's MFMAs, then registers -> LDS
#if F32_PROBE
    const bool probe = w == 0 && g.narrow_epilogue == 77 && g.range_flag;
    unsigned long long pc_ = 0, pl_ = 0, pb_ = 0, pt_ = 0;
    const unsigned long long t_loop_ = probe ? __builtin_readcyclecounter() : 0;
#define F32_CLK(var) if (probe) var = __builtin_readcyclecounter();
#else
#define F32_CLK(var)
#endif
    int spread_k0 = -1, cur_k0 = 0;   // (k of the next slab while its loads are spread under this one's MFMAs; k of this slab)
    for (int kt = 0; kt + 1 < nk; ++kt) {
#if F32_PROBE
        unsigned long long t0_ = 0, t1_ = 0, t2_ = 0, t3_ = 0;
#endif
        F32_CLK(t0_)
        cur_k0 = kt * DK;
        if (F32_SPREAD) spread_k0 = (kt + 1) * DK;
        else if (!(F32_ABLATE & 2)) { F32_GLOAD((kt + 1) * DK, (kt + 1) & 1) }
        __builtin_amdgcn_sched_barrier(0);   // (the compiler otherwise sinks the loads below the MFMAs, next to their LDS stores)
        F32_COMPUTE(kt & 1)
        F32_CLK(t1_)
        if (!(F32_ABLATE & 2)) { F32_LSTORE((kt + 1) & 1) }
        if constexpr (BD && DK == 16) { wc[0] = wn[0]; wc[1] = wn[1]; }
        F32_CLK(t2_)
        if (!(F32_ABLATE & 1)) __syncthreads();
        F32_CLK(t3_)
#if F32_PROBE
        pc_ += t1_ - t0_; pl_ += t2_ - t1_; pb_ += t3_ - t2_; pt_ += 1;
#endif
    }
#if F32_PROBE
    if (probe && lane == 0) {
        unsigned long long* pr = reinterpret_cast<unsigned long long*>(g.range_flag) + 4096 + 4 * blockIdx.x;
        atomicAdd(pr + 0, pc_); atomicAdd(pr + 1, pl_); atomicAdd(pr + 2, pb_); atomicAdd(pr + 3, pt_);
        atomicAdd(pr + 4096 + 0, t_loop_ - t_in_);   // prologue: first slab global -> LDS, barrier
        atomicAdd(pr + 4096 + 1, 1ull);              // tiles
    }
    const unsigned long long t_out_ = probe ? __builtin_readcyclecounter() : 0;
#define F32_EPILOGUE_PROBE                                                                                       \
    if (probe && lane == 0) {                                                                                    \
        unsigned long long* pr = reinterpret_cast<unsigned long long*>(g.range_flag) + 4096 + 4 * blockIdx.x;    \
        atomicAdd(pr + 4096 + 2, __builtin_readcyclecounter() - t_out_);   /* the last slab + the epilogue */     \
    }
#else
#define F32_EPILOGUE_PROBE
#endif
#undef F32_CLK
    // the last slab: the first tile's epilogue operands travel under its MFMAs
    {
        int lane_ = lane;
        asm volatile("" : "+v"(lane_));
        if (fast) { if (has_res) prefetch_fast(0, 0, lane_); }
        else prefetch(0, 0, lane_);
    }
    spread_k0 = -1;
    cur_k0 = (nk - 1) * DK;
    F32_COMPUTE((nk - 1) & 1)
    __syncthreads();
#undef F32_COMPUTE
#undef F32_MFMA
#undef F32_SLOT
#undef F32_GLOAD
#undef F32_GLOAD1
#undef F32_LSTORE

    // ---- epilogue: every 32 x 32 tile takes a turn through the wave's LDS patch and leaves as 16-byte row pieces
    // (the slab buffers are free: the loop ended with a barrier)
    int lane_e = lane;
    asm volatile("" : "+v"(lane_e));
    float* patch = lds + w * (32 * F_PATCH_LD);
    const int col4 = (lane_e & 7) * 4, n = n0 + 32 * w + col4, erow = lane_e >> 3;
    const bool col_ok = n < N;
    float bn[4] = {0.f, 0.f, 0.f, 0.f};
    if (bias_n) {
#pragma unroll
        for (int e = 0; e < 4; ++e) bn[e] = bias[n + e < N ? n + e : N - 1];
    }
#if F32_TRANSPOSED
    if (fast) {
        // The accumulators hold the tile transposed (see F32_COMPUTE): a lane's four registers of a group are four consecutive
        // output features of ITS token row -- a 16-byte piece of the output row as it stands.  No turn through LDS.
        const int ce = lane_e & 31, he = lane_e >> 5, nw = n0 + 32 * w + 4 * he;
        const int voC = (int)((((int64_t)m0 + ce) * ldc + nw) * 4);
        const bool relu = act == ACT_RELU;
        f32x4 bq[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            bq[q] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (bias_n) {
#pragma unroll
                for (int e = 0; e < 4; ++e) bq[q][e] = bias[nw + 8 * q + e];
            }
        }
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            if (i + 1 < TM && has_res) prefetch_fast(i + 1, (i + 1) & 1, lane_e);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float t = acc[i][4 * q + e] + bq[q][e];
                    if (relu) t = fmaxf(t, 0.f);
                    if (has_res) t = rv[i & 1][q][e] + alpha * t;
                    o[e] = t;
                }
                typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), rsC, voC, (int)((32 * i * ldc + 8 * q) * 4), 0);
                F32_AFTER_STORE(o)
#if F32_TRANSPOSED >= 2
                // the store reads its four data registers AFTER it has issued; the next piece's first VALU result must not land in
                // them before that (tools/store_war_probe.hip: more wait states than the compiler's hazard table pads on gfx950)
                __builtin_amdgcn_sched_barrier(0);
                asm volatile("s_nop 7");
#if F32_TRANSPOSED >= 3
                asm volatile("s_nop 7");
#endif
                __builtin_amdgcn_sched_barrier(0);
#endif
            }
        }
        F32_EPILOGUE_PROBE
        return;
    }
#else
    if constexpr (FAST) {
        const int voC = (int)(((unsigned)(m0 + erow) * (unsigned)ldc + n) * 4u);   // (32-bit unsigned, as prefetch_fast)
        // The activation and the residual are launch constants: the combinations the estimator's launches use (residual and no
        // activation, ReLU, neither) get their own copy of the loop, so an element costs its own arithmetic and no select
        // between the variants (the same operations either way).  A residual with a ReLU takes the residual's copy with the
        // ReLU as a select: a fourth copy does not fit the registers without spilling.
        auto epilogue = [&](auto relu_c, auto res_c) {
            const bool relu = relu_c;
            constexpr bool res = decltype(res_c)::value;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
#pragma unroll
                for (int r = 0; r < 16; ++r) patch[((r & 3) + 8 * (r >> 2) + 4 * h) * F_PATCH_LD + c] = acc[i][r];
                if (i + 1 < TM && res) prefetch_fast(i + 1, (i + 1) & 1, lane_e);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(patch + (erow + 8 * j) * F_PATCH_LD + col4);
                    f32x4 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float t = v[e] + bn[e];                      // (epi_value's arithmetic with bm = 0: acc + bn is never -0, so the
                        if (relu) t = fmaxf(t, 0.f);                 //  dropped "+ 0.f" changes no bit)
                        if (res) t = rv[i & 1][j][e] + alpha * t;
                        o[e] = t;
                    }
                    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), rsC, voC, (int)((unsigned)(32 * i + 8 * j) * (unsigned)ldc * 4u), 0);
                    F32_AFTER_STORE(o)
                }
            }
        };
        if (has_res) epilogue(act == ACT_RELU, std::true_type{});
        else if (act == ACT_RELU) epilogue(std::true_type{}, std::false_type{});
        else epilogue(std::false_type{}, std::false_type{});
        F32_EPILOGUE_PROBE
        return;
    }
#endif
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#if F32_TRANSPOSED
        // (the transposed accumulator: lane c is token row c of the patch, a register group four consecutive columns)
#pragma unroll
        for (int q = 0; q < 4; ++q)
            *reinterpret_cast<f32x4*>(patch + c * F_PATCH_LD + 8 * q + 4 * h) = f32x4{acc[i][4 * q], acc[i][4 * q + 1], acc[i][4 * q + 2], acc[i][4 * q + 3]};
#else
#pragma unroll
        for (int r = 0; r < 16; ++r) patch[((r & 3) + 8 * (r >> 2) + 4 * h) * F_PATCH_LD + c] = acc[i][r];
#endif
        // (a wave's own LDS writes and reads are in order: no barrier)
        if (i + 1 < TM) prefetch(i + 1, (i + 1) & 1, lane_e);   // (the registers of acc[i] are free now)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int row = erow + 8 * j, m = m0 + 32 * i + row;
            const f32x4 v = *reinterpret_cast<const f32x4*>(patch + row * F_PATCH_LD + col4);
            if (m >= M || !col_ok) continue;
            float* dst = C + (int64_t)m * ldc + n;
            const float bm = bias_m ? bias[m] : 0.f;   // (the mask head only: one launch per batch)
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = epi_value(v[e], bn[e], bm, act, has_res, rv[i & 1][j][e], alpha);
            if (wide) {
                *reinterpret_cast<f32x4*>(dst) = o;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (n + e < N) dst[e] = o[e];
            }
        }
    }
    F32_EPILOGUE_PROBE
#undef F32_EPILOGUE_PROBE
}

// A tile of TM units at the deepest slab its height may take (f32_max_depth) that divides K -- no remainder slabs: K = 512 and
// 1 024 take 64, the embedding's 1 824 takes 32, any other multiple of 16 takes 16.
// (Every entry point of the library takes K % 32 == 0 only, so through the library heights 1 - 3 always run deep: their depth-16
// bodies in gemm_f32_kernel<true, true> -- three of its eight tile bodies -- are reached by direct callers of
// launch_gemm with K = 16 (2 n + 1) alone, and no pytest case runs them; tools/gemm_f32_bench.hip's bit check does, built
// with -DF32_DEEP=0.)
template <int TM, bool BD, bool FAST>
__device__ __forceinline__ void f32_tile_any(const GemmArgs& g, const float* __restrict__ A, const float* __restrict__ B,
                                             float* __restrict__ C, const int m0, const int n0, float* __restrict__ lds) {
    constexpr int D = f32_max_depth(TM, BD && FAST);   // (the general epilogue's kernels have no registers for a deep body)
    if constexpr (D >= 64) {
        if (g.K % 64 == 0) return f32_tile<TM, BD, FAST, 64>(g, A, B, C, m0, n0, lds);
    }
    if constexpr (D >= 32) {
        if (g.K % 32 == 0) return f32_tile<TM, BD, FAST, 32>(g, A, B, C, m0, n0, lds);
    }
    f32_tile<TM, BD, FAST, 16>(g, A, B, C, m0, n0, lds);
}

}  // namespace

// The work of a launch as a line of units (32 rows x 128 columns): index = (batch entry * tiles_n + column panel) * u + row
// unit.  Virtual CU v of `ncu` takes [v U / ncu, (v + 1) U / ncu), its block j of four a quarter of that.
struct F32Plan {
    int u, tiles_n, ncu, max_tm; int64_t U;
#if F32_TOOLS
    unsigned long long* dbg;   // every block records where and when it ran (shader / wall clocks)
#endif
};

template <bool BD, bool FAST>
__global__ __launch_bounds__(256, 4) void gemm_f32_kernel(GemmArgs g, F32Plan p) {
    __shared__ __attribute__((aligned(16))) float lds[2 * F_BUF];
    const int b = blockIdx.x, v = b % p.ncu, j = b / p.ncu;
    const int64_t lo = p.U * v / p.ncu, hi = p.U * (v + 1) / p.ncu;
    int64_t pos = lo + (hi - lo) * j / 4;
    const int64_t end = lo + (hi - lo) * (j + 1) / 4;
    // first tile: 1 + (b + j) % 4 units -- neighbours in the grid AND blocks one stride apart differ, whichever of them the
    // dispatcher puts on one CU; afterwards the tallest tile that fits
    int want = std::min(1 + (b + j) % 4, p.max_tm);
    bool first = true;
#if F32_TOOLS
    if (p.dbg && threadIdx.x == 0) {   // (a census of the blocks -- where and when each ran)
        p.dbg[4 * b + 0] = wall_clock64();
        p.dbg[4 * b + 2] = ((unsigned long long)__builtin_amdgcn_s_getreg(63508) << 32) | (unsigned)__builtin_amdgcn_s_getreg(63492);   // XCC_ID | HW_ID
        p.dbg[4 * b + 3] = __builtin_readcyclecounter();
    }
#endif
    // (row unit r, column panel tn, batch entry bz of pos: divided out once, then stepped -- a tile never crosses a panel)
    const int64_t panel0 = pos / p.u;
    int r = (int)(pos - panel0 * p.u);
    int bz = (int)(panel0 / p.tiles_n), tn = (int)(panel0 - (int64_t)bz * p.tiles_n);
    while (pos < end) {
        const int tm = (int)std::min<int64_t>(std::min<int64_t>(want, end - pos), p.u - r);
        const float* A = g.A + (int64_t)bz * g.strideA;
        const float* B = g.B + (int64_t)bz * g.strideB;
        float* C = g.C + (int64_t)bz * g.strideC;
        if (!first) __syncthreads();   // the previous tile's epilogue patches lie over the slab buffers
        first = false;
        switch (tm) {
            case 1: f32_tile_any<1, BD, FAST>(g, A, B, C, 32 * r, tn * BN, lds); break;
            case 2: f32_tile_any<2, BD, FAST>(g, A, B, C, 32 * r, tn * BN, lds); break;
            case 3: f32_tile_any<3, BD, FAST>(g, A, B, C, 32 * r, tn * BN, lds); break;
            default: f32_tile_any<4, BD, FAST>(g, A, B, C, 32 * r, tn * BN, lds); break;
        }
        pos += tm;
        want = p.max_tm;
        r += tm;
        if (r == p.u) {
            r = 0;
            if (++tn == p.tiles_n) { tn = 0; ++bz; }
        }
    }
#if F32_TOOLS
    if (p.dbg && threadIdx.x == 0) { p.dbg[4 * b + 1] = wall_clock64(); p.dbg[4 * b + 3] = __builtin_readcyclecounter() - p.dbg[4 * b + 3]; }
#endif
}

// Whether a launch takes the fast epilogue (f32_tile): it depends on the launch arguments only, so the host picks the
// kernel -- 16-byte pieces (every batch entry's C aligned too), whole 128-column panels, column bias or none, no sigmoid, C and
// the residual below 2 GiB for the descriptors' 32-bit range.
static bool f32_fast_epilogue(const GemmArgs& g) {
    const int64_t lim = (int64_t)1 << 31;
    const bool has_res = g.residual != nullptr;
    const bool wide = (g.ldc % 4 == 0) && (g.N % 4 == 0) && ((reinterpret_cast<uintptr_t>(g.C) & 15) == 0) &&
                      (g.batch == 1 || g.strideC % 4 == 0) &&
                      (!has_res || ((g.ldr % 4 == 0) && ((reinterpret_cast<uintptr_t>(g.residual) & 15) == 0)));
    return F32_FAST_EPILOGUE && wide && !(g.bias && g.bias_along_m) && (g.N % BN == 0) && g.act != ACT_SIGMOID &&
           (int64_t)g.M * g.ldc * 4 < lim && (!has_res || (int64_t)g.M * g.ldr * 4 < lim);
}

// false: an operand the 32-bit buffer offsets cannot address, or a K that is not a multiple of 16 (use gemm_kernel)
bool launch_gemm_f32(const GemmArgs& g, hipStream_t s, int forced_tm) {
    if (g.M <= 0 || g.N <= 0 || g.batch <= 0) return true;
    if (g.K <= 0 || g.K % F_BK) return false;
    const int64_t lim = (int64_t)1 << 31;
    if ((((int64_t)g.M + 128) * g.lda + g.K) * 4 >= lim || (((int64_t)g.N + 128) * g.ldb + g.K) * 4 >= lim) return false;
#if F32_DMA
    if (g.b_frag32) return false;   // (the DMA path stages a row-major B: the caller's B_rows fallback, or a loud refusal)
#endif
    if (g.b_frag32 && (g.N % 32 || g.K % 16 || g.batch != 1 || ((int64_t)g.N * g.K * 4 >= lim))) return false;
    if ((g.lda % 4) || (!g.b_frag32 && (g.ldb % 4)) || (reinterpret_cast<uintptr_t>(g.A) & 15) || (reinterpret_cast<uintptr_t>(g.B) & 15)) return false;   // 16-byte operand loads
    constexpr int NCU = 256;
    F32Plan p;
    p.u = (g.M + 31) / 32;
    p.tiles_n = (g.N + BN - 1) / BN;
    p.ncu = NCU;
    p.max_tm = (forced_tm >= 1 && forced_tm <= 4) ? forced_tm : 4;
    p.U = (int64_t)p.u * p.tiles_n * g.batch;
#if F32_TOOLS
    p.dbg = g.narrow_epilogue == 77 ? reinterpret_cast<unsigned long long*>(g.range_flag) : nullptr;   // (tools/gemm_f32_bench.hip)
#endif
    const bool fast = f32_fast_epilogue(g);
    void (*kern)(GemmArgs, F32Plan) = g.b_frag32 ? (fast ? gemm_f32_kernel<true, true> : gemm_f32_kernel<true, false>)
                                                 : (fast ? gemm_f32_kernel<false, true> : gemm_f32_kernel<false, false>);
    hipLaunchKernelGGL(kern, dim3(4 * NCU), dim3(256), 0, s, g, p);
    return true;
}


// float32 W [N][K] (row stride ld_src; N % 32 == 0, K % 8 == 0) -> fragment order for gemm_f32_kernel<true> (see f32_tile)
__global__ void f32_fragments_kernel(const float* __restrict__ src, int64_t ld_src, float* __restrict__ dst, int N, int K) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;     // one float4 of dst
    const int64_t total = (int64_t)(N / 32) * (K / 8) * 64;
    if (idx >= total) return;
    const int lane = (int)(idx & 63);
    const int64_t t = idx >> 6;
    const int kc = (int)(t % (K / 8)), j = (int)(t / (K / 8));
    const float* p = src + (int64_t)(32 * j + (lane & 31)) * ld_src + 8 * kc + 4 * (lane >> 5);
    reinterpret_cast<float4*>(dst)[idx] = make_float4(p[0], p[1], p[2], p[3]);
}
void launch_f32_fragments(const float* src, int64_t ld_src, float* dst, int N, int K, hipStream_t s) {
    const int64_t total = (int64_t)(N / 32) * (K / 8) * 64;
    if (total <= 0) return;
    hipLaunchKernelGGL(f32_fragments_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, ld_src, dst, N, K);
}

}  // namespace css
