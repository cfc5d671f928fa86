// css_linear_host and css_gemm_host of include/css_mi355.h: one launch_gemm of the path on caller data (unit tests of the arithmetic;
// the companion of api_encoder.hip).  Both check first, then stage in h->stage, launch, download every allocation the launch
// could have written and synchronise.
#include <cmath>

#include "api_ctx.hpp"
#include "api_kernel_stage.hpp"   // (Stager, stage_and_upload, download_all)

using namespace css;
using namespace css::kstage;

extern "C" {

// torch.nn.Linear on caller data through one of the path's three GEMM kernels.
int css_linear_host(css_handle_t h, const float* x, const float* w, const float* bias, int32_t M, int32_t N, int32_t K,
                    int32_t kernel, int32_t layout, float* y) {
    CSS_DRAIN(h);
    if (!h || !x || !w || !y || M < 1 || N < 1 || K < 32 || K % 32) return fail(h, CSS_ERR_INVALID_ARG, "bad argument (K must be a multiple of 32)");
    if (kernel < 0 || kernel > 2) return fail(h, CSS_ERR_INVALID_ARG, "kernel must be 0 (split, weights direct), 1 (split, LDS staged) or 2 (exact float32)");
    const int Np = (N + 31) / 32 * 32;
    Stager sg;
    const size_t o_x = sg.arr(x, (int64_t)M * K, 4, UP), o_xs = sg.scratch((int64_t)M * K, 4);
    const size_t o_w = sg.arr(w, (int64_t)N * K, 4, UP), o_ws = sg.scratch((int64_t)Np * K, 4);
    const size_t o_y = sg.arr(y, (int64_t)M * N, 4, DOWN), o_b = sg.arr(bias, N, 4, UP);
    char* base = nullptr;
    int rc;
    if ((rc = stage_and_upload(h, sg, &base)) != CSS_OK) return rc;
    auto at = [&](size_t o) { return Stager::dev<float>(base, o); };   // (null for an absent array)
    float *xd = at(o_x), *xs = at(o_xs), *wd = at(o_w), *ws = at(o_ws);
    GemmArgs g = linear(xd, K, wd, K, at(o_b), at(o_y), N, M, N, K, ACT_NONE);
    if (kernel != 2) {
        launch_split_convert(xd, K, xs, M, K, K, h->stream);
        if (kernel == 0) launch_split_convert_tiled(wd, K, ws, N, K, h->stream);
        else launch_split_convert(wd, K, ws, N, K, K, h->stream);
        g.A = xs; g.B = ws; g.split_in = 1; g.b_tiled = kernel == 0;
        if (kernel == 0) g.tile_rows = layout; else g.layout = layout;
    } else {
        g.layout = layout;
    }
    launch_gemm(g, h->stream);
    return download_all(h, sg, base);
}

// One launch_gemm in any of the forms the path uses, on caller data.  Whatever a kernel's own comment excludes is refused here:
// the entry never launches something undefined.
int css_gemm_host(css_handle_t h, const CssGemmDesc* d, const float* a, const float* b, const float* bias, const float* residual,
                  float* c) {
    CSS_DRAIN(h);
    if (!h) return CSS_ERR_INVALID_ARG;
    auto bad = [&](const char* what) { return fail(h, CSS_ERR_INVALID_ARG, std::string("css_gemm_host: ") + what); };
    if (!d || !a || !b || !c) return bad("null argument");
    const int M = d->M, N = d->N, K = d->K, batch = d->batch, kernel = d->kernel;
    if (kernel < 0 || kernel > 2) return bad("kernel must be 0 (split, weights direct), 1 (split, LDS staged) or 2 (exact float32)");
    if (M < 1 || N < 1 || batch < 1 || K < 32 || K % 32 || M > (1 << 22) || N > (1 << 22) || K > (1 << 16) || batch > 1024)
        return bad("M, N, batch >= 1 and K a multiple of 32");
    if (d->lda < K || d->ldb < K || d->lda % 4 || d->ldb % 4 || d->lda > HOST_CAP || d->ldb > HOST_CAP) return bad("lda, ldb: multiples of 4, at least K");
    if (d->act < ACT_NONE || d->act > ACT_SIGMOID) return bad("act must be 0, 1 or 2");
    if (d->bias < 0 || d->bias > 2 || (d->bias != 0) != (bias != nullptr)) return bad("bias: 0 with NULL, 1 or 2 with an array");
    if (d->residual < 0 || d->residual > 2 || (d->residual == 1) != (residual != nullptr)) return bad("residual: 1 with an array, 0 or 2 with NULL");
    if (!(std::fabs(d->alpha) <= 3.0e38f)) return bad("alpha must be finite");
    if (d->a_off < 0 || d->c_off < 0 || d->r_off < 0 || d->a_off > 1024 || d->c_off > (1 << 20) || d->r_off > 1024) return bad("offsets");
    const bool tr = d->c_transposed != 0, has_res = d->residual != 0;
    const int rows_c = tr ? N : M, cols_c = tr ? M : N;   // the output as it lies in memory
    if (d->ldc < cols_c || d->ldc > HOST_CAP) return bad("ldc is shorter than a row of C");
    const int64_t ldr = d->residual == 2 ? d->ldc : d->ldr;
    if (d->residual == 1 && (ldr < N || ldr > HOST_CAP)) return bad("ldr is shorter than a row of the residual");
    if (d->residual == 2 && batch != 1) return bad("the in-place residual takes batch 1");
    // extents (in floats, from the start of each matrix) and the arrays that hold them
    const int64_t extA = (int64_t)(M - 1) * d->lda + K, extB = (int64_t)(N - 1) * d->ldb + K;
    const int64_t extC = (int64_t)(rows_c - 1) * d->ldc + cols_c, extR = (int64_t)(M - 1) * ldr + N;
    const int64_t sA = batch > 1 ? d->strideA : 0, sB = batch > 1 ? d->strideB : 0, sC = batch > 1 ? d->strideC : 0;
    if (sA < 0 || sB < 0 || sA > HOST_CAP || sB > HOST_CAP || sC > HOST_CAP || (sA && sA < extA) || (sB && sB < extB)) return bad("strideA, strideB: 0 or at least one matrix");
    if (batch > 1 && sC < extC) return bad("batch entries of C overlap");
    if (d->a_floats > HOST_CAP || d->b_floats > HOST_CAP || d->c_floats > HOST_CAP || d->r_floats > HOST_CAP) return bad("an array of more than 2^28 floats");
    if (d->a_floats < d->a_off + (batch - 1) * sA + extA) return bad("a is shorter than its description");
    if (d->b_floats < (batch - 1) * sB + extB) return bad("b is shorter than its description");
    if (d->c_floats < d->c_off + (batch - 1) * sC + extC) return bad("c is shorter than its description");
    if (d->residual == 1 && d->r_floats < d->r_off + extR) return bad("residual is shorter than its description");
    // what the kernels' comments exclude (kernels.hpp GemmArgs, gemm_common.hpp)
    if (d->split_out < 0 || d->split_out % 32 || d->split_out > N || (d->split_out && kernel == 2)) return bad("split_out: a multiple of 32 up to N, kernels 0 and 1");
    if (tr && (kernel != 0 || has_res || d->split_out || d->bias == 2)) return bad("c_transposed: kernel 0, column bias and activation only");
    if (kernel == 0 && (batch != 1 || N % 32)) return bad("kernel 0 takes batch 1 and whole 32-column weight tiles");
    if (kernel == 0 && !tr && (d->c_off % 4 || d->ldc % 4)) return bad("kernel 0 writes 16-byte pieces: c_off and ldc must be multiples of 4");
    if (d->b_frag32 && (kernel != 2 || batch != 1 || N % 32)) return bad("b_frag32: kernel 2, batch 1, N a multiple of 32");
    const int lay = d->layout, tile = d->tile_rows;
    const bool lay_ok = kernel == 0 ? lay == 0
                                    : (lay == 0 || lay == 8 || lay == 4 || lay == 64 || (kernel == 2 && (lay == 1 || lay == 2 || (lay >= 11 && lay <= 14))));
    const bool tile_ok = kernel == 0 ? (tile == 0 || tile == 32 || tile == 64 || tile == 96 || tile == 128 || tile == 4 || tile == 65) : tile == 0;
    if (!lay_ok || !tile_ok) return bad("layout / tile_rows: not a tile layout of this kernel");

    const int nA = sA ? batch : 1, nB = sB ? batch : 1;
    const int Np = (N + 31) / 32 * 32;
    Stager sg;
    const size_t o_a = sg.arr(a, d->a_floats, 4, UP), o_b = sg.arr(b, d->b_floats, 4, UP), o_c = sg.arr(c, d->c_floats, 4, UP | DOWN);
    const size_t o_r = sg.arr(residual, d->r_floats, 4, UP), o_bias = sg.arr(bias, d->bias == 2 ? M : N, 4, UP);
    // the operands as the kernels read them: split-f16 copies (kernels 0 and 1), float32 fragments (b_frag32)
    const size_t o_as = sg.scratch(kernel != 2 ? (int64_t)nA * M * K : 0, 4);
    const size_t o_bs = sg.scratch(kernel == 0 ? (int64_t)Np * K : kernel == 1 ? (int64_t)nB * N * K : 0, 4);
    const size_t o_bf = sg.scratch(d->b_frag32 ? (int64_t)N * K : 0, 4);
    char* base = nullptr;
    int rc;
    if ((rc = stage_and_upload(h, sg, &base)) != CSS_OK) return rc;
    auto at = [&](size_t o) { return Stager::dev<float>(base, o); };   // (null for an absent array)
    float *ad = at(o_a), *bd = at(o_b), *cd = at(o_c), *as = at(o_as), *bs = at(o_bs), *bf = at(o_bf);

    GemmArgs g{};
    g.A = ad + d->a_off; g.lda = d->lda; g.strideA = sA;
    g.B = bd; g.ldb = d->ldb; g.strideB = sB;
    g.C = cd + d->c_off; g.ldc = d->ldc; g.strideC = sC;
    g.M = M; g.N = N; g.K = K; g.batch = batch;
    g.bias = at(o_bias); g.bias_along_m = d->bias == 2; g.act = d->act;
    g.residual = d->residual == 1 ? at(o_r) + d->r_off : d->residual == 2 ? g.C : nullptr;
    g.ldr = has_res ? ldr : 0; g.alpha = has_res ? d->alpha : 1.f;
    g.split_out = d->split_out; g.c_transposed = tr; g.m_fastest = d->m_fastest != 0; g.nt_store = d->nt_store != 0;
    g.concurrent = d->concurrent != 0;
    if (kernel != 2) {
        // split-f16 copies of the operands, as css_linear_host makes them: rows of K, entries M * K / N * K apart
        for (int z = 0; z < nA; ++z) launch_split_convert(g.A + z * sA, d->lda, as + (int64_t)z * M * K, M, K, K, h->stream);
        if (kernel == 0) launch_split_convert_tiled(bd, d->ldb, bs, N, K, h->stream);
        else for (int z = 0; z < nB; ++z) launch_split_convert(bd + z * sB, d->ldb, bs + (int64_t)z * N * K, N, K, K, h->stream);
        g.A = as; g.lda = K; g.strideA = sA ? (int64_t)M * K : 0;
        g.B = bs; g.ldb = K; g.strideB = sB ? (int64_t)N * K : 0;
        g.split_in = 1; g.b_tiled = kernel == 0;
        g.tile_rows = tile; g.layout = lay;
    } else {
        g.layout = lay;
        if (d->b_frag32) {
            launch_f32_fragments(bd, d->ldb, bf, N, K, h->stream);
            g.B = bf; g.b_frag32 = 1; g.B_rows = bd;
        }
    }
    launch_gemm(g, h->stream);
    return download_all(h, sg, base);
}

}  // extern "C"
