// include/css_mi355_encoder.h: the kernels of encoder.hip on caller data, one entry per family (unit tests of the arithmetic;
// the companion of css_gemm_host).  Every entry checks first, then stages in h->stage, launches exactly what masknet_lane
// (api_stages.hip) launches, downloads every allocation a launch could have written and synchronises.
#include "api_ctx.hpp"
#include "api_kernel_stage.hpp"   // (Stager, stage_and_upload, download_all)
#include "../../include/css_mi355_encoder.h"

using namespace css;
using namespace css::kstage;

namespace {

bool ln_width(int D) { return D >= 256 && D <= 1024 && D % 256 == 0; }

}  // namespace

extern "C" {

int css_layernorm_host(css_handle_t h, const CssLayerNormDesc* d, float* x, const float* w, const float* b, const float* w2,
                       const float* b2, float* y, float* z, float* ys) {
    CSS_DRAIN(h);
    if (!h) return CSS_ERR_INVALID_ARG;
    auto bad = [&](const char* what) { return fail(h, CSS_ERR_INVALID_ARG, std::string("css_layernorm_host: ") + what); };
    if (!d || !x || !w || !b) return bad("null argument");
    const int form = d->form, rows = d->rows, D = d->D;
    const bool inplace = d->inplace != 0;
    if (form < 0 || form > 3) return bad("form must be 0 .. 3");
    if (!ln_width(D)) return bad("D must be 256, 512, 768 or 1024");
    if (rows < 1 || (int64_t)rows * D > HOST_CAP) return bad("rows >= 1, rows * D <= 2^28");
    const int64_t need = (int64_t)rows * D;
    if (d->x_floats < need || d->x_floats > HOST_CAP) return bad("x is shorter than its description");
    if ((y || z || ys) && (d->out_floats < need || d->out_floats > HOST_CAP)) return bad("an output is shorter than its description");
    if (inplace && y) return bad("inplace: y must be NULL");
    if (form <= 1 && (z || (!y && !inplace && !ys))) return bad("forms 0 and 1: at least one of y / inplace / ys, no z");
    if (form == 2 && (!w2 || !y || inplace || z || ys)) return bad("form 2: pw and y, nothing else");
    if (form == 3 && (!w2 || !b2 || (!y && !inplace))) return bad("form 3: w2, b2 and y or inplace");
    if (form <= 1 && (w2 || b2)) return bad("forms 0 and 1 take no second weights");

    Stager sg;
    const size_t o_x = sg.arr(x, d->x_floats, 4, UP | DOWN);
    const size_t o_y = sg.arr(y, d->out_floats, 4, UP | DOWN), o_z = sg.arr(z, d->out_floats, 4, UP | DOWN);
    const size_t o_s = sg.arr(ys, d->out_floats, 4, UP | DOWN);
    const size_t o_w = sg.arr(w, D, 4, UP), o_b = sg.arr(b, D, 4, UP);
    const size_t o_w2 = sg.arr(w2, form == 2 ? 6 : D, 4, UP), o_b2 = sg.arr(b2, D, 4, UP);
    char* base = nullptr;
    int rc;
    if ((rc = stage_and_upload(h, sg, &base)) != CSS_OK) return rc;
    auto at = [&](size_t o) { return Stager::dev<float>(base, o); };   // (null for an absent array)
    hipStream_t st = h->stream;
    float *xd = at(o_x), *yd = at(o_y), *yo = inplace ? xd : yd;
    if (form <= 1) launch_layernorm(xd, yo, at(o_s), at(o_w), at(o_b), rows, D, form, st);
    else if (form == 2) launch_ln_glu(xd, yd, at(o_w), at(o_b), at(o_w2), rows, D, st);
    else launch_layernorm2(xd, yo, at(o_w), at(o_b), at(o_z), at(o_s), at(o_w2), at(o_b2), rows, D, st);
    return download_all(h, sg, base);
}

int css_conv_module_host(css_handle_t h, const CssConvModuleDesc* d, float* x, const float* ln_w, const float* ln_b,
                         const float* pw, const float* dw_wt, const float* dw_b, const float* bn_alpha, const float* bn_beta,
                         const float* ln2_w, const float* ln2_b, float* x_out, float* z, float* zs, int32_t* launched) {
    CSS_DRAIN(h);
    if (!h) return CSS_ERR_INVALID_ARG;
    auto bad = [&](const char* what) { return fail(h, CSS_ERR_INVALID_ARG, std::string("css_conv_module_host: ") + what); };
    if (!d || !x || !ln_w || !ln_b || !pw || !dw_wt || !dw_b || !bn_alpha || !bn_beta || !launched) return bad("null argument");
    const int form = d->form, nseg = d->nseg, T = d->T, D = d->D, taps = d->taps;
    if (form < 0 || form > 1) return bad("form must be 0 (fused) or 1 (LayerNorm + GLU, depthwise conv)");
    if (!ln_width(D)) return bad("D must be 256, 512, 768 or 1024");
    if (taps != 17 && taps != 31 && taps != 33) return bad("taps must be 17, 31 or 33");
    if (nseg < 1 || T < 1 || (int64_t)nseg * T * D > HOST_CAP || (int64_t)nseg * T > (1 << 22)) return bad("nseg, T >= 1, nseg * T * D <= 2^28");
    const int64_t need = (int64_t)nseg * T * D;
    if (d->x_floats < need || d->x_floats > HOST_CAP) return bad("x is shorter than its description");
    if ((x_out || z || zs) && (d->out_floats < need || d->out_floats > HOST_CAP)) return bad("an output is shorter than its description");
    if (form == 0 && !x_out) return bad("form 0 writes x_out");
    if (form == 0 && (z || zs) && (!ln2_w || !ln2_b)) return bad("z / zs need ln2_w and ln2_b");
    if (form == 1 && (x_out || z || zs)) return bad("form 1 works in place: x_out, z and zs must be NULL");

    Stager sg;
    const size_t o_x = sg.arr(x, d->x_floats, 4, UP | DOWN), o_o = sg.arr(x_out, d->out_floats, 4, UP | DOWN);
    const size_t o_z = sg.arr(z, d->out_floats, 4, UP | DOWN), o_s = sg.arr(zs, d->out_floats, 4, UP | DOWN);
    const size_t o_u = sg.scratch(form == 1 ? need : 0, 4);   // form 1: the GLU rows between the two kernels
    const size_t o_lnw = sg.arr(ln_w, D, 4, UP), o_lnb = sg.arr(ln_b, D, 4, UP), o_dwb = sg.arr(dw_b, D, 4, UP);
    const size_t o_al = sg.arr(bn_alpha, D, 4, UP), o_be = sg.arr(bn_beta, D, 4, UP);
    const size_t o_l2w = sg.arr(ln2_w, D, 4, UP), o_l2b = sg.arr(ln2_b, D, 4, UP);
    const size_t o_wt = sg.arr(dw_wt, (int64_t)taps * D, 4, UP), o_pw = sg.arr(pw, 6, 4, UP);
    char* base = nullptr;
    int rc;
    if ((rc = stage_and_upload(h, sg, &base)) != CSS_OK) return rc;
    auto at = [&](size_t o) { return Stager::dev<float>(base, o); };   // (null for an absent array)
    hipStream_t st = h->stream;
    if (form == 0) {
        *launched = launch_conv_module(at(o_x), at(o_o), at(o_lnw), at(o_lnb), at(o_pw), at(o_wt), at(o_dwb), at(o_al), at(o_be), at(o_l2w),
                                       at(o_l2b), at(o_z), at(o_s), nseg, T, D, taps, st) ? 1 : 0;
    } else {
        launch_ln_glu(at(o_x), at(o_u), at(o_lnw), at(o_lnb), at(o_pw), nseg * T, D, st);
        launch_dwconv(at(o_u), at(o_x), at(o_wt), at(o_dwb), at(o_al), at(o_be), at(o_pw), nseg, T, D, taps, st);
        *launched = 1;
    }
    return download_all(h, sg, base);
}

int css_attention_host(css_handle_t h, const CssAttentionDesc* d, const float* x, const float* w, const float* bias,
                       const float* pe, float* qkv, float* ctx) {
    CSS_DRAIN(h);
    if (!h) return CSS_ERR_INVALID_ARG;
    auto bad = [&](const char* what) { return fail(h, CSS_ERR_INVALID_ARG, std::string("css_attention_host: ") + what); };
    if (!d || !x || !w || !bias || !pe || !qkv || !ctx) return bad("null argument");
    const int mode = d->mode, nseg = d->nseg, T = d->T, D = d->D, H = d->H, maxlen = d->maxlen, K = d->K;
    if (mode < 0 || mode > 2) return bad("mode must be 0 (exact float32), 1 (split-f16) or 2 (any length)");
    if (!ln_width(D)) return bad("D must be 256, 512, 768 or 1024");
    if (H < 1 || D != 64 * H) return bad("D must be 64 * H");
    if (K < 32 || K % 32 || K > (1 << 16)) return bad("K must be a multiple of 32");
    if (nseg < 1 || T < 1 || maxlen < 1 || maxlen > (1 << 20)) return bad("nseg, T, maxlen >= 1");
    if (mode != 2 && (T < 2 || T > 512)) return bad("modes 0 and 1 take segments of 2 .. 512 frames");
    if (d->split_out < 0 || d->split_out > 1 || (mode != 2 && d->split_out)) return bad("split_out: 0 or 1, mode 2 only");
    const int64_t M = (int64_t)nseg * T;
    // (the fragment epilogue's token -> segment rule is exact for fewer than 4e6 rows: gemm_common.hpp emit_tile_frag)
    if (M > (1 << 21) || M * 3 * D > HOST_CAP || M * K > HOST_CAP) return bad("nseg * T <= 2^21, nseg * T * 3 D and nseg * T * K <= 2^28");
    if (d->x_floats < M * K || d->x_floats > HOST_CAP) return bad("x is shorter than its description");
    if (d->w_floats < (int64_t)3 * D * K || d->w_floats > HOST_CAP) return bad("w is shorter than its description");
    if (d->pe_floats < (int64_t)2 * maxlen * 64 || d->pe_floats > HOST_CAP) return bad("pe is shorter than its description");
    if (d->qkv_floats < M * 3 * D || d->qkv_floats > HOST_CAP) return bad("qkv is shorter than its description");
    if (d->ctx_floats < M * D || d->ctx_floats > HOST_CAP) return bad("ctx is shorter than its description");
    if (mode == 2) {   // launch_relpos_attention_long's own limit: one query's rows must fit the LDS
        if (((size_t)64 + (size_t)T) * sizeof(float) > 150 * 1024) return bad("mode 2: a segment of more than ~ 38 000 frames");
    }

    const int N = 3 * D;
    const int64_t qkf_n = mode == 1 ? qk_fragment_floats(nseg, T, H) : 0;
    const int64_t pef_n = mode != 2 ? (int64_t)pe_fragment_tiles(T) * 2048 : 0;
    Stager sg;
    const int64_t pe_n = (int64_t)2 * maxlen * 64;
    const size_t o_x = sg.arr(x, M * K, 4, UP), o_xs = sg.scratch(M * K, 4);                     // x, x split
    const size_t o_w = sg.arr(w, (int64_t)N * K, 4, UP), o_wc = sg.scratch((int64_t)N * K, 4);   // w, w converted
    const size_t o_b = sg.arr(bias, N, 4, UP);
    const size_t o_pe = sg.arr(pe, pe_n, 4, UP), o_pes = sg.scratch(pe_n, 4);                    // pe, pe split
    // the outputs start as the caller's canary, not as the caller's arrays
    const size_t o_q = sg.filled(d->qkv_floats, d->canary, qkv), o_c = sg.filled(d->ctx_floats, d->canary, ctx);
    const size_t o_qf = sg.filled(qkf_n, d->canary, nullptr), o_pf = sg.scratch(pef_n, 4);       // fragments
    char* base = nullptr;
    int rc;
    if ((rc = stage_and_upload(h, sg, &base)) != CSS_OK) return rc;
    auto at = [&](size_t o) { return Stager::dev<float>(base, o); };
    float *xd = at(o_x), *xs = at(o_xs), *wd = at(o_w), *wc = at(o_wc), *bd = at(o_b), *ped = at(o_pe), *pes = at(o_pes);
    float *qd = at(o_q), *cd = at(o_c), *qkf = at(o_qf), *pef = at(o_pf);
    hipStream_t st = h->stream;

    // the QKV product as masknet_lane's lin() describes it
    GemmArgs g = linear(xd, K, wd, K, bd, qd, N, (int)M, N, K, ACT_NONE);
    if (mode == 1) {
        launch_split_convert(xd, K, xs, M, K, K, st);
        launch_split_convert_tiled(wd, K, wc, N, K, st);
        g.A = xs; g.B = wc; g.split_in = 1; g.b_tiled = 1; g.split_out = N;
        g.range_flag = h->range_flag_dev.as<unsigned int>();
        g.frag_out = qkf; g.frag_D = D; g.frag_T = T; g.frag_heads = H; g.frag_invT = 1.0f / T;
    } else {
        launch_f32_fragments(wd, K, wc, N, K, st);
        g.B = wc; g.b_frag32 = 1; g.B_rows = wd;
    }
    launch_gemm(g, st);
    if (mode == 2) {
        if (!launch_relpos_attention_long(qd, ped, cd, nseg, T, D, H, maxlen, d->split_out, st))
            return fail(h, CSS_ERR_INVALID_ARG, "css_attention_host: the any-length kernel's LDS could not be reserved");
    } else {
        if (mode == 1) launch_split_convert(ped, 64, pes, 2 * (int64_t)maxlen, 64, 64, st);
        launch_pe_fragments(mode == 1 ? pes : ped, pef, T, maxlen, mode, st);
        launch_relpos_attention(qd, mode == 1 ? qkf : nullptr, pef, cd, nseg, T, D, H, maxlen, mode, mode, st);
    }
    return download_all(h, sg, base);
}

}  // extern "C"
