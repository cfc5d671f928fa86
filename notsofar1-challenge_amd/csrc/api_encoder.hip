// include/css_mi355_encoder.h: the kernels of encoder.hip on caller data, one entry per family (unit tests of the arithmetic;
// the companion of css_gemm_host).  Every entry checks first, then stages in h->stage, launches exactly what masknet_lane
// (api_stages.hip) launches, downloads every allocation a launch could have written and synchronises.
#include "api_ctx.hpp"
#include "../../include/css_mi355_encoder.h"

using namespace css;

namespace {

constexpr int64_t HOST_CAP = (int64_t)1 << 28;   // floats per array: far below the kernels' 32-bit buffer offsets

inline size_t pad64(int64_t n) { return (size_t)((n + 63) / 64 * 64); }   // every staged region starts on 256 bytes

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

    HIPCHK(h, hipSetDevice(h->device));
    const size_t f_x = pad64(d->x_floats), f_o = pad64(d->out_floats), f_w = pad64(D);
    int rc;
    if ((rc = ensure(h, h->stage, (f_x + 3 * f_o + 4 * f_w) * sizeof(float))) != CSS_OK) return rc;
    float* xd = (float*)h->stage.p;
    float* yd = xd + f_x;
    float* zd = yd + f_o;
    float* sd = zd + f_o;
    float* wd = sd + f_o;
    float* bd = wd + f_w;
    float* w2d = bd + f_w;
    float* b2d = w2d + f_w;
    hipStream_t st = h->stream;
    HIPCHK(h, hipMemcpyAsync(xd, x, (size_t)d->x_floats * sizeof(float), hipMemcpyHostToDevice, st));
    if (y) HIPCHK(h, hipMemcpyAsync(yd, y, (size_t)d->out_floats * sizeof(float), hipMemcpyHostToDevice, st));
    if (z) HIPCHK(h, hipMemcpyAsync(zd, z, (size_t)d->out_floats * sizeof(float), hipMemcpyHostToDevice, st));
    if (ys) HIPCHK(h, hipMemcpyAsync(sd, ys, (size_t)d->out_floats * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(wd, w, (size_t)D * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(bd, b, (size_t)D * sizeof(float), hipMemcpyHostToDevice, st));
    if (w2) HIPCHK(h, hipMemcpyAsync(w2d, w2, (size_t)(form == 2 ? 6 : D) * sizeof(float), hipMemcpyHostToDevice, st));
    if (b2) HIPCHK(h, hipMemcpyAsync(b2d, b2, (size_t)D * sizeof(float), hipMemcpyHostToDevice, st));
    float* yo = inplace ? xd : (y ? yd : nullptr);
    if (form <= 1) launch_layernorm(xd, yo, ys ? sd : nullptr, wd, bd, rows, D, form, st);
    else if (form == 2) launch_ln_glu(xd, yd, wd, bd, w2d, rows, D, st);
    else launch_layernorm2(xd, yo, wd, bd, z ? zd : nullptr, ys ? sd : nullptr, w2d, b2d, rows, D, st);
    HIPCHK(h, hipMemcpyAsync(x, xd, (size_t)d->x_floats * sizeof(float), hipMemcpyDeviceToHost, st));
    if (y) HIPCHK(h, hipMemcpyAsync(y, yd, (size_t)d->out_floats * sizeof(float), hipMemcpyDeviceToHost, st));
    if (z) HIPCHK(h, hipMemcpyAsync(z, zd, (size_t)d->out_floats * sizeof(float), hipMemcpyDeviceToHost, st));
    if (ys) HIPCHK(h, hipMemcpyAsync(ys, sd, (size_t)d->out_floats * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    HIPCHK(h, hipGetLastError());
    return CSS_OK;
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

    HIPCHK(h, hipSetDevice(h->device));
    const size_t f_x = pad64(d->x_floats), f_o = pad64(d->out_floats), f_w = pad64(D), f_t = pad64((int64_t)taps * D), f_u = pad64(need);
    int rc;
    if ((rc = ensure(h, h->stage, (f_x + 3 * f_o + f_u + 7 * f_w + f_t + 64) * sizeof(float))) != CSS_OK) return rc;
    float* xd = (float*)h->stage.p;
    float* od = xd + f_x;
    float* zd = od + f_o;
    float* sd = zd + f_o;
    float* ud = sd + f_o;            // form 1: the GLU rows between the two kernels
    float* lnwd = ud + f_u;
    float* lnbd = lnwd + f_w;
    float* dwbd = lnbd + f_w;
    float* ald = dwbd + f_w;
    float* bed = ald + f_w;
    float* l2wd = bed + f_w;
    float* l2bd = l2wd + f_w;
    float* wtd = l2bd + f_w;
    float* pwd = wtd + f_t;
    hipStream_t st = h->stream;
    const size_t xb = (size_t)d->x_floats * sizeof(float), ob = (size_t)d->out_floats * sizeof(float), wb = (size_t)D * sizeof(float);
    HIPCHK(h, hipMemcpyAsync(xd, x, xb, hipMemcpyHostToDevice, st));
    if (x_out) HIPCHK(h, hipMemcpyAsync(od, x_out, ob, hipMemcpyHostToDevice, st));
    if (z) HIPCHK(h, hipMemcpyAsync(zd, z, ob, hipMemcpyHostToDevice, st));
    if (zs) HIPCHK(h, hipMemcpyAsync(sd, zs, ob, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(lnwd, ln_w, wb, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(lnbd, ln_b, wb, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(dwbd, dw_b, wb, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(ald, bn_alpha, wb, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(bed, bn_beta, wb, hipMemcpyHostToDevice, st));
    if (ln2_w) HIPCHK(h, hipMemcpyAsync(l2wd, ln2_w, wb, hipMemcpyHostToDevice, st));
    if (ln2_b) HIPCHK(h, hipMemcpyAsync(l2bd, ln2_b, wb, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(wtd, dw_wt, (size_t)taps * D * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(pwd, pw, 6 * sizeof(float), hipMemcpyHostToDevice, st));
    if (form == 0) {
        *launched = launch_conv_module(xd, od, lnwd, lnbd, pwd, wtd, dwbd, ald, bed, l2wd, l2bd, z ? zd : nullptr, zs ? sd : nullptr,
                                       nseg, T, D, taps, st) ? 1 : 0;
    } else {
        launch_ln_glu(xd, ud, lnwd, lnbd, pwd, nseg * T, D, st);
        launch_dwconv(ud, xd, wtd, dwbd, ald, bed, pwd, nseg, T, D, taps, st);
        *launched = 1;
    }
    HIPCHK(h, hipMemcpyAsync(x, xd, xb, hipMemcpyDeviceToHost, st));
    if (x_out) HIPCHK(h, hipMemcpyAsync(x_out, od, ob, hipMemcpyDeviceToHost, st));
    if (z) HIPCHK(h, hipMemcpyAsync(z, zd, ob, hipMemcpyDeviceToHost, st));
    if (zs) HIPCHK(h, hipMemcpyAsync(zs, sd, ob, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    HIPCHK(h, hipGetLastError());
    return CSS_OK;
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

    HIPCHK(h, hipSetDevice(h->device));
    const int N = 3 * D;
    const int64_t qkf_n = mode == 1 ? qk_fragment_floats(nseg, T, H) : 0;
    const int64_t pef_n = mode != 2 ? (int64_t)pe_fragment_tiles(T) * 2048 : 0;
    const size_t f_x = pad64(M * K), f_w = pad64((int64_t)N * K), f_b = pad64(N), f_pe = pad64((int64_t)2 * maxlen * 64);
    const size_t f_q = pad64(d->qkv_floats), f_c = pad64(d->ctx_floats), f_qf = pad64(qkf_n), f_pf = pad64(pef_n);
    int rc;
    //           x, x split   w, w converted   bias  pe, pe split   qkv   ctx   fragments
    if ((rc = ensure(h, h->stage, (2 * f_x + 2 * f_w + f_b + 2 * f_pe + f_q + f_c + f_qf + f_pf) * sizeof(float))) != CSS_OK) return rc;
    float* xd = (float*)h->stage.p;
    float* xs = xd + f_x;
    float* wd = xs + f_x;
    float* wc = wd + f_w;
    float* bd = wc + f_w;
    float* ped = bd + f_b;
    float* pes = ped + f_pe;
    float* qd = pes + f_pe;
    float* cd = qd + f_q;
    float* qkf = cd + f_c;
    float* pef = qkf + f_qf;
    hipStream_t st = h->stream;
    HIPCHK(h, hipMemcpyAsync(xd, x, (size_t)M * K * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(wd, w, (size_t)N * K * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(bd, bias, (size_t)N * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(ped, pe, (size_t)2 * maxlen * 64 * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)qd, (int)d->canary, (size_t)d->qkv_floats, st));
    HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)cd, (int)d->canary, (size_t)d->ctx_floats, st));
    if (qkf_n) HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)qkf, (int)d->canary, (size_t)qkf_n, st));

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
    HIPCHK(h, hipMemcpyAsync(qkv, qd, (size_t)d->qkv_floats * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(ctx, cd, (size_t)d->ctx_floats * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    HIPCHK(h, hipGetLastError());
    return CSS_OK;
}

}  // extern "C"
