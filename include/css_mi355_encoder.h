/* css_mi355_encoder.h -- the non-GEMM kernels of the mask estimator (csrc/encoder.hip) on caller data.
 *
 * An addition to css_mi355.h (included below; same library, same conventions), the companion of css_gemm_host: one entry per
 * kernel family -- LayerNorm, the conv module, relative-position attention -- for unit tests of the arithmetic; not on the
 * hot path.  Each entry takes caller arrays and a plain descriptor, uploads the inputs and the WHOLE of every output
 * allocation, makes the launches exactly as the mask estimator makes them (api_stages.hip masknet_lane), downloads everything
 * a launch could have written and synchronises, so a caller sees every float a launch did not own.  Whatever a kernel's own
 * comment excludes is refused with CSS_ERR_INVALID_ARG and a message (css_last_error) before anything is launched or
 * written: a NULL handle or descriptor, D not a multiple of 256 or above 1024, D != 64 H, a tap count outside {17, 31, 33},
 * more than 512 frames in the register-resident attention, K % 32, an array shorter than its description.
 * All lengths are in floats; a split-f16 output (split_f16.hpp) has the float count of its float32 form.
 */
#ifndef CSS_MI355_ENCODER_H
#define CSS_MI355_ENCODER_H

#include "css_mi355.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

/* LayerNorm over `rows` rows of D floats (eps 1e-5, biased variance).  form:
 *   0  launch_layernorm:          y = LN(x; w, b)
 *   1  launch_layernorm, relu:    y = max(LN(x; w, b), 0)
 *   2  launch_ln_glu:             u = LN(x; w, b), y = (pw[0] u + pw[1]) sigmoid(pw[2] u + pw[3])     (w2 = pw, 6 floats)
 *   3  launch_layernorm2:         y = LN(x; w, b), z = LN(y; w2, b2)
 * x [x_floats] is uploaded and downloaded again; y, z, ys [out_floats each] are output allocations, each NULL when the
 * launch does not get that pointer.  inplace = 1 passes x as y (forms 0, 1, 3; y must then be NULL).  ys is the split-f16
 * output: of y in forms 0 and 1, of z in form 3.  Forms 0 and 1 need at least one output, form 2 needs y and takes neither
 * inplace nor ys, form 3 needs y (or inplace) and takes z and ys as they come.  z is form 3's alone. */
typedef struct CssLayerNormDesc {
    int32_t form, rows, D, inplace;
    int64_t x_floats, out_floats;
} CssLayerNormDesc;
int css_layernorm_host(css_handle_t h, const CssLayerNormDesc* d, float* x, const float* w, const float* b, const float* w2,
                       const float* b2, float* y, float* z, float* ys);

/* The conv module over nseg adjacent segments of T frames of D channels:
 *   x_out = x + pw[4] relu((dwconv(glu(LN(x; ln_w, ln_b))) + dw_b) bn_alpha + bn_beta) + pw[5]
 * with the operands as the kernels take them: pw [6], dw_wt [taps][D], dw_b, bn_alpha, bn_beta (the folded BatchNorm), and
 * ln2_w, ln2_b of the LayerNorm that follows.  form:
 *   0  launch_conv_module: x -> x_out (required), z / zs = LN(x_out; ln2_w, ln2_b) as float32 / split-f16 rows (each
 *      optional; ln2_w and ln2_b are needed with either).  *launched = 0, CSS_OK and nothing written when (D, taps) is not
 *      covered or the device refused the LDS reservation, else 1.
 *   1  launch_ln_glu + launch_dwconv, in place: the result replaces x; x_out, z and zs must be NULL.  *launched = 1.
 * x [x_floats] is uploaded and downloaded again in both forms; x_out, z, zs [out_floats each]. */
typedef struct CssConvModuleDesc {
    int32_t form, nseg, T, D, taps, reserved;
    int64_t x_floats, out_floats;
} CssConvModuleDesc;
int css_conv_module_host(css_handle_t h, const CssConvModuleDesc* d, float* x, const float* ln_w, const float* ln_b,
                         const float* pw, const float* dw_wt, const float* dw_b, const float* bn_alpha, const float* bn_beta,
                         const float* ln2_w, const float* ln2_b, float* x_out, float* z, float* zs, int32_t* launched);

/* Relative-position attention of nseg segments of T frames, H heads of 64: qkv = x w^T + bias (x [nseg T][K], w [3 D][K],
 * bias [3 D]), then ctx = softmax((q k^T + q pe[clip(i - j, -maxlen, maxlen - 1) + maxlen]^T) / 8) v per segment and head;
 * pe [2 maxlen][64] float32.  mode:
 *   0  exact float32: the float32 QKV product on fragment-ordered weights, launch_pe_fragments(split = 0), the
 *      register-resident kernel on float32 rows, float32 ctx
 *   1  split-f16: x and w converted as css_create converts them, the weights-direct product with split_out = 3 D and the
 *      q and k tiles leaving in operand order (GemmArgs::frag_out), the table through launch_split_convert and
 *      launch_pe_fragments(split = 1), the kernel reading the fragments; split-f16 ctx, and the q and k columns of qkv are
 *      not written
 *   2  the any-length kernel on float32 rows (the float32 QKV product), ctx float32 (split_out = 0) or split-f16 (1)
 * Modes 0 and 1 take 2 <= T <= 512 (css_make_run_cfg's rule and the kernel's 16 key tiles), mode 2 any T >= 1.  Before the
 * product qkv [qkv_floats], ctx [ctx_floats] and the fragment buffer are filled with the word `canary` on the device; both
 * arrays are downloaded whole. */
typedef struct CssAttentionDesc {
    int32_t mode, nseg, T, D, H, maxlen, K, split_out;
    uint32_t canary;
    int32_t reserved;
    int64_t x_floats, w_floats, pe_floats, qkv_floats, ctx_floats;
} CssAttentionDesc;
int css_attention_host(css_handle_t h, const CssAttentionDesc* d, const float* x, const float* w, const float* bias,
                       const float* pe, float* qkv, float* ctx);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CSS_MI355_ENCODER_H */
