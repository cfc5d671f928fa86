// include/css_mi355_frontend.h: the kernels of stft.hip and frontend.hip on caller data, one entry per family (unit tests of the
// arithmetic; the companion of api_encoder.hip).  Every entry checks first, then stages in h->stage, makes the launch the path
// makes, downloads every allocation a launch could have written and synchronises.
#include <vector>

#include "api_ctx.hpp"
#include "api_kernel_stage.hpp"   // (Stager, stage_and_upload, download_all)
#include "../../include/css_mi355_frontend.h"

using namespace css;
using namespace css::kstage;

extern "C" {

int css_analysis_host(css_handle_t h, const CssAnalysisDesc* d, const float* x, float* out, float* phase) {
    CSS_DRAIN(h);
    if (!h) return CSS_ERR_INVALID_ARG;
    auto bad = [&](const char* what) { return fail(h, CSS_ERR_INVALID_ARG, std::string("css_analysis_host: ") + what); };
    if (!d || !x || !out) return bad("null argument");
    const int C = d->C, off = d->offset;
    const int64_t t_lo = d->t_lo, t_hi = d->t_hi, row_ld = d->row_ld, xs = d->x_stride;
    if (C < 1 || C > 64) return bad("C must be 1 .. 64");
    if (t_lo < 0) return bad("t_lo must not be negative");
    if (t_hi < t_lo || t_hi > (1 << 20)) return bad("t_lo <= t_hi <= 2^20");
    if (xs < 0 || xs % 2) return bad("x_stride must be even: the kernel reads samples as float2");
    if (t_hi > t_lo && xs < 256 * (t_hi - 1) + 512) return bad("x_stride is shorter than the last frame's end");
    if (off < 0 || off > 3) return bad("offset must be 0 .. 3 floats");
    if (d->window < 0 || d->window > 1) return bad("window must be 0 (hann) or 1 (sqrt_hann / 16)");
    if (row_ld < t_hi || row_ld < 1 || row_ld > (1 << 22)) return bad("row_ld must cover t_hi");
    if ((d->want_phase != 0) != (phase != nullptr)) return bad("phase goes with want_phase");
    if (d->x_floats < (int64_t)C * xs || d->x_floats > HOST_CAP) return bad("x is shorter than its description");
    if (d->out_floats < off + (int64_t)C * 514 * row_ld || d->out_floats > HOST_CAP) return bad("out is shorter than its description");
    if (phase && (d->phase_floats < off + (int64_t)C * 257 * row_ld || d->phase_floats > HOST_CAP))
        return bad("phase is shorter than its description");

    std::vector<float> tab(stft_table_floats());
    stft_build_tables(tab.data(), d->window);
    Stager sg;
    const size_t o_x = sg.arr(x, d->x_floats, 4, UP), o_o = sg.arr(out, d->out_floats, 4, UP | DOWN);
    const size_t o_p = sg.arr(phase, d->phase_floats, 4, UP | DOWN), o_t = sg.arr(tab.data(), (int64_t)tab.size(), 4, UP);
    char* base = nullptr;
    int rc;
    if ((rc = stage_and_upload(h, sg, &base)) != CSS_OK) return rc;
    auto at = [&](size_t o) { return Stager::dev<float>(base, o); };   // (null for an absent array)
    // the phase base carries the plane base's offset: launch_stft_fft decides float4 against scalar stores on `out` alone
    if (!launch_stft_fft(at(o_x), xs, C, t_lo, t_hi, at(o_t), at(o_o) + off, row_ld, h->stream, phase ? at(o_p) + off : nullptr))
        return fail(h, CSS_ERR_HIP, "css_analysis_host: the kernel's LDS could not be reserved");
    return download_all(h, sg, base);
}

int css_features_host(css_handle_t h, const CssFeaturesDesc* d, const float* X, const float* PH, const float* in_bias,
                      const float* in_scale, float* feat) {
    CSS_DRAIN(h);
    if (!h) return CSS_ERR_INVALID_ARG;
    auto bad = [&](const char* what) { return fail(h, CSS_ERR_INVALID_ARG, std::string("css_features_host: ") + what); };
    if (!d || !X || !in_bias || !in_scale || !feat) return bad("null argument");
    const int C = d->C, F = d->F, nseg = d->nseg, T = d->T, hop = d->hop, Kp = d->Kp;
    const CssFeatureCfg& c = d->cfg;
    if (C < 1 || C > 64 || F < 1 || F > 4096) return bad("C must be 1 .. 64, F 1 .. 4096");
    if (T < 2 || T > (1 << 20)) return bad("T must be at least 2 (the unbiased std divides by T - 1)");
    if (nseg < 1 || nseg > 65535 || hop < 1 || d->seg_lo < 0 || d->seg_lo > (1 << 24)) return bad("nseg 1 .. 65535, hop >= 1, seg_lo >= 0");
    if (c.num_pairs < 0 || c.num_pairs > CSS_MAX_IPD_PAIRS) return bad("at most 16 IPD pairs");
    for (int p = 0; p < c.num_pairs; ++p)
        if (c.pair_l[p] < 0 || c.pair_l[p] >= C || c.pair_r[p] < 0 || c.pair_r[p] >= C) return bad("IPD pair index outside [0, C)");
    if (c.ipd_mean_normalize && (c.ipd_mean_normalize_version < 1 || c.ipd_mean_normalize_version > 3))
        return bad("ipd_mean_normalize_version must be 1, 2 or 3");
    const int64_t cols = (int64_t)F * (1 + c.num_pairs);
    if (Kp < cols) return bad("Kp must be at least F (1 + pairs)");
    if (d->split_out < 0 || d->split_out > 1 || (d->split_out && Kp % 32)) return bad("split_out: 0 or 1, and Kp % 32 == 0 with it");
    if (d->stft_frames < 0 || d->T_ld < 1 || d->stft_frames > d->T_ld) return bad("0 <= stft_frames <= T_ld");
    const int64_t x_need = (int64_t)C * 2 * F * d->T_ld, f_need = (int64_t)nseg * T * Kp;
    if (x_need > HOST_CAP || f_need > HOST_CAP) return bad("C * 2 F * T_ld and nseg * T * Kp <= 2^28");
    if (d->x_floats < x_need || d->x_floats > HOST_CAP) return bad("X is shorter than its description");
    if (PH && (d->ph_floats < x_need / 2 || d->ph_floats > HOST_CAP)) return bad("PH is shorter than its description");
    if (d->feat_floats < f_need || d->feat_floats > HOST_CAP) return bad("feat is shorter than its description");

    FeatOpts o{};
    o.log_mag = c.log_spectrogram != 0; o.mvn = c.mvn_spectrogram != 0; o.ipd_norm = c.ipd_mean_normalize != 0;
    o.ipd_version = c.ipd_mean_normalize_version; o.ipd_cos = c.ipd_cos != 0; o.num_pairs = c.num_pairs;
    for (int p = 0; p < c.num_pairs; ++p) { o.pair_l[p] = (unsigned char)c.pair_l[p]; o.pair_r[p] = (unsigned char)c.pair_r[p]; }

    Stager sg;
    const size_t o_x = sg.arr(X, d->x_floats, 4, UP), o_p = sg.arr(PH, d->ph_floats, 4, UP);
    const size_t o_b = sg.arr(in_bias, cols, 4, UP), o_s = sg.arr(in_scale, cols, 4, UP);
    const size_t o_f = sg.arr(feat, d->feat_floats, 4, UP | DOWN);
    char* base = nullptr;
    int rc;
    if ((rc = stage_and_upload(h, sg, &base)) != CSS_OK) return rc;
    auto at = [&](size_t o) { return Stager::dev<float>(base, o); };   // (null for an absent array)
    launch_features(at(o_x), d->T_ld, d->stft_frames, C, F, at(o_f), Kp, at(o_b), at(o_s), d->seg_lo, nseg, T, hop, d->split_out, o, h->stream,
                    at(o_p));
    return download_all(h, sg, base);
}

int css_synthesis_tail_host(css_handle_t h, const CssSynthesisTailDesc* d, const float* in, float* out) {
    CSS_DRAIN(h);
    if (!h) return CSS_ERR_INVALID_ARG;
    auto bad = [&](const char* what) { return fail(h, CSS_ERR_INVALID_ARG, std::string("css_synthesis_tail_host: ") + what); };
    if (!d || !in || !out) return bad("null argument");
    const int form = d->form;
    if (form < 0 || form > 2) return bad("form must be 0 (wave_ola), 1 (join_shards) or 2 (planes_to_rows)");
    if (d->in_floats < 1 || d->in_floats > HOST_CAP || d->out_floats < 1 || d->out_floats > HOST_CAP) return bad("in_floats, out_floats: 1 .. 2^28");
    if (form == 0) {
        if (d->B < 1 || d->B > 65535 || d->hop < 1 || d->L < 1 || d->L > (1 << 16) || d->hop > d->L) return bad("form 0: B >= 1, 1 <= hop <= L <= 2^16");
        if (d->T_frames < 0 || d->T_frames > (1 << 24)) return bad("form 0: T_frames 0 .. 2^24");
        if (d->q_lo < d->out_q0) return bad("form 0: q_lo must not lie before out_q0");
        if (d->q_hi < d->q_lo || d->q_hi - d->q_lo > (1 << 24)) return bad("form 0: q_lo <= q_hi");
        if (d->f_hi > d->f_lo && (d->f_lo < 0 || d->f_hi > d->T_frames)) return bad("form 0: frames [f_lo, f_hi) outside [0, T_frames)");
        if (d->out_ld < 1) return bad("form 0: out_ld >= 1");
        if (d->has_level < 0 || d->has_level > 1) return bad("form 0: has_level is 0 or 1");
        if (d->in_floats < (int64_t)d->B * d->T_frames * d->L) return bad("form 0: G is shorter than its description");
        if (d->out_floats < (int64_t)d->B * d->out_ld) return bad("form 0: out is shorter than its description");
    } else if (form == 1) {
        if (d->world < 1 || d->world > 64 || d->S < 1 || d->S > 65535) return bad("form 1: world 1 .. 64, S >= 1");
        if (d->hop < 4 || d->hop % 4 || d->ld < 4 || d->ld % 4) return bad("form 1: hop and ld must be multiples of 4 (float4 reads)");
        if (d->n_out < 1 || d->out_ld < d->n_out) return bad("form 1: 1 <= n_out <= out_ld");
        for (int k = 0; k < d->world; ++k) {
            if (d->t_lo[k] < 0 || d->t_hi[k] < d->t_lo[k]) return bad("form 1: 0 <= t_lo <= t_hi for every rank");
            if (d->t_hi[k] > d->t_lo[k] && (d->t_hi[k] - d->t_lo[k] + 1) * d->hop > d->ld) return bad("form 1: a rank's blocks t_lo .. t_hi do not fit ld");
        }
        if (d->in_floats < (int64_t)d->world * d->S * d->ld) return bad("form 1: gathered is shorter than its description");
        if (d->out_floats < (int64_t)d->S * d->out_ld) return bad("form 1: out is shorter than its description");
    } else {
        if (d->B < 1 || d->B > 65535 || d->F2 < 1 || d->KIp < d->F2 || d->KIp > (1 << 20)) return bad("form 2: B >= 1, 1 <= F2 <= KIp");
        if (d->T_frames < 1 || d->T_frames > (1 << 24)) return bad("form 2: T_frames >= 1");
        if (d->in_floats < (int64_t)d->B * d->F2 * d->T_frames) return bad("form 2: planes is shorter than its description");
        if (d->out_floats < (int64_t)d->B * d->T_frames * d->KIp) return bad("form 2: rows is shorter than its description");
    }

    const uint32_t level = d->level;
    Stager sg;
    const size_t o_i = sg.arr(in, d->in_floats, 4, UP), o_o = sg.arr(out, d->out_floats, 4, UP | DOWN), o_lv = sg.arr(&level, 1, 4, UP);
    char* base = nullptr;
    int rc;
    if ((rc = stage_and_upload(h, sg, &base)) != CSS_OK) return rc;
    const float* id = Stager::dev<float>(base, o_i);
    float* od = Stager::dev<float>(base, o_o);
    unsigned int* lv = Stager::dev<unsigned int>(base, o_lv);
    hipStream_t st = h->stream;
    if (form == 0)
        launch_wave_ola(id, od, d->B, d->T_frames, d->hop, d->L, d->q_lo, d->q_hi, d->f_lo, d->f_hi, d->out_ld, d->out_q0,
                        d->has_level ? lv : nullptr, st);
    else if (form == 1)
        launch_join_shards(id, d->ld, d->t_lo, d->t_hi, d->world, d->S, d->hop, d->n_out, od, d->out_ld, st);
    else
        launch_planes_to_rows(id, od, d->B, d->F2, d->T_frames, d->KIp, st);
    return download_all(h, sg, base);
}

int css_pcm_edges_host(css_handle_t h, const CssPcmEdgesDesc* d, const void* in, void* out, uint32_t* peak) {
    CSS_DRAIN(h);
    if (!h) return CSS_ERR_INVALID_ARG;
    auto bad = [&](const char* what) { return fail(h, CSS_ERR_INVALID_ARG, std::string("css_pcm_edges_host: ") + what); };
    if (!d || !in) return bad("null argument");
    const int form = d->form, C = d->C, S = d->S;
    if (form < 0 || form > 5) return bad("form must be 0 .. 5");
    const bool is_peak = form == 3 || form == 4;
    if (is_peak ? (out != nullptr || !peak) : !out) return bad("forms 3 and 4 take peak and no out, the others out");
    if (form == 5 && !peak) return bad("form 5 writes the peaks");
    if (d->in_elems < 1 || d->in_elems > HOST_CAP) return bad("in_elems: 1 .. 2^28");
    if (!is_peak && (d->out_elems < 1 || d->out_elems > HOST_CAP)) return bad("out_elems: 1 .. 2^28");
    const int64_t n = d->n;
    size_t in_size = sizeof(float), out_size = sizeof(float);
    if (form <= 2) {
        if (C < 1 || C > 64 || n < 1) return bad("C 1 .. 64, n >= 1");
        if (d->in_elems < n * C) return bad("in is shorter than its description");
        if (form != 0) in_size = sizeof(int16_t);
        if (form == 1) {
            if (d->out_elems < n * C) return bad("out is shorter than its description");
        } else {
            if (d->i_lo < 0 || d->i_hi < d->i_lo || d->i_hi > d->n_pad) return bad("0 <= i_lo <= i_hi <= n_pad");
            if (d->out_elems < (int64_t)C * d->n_pad) return bad("out is shorter than its description");
            if (form == 0 && (d->split_out < 0 || d->split_out > 1 || (d->split_out && d->n_pad % 32)))
                return bad("split_out: 0 or 1, and n_pad % 32 == 0 with it");
        }
    } else if (is_peak) {
        if (d->src_offset < 0 || d->src_offset > 7) return bad("src_offset must be 0 .. 7 elements");
        if (d->count < 1 || d->in_elems < d->src_offset + d->count) return bad("in is shorter than src_offset + count");
        if (form == 4) in_size = sizeof(int16_t);
    } else {
        if (S < 1 || S > 65535 || n < 1) return bad("form 5: S >= 1, n >= 1");
        if (d->out_ld < n) return bad("form 5: out_ld must cover n");
        if (d->in_elems < (int64_t)S * n) return bad("form 5: wav is shorter than its description");
        if (d->out_elems < (int64_t)S * d->out_ld) return bad("form 5: out is shorter than its description");
        out_size = sizeof(int16_t);
    }

    const size_t n_pk = form == 5 ? (size_t)S : 1;
    const uint32_t before = d->peak_before;
    Stager sg;
    const size_t o_i = sg.arr(in, d->in_elems, in_size, UP), o_o = sg.arr(out, d->out_elems, out_size, UP | DOWN);
    // the peak words: forms 3 and 4 start from peak_before, form 5 writes every one; all return them where the caller asks
    const size_t o_pk = sg.region(n_pk * sizeof(unsigned int), is_peak ? &before : nullptr, peak);
    char* base = nullptr;
    int rc;
    if ((rc = stage_and_upload(h, sg, &base)) != CSS_OK) return rc;
    char *id = base + o_i, *od = Stager::dev<char>(base, o_o);
    unsigned int* pk = Stager::dev<unsigned int>(base, o_pk);
    hipStream_t st = h->stream;
    switch (form) {
    case 0: launch_deinterleave((const float*)id, (float*)od, n, C, d->n_pad, d->i_lo, d->i_hi, d->split_out, st); break;
    case 1: launch_pcm16_to_float((const int16_t*)id, (float*)od, n, C, st); break;
    case 2: launch_pcm16_to_channel_major((const int16_t*)id, (float*)od, n, C, d->n_pad, d->i_lo, d->i_hi, st); break;
    case 3: launch_pcm_peak_f32((const float*)id + d->src_offset, d->count, pk, st); break;
    case 4: launch_pcm_peak_i16((const int16_t*)id + d->src_offset, d->count, pk, st); break;
    default: launch_encode_pcm16((const float*)id, S, n, pk, (int16_t*)od, d->out_ld, st); break;
    }
    return download_all(h, sg, base);
}

}  // extern "C"
