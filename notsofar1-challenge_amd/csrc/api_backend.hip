// include/css_mi355_backend.h: the kernels of mvdr.hip and stitch.hip on caller data, one entry per family (unit tests of the
// arithmetic; the companion of api_frontend.hip).  Every entry checks first, then stages in h->stage, makes the launch the path
// makes, downloads every allocation a launch could have written and synchronises.
#include <vector>

#include "api_ctx.hpp"
#include "api_kernel_stage.hpp"   // (Stager, stage_and_upload, download_all)
#include "../../include/css_mi355_backend.h"
#include "../../include/css_mi355_array.h"

using namespace css;
using namespace css::kstage;

namespace {

inline bool is_permutation(const int32_t* p, int S) {
    unsigned seen = 0;
    for (int a = 0; a < S; ++a) {
        if (p[a] < 0 || p[a] >= S || (seen >> p[a] & 1u)) return false;
        seen |= 1u << p[a];
    }
    return true;
}

// css_mvdr_host (ARRAY = false: the 7-microphone kernels and the power normalisation, forms 0 .. 4) and css_mvdr_array_host
// (ARRAY = true: every microphone count of mvdr.hip, forms 0 .. 3): one body, the descriptors have the same members
static_assert(CSS_ARRAY_MAX_SETS == CSS_BACKEND_MAX_SETS && sizeof(CssMvdrArrayDesc) == sizeof(CssMvdrDesc), "one body, one layout");
template <bool ARRAY, class Desc>
int mvdr_host_impl(css_handle_t h, const Desc* d, const float* X, const float* masks, const uint8_t* wta_override,
                   double* scm, double* bfw, float* sep) {
    CSS_DRAIN(h);
    if (!h) return CSS_ERR_INVALID_ARG;
    const char* const name = ARRAY ? "css_mvdr_array_host: " : "css_mvdr_host: ";
    auto bad = [&](const char* what) { return fail(h, CSS_ERR_INVALID_ARG, std::string(name) + what); };
    if (!d) return bad("null argument");
    const int form = d->form, C = d->C, F = d->F, S = d->S, T = d->T, hop = d->hop;
    if (ARRAY ? (form < 0 || form > 3) : (form < 0 || form > 4)) return bad(ARRAY ? "form must be 0 .. 3" : "form must be 0 .. 4");
    const bool need_x = form == 0 || form == 3 || form == 4, need_m = form == 0 || form == 3;
    const bool need_scm = form <= 2, need_bfw = form == 1 || form == 2 || (form == 3 && d->use_mvdr), need_sep = form >= 3;
    if ((need_x && !X) || (need_m && !masks) || (need_scm && !scm) || (need_bfw && !bfw) || (need_sep && !sep)) return bad("null argument");
    if (d->use_mvdr < 0 || d->use_mvdr > 1) return bad("use_mvdr is 0 or 1");
    if (ARRAY) {
        if (C < 2 || C > 8) return bad("C must be 2 .. 8");
    } else if ((form <= 2 || d->use_mvdr) ? C != 7 : (C < 1 || C > 64)) return bad("C must be 7 for the covariances, the solve and the MVDR beamformer (1 .. 64 otherwise)");
    if (S < 1 || S > 3) return bad("S must be 1 .. 3 (S + 1 mask rows in four lane groups)");
    if (F < 1 || F > 4096 || T < 1 || T > 65535 || hop < 1 || hop > (1 << 20)) return bad("F 1 .. 4096, T 1 .. 65535, hop >= 1");
    const int nm = S + 1;
    int64_t segs = 0;   // segments the arrays of a single-set form must hold
    if (form != 2) {
        if (d->nseg < 1 || d->nseg > 4096 || d->seg_lo < 0 || d->seg_lo > (1 << 20)) return bad("nseg 1 .. 4096, seg_lo >= 0");
        segs = d->seg_lo + d->nseg;
    }
    if (need_x) {
        if (d->stft_frames < 0 || d->T_ld < 1 || d->T_ld > HOST_CAP) return bad("stft_frames >= 0, T_ld 1 .. 2^28");
        const int64_t last = std::min<int64_t>(d->stft_frames, (segs - 1) * (int64_t)hop + T);
        if (d->T_ld < last) return bad("T_ld is shorter than the last valid frame");
        const int64_t need = (int64_t)C * 2 * F * d->T_ld;
        if (need > HOST_CAP || d->x_floats < need || d->x_floats > HOST_CAP) return bad("X is shorter than its description");
    }
    if (need_m) {
        if (d->mask_ld < segs * T || d->mask_ld > HOST_CAP) return bad("mask_ld < (seg_lo + nseg) T, or above 2^28");
        const int64_t need = (int64_t)nm * F * d->mask_ld;
        if (need > HOST_CAP || d->mask_floats < need || d->mask_floats > HOST_CAP) return bad("masks is shorter than its description");
    }
    if (form == 0 && wta_override) {
        const int64_t need = segs * F * T;
        if (need > HOST_CAP || d->override_bytes < need || d->override_bytes > HOST_CAP) return bad("the override is shorter than its description");
        for (int64_t i = d->seg_lo * F * T; i < need; ++i) {
            const int v = wta_override[i];
            if (!(v < nm || (v >= 16 && v < 32 && (v & ((1 << nm) - 1))))) return bad("an override byte is neither a winner index below S + 1 nor 16 | bits with a bit below S + 1");
        }
    }
    const int64_t scm_per = (int64_t)nm * F * C * C, bfw_per = (int64_t)S * F * 2 * C, sep_per = (int64_t)S * F * T * 2;
    if (need_scm && (d->scm_doubles < 1 || d->scm_doubles > HOST_CAP)) return bad("scm_doubles: 1 .. 2^28");
    if (need_bfw && (d->bfw_doubles < 1 || d->bfw_doubles > HOST_CAP)) return bad("bfw_doubles: 1 .. 2^28");
    if (need_sep && (d->sep_floats < 1 || d->sep_floats > HOST_CAP)) return bad("sep_floats: 1 .. 2^28");
    if (form == 2) {
        if (d->n_sets < 1 || d->n_sets > CSS_BACKEND_MAX_SETS) return bad("n_sets must be 1 .. 16");
        for (int i = 0; i < d->n_sets; ++i) {
            const auto& s = d->sets[i];
            if (s.nseg < 1 || s.nseg > 4096 || s.seg_lo < 0 || s.seg_lo > (1 << 20) || s.scm_off < 0 || s.bfw_off < 0) return bad("a set: nseg 1 .. 4096, seg_lo >= 0, offsets >= 0");
            if (s.scm_off > HOST_CAP || s.scm_off + (s.seg_lo + s.nseg) * scm_per > d->scm_doubles) return bad("a set's covariances lie outside scm");
            if (s.bfw_off > HOST_CAP || s.bfw_off + (s.seg_lo + s.nseg) * bfw_per > d->bfw_doubles) return bad("a set's weights lie outside bfw");
        }
    } else {
        if (need_scm && d->scm_doubles < segs * scm_per) return bad("scm is shorter than its description");
        if (need_bfw && d->bfw_doubles < segs * bfw_per) return bad("bfw is shorter than its description");
        if (need_sep && d->sep_floats < segs * sep_per) return bad("sep is shorter than its description");
    }

    // an array a form does not take is absent, whatever the caller passed; each form brings back what its launch writes
    Stager sg;
    const size_t o_x = sg.arr(need_x ? X : nullptr, d->x_floats, 4, UP), o_m = sg.arr(need_m ? masks : nullptr, d->mask_floats, 4, UP);
    const size_t o_ov = sg.arr(form == 0 ? wta_override : nullptr, d->override_bytes, 1, UP);
    const size_t o_scm = sg.arr(need_scm ? scm : nullptr, d->scm_doubles, 8, form == 0 ? UP | DOWN : UP);
    const size_t o_bfw = sg.arr(need_bfw ? bfw : nullptr, d->bfw_doubles, 8, form == 1 || form == 2 ? UP | DOWN : UP);
    const size_t o_sep = sg.arr(need_sep ? sep : nullptr, d->sep_floats, 4, UP | DOWN);
    const size_t o_scr = sg.scratch(form == 4 ? d->nseg : 0, 8);
    char* base = nullptr;
    int rc;
    if ((rc = stage_and_upload(h, sg, &base)) != CSS_OK) return rc;
    hipStream_t st = h->stream;

    MvdrArgs a{};
    a.X = Stager::dev<const float>(base, o_x); a.T_ld = d->T_ld; a.stft_frames = d->stft_frames; a.C = C; a.F = F;
    a.masks = Stager::dev<const float>(base, o_m); a.mask_ld = d->mask_ld;
    a.S = S; a.T = T; a.hop = hop; a.seg_lo = d->seg_lo; a.nseg = d->nseg;
    a.wta_override = Stager::dev<const uint8_t>(base, o_ov);
    a.scm = Stager::dev<double>(base, o_scm);
    a.bfw = Stager::dev<double>(base, o_bfw);
    a.sep = Stager::dev<float>(base, o_sep);
    a.mask_floor = d->mask_floor; a.use_mvdr = d->use_mvdr;
    switch (form) {
    case 0:
        if (!launch_scm(a, st)) return fail(h, CSS_ERR_HIP, std::string(name) + "the covariance kernel's LDS could not be reserved");
        break;
    case 1: launch_mvdr_solve(a, st); break;
    case 2: {
        std::vector<MvdrArgs> sets((size_t)d->n_sets, a);
        for (int i = 0; i < d->n_sets; ++i) {
            sets[(size_t)i].seg_lo = d->sets[i].seg_lo; sets[(size_t)i].nseg = (int)d->sets[i].nseg;
            sets[(size_t)i].scm = a.scm + d->sets[i].scm_off; sets[(size_t)i].bfw = a.bfw + d->sets[i].bfw_off;
        }
        launch_mvdr_solve_multi(sets.data(), d->n_sets, st);
        break;
    }
    case 3: launch_beamform(a, st); break;
    default: launch_segment_power_norm(a, Stager::dev<double>(base, o_scr), st); break;
    }
    return download_all(h, sg, base);
}

}  // namespace

extern "C" {

int css_mvdr_host(css_handle_t h, const CssMvdrDesc* d, const float* X, const float* masks, const uint8_t* wta_override,
                  double* scm, double* bfw, float* sep) {
    return mvdr_host_impl<false>(h, d, X, masks, wta_override, scm, bfw, sep);
}

int css_mvdr_array_host(css_handle_t h, const CssMvdrArrayDesc* d, const float* X, const float* masks, const uint8_t* wta_override,
                        double* scm, double* bfw, float* sep) {
    return mvdr_host_impl<true>(h, d, X, masks, wta_override, scm, bfw, sep);
}

int css_stitch_host(css_handle_t h, const CssStitchDesc* d, const float* masks, const float* sep, const float* windows,
                    double* costs, int32_t* perms, float* mask_st, float* activity, uint8_t* act_b, uint8_t* act_tmp,
                    uint8_t* act_final, float* Y) {
    CSS_DRAIN(h);
    if (!h) return CSS_ERR_INVALID_ARG;
    auto bad = [&](const char* what) { return fail(h, CSS_ERR_INVALID_ARG, std::string("css_stitch_host: ") + what); };
    if (!d) return bad("null argument");
    const int form = d->form, S = d->S, F = d->F, T = d->T, hop = d->hop;
    if (form < 0 || form > 5) return bad("form must be 0 .. 5");
    const bool is_cost = form <= 1;
    if (is_cost && (d->loss < 0 || d->loss > 1 || d->input < 0 || d->input > 1)) return bad("loss and input are 0 or 1");
    const bool need_m = (is_cost && d->input == 0) || form == 3, need_sep = (is_cost && d->input == 1) || form == 5;
    const bool need_w = form == 3 || form == 5, need_costs = form <= 2, need_perms = form == 2 || form == 3 || form == 5;
    const bool need_st = form == 3, need_b = form == 3 || form == 4, need_tmp = form == 4, need_fin = form == 4 || form == 5, need_y = form == 5;
    if ((need_m && !masks) || (need_sep && !sep) || (need_w && !windows) || (need_costs && !costs) || (need_perms && !perms) ||
        (need_st && (!mask_st || !activity)) || (need_b && !act_b) || (need_tmp && !act_tmp) || (need_fin && !act_final) || (need_y && !Y))
        return bad("null argument");
    if (S < 1 || S > SMAX) return bad("S must be 1 .. 4");
    if (form != 2 && form != 4) {
        if (F < 1 || F > (form == 5 ? 511 : 4096)) return bad("F must be 1 .. 4096 (1 .. 511 for form 5: the tile's LDS)");
        if (T < 1 || T > 65535 || hop < 1 || hop > T) return bad("T 1 .. 65535, 1 <= hop <= T");
        if (is_cost && hop == T) return bad("hop == T: no overlap, the mean divides by F (T - hop)");
    }
    const int64_t lo = d->lo, hi = d->hi, NS = d->num_segments, TL = d->T_long;
    const int64_t ss = (int64_t)S * S;
    if (form != 1 && form != 2 && form != 4 && (NS < 1 || NS > (1 << 20))) return bad("num_segments: 1 .. 2^20");
    if (need_costs && (d->costs_doubles < 1 || d->costs_doubles > HOST_CAP)) return bad("costs_doubles: 1 .. 2^28");
    if (need_m && (d->mask_floats < 1 || d->mask_floats > HOST_CAP || d->mask_ld < 1 || d->mask_ld > HOST_CAP)) return bad("mask_floats and mask_ld: 1 .. 2^28");
    if (need_sep && (d->sep_floats < 1 || d->sep_floats > HOST_CAP)) return bad("sep_floats: 1 .. 2^28");
    int64_t total_b = 0;    // boundaries the scratch of the cost forms must hold (form 1: all sets, one after the other)
    if (form == 0) {
        if (lo < 0 || hi < lo || hi > NS - 1) return bad("boundaries [lo, hi) outside [0, num_segments - 1]");
        if (d->input == 0 && (d->mask_ld < NS * T || (int64_t)S * F * d->mask_ld > d->mask_floats)) return bad("masks is shorter than its description");
        if (d->input == 1 && NS * S * F * T * 2 > d->sep_floats) return bad("sep is shorter than its description");
        if ((NS - 1) * ss > d->costs_doubles) return bad("costs is shorter than its description");
        total_b = NS - 1;
    } else if (form == 1) {
        if (d->n_sets < 1 || d->n_sets > CSS_BACKEND_MAX_SETS) return bad("n_sets must be 1 .. 16");
        for (int i = 0; i < d->n_sets; ++i) {
            const CssStitchSet& s = d->sets[i];
            if (s.num_segments < 1 || s.num_segments > (1 << 20) || s.mask_off < 0 || s.sep_off < 0 || s.costs_off < 0 || s.sep_off % 2)
                return bad("a set: num_segments >= 1, offsets >= 0, sep_off even");
            if (d->input == 0 && (s.mask_off > HOST_CAP || s.mask_off + ((int64_t)S * F - 1) * d->mask_ld + s.num_segments * T > d->mask_floats))
                return bad("a set's masks lie outside masks");
            if (d->input == 1 && (s.sep_off > HOST_CAP || s.sep_off + s.num_segments * S * F * T * 2 > d->sep_floats)) return bad("a set's spectra lie outside sep");
            if (s.costs_off > HOST_CAP || s.costs_off + (s.num_segments - 1) * ss > d->costs_doubles) return bad("a set's costs lie outside costs");
            total_b += std::max<int64_t>(s.num_segments - 1, 1);
        }
    } else if (form == 2) {
        if (lo < 0 || hi < lo || hi > (1 << 20)) return bad("boundaries: 0 <= lo <= hi <= 2^20");
        if (hi * ss > d->costs_doubles) return bad("costs is shorter than its description");
        if (d->perms_ints < (hi + 1) * S || d->perms_ints > HOST_CAP) return bad("perms is shorter than its description");
        if (lo > 0 && !is_permutation(perms + lo * S, S)) return bad("perms row lo is not a permutation");
    } else {
        if (TL < 1 || TL > (1 << 24)) return bad("T_long: 1 .. 2^24");
        if (lo < 0 || hi < lo || hi > TL) return bad("frames [lo, hi) outside [0, T_long]");
        if ((int64_t)S * TL > HOST_CAP) return bad("S T_long <= 2^28");
        if (form != 4) {
            if (TL > (NS - 1) * (int64_t)hop + T) return bad("T_long lies beyond the segments' coverage");
            if (d->perms_ints < NS * S || d->perms_ints > HOST_CAP) return bad("perms is shorter than its description");
            for (int64_t s = 0; s < NS; ++s)
                if (!is_permutation(perms + s * S, S)) return bad("a perms row is not a permutation");
        }
        if (form == 3) {
            if (d->mask_ld < NS * T || (int64_t)S * F * d->mask_ld > d->mask_floats) return bad("masks is shorter than its description");
            if ((int64_t)S * F * TL > HOST_CAP || d->mask_st_floats < (int64_t)S * F * TL || d->mask_st_floats > HOST_CAP) return bad("mask_st is shorter than its description");
            if (d->activity_floats < S * TL || d->activity_floats > HOST_CAP) return bad("activity is shorter than its description");
        }
        if (form == 4 && (d->dilation < 0 || d->dilation > (1 << 16) || d->erosion < 0 || d->erosion > (1 << 16))) return bad("radii: 0 .. 2^16");
        if (d->act_bytes < S * TL || d->act_bytes > HOST_CAP) return bad("the activity bytes are shorter than their description");
        if (form == 5) {
            if (d->y_split < 0 || d->y_split > 1 || d->has_level < 0 || d->has_level > 1) return bad("y_split and has_level are 0 or 1");
            if (d->KIp < 2 * F || d->KIp > (1 << 16) || (d->y_split && d->KIp % 32)) return bad("KIp >= 2 F, and KIp % 32 == 0 with y_split");
            if (NS * S * F * T * 2 > d->sep_floats) return bad("sep is shorter than its description");
            if ((int64_t)S * TL * d->KIp > HOST_CAP || d->y_floats < (int64_t)S * TL * d->KIp || d->y_floats > HOST_CAP) return bad("Y is shorter than its description");
        }
    }

    // an array a form does not take is absent, whatever the caller passed; each form brings back what its launch writes
    const uint32_t level = d->level;
    Stager sg;
    const size_t o_m = sg.arr(need_m ? masks : nullptr, d->mask_floats, 4, UP), o_sep = sg.arr(need_sep ? sep : nullptr, d->sep_floats, 4, UP);
    const size_t o_w = sg.arr(need_w ? windows : nullptr, 3 * (int64_t)T, 4, UP);
    const size_t o_c = sg.arr(need_costs ? costs : nullptr, d->costs_doubles, 8, is_cost ? UP | DOWN : UP);
    const size_t o_p = sg.arr(need_perms ? perms : nullptr, d->perms_ints, 4, form == 2 ? UP | DOWN : UP);
    const size_t o_st = sg.arr(need_st ? mask_st : nullptr, d->mask_st_floats, 4, UP | DOWN);
    const size_t o_a = sg.arr(need_st ? activity : nullptr, d->activity_floats, 4, UP | DOWN);
    const size_t o_b = sg.arr(need_b ? act_b : nullptr, d->act_bytes, 1, form == 3 ? UP | DOWN : UP);
    const size_t o_t = sg.arr(need_tmp ? act_tmp : nullptr, d->act_bytes, 1, UP | DOWN);
    const size_t o_f = sg.arr(need_fin ? act_final : nullptr, d->act_bytes, 1, form == 4 ? UP | DOWN : UP);
    const size_t o_y = sg.arr(need_y ? Y : nullptr, d->y_floats, 4, UP | DOWN), o_lv = sg.arr(&level, 1, 4, UP);
    const size_t o_scr = sg.scratch(is_cost ? (int64_t)pit_cost_scratch_bytes(total_b) : 0, 1);
    char* base = nullptr;
    int rc;
    if ((rc = stage_and_upload(h, sg, &base)) != CSS_OK) return rc;
    hipStream_t st = h->stream;

    StitchArgs a{};
    a.masks = Stager::dev<const float>(base, o_m); a.mask_ld = d->mask_ld;
    a.sep = Stager::dev<const float>(base, o_sep);
    a.S = S; a.F = F; a.T = T; a.hop = hop; a.num_segments = NS; a.T_long = TL;
    if (need_w) { a.w_first = Stager::dev<const float>(base, o_w); a.w_mid = a.w_first + T; a.w_last = a.w_mid + T; }
    a.perms = Stager::dev<const int32_t>(base, o_p);
    a.mask_st = Stager::dev<float>(base, o_st); a.activity = Stager::dev<float>(base, o_a);
    a.act_b = Stager::dev<uint8_t>(base, o_b); a.act_tmp = Stager::dev<uint8_t>(base, o_t);
    a.act_final = Stager::dev<uint8_t>(base, o_f);
    a.activity_th = d->activity_th; a.dilation = d->dilation; a.erosion = d->erosion;
    a.Y = Stager::dev<float>(base, o_y); a.KIp = d->KIp; a.y_split = d->y_split;
    a.level = form == 5 && d->has_level ? Stager::dev<const unsigned int>(base, o_lv) : nullptr;
    double* cd = Stager::dev<double>(base, o_c);
    switch (form) {
    case 0: launch_pit_costs(a, d->loss, d->input, lo, hi, (double*)(base + o_scr), cd, st); break;
    case 1: {
        std::vector<StitchArgs> sets((size_t)d->n_sets, a);
        std::vector<double*> scr((size_t)d->n_sets), cst((size_t)d->n_sets);
        size_t at = o_scr;
        for (int i = 0; i < d->n_sets; ++i) {
            const CssStitchSet& s = d->sets[i];
            sets[(size_t)i].num_segments = s.num_segments;
            if (need_m) sets[(size_t)i].masks = a.masks + s.mask_off;
            if (need_sep) sets[(size_t)i].sep = a.sep + s.sep_off;
            scr[(size_t)i] = (double*)(base + at); cst[(size_t)i] = cd + s.costs_off;
            at += pit_cost_scratch_bytes(s.num_segments - 1);
        }
        launch_pit_costs_multi(sets.data(), scr.data(), cst.data(), d->n_sets, d->loss, d->input, st);
        break;
    }
    case 2: launch_pit_scan(cd, lo, hi, S, (int32_t*)(base + o_p), st); break;
    case 3: launch_ola_masks(a, lo, hi, st); break;
    case 4: launch_morphology(a, lo, hi, st); break;
    default: launch_ola_stft(a, lo, hi, st); break;
    }
    return download_all(h, sg, base);
}

}  // extern "C"
