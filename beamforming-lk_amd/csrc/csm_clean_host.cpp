// csm_clean_host.cpp -- the host functions of include/awpu_hip_csm_clean.h: step 7 of the cross-spectral rule as executable C++,
// pure host code with no handle.  Written for reading, not for speed: row by row and entry by entry, as the rule states it
// (csm_clean_rule.h).  The kernels (csm_clean_kernels.hip) take the same functions lane by lane.  A host compiler alone takes
// this file.
#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC optimize("fp-contract=off")
#endif

#include <cstring>
#include <vector>

#include "csm_clean_rule.h"
#include "tones_rule.h"  // the twiddles

namespace {

using awpu::CsmComplex;

float *entry(float *D, size_t U, size_t a, size_t b) { return D + (a * U + b) * 2; }

// Load, in place or from C: the entries b <= a as D keeps them, and their mirrors
void load(const float *C, float *D, size_t U) {
    for (size_t a = 0; a < U; a++)
        for (size_t b = 0; b <= a; b++) {
            const CsmComplex d = awpu::csm_clean_load(C[(a * U + b) * 2], C[(a * U + b) * 2 + 1], a == b);
            entry(D, U, a, b)[0] = d.re, entry(D, U, a, b)[1] = d.im;
            if (b < a) {
                const CsmComplex m = awpu::csm_clean_mirror(d);
                entry(D, U, b, a)[0] = m.re, entry(D, U, b, a)[1] = m.im;
            }
        }
}

// Component: v [U] and qs of a loaded D and the picked pixel's steering vector s [U]
float component(const float *D, size_t U, const CsmComplex *s, CsmComplex *v) {
    for (size_t a = 0; a < U; a++) {
        v[a] = {0.0f, 0.0f};
        for (size_t b = 0; b < U; b++) awpu::csm_clean_add_v(v[a], {D[(a * U + b) * 2], D[(a * U + b) * 2 + 1]}, s[b]);
    }
    float qs = 0.0f;
    for (size_t a = 0; a < U; a++) qs = awpu::csm_clean_add_qs(qs, s[a], v[a]);
    return qs;
}

// Update of a loaded D with r = gain / qs
void update(float *D, size_t U, const CsmComplex *v, float r) {
    for (size_t a = 0; a < U; a++) {
        const CsmComplex t = awpu::csm_clean_t(v[a], r);
        for (size_t b = 0; b < a; b++) {
            CsmComplex d{entry(D, U, a, b)[0], entry(D, U, a, b)[1]};
            awpu::csm_clean_update(d, t, v[b]);
            const CsmComplex m = awpu::csm_clean_mirror(d);
            entry(D, U, a, b)[0] = d.re, entry(D, U, a, b)[1] = d.im;
            entry(D, U, b, a)[0] = m.re, entry(D, U, b, a)[1] = m.im;
        }
        entry(D, U, a, a)[0] = awpu::csm_clean_update_diag(entry(D, U, a, a)[0], t, v[a]);
        entry(D, U, a, a)[1] = 0.0f;
    }
}

// step 3 of one pixel and bin
void steer(const float *tw, int32_t k, const int32_t *off, const float *frac, int32_t lut_stride, int32_t p, const int32_t *index, size_t U,
           CsmComplex *s) {
    for (size_t a = 0; a < U; a++) {
        const size_t at = (size_t) p * (size_t) lut_stride + (size_t) index[a];
        s[a] = awpu::csm_steer(tw, k, off[at], frac[at]);
    }
}

int check_table(const float *matrix, const int32_t *off, const float *frac, int32_t lut_stride, int32_t n_pixels, const int32_t *index,
                int32_t usable, const awpu_csm_t *c) {
    if (!matrix || !index || awpu::csm_clean_kind_refusal(c)) return AWPU_ERR_INVALID;
    return awpu::csm_check_table(off, frac, lut_stride, n_pixels, index, usable);
}

}  // namespace

extern "C" int awpu_hip_csm_clean_step_host(float *matrix, const int32_t *pixel, float gain, const int32_t *off, const float *frac,
                                            int32_t lut_stride, int32_t n_pixels, const int32_t *index, int32_t usable, const awpu_csm_t *c,
                                            float *component_out, float *qs_out) {
    if (!pixel || awpu::csm_clean_gain_refusal(gain)) return AWPU_ERR_INVALID;
    if (const int rc = check_table(matrix, off, frac, lut_stride, n_pixels, index, usable, c)) return rc;
    float tw[awpu::kCsmSamples / 2][2];
    awpu::tones_twiddles(tw);
    const size_t U = (size_t) usable;
    std::vector<CsmComplex> s(U), v(U);
    for (int32_t kb = 0; kb < c->n_bins; kb++) {
        float *D = matrix + (size_t) kb * U * U * 2;
        load(D, D, U);
        float qs = 0.0f;
        std::fill(v.begin(), v.end(), CsmComplex{0.0f, 0.0f});
        if (pixel[kb] >= 0 && pixel[kb] < n_pixels) {
            steer(&tw[0][0], c->bin[kb], off, frac, lut_stride, pixel[kb], index, U, s.data());
            qs = component(D, U, s.data(), v.data());
            if (awpu::csm_clean_qs_ok(qs)) update(D, U, v.data(), awpu::csm_clean_r(gain, qs));
        }
        if (component_out) std::memcpy(component_out + (size_t) kb * U * 2, v.data(), U * sizeof(CsmComplex));
        if (qs_out) qs_out[kb] = qs;
    }
    return AWPU_OK;
}

extern "C" int awpu_hip_csm_clean_host(const float *matrix, int32_t block_count, const int32_t *off, const float *frac, int32_t lut_stride,
                                       int32_t n_pixels, const int32_t *index, int32_t usable, const awpu_csm_t *c, const awpu_csm_clean_t *cl,
                                       awpu_csm_clean_step_t *steps, float *clean, float *residual, float *map, float *residual_matrix) {
    if (awpu::csm_clean_refusal(cl) || block_count < 1) return AWPU_ERR_INVALID;
    if (!steps && !clean && !residual && !map && !residual_matrix) return AWPU_ERR_INVALID;
    if (const int rc = check_table(matrix, off, frac, lut_stride, n_pixels, index, usable, c)) return rc;
    float tw[awpu::kCsmSamples / 2][2];
    awpu::tones_twiddles(tw);
    const size_t U = (size_t) usable, P = (size_t) n_pixels;
    const float scale = awpu::csm_scale(*c, usable, block_count);
    std::vector<float> D(U * U * 2), row(P);
    std::vector<CsmComplex> S(P * U), v(U), y(U);  // the bin's steering vectors, every pixel's
    std::vector<awpu_csm_clean_step_t> rec((size_t) cl->steps);
    for (int32_t kb = 0; kb < c->n_bins; kb++) {
        const int32_t k = c->bin[kb];
        for (size_t p = 0; p < P; p++) steer(&tw[0][0], k, off, frac, lut_stride, (int32_t) p, index, U, S.data() + p * U);
        const auto dirty_row = [&] {
            for (size_t p = 0; p < P; p++)
                row[p] = awpu::csm_map_value(c->kind, k, awpu::csm_quadratic(D.data(), usable, c->kind, S.data() + p * U, y.data()), scale);
        };
        load(matrix + (size_t) kb * U * U * 2, D.data(), U);
        std::fill(rec.begin(), rec.end(), awpu::csm_clean_unused());
        float first = 0.0f;
        for (int i = 0; i < cl->steps; i++) {
            dirty_row();
            unsigned long long best = 0;
            for (size_t p = 0; p < P; p++) {
                const unsigned long long key = awpu::peel_key(row[p], (uint32_t) p);
                best = key > best ? key : best;
            }
            const int32_t pick = awpu::csm_clean_pick(best, row.data(), i, cl->stop_ratio, &first);
            if (pick < 0) break;
            const float qs = component(D.data(), U, S.data() + (size_t) pick * U, v.data());
            if (!awpu::csm_clean_qs_ok(qs)) break;
            update(D.data(), U, v.data(), awpu::csm_clean_r(cl->gain, qs));
            rec[(size_t) i] = {pick, row[(size_t) pick], awpu::csm_clean_removed(cl->gain, row[(size_t) pick])};
        }
        dirty_row();  // the residual: one more map closes the loop
        if (steps) std::copy(rec.begin(), rec.end(), steps + (size_t) kb * cl->steps);
        for (size_t p = 0; p < P; p++) {
            const float cv = awpu::csm_clean_at(rec.data(), cl->steps, (int32_t) p);
            if (clean) clean[(size_t) kb * P + p] = cv;
            if (residual) residual[(size_t) kb * P + p] = row[p];
            if (map) map[(size_t) kb * P + p] = awpu::csm_clean_map(cv, row[p]);
        }
        if (residual_matrix) std::memcpy(residual_matrix + (size_t) kb * U * U * 2, D.data(), D.size() * sizeof(float));
    }
    return AWPU_OK;
}
