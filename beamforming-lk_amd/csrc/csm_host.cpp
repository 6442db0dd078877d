// csm_host.cpp -- the host functions of include/awpu_hip_csm.h: the rule as executable C++, pure host code with no handle (like
// awpu_hip_tones_host), and step 6, the loaded inverse, which exists on the host alone.  Written for reading, not for speed: entry
// by entry, as the rule states it (csm_rule.h).  The kernels (csm_kernels.hip) take the same functions lane by lane.  A host
// compiler alone takes this file.
#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC optimize("fp-contract=off")
#endif

#include <cmath>
#include <complex>
#include <cstring>
#include <vector>

#include "csm_rule.h"
#include "tones_rule.h"  // the two tables

namespace {

using awpu::CsmComplex;
constexpr int N = awpu::kCsmSamples;

struct Tables {
    float w[N], tw[N / 2][2];
    explicit Tables(int32_t window) {
        awpu::tones_window(window, w);
        awpu::tones_twiddles(tw);
    }
    const float *twiddles() const { return &tw[0][0]; }
};

int check_samples(const float *samples, int64_t pitch, int32_t n_streams, int32_t n_blocks, const int32_t *index, int32_t usable, const awpu_csm_t *c) {
    if (!samples || !index || awpu::csm_refusal(c) || n_blocks < 1 || pitch < (int64_t) N * n_blocks) return AWPU_ERR_INVALID;
    return awpu::csm_check_mics(n_streams, index, usable);
}

// step 1 of one block: X [n_bins][usable]
void block_spectra(const float *samples, int64_t pitch, int32_t block, const int32_t *index, int32_t usable, const float *gain, const awpu_csm_t &c,
                   const Tables &t, CsmComplex *X) {
    float v[N];
    for (int32_t a = 0; a < usable; a++) {
        const float *x = samples + (size_t) index[a] * (size_t) pitch + (size_t) block * N;
        for (int i = 0; i < N; i++) v[i] = gain ? awpu::csm_stage(x[i], gain[a], t.w[i]) : awpu::csm_stage(x[i], t.w[i]);
        for (int32_t kb = 0; kb < c.n_bins; kb++) X[(size_t) kb * usable + a] = awpu::csm_bin(v, t.twiddles(), c.bin[kb]);
    }
}

}  // namespace

extern "C" int awpu_hip_csm_spectra_host(const float *samples, int64_t pitch, int32_t n_streams, int32_t n_blocks, const int32_t *index,
                                         int32_t usable, const float *gain, const awpu_csm_t *c, float *spectra) {
    if (!spectra) return AWPU_ERR_INVALID;
    if (const int rc = check_samples(samples, pitch, n_streams, n_blocks, index, usable, c)) return rc;
    const Tables t(c->window);
    static_assert(sizeof(CsmComplex) == 2 * sizeof(float), "spectra are (re, im) pairs");
    for (int32_t b = 0; b < n_blocks; b++)
        block_spectra(samples, pitch, b, index, usable, gain, *c, t, reinterpret_cast<CsmComplex *>(spectra) + (size_t) b * c->n_bins * usable);
    return AWPU_OK;
}

extern "C" int awpu_hip_csm_accumulate_host(const float *samples, int64_t pitch, int32_t n_streams, int32_t n_blocks, const int32_t *index,
                                            int32_t usable, const float *gain, const awpu_csm_t *c, float *matrix, int32_t *block_count) {
    if (!matrix || !block_count) return AWPU_ERR_INVALID;
    if (const int rc = check_samples(samples, pitch, n_streams, n_blocks, index, usable, c)) return rc;
    if (*block_count < 0 || *block_count > INT32_MAX - n_blocks) return AWPU_ERR_INVALID;
    const Tables t(c->window);
    const size_t U = (size_t) usable;
    std::vector<CsmComplex> X((size_t) c->n_bins * U);
    for (int32_t b = 0; b < n_blocks; b++) {
        block_spectra(samples, pitch, b, index, usable, gain, *c, t, X.data());
        for (int32_t kb = 0; kb < c->n_bins; kb++) {
            const CsmComplex *x = X.data() + (size_t) kb * U;
            float *C = matrix + (size_t) kb * U * U * 2;
            for (size_t a = 0; a < U; a++) {
                for (size_t bb = 0; bb < a; bb++) {
                    CsmComplex e{C[(a * U + bb) * 2], C[(a * U + bb) * 2 + 1]};
                    awpu::csm_add_cross(e, x[a], x[bb]);
                    C[(a * U + bb) * 2] = e.re, C[(a * U + bb) * 2 + 1] = e.im;
                    C[(bb * U + a) * 2] = e.re, C[(bb * U + a) * 2 + 1] = -e.im;
                }
                awpu::csm_add_auto(C[(a * U + a) * 2], x[a]);
                C[(a * U + a) * 2 + 1] = 0.0f;
            }
        }
    }
    *block_count += n_blocks;
    return AWPU_OK;
}

extern "C" int awpu_hip_csm_steer_host(const int32_t *off, const float *frac, int32_t lut_stride, int32_t n_pixels, const int32_t *index,
                                       int32_t usable, const awpu_csm_t *c, float *steer) {
    if (!steer || !index || awpu::csm_refusal(c)) return AWPU_ERR_INVALID;
    if (const int rc = awpu::csm_check_table(off, frac, lut_stride, n_pixels, index, usable)) return rc;
    const Tables t(c->window);
    for (int32_t p = 0; p < n_pixels; p++)
        for (int32_t kb = 0; kb < c->n_bins; kb++)
            for (int32_t a = 0; a < usable; a++) {
                const size_t at = (size_t) p * (size_t) lut_stride + (size_t) index[a];
                const CsmComplex s = awpu::csm_steer(t.twiddles(), c->bin[kb], off[at], frac[at]);
                float *dst = steer + (((size_t) p * c->n_bins + kb) * usable + a) * 2;
                dst[0] = s.re, dst[1] = s.im;
            }
    return AWPU_OK;
}

extern "C" int awpu_hip_csm_map_host(const float *matrix, int32_t block_count, const int32_t *off, const float *frac, int32_t lut_stride,
                                     int32_t n_pixels, const int32_t *index, int32_t usable, const awpu_csm_t *c, float *map, float *q) {
    if (!matrix || !index || (!map && !q) || awpu::csm_refusal(c) || block_count < 1) return AWPU_ERR_INVALID;
    if (const int rc = awpu::csm_check_table(off, frac, lut_stride, n_pixels, index, usable)) return rc;
    if (c->kind == AWPU_CSM_DIAGONAL_REMOVED && usable == 1) return AWPU_ERR_INVALID;
    const Tables t(c->window);
    const size_t U = (size_t) usable;
    const float scale = c->kind == AWPU_CSM_CAPON ? awpu::csm_wss(c->window) * 256.0f : awpu::csm_scale(*c, usable, block_count);
    std::vector<CsmComplex> s(U), y(U);
    for (int32_t kb = 0; kb < c->n_bins; kb++)
        for (int32_t p = 0; p < n_pixels; p++) {
            for (size_t a = 0; a < U; a++) {
                const size_t at = (size_t) p * (size_t) lut_stride + (size_t) index[a];
                s[a] = awpu::csm_steer(t.twiddles(), c->bin[kb], off[at], frac[at]);
            }
            const float qv = awpu::csm_quadratic(matrix + (size_t) kb * U * U * 2, usable, c->kind, s.data(), y.data());
            const size_t at = (size_t) kb * (size_t) n_pixels + (size_t) p;
            if (q) q[at] = qv;
            if (map) map[at] = awpu::csm_map_value(c->kind, c->bin[kb], qv, scale);
        }
    return AWPU_OK;
}

// Step 6 in double.  A = L L^H (Cholesky, lower), M = L^-1 by forward substitution, G = M^H M.
extern "C" int awpu_hip_csm_invert_host(const float *matrix, int32_t block_count, int32_t usable, const awpu_csm_t *c, float *inverse) {
    if (!matrix || !inverse || awpu::csm_refusal(c) || block_count < 1 || usable < 1) return AWPU_ERR_INVALID;
    using cd = std::complex<double>;
    const size_t U = (size_t) usable;
    std::vector<float> out((size_t) c->n_bins * U * U * 2);
    std::vector<cd> L(U * U), M(U * U);
    for (int32_t kb = 0; kb < c->n_bins; kb++) {
        const float *C = matrix + (size_t) kb * U * U * 2;
        double trace = 0.0;
        for (size_t a = 0; a < U; a++) {
            for (size_t b = 0; b < a; b++) L[a * U + b] = cd(C[(a * U + b) * 2], C[(a * U + b) * 2 + 1]) / (double) block_count;
            L[a * U + a] = cd((double) C[(a * U + a) * 2] / (double) block_count, 0.0);
            trace += L[a * U + a].real();
        }
        const double load = (double) c->loading * (trace / (double) usable);
        for (size_t a = 0; a < U; a++) L[a * U + a] += load;
        // in place: row a of L from rows 0 .. a-1
        for (size_t a = 0; a < U; a++) {
            for (size_t b = 0; b <= a; b++) {
                cd sum = L[a * U + b];
                for (size_t j = 0; j < b; j++) sum -= L[a * U + j] * std::conj(L[b * U + j]);
                if (b < a) {
                    L[a * U + b] = sum / L[b * U + b].real();
                } else {
                    if (!(sum.real() > 0.0) || !std::isfinite(sum.real())) return AWPU_ERR_RANGE;
                    L[a * U + a] = cd(std::sqrt(sum.real()), 0.0);
                }
            }
        }
        // M = L^-1, lower triangular
        for (size_t col = 0; col < U; col++)
            for (size_t a = col; a < U; a++) {
                cd sum = a == col ? cd(1.0, 0.0) : cd(0.0, 0.0);
                for (size_t j = col; j < a; j++) sum -= L[a * U + j] * M[j * U + col];
                M[a * U + col] = sum / L[a * U + a].real();
            }
        // G[a][b] = sum over j >= a of conj(M[j][a]) M[j][b], for b <= a; mirrored
        float *G = out.data() + (size_t) kb * U * U * 2;
        for (size_t a = 0; a < U; a++)
            for (size_t b = 0; b <= a; b++) {
                cd sum(0.0, 0.0);
                for (size_t j = a; j < U; j++) sum += std::conj(M[j * U + a]) * M[j * U + b];
                if (!std::isfinite(sum.real()) || !std::isfinite(sum.imag())) return AWPU_ERR_RANGE;
                const float re = (float) sum.real(), im = b < a ? (float) sum.imag() : 0.0f;
                G[(a * U + b) * 2] = re, G[(a * U + b) * 2 + 1] = im;
                if (b < a) G[(b * U + a) * 2] = re, G[(b * U + a) * 2 + 1] = -im;
            }
    }
    std::memcpy(inverse, out.data(), out.size() * sizeof(float));
    return AWPU_OK;
}
