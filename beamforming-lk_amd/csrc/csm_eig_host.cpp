// csm_eig_host.cpp -- step 8 of include/awpu_hip_csm.h on the host: awpu_hip_csm_eig_host, the eigendecomposition by the written
// arithmetic of csm_eig_rule.h, awpu_hip_csm_eig_weigh_host, the weighed matrix H of step 8b, and awpu_hip_csm_eig_map_host, step
// 8c's map of it.  Pure host code with no handle, as the rule states it; the kernels (csm_eig_kernels.hip) take the same
// functions.  A host compiler alone takes this file.
#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC optimize("fp-contract=off")
#endif

#include <vector>

#include "csm_eig_rule.h"
#include "tones_rule.h"  // the twiddles

namespace {

using awpu::CsmZ;

// one bin of step 8a: A and V [U][U] are scratch; lambda [U] is written where the bin converges.  -> solved
bool eig_bin(const float *C, double n, int32_t usable, CsmZ *A, CsmZ *V, double *lambda, int32_t &sweeps) {
    const size_t U = (size_t) usable;
    sweeps = 0;
    // Load
    bool finite = true;
    double trace = 0.0;
    for (size_t a = 0; a < U; a++) {
        for (size_t b = 0; b < a; b++) {
            const CsmZ z = awpu::csm_inv_load(C[(a * U + b) * 2], C[(a * U + b) * 2 + 1], n);
            finite = finite && awpu::csm_inv_finite(z.re) && awpu::csm_inv_finite(z.im);
            A[a * U + b] = z;
            A[b * U + a] = {z.re, -z.im};
        }
        const double d = awpu::csm_inv_load_diag(C[(a * U + a) * 2], n);
        finite = finite && awpu::csm_inv_finite(d);
        A[a * U + a] = {d, 0.0};
        trace = trace + d;
        for (size_t b = 0; b < U; b++) V[a * U + b] = {a == b ? 1.0 : 0.0, 0.0};
    }
    if (!finite || !awpu::csm_eig_trace_ok(trace)) return false;
    const double thr = awpu::csm_eig_threshold(trace, usable);
    // Sweeps
    const int32_t M = usable + (usable & 1), pairs = M / 2;
    std::vector<awpu::CsmEigRotation> rot((size_t) pairs);
    std::vector<int32_t> P((size_t) pairs), Q((size_t) pairs);
    bool converged = false;
    while (!converged && sweeps < awpu::kCsmEigMaxSweeps) {
        sweeps++;
        bool rotated = false;
        for (int32_t round = 0; round < M - 1; round++) {
            for (int32_t i = 0; i < pairs; i++) {
                rot[i].rotates = false;
                if (!awpu::csm_eig_pair(usable, round, i, P[i], Q[i])) continue;
                const size_t p = (size_t) P[i], q = (size_t) Q[i];
                rot[i] = awpu::csm_eig_rotation(A[q * U + p], A[p * U + p].re, A[q * U + q].re, thr);
                rotated = rotated || rot[i].rotates;
            }
            for (int32_t i = 0; i < pairs; i++) {  // phase 1: the columns p and q of A and of V
                if (!rot[i].rotates) continue;
                const awpu::CsmEigRotation &r = rot[i];
                const size_t p = (size_t) P[i], q = (size_t) Q[i];
                for (CsmZ *X : {A, V})
                    for (size_t row = 0; row < U; row++) awpu::csm_eig_columns(r.c, r.s, r.phr, r.phi, X[row * U + p], X[row * U + q]);
            }
            for (int32_t i = 0; i < pairs; i++) {  // phase 2: the rows p and q of A, four entries in closed form
                if (!rot[i].rotates) continue;
                const awpu::CsmEigRotation &r = rot[i];
                const size_t p = (size_t) P[i], q = (size_t) Q[i];
                for (size_t j = 0; j < U; j++)
                    if (j != p && j != q) awpu::csm_eig_rows(r.c, r.s, r.phr, r.phi, A[p * U + j], A[q * U + j]);
                A[p * U + p] = {r.npp, 0.0}, A[q * U + q] = {r.nqq, 0.0};
                A[p * U + q] = {0.0, 0.0}, A[q * U + p] = {0.0, 0.0};
            }
        }
        converged = !rotated;
    }
    if (!converged) return false;
    for (size_t j = 0; j < U; j++) {
        lambda[j] = A[j * U + j].re;
        if (!awpu::csm_eig_fits(lambda[j])) return false;
    }
    return true;
}

}  // namespace

extern "C" int awpu_hip_csm_eig_host(const float *matrix, int32_t block_count, int32_t usable, const awpu_csm_t *c, float *values, float *vectors,
                                     int32_t *solved, int32_t *sweeps) {
    if (!matrix || !values || !vectors || awpu::csm_refusal(c) || block_count < 1 || usable < 1) return AWPU_ERR_INVALID;
    const size_t U = (size_t) usable;
    std::vector<CsmZ> A(U * U), V(U * U);
    std::vector<double> lambda(U);
    for (int32_t kb = 0; kb < c->n_bins; kb++) {
        float *val = values + (size_t) kb * U, *vec = vectors + (size_t) kb * U * U * 2;
        int32_t ran = 0;
        const bool ok = eig_bin(matrix + (size_t) kb * U * U * 2, (double) block_count, usable, A.data(), V.data(), lambda.data(), ran);
        if (ok) {  // Sort and round
            for (size_t j = 0; j < U; j++) {
                size_t rank = 0;
                for (size_t i = 0; i < U; i++) rank += awpu::csm_eig_before(lambda[i], (int32_t) i, lambda[j], (int32_t) j) ? 1 : 0;
                val[rank] = (float) lambda[j];
                for (size_t a = 0; a < U; a++) vec[(rank * U + a) * 2] = (float) V[a * U + j].re, vec[(rank * U + a) * 2 + 1] = (float) V[a * U + j].im;
            }
        } else {  // an unsolved bin: +0 everywhere
            for (size_t i = 0; i < U; i++) val[i] = 0.0f;
            for (size_t i = 0; i < U * U * 2; i++) vec[i] = 0.0f;
        }
        if (solved) solved[kb] = ok ? 1 : 0;
        if (sweeps) sweeps[kb] = ran;
    }
    return AWPU_OK;
}

extern "C" int awpu_hip_csm_eig_weigh_host(const float *values, const float *vectors, int32_t usable, const awpu_csm_t *c, const awpu_csm_eig_t *e,
                                           float *weighed) {
    if (!values || !vectors || !weighed || awpu::csm_refusal(c) || usable < 1 || awpu::csm_eig_refusal(e, usable)) return AWPU_ERR_INVALID;
    if (c->kind != AWPU_CSM_CONVENTIONAL) return AWPU_ERR_INVALID;
    const size_t U = (size_t) usable;
    std::vector<float> w(U);
    for (int32_t kb = 0; kb < c->n_bins; kb++) {
        const float *val = values + (size_t) kb * U, *vec = vectors + (size_t) kb * U * U * 2;
        float *H = weighed + (size_t) kb * U * U * 2;
        for (size_t r = 0; r < U; r++) w[r] = awpu::csm_eig_weight(e->kind, e->n_sources, e->root, (int32_t) r, val[r]);
        for (size_t a = 0; a < U; a++)
            for (size_t b = 0; b <= a; b++) {
                awpu::CsmComplex h{0.0f, 0.0f};
                for (size_t r = 0; r < U; r++)
                    awpu::csm_eig_weigh_step(h, w[r], {vec[(r * U + a) * 2], vec[(r * U + a) * 2 + 1]}, {vec[(r * U + b) * 2], vec[(r * U + b) * 2 + 1]});
                if (b == a) h.im = 0.0f;
                H[(a * U + b) * 2] = h.re, H[(a * U + b) * 2 + 1] = h.im;
                if (b < a) H[(b * U + a) * 2] = h.re, H[(b * U + a) * 2 + 1] = -h.im;
            }
    }
    return AWPU_OK;
}

extern "C" int awpu_hip_csm_eig_map_host(const float *weighed, const int32_t *solved, const int32_t *off, const float *frac, int32_t lut_stride,
                                         int32_t n_pixels, const int32_t *index, int32_t usable, const awpu_csm_t *c, const awpu_csm_eig_t *e,
                                         float *map) {
    if (!weighed || !index || !map || awpu::csm_refusal(c) || usable < 1 || awpu::csm_eig_refusal(e, usable)) return AWPU_ERR_INVALID;
    if (c->kind != AWPU_CSM_CONVENTIONAL) return AWPU_ERR_INVALID;
    if (const int rc = awpu::csm_check_table(off, frac, lut_stride, n_pixels, index, usable)) return rc;
    float tw[awpu::kCsmSamples / 2][2];
    awpu::tones_twiddles(tw);
    const size_t U = (size_t) usable;
    const float uf = (float) usable, scale = awpu::csm_wss(c->window) * 256.0f;
    std::vector<awpu::CsmComplex> s(U), y(U);
    for (int32_t kb = 0; kb < c->n_bins; kb++)
        for (int32_t p = 0; p < n_pixels; p++) {
            const size_t at = (size_t) kb * (size_t) n_pixels + (size_t) p;
            if (solved && !solved[kb]) {  // an unsolved bin: a +0 plane
                map[at] = 0.0f;
                continue;
            }
            for (size_t a = 0; a < U; a++) {  // steps 3 and 4, as awpu_hip_csm_map_host performs them
                const size_t in = (size_t) p * (size_t) lut_stride + (size_t) index[a];
                s[a] = awpu::csm_steer(&tw[0][0], c->bin[kb], off[in], frac[in]);
            }
            const float q = awpu::csm_quadratic(weighed + (size_t) kb * U * U * 2, usable, AWPU_CSM_CONVENTIONAL, s.data(), y.data());
            map[at] = awpu::csm_eig_map_value(e->kind, e->root, c->bin[kb], q, uf, scale);
        }
    return AWPU_OK;
}
