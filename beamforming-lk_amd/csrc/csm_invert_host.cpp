// csm_invert_host.cpp -- step 6a of include/awpu_hip_csm.h on the host: awpu_hip_csm_invert_rule_host, the loaded inverse by the
// written arithmetic of csm_invert_rule.h.  Pure host code with no handle, entry by entry as the rule states it; the kernels
// (csm_invert_kernels.hip) take the same functions.  A host compiler alone takes this file.  (awpu_hip_csm_invert_host in
// csm_host.cpp is the same mathematics in std::complex<double>, with whatever bits the compiler gives it.)
#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC optimize("fp-contract=off")
#endif

#include <vector>

#include "csm_invert_rule.h"

extern "C" int awpu_hip_csm_invert_rule_host(const float *matrix, int32_t block_count, int32_t usable, const awpu_csm_t *c, float *inverse,
                                             int32_t *solved) {
    if (!matrix || !inverse || awpu::csm_refusal(c) || block_count < 1 || usable < 1) return AWPU_ERR_INVALID;
    using awpu::CsmZ;
    const size_t U = (size_t) usable;
    const double n = (double) block_count;
    std::vector<CsmZ> L(U * U), M(U * U);  // the lower triangles
    for (int32_t kb = 0; kb < c->n_bins; kb++) {
        const float *C = matrix + (size_t) kb * U * U * 2;
        float *G = inverse + (size_t) kb * U * U * 2;
        // Load (into L, which the factorisation then replaces entry by entry)
        double trace = 0.0;
        for (size_t a = 0; a < U; a++) {
            for (size_t b = 0; b < a; b++) L[a * U + b] = awpu::csm_inv_load(C[(a * U + b) * 2], C[(a * U + b) * 2 + 1], n);
            L[a * U + a] = {awpu::csm_inv_load_diag(C[(a * U + a) * 2], n), 0.0};
            trace = trace + L[a * U + a].re;
        }
        const double load = awpu::csm_inv_loading(c->loading, trace, usable);
        for (size_t a = 0; a < U; a++) L[a * U + a].re = awpu::csm_inv_loaded(L[a * U + a].re, load);
        // Factor: row a of L from rows 0 .. a-1
        bool ok = true;
        for (size_t a = 0; a < U && ok; a++) {
            for (size_t b = 0; b < a; b++) {
                CsmZ s = L[a * U + b];
                for (size_t j = 0; j < b; j++) awpu::csm_inv_factor_step(s, L[a * U + j], L[b * U + j]);
                L[a * U + b] = awpu::csm_inv_over(s, L[b * U + b].re);
            }
            double sr = L[a * U + a].re;
            for (size_t j = 0; j < a; j++) sr = awpu::csm_inv_factor_step_diag(sr, L[a * U + j]);
            ok = awpu::csm_inv_pivot_ok(sr);
            if (ok) L[a * U + a] = {awpu::csm_inv_pivot(sr), 0.0};
        }
        // Invert the factor: M = L^-1, lower triangular
        for (size_t col = 0; col < U && ok; col++)
            for (size_t a = col; a < U; a++) {
                CsmZ s{a == col ? 1.0 : 0.0, 0.0};
                for (size_t j = col; j < a; j++) awpu::csm_inv_solve_step(s, L[a * U + j], M[j * U + col]);
                M[a * U + col] = awpu::csm_inv_over(s, L[a * U + a].re);
            }
        // G = M^H M, rounded to float and mirrored
        for (size_t a = 0; a < U && ok; a++)
            for (size_t b = 0; b <= a && ok; b++) {
                CsmZ s{0.0, 0.0};
                for (size_t j = a; j < U; j++) awpu::csm_inv_gram_step(s, M[j * U + a], M[j * U + b]);
                ok = awpu::csm_inv_gram_ok(s);
                const float re = (float) s.re, im = b < a ? (float) s.im : 0.0f;
                G[(a * U + b) * 2] = re, G[(a * U + b) * 2 + 1] = im;
                if (b < a) G[(b * U + a) * 2] = re, G[(b * U + a) * 2 + 1] = -im;
            }
        if (!ok)  // an unsolved bin: +0 everywhere
            for (size_t i = 0; i < U * U * 2; i++) G[i] = 0.0f;
        if (solved) solved[kb] = ok ? 1 : 0;
    }
    return AWPU_OK;
}
