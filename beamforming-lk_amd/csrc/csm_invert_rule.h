// csm_invert_rule.h -- step 6a of include/awpu_hip_csm.h, the loaded inverse with a written arithmetic: every step as a small
// function that the host definition (csm_invert_host.cpp), the kernels (csm_invert_kernels.hip) and the stand-alone checker
// (tests/host/csm_invert_check.cpp) all compile, so that host and device perform the same operations on the same operands.  Built
// like csm_rule.h: no HIP types, contraction off, every fused operation a written-out __builtin_fma on doubles; `/` and sqrt are
// the IEEE double operations.  Each entry's sum is serial in ascending j: who runs which entry, and when, does not change a bit.
#pragma once

#include "csm_rule.h"

namespace awpu {

constexpr int kCsmInvertMaxUsable = AWPU_CSM_INVERT_MAX_MICS;  // the handle forms' bound

struct CsmZ {
    double re, im;
};

AWPU_CSM_HD bool csm_inv_finite(double x) { return __builtin_fabs(x) <= 1.7976931348623157e308; }  // (false for a NaN)

// Load: A[a][b] for b < a, and the diagonal's real part before loading; n = (double) block_count
AWPU_CSM_HD CsmZ csm_inv_load(float re, float im, double n) {
    AWPU_CSM_NO_CONTRACT
    return {(double) re / n, (double) im / n};
}
AWPU_CSM_HD double csm_inv_load_diag(float re, double n) {
    AWPU_CSM_NO_CONTRACT
    return (double) re / n;
}
// load = (double) loading * (trace / (double) U), trace the plain sum of the unloaded diagonal, a ascending from 0
AWPU_CSM_HD double csm_inv_loading(float loading, double trace, int32_t usable) {
    AWPU_CSM_NO_CONTRACT
    const double mean = trace / (double) usable;
    return (double) loading * mean;
}
AWPU_CSM_HD double csm_inv_loaded(double diag, double load) {
    AWPU_CSM_NO_CONTRACT
    return diag + load;
}

// Factor, one step j of the entry (a, b): l = L[a][j], m = L[b][j]; the diagonal's step forms no imaginary part (m = l)
AWPU_CSM_HD void csm_inv_factor_step(CsmZ &s, CsmZ l, CsmZ m) {
    AWPU_CSM_NO_CONTRACT
    s.re = __builtin_fma(-l.re, m.re, s.re);
    s.re = __builtin_fma(-l.im, m.im, s.re);
    s.im = __builtin_fma(-l.im, m.re, s.im);
    s.im = __builtin_fma(l.re, m.im, s.im);
}
AWPU_CSM_HD double csm_inv_factor_step_diag(double sr, CsmZ l) {
    AWPU_CSM_NO_CONTRACT
    sr = __builtin_fma(-l.re, l.re, sr);
    return __builtin_fma(-l.im, l.im, sr);
}
// the pivot of column a: whether the bin can go on, and L[a][a]
AWPU_CSM_HD bool csm_inv_pivot_ok(double sr) { return sr > 0.0 && csm_inv_finite(sr); }
AWPU_CSM_HD double csm_inv_pivot(double sr) { return __builtin_sqrt(sr); }
// L[a][b] = s / L[b][b], and M[a][col] = s / L[a][a]: both parts divided by the real diagonal
AWPU_CSM_HD CsmZ csm_inv_over(CsmZ s, double d) {
    AWPU_CSM_NO_CONTRACT
    return {s.re / d, s.im / d};
}

// Invert the factor, one step j of the entry (a, col): l = L[a][j], m = M[j][col]; the sum starts from (a == col ? 1 : 0, 0)
AWPU_CSM_HD void csm_inv_solve_step(CsmZ &s, CsmZ l, CsmZ m) {
    AWPU_CSM_NO_CONTRACT
    s.re = __builtin_fma(-l.re, m.re, s.re);
    s.re = __builtin_fma(l.im, m.im, s.re);
    s.im = __builtin_fma(-l.re, m.im, s.im);
    s.im = __builtin_fma(-l.im, m.re, s.im);
}

// G = M^H M, one step j of the entry (a, b): u = M[j][a], v = M[j][b]; the sum starts from 0
AWPU_CSM_HD void csm_inv_gram_step(CsmZ &s, CsmZ u, CsmZ v) {
    AWPU_CSM_NO_CONTRACT
    s.re = __builtin_fma(u.re, v.re, s.re);
    s.re = __builtin_fma(u.im, v.im, s.re);
    s.im = __builtin_fma(u.re, v.im, s.im);
    s.im = __builtin_fma(-u.im, v.re, s.im);
}
AWPU_CSM_HD bool csm_inv_gram_ok(CsmZ s) { return csm_inv_finite(s.re) && csm_inv_finite(s.im); }

}  // namespace awpu
