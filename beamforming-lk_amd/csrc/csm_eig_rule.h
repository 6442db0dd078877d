// csm_eig_rule.h -- step 8 of include/awpu_hip_csm.h, the Hermitian eigendecomposition by parallel-order cyclic Jacobi and the two
// subspace maps, with a written arithmetic: every step as a small function that the host definition (csm_eig_host.cpp), the
// kernels (csm_eig_kernels.hip) and the stand-alone checker (tests/host/csm_eig_check.cpp) all compile, so that host and device
// perform the same operations on the same operands.  Built like csm_invert_rule.h, whose load and CsmZ it takes: no HIP types,
// contraction off, every fused operation a written-out __builtin_fma / __builtin_fmaf; `/` and sqrt are the IEEE operations.
// Every stored word comes from one rotation (or one entry's serial sum): who runs which entry, and when, does not change a bit.
#pragma once

#include "csm_invert_rule.h"

namespace awpu {

constexpr int kCsmEigMaxUsable = AWPU_CSM_EIG_MAX_MICS;  // the handle forms' bound
constexpr int kCsmEigMaxSweeps = AWPU_CSM_EIG_MAX_SWEEPS;

// what is wrong with a request, or null
inline const char *csm_eig_refusal(const awpu_csm_eig_t *e, int32_t usable) {
    if (!e) return "null argument";
    if (e->kind != AWPU_CSM_EIG_MUSIC && e->kind != AWPU_CSM_EIG_FUNCTIONAL) return "kind is AWPU_CSM_EIG_MUSIC or AWPU_CSM_EIG_FUNCTIONAL";
    if (e->n_sources < 0 || e->n_sources > usable - 1) return "n_sources lies in [0, usable - 1]";
    if (e->root < 0 || e->root > AWPU_CSM_EIG_MAX_ROOT) return "root lies in [0, 6]";
    if (e->reserved != 0) return "reserved is 0";
    return nullptr;
}

// ---- 8a.  thr = (trace / (double) U) * 2^-52; whether the loaded bin can be solved at all
AWPU_CSM_HD double csm_eig_threshold(double trace, int32_t usable) {
    AWPU_CSM_NO_CONTRACT
    const double mean = trace / (double) usable;
    return mean * 0x1p-52;
}
AWPU_CSM_HD bool csm_eig_trace_ok(double trace) { return trace > 0.0 && csm_inv_finite(trace); }

// The order: M = U + (U & 1) players, M - 1 rounds a sweep, M / 2 pairs a round.  Pair i of round r, as p < q; false where the
// pair holds the dummy of an odd U and is dropped.
AWPU_CSM_HD bool csm_eig_pair(int32_t usable, int32_t round, int32_t i, int32_t &p, int32_t &q) {
    const int32_t M = usable + (usable & 1), m1 = M - 1;
    int32_t a, b;
    if (i == 0) {
        a = m1, b = round;
    } else {
        a = (round + i) % m1, b = (round + m1 - i) % m1;
    }
    p = a < b ? a : b, q = a < b ? b : a;
    return q < usable;
}

// A pair's rotation from beta = A[q][p], app = A[p][p].re and aqq = A[q][q].re as the round finds them.  npp and nqq are the two
// diagonal entries phase 2 writes in closed form.
struct CsmEigRotation {
    double c, s, phr, phi, npp, nqq;
    bool rotates;
};
AWPU_CSM_HD CsmEigRotation csm_eig_rotation(CsmZ beta, double app, double aqq, double thr) {
    AWPU_CSM_NO_CONTRACT
    CsmEigRotation o{1.0, 0.0, 1.0, 0.0, app, aqq, false};
    const double im2 = beta.im * beta.im;
    const double g = __builtin_sqrt(__builtin_fma(beta.re, beta.re, im2));
    if (!(g > thr)) return o;
    o.rotates = true;
    o.phr = beta.re / g, o.phi = beta.im / g;
    const double theta = (aqq - app) / (g + g);
    const double r = __builtin_sqrt(__builtin_fma(theta, theta, 1.0));
    double t = 1.0 / (__builtin_fabs(theta) + r);
    if (theta < 0.0) t = -t;
    o.c = 1.0 / __builtin_sqrt(__builtin_fma(t, t, 1.0));
    o.s = t * o.c;
    o.npp = __builtin_fma(-t, g, app);
    o.nqq = __builtin_fma(t, g, aqq);
    return o;
}

// the two combinations both phases share: x' = c x - s w, y' = s x + c w
AWPU_CSM_HD void csm_eig_combine(double c, double s, CsmZ &x, CsmZ &y, CsmZ w) {
    AWPU_CSM_NO_CONTRACT
    const double swr = s * w.re, swi = s * w.im, cwr = c * w.re, cwi = c * w.im;
    const CsmZ nx{__builtin_fma(c, x.re, -swr), __builtin_fma(c, x.im, -swi)};
    const CsmZ ny{__builtin_fma(s, x.re, cwr), __builtin_fma(s, x.im, cwi)};
    x = nx, y = ny;
}
// Phase 1, columns: x = X[i][p], y = X[i][q], w = y phi
AWPU_CSM_HD void csm_eig_columns(double c, double s, double phr, double phi, CsmZ &x, CsmZ &y) {
    AWPU_CSM_NO_CONTRACT
    const double a = y.im * phi, b = y.im * phr;
    const CsmZ w{__builtin_fma(y.re, phr, -a), __builtin_fma(y.re, phi, b)};
    csm_eig_combine(c, s, x, y, w);
}
// Phase 2, rows of A: x = A[p][j], y = A[q][j], w = y conj(phi)
AWPU_CSM_HD void csm_eig_rows(double c, double s, double phr, double phi, CsmZ &x, CsmZ &y) {
    AWPU_CSM_NO_CONTRACT
    const double a = y.im * phi, b = y.re * phi;
    const CsmZ w{__builtin_fma(y.re, phr, a), __builtin_fma(y.im, phr, -b)};
    csm_eig_combine(c, s, x, y, w);
}

// Sort and round: whether an eigenvalue fits a float, i.e. (float) lambda is finite (false for a NaN, for an infinite double and
// for a finite one that rounds to inf); a bin with one that does not is unsolved
AWPU_CSM_HD bool csm_eig_fits(double lambda) { return csm_inv_finite((double) (float) lambda); }

// Sort: whether eigenvalue i comes before eigenvalue j (descending; equal values keep index order)
AWPU_CSM_HD bool csm_eig_before(double li, int32_t i, double lj, int32_t j) { return li > lj || (li == lj && i < j); }

// ---- 8b.  The weight of eigenvalue r; and one term w u conj(v) of an entry of H
AWPU_CSM_HD float csm_eig_weight(int32_t kind, int32_t n_sources, int32_t root, int32_t r, float lambda) {
    AWPU_CSM_NO_CONTRACT
    if (kind == AWPU_CSM_EIG_MUSIC) return r < n_sources ? 0.0f : 1.0f;
    if (!(lambda > 0.0f)) return 0.0f;
    double w = (double) lambda;
    for (int32_t i = 0; i < root; i++) w = __builtin_sqrt(w);
    return (float) w;
}
AWPU_CSM_HD void csm_eig_weigh_step(CsmComplex &h, float w, CsmComplex u, CsmComplex v) {
    AWPU_CSM_NO_CONTRACT
    const float t = w * u.re;
    h.re = __builtin_fmaf(t, v.re, h.re);
    const float t2 = w * u.im;
    h.re = __builtin_fmaf(t2, v.im, h.re);
    h.im = __builtin_fmaf(t2, v.re, h.im);
    h.im = __builtin_fmaf(-t, v.im, h.im);
}

// ---- 8c.  The map's value from q of the weighed matrix; scale = wss * 256.0f, uf = (float) usable
AWPU_CSM_HD float csm_eig_map_value(int32_t kind, int32_t root, int32_t k, float q, float uf, float scale) {
    AWPU_CSM_NO_CONTRACT
    if (kind == AWPU_CSM_EIG_MUSIC) {
        const float floor = uf * 0x1p-24f;
        return uf / (q > floor ? q : floor);
    }
    float y = (q > 0.0f ? q : 0.0f) / uf;
    for (int32_t i = 0; i < root; i++) y = y * y;
    const float top = csm_ck(k) * y, bottom = scale * uf;
    return top / bottom;
}

}  // namespace awpu
