// csm_clean_rule.h -- step 7 of include/awpu_hip_csm.h (awpu_hip_csm_clean.h states it), CLEAN-SC: the argument checks and every
// arithmetic step as a small function that the host definition (csm_clean_host.cpp) and the kernels (csm_clean_kernels.hip) both
// compile, so that host and device perform the same operations on the same operands.  Built like csm_rule.h and
// csm_invert_rule.h: no HIP types, contraction off, every fused operation a written-out fmaf.  The component's term and qs's term
// are step 4's (csm_add_y, csm_add_x); the pick is peel's (peel_key, find_floor_ratio).  Each sum is serial in its own order: who
// runs which row or entry, and when, does not change a bit.
#pragma once

#include "csm_rule.h"
#include "peel_rule.h"  // peel_key: the pick's order

namespace awpu {

constexpr int kCsmCleanMaxSteps = AWPU_CSM_CLEAN_MAX_STEPS;

// what is wrong with a request, or null
inline const char *csm_clean_gain_refusal(float gain) { return gain > 0.0f && gain <= 1.0f ? nullptr : "gain outside (0, 1]"; }
inline const char *csm_clean_refusal(const awpu_csm_clean_t *cl) {
    if (!cl) return "null argument";
    if (cl->steps < 1 || cl->steps > kCsmCleanMaxSteps) return "steps outside [1, 32]";
    if (const char *why = csm_clean_gain_refusal(cl->gain)) return why;
    if (!(cl->stop_ratio >= 0.0f && cl->stop_ratio < 1.0f)) return "stop_ratio outside [0, 1)";
    return nullptr;
}
// of the map request of a clean call: csm_refusal's, and the kind
inline const char *csm_clean_kind_refusal(const awpu_csm_t *c) {
    if (const char *why = csm_refusal(c)) return why;
    return c->kind == AWPU_CSM_CONVENTIONAL ? nullptr : "CLEAN-SC takes AWPU_CSM_CONVENTIONAL alone";
}

AWPU_CSM_HD bool csm_clean_finite(float x) { return __builtin_fabsf(x) <= 3.402823466e38f; }  // (false for a NaN)

// Load: the entry (a, b), b <= a, as D keeps it, from C's; the mirror of an entry b < a
AWPU_CSM_HD CsmComplex csm_clean_load(float re, float im, bool diagonal) { return {re, diagonal ? 0.0f : im}; }
AWPU_CSM_HD CsmComplex csm_clean_mirror(CsmComplex d) { return {d.re, -d.im}; }

// Component: D[a][b] as the rule reads it, from what the ROW b keeps in column a (D[b][a]) -- the exact conjugate off the diagonal,
// (re, +0) on it.  The same bits as the strided read of row a, whichever triangle (a, b) lies in.
AWPU_CSM_HD CsmComplex csm_clean_entry_from_column(float re, float im, bool diagonal) { return {re, diagonal ? 0.0f : -im}; }
// ... one term of v_a = sum_b D[a][b] conj(s_b): step 4's four fmaf
AWPU_CSM_HD void csm_clean_add_v(CsmComplex &v, CsmComplex d, CsmComplex sb) { csm_add_y(v, d.re, d.im, sb); }
// ... one term of qs = sum_a Re(s_a v_a): step 4's two
AWPU_CSM_HD float csm_clean_add_qs(float qs, CsmComplex sa, CsmComplex va) { return csm_add_x(qs, sa, va); }
AWPU_CSM_HD bool csm_clean_qs_ok(float qs) { return qs > 0.0f && csm_clean_finite(qs); }
AWPU_CSM_HD float csm_clean_r(float gain, float qs) {
    AWPU_CSM_NO_CONTRACT
    return gain / qs;
}

// Update of the entry (a, b): t = v_a r, then D -= t conj(v_b); the diagonal's real part alone
AWPU_CSM_HD CsmComplex csm_clean_t(CsmComplex va, float r) {
    AWPU_CSM_NO_CONTRACT
    const float re = va.re * r, im = va.im * r;
    return {re, im};
}
AWPU_CSM_HD void csm_clean_update(CsmComplex &d, CsmComplex t, CsmComplex vb) {
    AWPU_CSM_NO_CONTRACT
    d.re = __builtin_fmaf(-t.re, vb.re, d.re);
    d.re = __builtin_fmaf(-t.im, vb.im, d.re);
    d.im = __builtin_fmaf(-t.im, vb.re, d.im);
    d.im = __builtin_fmaf(t.re, vb.im, d.im);
}
AWPU_CSM_HD float csm_clean_update_diag(float re, CsmComplex t, CsmComplex va) {
    AWPU_CSM_NO_CONTRACT
    re = __builtin_fmaf(-t.re, va.re, re);
    return __builtin_fmaf(-t.im, va.im, re);
}

// Record
AWPU_CSM_HD float csm_clean_removed(float gain, float before) {
    AWPU_CSM_NO_CONTRACT
    return gain * before;
}
AWPU_CSM_HD awpu_csm_clean_step_t csm_clean_unused() { return {-1, 0.0f, 0.0f}; }

// clean[p]: the `removed` of the steps at p, added in step order from +0; and the map's entry
AWPU_CSM_HD float csm_clean_at(const awpu_csm_clean_step_t *steps, int n_steps, int32_t p) {
    AWPU_CSM_NO_CONTRACT
    float c = 0.0f;
    for (int i = 0; i < n_steps; i++)
        if (steps[i].pixel == p) c = c + steps[i].removed;
    return c;
}
AWPU_CSM_HD float csm_clean_map(float clean, float residual) {
    AWPU_CSM_NO_CONTRACT
    return clean + residual;
}

// The pick's verdict on a dirty row's greatest key (peel_key over the row; 0: no pixel) for iteration i: the pixel to step at, or
// -1 where the bin is done.  `first` is set at i == 0.
AWPU_CSM_HD int32_t csm_clean_pick(unsigned long long best, const float *P, int i, float stop_ratio, float *first) {
    if (!best) return -1;
    const int32_t pick = (int32_t) find_key_pixel(best);
    const float before = P[pick];
    if (i == 0) *first = before;
    return before < find_floor_ratio(stop_ratio, *first) ? -1 : pick;
}

}  // namespace awpu
