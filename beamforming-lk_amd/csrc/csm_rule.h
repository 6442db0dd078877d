// csm_rule.h -- the rule of include/awpu_hip_csm.h: the argument checks, and every arithmetic step as a small function that the
// host definition (csm_host.cpp), the kernels (csm_kernels.hip) and the stand-alone checker (tests/host/csm_rule_check.cpp) all
// compile, so that host and device perform the same operations on the same operands.  No HIP types: a host compiler alone takes
// it (AWPU_CSM_HD is empty there).  Every fused operation is a written-out fmaf; nothing else may be fused: the functions switch
// contraction off for clang, and host users switch it off for GCC (#pragma GCC optimize at their top).
#pragma once

#include <cstddef>
#include <cstdint>

#include "awpu_hip_csm.h"

#if defined(__HIPCC__)
#define AWPU_CSM_HD __host__ __device__ inline
#else
#define AWPU_CSM_HD inline
#endif
#if defined(__clang__)
#define AWPU_CSM_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define AWPU_CSM_NO_CONTRACT
#endif

namespace awpu {

constexpr int kCsmSamples = 256;  // a block, and the transform's length
constexpr int kCsmMaxBins = AWPU_CSM_MAX_BINS;

struct CsmComplex {
    float re, im;
};

// what is wrong with a request, or null
inline const char *csm_refusal(const awpu_csm_t *c) {
    if (!c) return "null argument";
    if (c->window != AWPU_TONES_RECT && c->window != AWPU_TONES_HANN) return "window is AWPU_TONES_RECT or AWPU_TONES_HANN";
    if (c->n_bins < 1 || c->n_bins > kCsmMaxBins) return "n_bins lies in [1, 8]";
    if (c->bin[0] < 0 || c->bin[c->n_bins - 1] > kCsmSamples / 2) return "the bins lie in [0, 128]";
    for (int i = 1; i < c->n_bins; i++)
        if (c->bin[i - 1] >= c->bin[i]) return "the bins are strictly ascending";
    if (c->kind != AWPU_CSM_CONVENTIONAL && c->kind != AWPU_CSM_DIAGONAL_REMOVED && c->kind != AWPU_CSM_CAPON)
        return "kind is AWPU_CSM_CONVENTIONAL, AWPU_CSM_DIAGONAL_REMOVED or AWPU_CSM_CAPON";
    if (!(c->loading >= 0.0f) || c->loading > 3.0e38f) return "loading is finite and not negative";
    return nullptr;
}

// the active list against the streams: AWPU_OK or AWPU_ERR_INVALID
inline int csm_check_mics(int32_t n_streams, const int32_t *index, int32_t usable) {
    if (n_streams < 1 || usable < 1 || !index) return AWPU_ERR_INVALID;
    for (int32_t s = 0; s < usable; s++)
        if (index[s] < 0 || index[s] >= n_streams) return AWPU_ERR_INVALID;
    return AWPU_OK;
}

// the table at the active mics: AWPU_OK or AWPU_ERR_INVALID
inline int csm_check_table(const int32_t *off, const float *frac, int32_t lut_stride, int32_t n_pixels, const int32_t *index, int32_t usable) {
    if (!off || !frac || n_pixels < 1) return AWPU_ERR_INVALID;
    if (const int rc = csm_check_mics(lut_stride, index, usable)) return rc;
    for (int32_t p = 0; p < n_pixels; p++)
        for (int32_t s = 0; s < usable; s++) {
            const size_t at = (size_t) p * (size_t) lut_stride + (size_t) index[s];
            if (!(frac[at] >= 0.0f && frac[at] <= 1.0f) || off[at] < 0) return AWPU_ERR_INVALID;
        }
    return AWPU_OK;
}

inline float csm_wss(int32_t window) { return window == AWPU_TONES_HANN ? 96.0f : 256.0f; }
AWPU_CSM_HD float csm_ck(int32_t k) { return (k == 0 || k == kCsmSamples / 2) ? 1.0f : 2.0f; }

// step 5's divisor of the conventional and the diagonal-removed map
inline float csm_scale(const awpu_csm_t &c, int32_t usable, int32_t n_blocks) {
    AWPU_CSM_NO_CONTRACT
    const int32_t pairs = c.kind == AWPU_CSM_DIAGONAL_REMOVED ? usable * (usable - 1) : usable * usable;
    const float norm = (float) pairs * (float) n_blocks;
    return (csm_wss(c.window) * 256.0f) * norm;
}

// t_j = e^{-j 2 pi j / 256}, j in [0, 255], from the 128-entry table tw [128][2]
AWPU_CSM_HD CsmComplex csm_twiddle(const float *tw, unsigned j) {
    const float re = tw[2 * (j & 127u)], im = tw[2 * (j & 127u) + 1];
    return (j & 128u) ? CsmComplex{-re, -im} : CsmComplex{re, im};
}

// step 1, one sample: v = x w, or (x g) w
AWPU_CSM_HD float csm_stage(float x, float w) {
    AWPU_CSM_NO_CONTRACT
    return x * w;
}
AWPU_CSM_HD float csm_stage(float x, float g, float w) {
    AWPU_CSM_NO_CONTRACT
    const float xg = x * g;
    return xg * w;
}

// step 1, one bin of one block: v[256] staged samples
AWPU_CSM_HD CsmComplex csm_bin(const float *v, const float *tw, int32_t k) {
    AWPU_CSM_NO_CONTRACT
    float re = 0.0f, im = 0.0f;
    for (int i = 0; i < kCsmSamples; i++) {
        const CsmComplex t = csm_twiddle(tw, (unsigned) (k * i) & 255u);
        re = __builtin_fmaf(v[i], t.re, re);
        im = __builtin_fmaf(v[i], t.im, im);
    }
    return {re, im};
}

// step 2, one block into one entry b < a; and into a diagonal entry's real part
AWPU_CSM_HD void csm_add_cross(CsmComplex &c, CsmComplex xa, CsmComplex xb) {
    AWPU_CSM_NO_CONTRACT
    c.re = __builtin_fmaf(xa.re, xb.re, c.re);
    c.re = __builtin_fmaf(xa.im, xb.im, c.re);
    c.im = __builtin_fmaf(xa.im, xb.re, c.im);
    c.im = __builtin_fmaf(-xa.re, xb.im, c.im);
}
AWPU_CSM_HD void csm_add_auto(float &re, CsmComplex xa) {
    AWPU_CSM_NO_CONTRACT
    re = __builtin_fmaf(xa.re, xa.re, re);
    re = __builtin_fmaf(xa.im, xa.im, re);
}

// step 3: s of one (pixel, mic, bin)
AWPU_CSM_HD CsmComplex csm_steer(const float *tw, int32_t k, int32_t off, float frac) {
    AWPU_CSM_NO_CONTRACT
    const unsigned n = 256u - (unsigned) off;
    const float g = (float) k * frac;
    const int gi = (int) g;
    const float gf = g - (float) gi;
    const CsmComplex t = csm_twiddle(tw, ((unsigned) k * n + (unsigned) gi) & 255u);
    const float th = gf * 0.024543693f;
    const float t2 = th * th;
    float cr = __builtin_fmaf(t2, 1.0f / 24.0f, -0.5f);
    cr = __builtin_fmaf(cr, t2, 1.0f);
    float sn = __builtin_fmaf(t2, 1.0f / 120.0f, -1.0f / 6.0f);
    sn = __builtin_fmaf(sn, t2, 1.0f);
    sn = sn * th;
    const float p0 = t.re * cr, p1 = t.im * sn, p2 = t.im * cr, p3 = t.re * sn;
    return {p0 + p1, p2 - p3};
}

// step 4: one term of y_a, and one row's term of x
AWPU_CSM_HD void csm_add_y(CsmComplex &y, float h_re, float h_im, CsmComplex sb) {
    AWPU_CSM_NO_CONTRACT
    y.re = __builtin_fmaf(h_re, sb.re, y.re);
    y.re = __builtin_fmaf(h_im, sb.im, y.re);
    y.im = __builtin_fmaf(h_im, sb.re, y.im);
    y.im = __builtin_fmaf(-h_re, sb.im, y.im);
}
AWPU_CSM_HD float csm_add_x(float x, CsmComplex sa, CsmComplex ya) {
    AWPU_CSM_NO_CONTRACT
    x = __builtin_fmaf(sa.re, ya.re, x);
    return __builtin_fmaf(-sa.im, ya.im, x);
}
AWPU_CSM_HD float csm_q(int32_t kind, float d, float x) {
    AWPU_CSM_NO_CONTRACT
    const float twice = x + x;
    return kind == AWPU_CSM_DIAGONAL_REMOVED ? twice : d + twice;
}

// step 5: scale is csm_scale's (conventional, diagonal-removed) or wss * 256.0f (Capon)
AWPU_CSM_HD float csm_map_value(int32_t kind, int32_t k, float q, float scale) {
    AWPU_CSM_NO_CONTRACT
    const float ck = csm_ck(k);
    if (kind == AWPU_CSM_CAPON) return q > 0.0f ? ck / (scale * q) : 0.0f;
    const float v = (ck * q) / scale;
    return kind == AWPU_CSM_DIAGONAL_REMOVED && v < 0.0f ? 0.0f : v;
}

// steps 3 and 4 of one pixel and bin as the rule reads: H [usable][usable][2]; s and y are scratch [usable]
inline float csm_quadratic(const float *H, int32_t usable, int32_t kind, const CsmComplex *s, CsmComplex *y) {
    AWPU_CSM_NO_CONTRACT
    float d = 0.0f, x = 0.0f;
    for (int32_t a = 0; a < usable; a++) {
        const float *row = H + (size_t) a * (size_t) usable * 2;
        y[a] = {0.0f, 0.0f};
        for (int32_t b = 0; b < a; b++) csm_add_y(y[a], row[2 * b], row[2 * b + 1], s[b]);
        d = d + row[2 * a];
    }
    for (int32_t a = 0; a < usable; a++) x = csm_add_x(x, s[a], y[a]);
    return csm_q(kind, d, x);
}

}  // namespace awpu
