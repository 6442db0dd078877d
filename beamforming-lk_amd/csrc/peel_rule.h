// peel_rule.h -- the arithmetic of include/awpu_hip_peel.h that the host definition (peel_host.cpp) and the kernels
// (peel_kernels.hip) share, so that both evaluate the same expressions on the same operands: the lerp, the subtraction, the
// pick's test, a step's close; and, host only, the argument checks, the reach and one step of one frame, written for reading in
// the rule's own order.  No HIP types: a host compiler alone takes it.  Its users switch contraction off for GCC (#pragma GCC
// optimize at their top); for clang the functions below do.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

#include "awpu_hip_peel.h"
#include "find_rule.h"

#if defined(__HIPCC__)
#define AWPU_PEEL_HD __host__ __device__
#else
#define AWPU_PEEL_HD
#endif

namespace awpu {

constexpr int kPeelSamples = 256;  // a block (N_SAMPLES of the reference)

// the delayed sample: delay() of src/dsp/delay.cpp:19-25 on (x[i], x[i+1]); also the beam at i + f from (b[i+1], b[i]) -> (b, a)
AWPU_PEEL_HD inline float peel_lerp(float f, float a, float b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float d = a - b;
    return __builtin_fmaf(f, d, b);
}

// mic sample x with the beam (b0 = b[i], b1 = b[i+1]) taken out
AWPU_PEEL_HD inline float peel_subtract(float u, float f, float b0, float b1, float x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float c = peel_lerp(f, b1, b0);
    return __builtin_fmaf(-u, c, x);
}

// the pick's key: 0 where the pixel cannot be picked (not finite, or not > 0)
AWPU_PEEL_HD inline unsigned long long peel_key(float power, uint32_t pixel) {
    uint32_t bits;
    __builtin_memcpy(&bits, &power, 4);
    const bool takes = power > 0.0f && bits < 0x7F800000u;
    return takes ? find_key(bits, pixel) : 0ull;
}

AWPU_PEEL_HD inline float peel_removed(float before, float after) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float d = before - after;
    return d > 0.0f ? d : 0.0f;
}

// clean[p]: the `removed` of the steps at p, added in step order
AWPU_PEEL_HD inline float peel_clean_at(const awpu_peel_step_t *steps, int n_steps, int32_t p) {
    float c = 0.0f;
    for (int k = 0; k < n_steps; k++)
        if (steps[k].pixel == p) c = c + steps[k].removed;
    return c;
}

// what is wrong with a request, or null
inline const char *peel_gain_refusal(float gain) { return gain > 0.0f && gain <= 1.0f ? nullptr : "loop gain outside (0, 1]"; }
inline const char *peel_refusal(const awpu_peel_t *pe) {
    if (!pe) return "null argument";
    if (pe->steps < 1 || pe->steps > AWPU_PEEL_MAX_STEPS) return "steps outside [1, 32]";
    if (const char *why = peel_gain_refusal(pe->gain)) return why;
    if (!(pe->stop_ratio >= 0.0f && pe->stop_ratio < 1.0f)) return "stop_ratio outside [0, 1)";
    return nullptr;
}

// u[s] of the rule
inline float peel_u(float loop_gain, const float *gain, int32_t s) {
    if (!gain) return loop_gain;
    return gain[s] == 0.0f ? 0.0f : loop_gain / gain[s];
}

// the reach of a table at its active mics: the beam is formed for i in [lo, lo + len)
struct PeelReach {
    int32_t min_off, max_off, lo, len;
};
inline PeelReach peel_reach(const int32_t *off, int32_t lut_stride, int32_t n_pixels, const int32_t *index, int32_t usable) {
    PeelReach r{INT32_MAX, INT32_MIN, 0, 0};
    for (int32_t p = 0; p < n_pixels; p++)
        for (int32_t s = 0; s < usable; s++) {
            const int32_t o = off[(size_t) p * (size_t) lut_stride + (size_t) index[s]];
            r.min_off = o < r.min_off ? o : r.min_off;
            r.max_off = o > r.max_off ? o : r.max_off;
        }
    const int32_t E = r.max_off - r.min_off;
    r.lo = -E - 1;
    r.len = kPeelSamples + 2 * E + 2;  // hi - lo + 1, hi = 256 + E
    return r;
}
// the step reads X[off + lo .. off + hi + 1] of every active entry
inline bool peel_in_range(const PeelReach &r, int32_t hist) {
    return (long long) r.min_off + r.lo >= 0 && (long long) r.max_off + r.lo + r.len <= (long long) hist - 1;
}

inline bool peel_listed_twice(const int32_t *index, int32_t usable) {
    for (int32_t s = 1; s < usable; s++)
        for (int32_t t = 0; t < s; t++)
            if (index[s] == index[t]) return true;
    return false;
}

// one step of one frame: off_row / frac_row = the pixel's table row [lut_stride]; b [reach.len] is written; u [usable]
inline void peel_step_frame(float *frame, int32_t hist, const int32_t *off_row, const float *frac_row, const int32_t *index, int32_t usable,
                            const float *gain, const float *u, const PeelReach &reach, float *b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float norm = 1.0f / (float) usable;
    for (int32_t j = 0; j < reach.len; j++) {  // i = lo + j
        float out = 0.0f;
        for (int32_t s = 0; s < usable; s++) {
            const int32_t id = index[s];
            const float *x = frame + (size_t) id * (size_t) hist + off_row[id] + reach.lo + j;
            float x0 = x[0], x1 = x[1];
            if (gain) x0 = x0 * gain[s], x1 = x1 * gain[s];
            out = out + peel_lerp(frac_row[id], x0, x1);
        }
        b[j] = out * norm;
    }
    for (int32_t s = 0; s < usable; s++) {
        const int32_t id = index[s];
        float *x = frame + (size_t) id * (size_t) hist + off_row[id] + reach.lo + 1;  // sample o + i + 1 at x[j]
        for (int32_t j = 0; j < reach.len - 1; j++) x[j] = peel_subtract(u[s], frac_row[id], b[j], b[j + 1], x[j]);
    }
}

}  // namespace awpu
