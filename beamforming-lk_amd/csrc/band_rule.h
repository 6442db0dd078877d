// band_rule.h -- the arithmetic of include/awpu_hip_band.h that the host definition (band_host.cpp) and the kernel
// (band_kernels.hip) share, so that both take the same steps in the same order: one fused multiply-add per tap, ascending taps.
// No HIP types: a host compiler alone takes it.
#pragma once

#include <cstdint>

#include "awpu_hip_band.h"

#if defined(__HIPCC__)
#define AWPU_BAND_HD __host__ __device__
#else
#define AWPU_BAND_HD
#endif

namespace awpu {

// one step of the rule: acc = fmaf(c[k], x[t-k], acc), one rounding (v_fma_f32 on the device, the C library's fmaf on a host
// without the instruction); nothing here for a compiler to contract or re-order
AWPU_BAND_HD inline float band_step(float c, float x, float acc) { return __builtin_fmaf(c, x, acc); }

// y[t] of a row x whose samples before t = 0 are +0.  Every step is taken, those on the zero history too: an accumulator that
// has rounded to -0 becomes +0 again on them, as the rule says
AWPU_BAND_HD inline float band_output(const float *c, int taps, const float *x, int t) {
    float acc = 0.0f;
    for (int k = 0; k < taps; k++) acc = band_step(c[k], k <= t ? x[t - k] : 0.0f, acc);
    return acc;
}

// what is wrong with a set of coefficients, or null
inline const char *band_refusal(const float *c, int32_t taps) {
    if (!c) return "null argument";
    if (taps < 1 || taps > AWPU_BAND_MAX_TAPS) return "taps outside [1, 128]";
    for (int k = 0; k < taps; k++)
        if (!(c[k] - c[k] == 0.0f)) return "band coefficient not finite";
    return nullptr;
}

}  // namespace awpu
