// cohere_rule.h -- the rule of include/awpu_hip_cohere.h as host C++: the argument checks and one pixel of one frame, written
// for reading, in the rule's own order.  Host only (the kernel, cohere_kernels.hip, takes the same operations on the same operands
// lane by lane); shared by the host definition (cohere_host.cpp) and the stand-alone checker (tests/host/cohere_rule_check.cpp).
// No HIP types: a host compiler alone takes it.  Its users switch contraction off for GCC (#pragma GCC optimize at their top);
// for clang the functions below do.
#pragma once

#include <cstddef>
#include <cstdint>

#include "awpu_hip_cohere.h"

namespace awpu {

constexpr int kCohereSamples = 256;  // a block (N_SAMPLES of the reference)

// what is wrong with a request, or null
inline const char *cohere_refusal(const awpu_cohere_t *co) {
    if (!co) return "null argument";
    if (co->show != AWPU_COHERE_WEIGHTED && co->show != AWPU_COHERE_FACTOR) return "show is AWPU_COHERE_WEIGHTED or AWPU_COHERE_FACTOR";
    return nullptr;
}

// the table and the active list against the frame: AWPU_OK, AWPU_ERR_INVALID or AWPU_ERR_RANGE (awpu_hip_beams' refusals)
inline int cohere_check_table(int32_t n_streams, int32_t hist, const int32_t *off, const float *frac, int32_t lut_stride, int32_t n_pixels,
                              const int32_t *index, int32_t usable) {
    if (n_streams < 1 || hist < kCohereSamples + 1 || lut_stride < 1 || n_pixels < 1 || usable < 1) return AWPU_ERR_INVALID;
    for (int32_t s = 0; s < usable; s++)
        if (index[s] < 0 || index[s] >= n_streams || index[s] >= lut_stride) return AWPU_ERR_INVALID;
    for (int32_t p = 0; p < n_pixels; p++)
        for (int32_t s = 0; s < usable; s++) {
            const size_t at = (size_t) p * (size_t) lut_stride + (size_t) index[s];
            if (!(frac[at] >= 0.0f && frac[at] <= 1.0f)) return AWPU_ERR_INVALID;
            if (off[at] < 0 || off[at] > hist - (kCohereSamples + 1)) return AWPU_ERR_RANGE;  // delay() reads x[0 .. 256]
        }
    return AWPU_OK;
}

struct CoherePixel {
    float power, coherence, weighted;
};

// one pixel of one frame: off_row / frac_row = the pixel's table row [lut_stride]; out and e [256] are written (e[0] = e[255] = 0)
inline CoherePixel cohere_pixel(const float *frame, int32_t hist, const int32_t *off_row, const float *frac_row, const int32_t *index,
                                int32_t usable, const float *gain, float *out, float *e) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    constexpr int N = kCohereSamples;
    float x[N + 1], t[N];
    for (int i = 0; i < N; i++) out[i] = 0.0f, e[i] = 0.0f;
    for (int32_t s = 0; s < usable; s++) {
        const int32_t id = index[s];
        const float *src = frame + (size_t) id * (size_t) hist + off_row[id];
        const float f = frac_row[id];
        if (gain) {
            const float g = gain[s];
            for (int i = 0; i <= N; i++) x[i] = src[i] * g;
        } else {
            for (int i = 0; i <= N; i++) x[i] = src[i];
        }
        for (int i = 0; i < N; i++) {
            const float d = x[i] - x[i + 1];
            t[i] = __builtin_fmaf(f, d, x[i + 1]);
        }
        for (int i = 0; i < N; i++) out[i] = out[i] + t[i];
        for (int i = 1; i < N - 1; i++) {
            const float ma = t[i] * 0.5f - 0.25f * (t[i + 1] + t[i - 1]);
            e[i] = __builtin_fmaf(ma, ma, e[i]);
        }
    }
    float num = 0.0f, den = 0.0f;
    for (int i = 1; i < N - 1; i++) {
        const float ma = out[i] * 0.5f - 0.25f * (out[i + 1] + out[i - 1]);
        const float sq = ma * ma;
        num = num + sq;
    }
    for (int i = 1; i < N - 1; i++) den = den + e[i];
    CoherePixel r;
    r.power = num / (float) (N * usable);
    float c = den > 0.0f ? num / ((float) usable * den) : 0.0f;
    if (c > 1.0f) c = 1.0f;
    r.coherence = c;
    r.weighted = r.power * c;
    return r;
}

}  // namespace awpu
