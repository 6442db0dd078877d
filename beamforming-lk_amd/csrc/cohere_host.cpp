// cohere_host.cpp -- awpu_hip_cohere_host: the rule of include/awpu_hip_cohere.h as executable C++, pure host code with no
// handle (like awpu_hip_find_peaks).  Written for reading, not for speed: pixel by pixel, mic by mic, as the rule states it
// (cohere_rule.h).  The kernel (cohere_kernels.hip) takes the same operations lane by lane.  A host compiler alone takes this file.
#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC optimize("fp-contract=off")
#endif

#include <cstring>

#include "cohere_rule.h"

extern "C" int awpu_hip_cohere_host(const float *frames, int32_t batch, int32_t n_streams, int32_t hist, const int32_t *off, const float *frac,
                                    int32_t lut_stride, int32_t n_pixels, const int32_t *index, int32_t usable, const float *gain, float *power,
                                    float *coherence, float *weighted, float *sums, float *energy) {
    if (!frames || !off || !frac || !index || batch < 1) return AWPU_ERR_INVALID;
    if (const int rc = awpu::cohere_check_table(n_streams, hist, off, frac, lut_stride, n_pixels, index, usable)) return rc;
    constexpr int N = awpu::kCohereSamples;
    float out[N], e[N];
    for (int32_t b = 0; b < batch; b++) {
        const float *frame = frames + (size_t) b * (size_t) n_streams * (size_t) hist;
        for (int32_t p = 0; p < n_pixels; p++) {
            const size_t row = (size_t) p * (size_t) lut_stride, at = (size_t) b * (size_t) n_pixels + (size_t) p;
            const awpu::CoherePixel r = awpu::cohere_pixel(frame, hist, off + row, frac + row, index, usable, gain, out, e);
            if (power) power[at] = r.power;
            if (coherence) coherence[at] = r.coherence;
            if (weighted) weighted[at] = r.weighted;
            if (sums) std::memcpy(sums + at * N, out, sizeof out);
            if (energy) std::memcpy(energy + at * N, e, sizeof e);
        }
    }
    return AWPU_OK;
}
