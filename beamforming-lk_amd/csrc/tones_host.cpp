// tones_host.cpp -- the host functions of include/awpu_hip_tones.h: the two tables, awpu_hip_tones_linear, and awpu_hip_tones_host,
// the rule as executable C++, pure host code with no handle (like awpu_hip_cohere_host).  Written for reading, not for speed: pixel
// by pixel, as the rule states it (tones_rule.h).  The kernel (tones_kernels.hip) takes the same operations lane by lane.  A host
// compiler alone takes this file.
#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC optimize("fp-contract=off")
#endif

#include <cstring>

#include "tones_rule.h"

extern "C" int awpu_hip_tones_window(int32_t window, float w[256]) {
    if (!w || (window != AWPU_TONES_RECT && window != AWPU_TONES_HANN)) return AWPU_ERR_INVALID;
    awpu::tones_window(window, w);
    return AWPU_OK;
}

extern "C" int awpu_hip_tones_twiddles(float t[128][2]) {
    if (!t) return AWPU_ERR_INVALID;
    awpu::tones_twiddles(t);
    return AWPU_OK;
}

extern "C" int awpu_hip_tones_linear(float lo_hz, float hi_hz, int32_t n_groups, float sample_rate, awpu_tones_t *t) {
    if (!t || n_groups < 1 || n_groups > awpu::kTonesBins || !(sample_rate > 0.0f)) return AWPU_ERR_INVALID;
    int first = -1, count = 0;  // the bins whose centres lie in [lo, hi): one run, the centres ascend
    for (int k = 0; k < awpu::kTonesBins; k++) {
        const double centre = (double) k * (double) sample_rate / awpu::kTonesSamples;
        if (centre >= (double) lo_hz && centre < (double) hi_hz) {
            if (first < 0) first = k;
            count++;
        }
    }
    if (count < n_groups) return AWPU_ERR_INVALID;
    t->n_groups = n_groups;
    t->edge[0] = first;
    for (int g = 0; g < n_groups; g++) t->edge[g + 1] = t->edge[g] + count / n_groups + (g < count % n_groups ? 1 : 0);
    for (int g = n_groups + 1; g <= awpu::kTonesBins; g++) t->edge[g] = 0;
    return AWPU_OK;
}

extern "C" int awpu_hip_tones_host(const float *frames, int32_t batch, int32_t n_streams, int32_t hist, const int32_t *off, const float *frac,
                                   int32_t lut_stride, int32_t n_pixels, const int32_t *index, int32_t usable, const float *gain,
                                   const awpu_tones_t *t, float *tone, int32_t *pitch, float *bins, float *spectrum) {
    if (!frames || !off || !frac || !index || batch < 1) return AWPU_ERR_INVALID;
    if (awpu::tones_refusal(t) || (!tone && !pitch && !bins && !spectrum)) return AWPU_ERR_INVALID;
    if (const int rc = awpu::cohere_check_table(n_streams, hist, off, frac, lut_stride, n_pixels, index, usable)) return rc;
    constexpr int N = awpu::kTonesSamples, K = awpu::kTonesBins;
    float w[N], tw[N / 2][2];
    awpu::tones_window(t->window, w);
    awpu::tones_twiddles(tw);
    float out[N], z[K][2], b[K], groups[K];
    for (int32_t f = 0; f < batch; f++) {
        const float *frame = frames + (size_t) f * (size_t) n_streams * (size_t) hist;
        for (int32_t p = 0; p < n_pixels; p++) {
            const size_t row = (size_t) p * (size_t) lut_stride, at = (size_t) f * (size_t) n_pixels + (size_t) p;
            awpu::tones_sums(frame, hist, off + row, frac + row, index, usable, gain, out);
            awpu::tones_transform(out, w, tw, awpu::tones_wss(t->window), usable, z, b);
            if (tone) {
                awpu::tones_groups(b, t, groups);
                for (int g = 0; g < t->n_groups; g++) tone[((size_t) f * (size_t) t->n_groups + (size_t) g) * (size_t) n_pixels + (size_t) p] = groups[g];
            }
            if (pitch) pitch[at] = awpu::tones_pitch(b, t);
            if (bins) std::memcpy(bins + at * K, b, sizeof b);
            if (spectrum) std::memcpy(spectrum + at * K * 2, z, sizeof z);
        }
    }
    return AWPU_OK;
}
