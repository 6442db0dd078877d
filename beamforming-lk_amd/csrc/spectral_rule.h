// spectral_rule.h -- the steps of include/awpu_hip_spectral.h that the host definition (spectral_host.cpp) and the kernels
// (spectral_kernels.hip) share, so that both take the same steps: the running maximum, the level of a pixel, the order that
// names the dominant band; and what is wrong with a set of bands.  No HIP types: a host compiler alone takes it.
#pragma once

#include <cstdint>
#include <cstring>

#include "awpu_hip_spectral.h"
#include "band_rule.h"

namespace awpu {

// awpu_hip_heatmap_u8's running maximum (mimo.cpp:62-73): it starts at +0 and a value replaces it only where it is greater, so a
// NaN, a negative power and -0 never do, and the result does not depend on the order the values are visited in
AWPU_BAND_HD inline float spectral_max_step(float max_v, float v) { return v > max_v ? v : max_v; }

// ... and its level (mimo.cpp:85-91 with USE_DB 0): float division, double scaling, clip, truncate; a NaN level is 0
AWPU_BAND_HD inline uint8_t spectral_level(float power, float max_v) {
    double level = static_cast<double>(power / max_v) * 255.0;
    level = !(level >= 0.0) ? 0.0 : (level > 255.0 ? 255.0 : level);
    return static_cast<uint8_t>(level);
}

// awpu_hip_find.h's order over the bands of one pixel: the greater bits win, equal bits go to the lower band
AWPU_BAND_HD inline int spectral_dominant(const uint32_t *bits, int n_bands) {
    int best = 0;
    uint32_t top = bits[0];
    for (int b = 1; b < n_bands; b++)
        if (bits[b] > top) top = bits[b], best = b;
    return best;
}

inline uint32_t spectral_bits(float v) {
    uint32_t u;
    std::memcpy(&u, &v, sizeof(u));
    return u;
}

// what is wrong with the display half of a set of bands, or null
inline const char *spectral_display_refusal(int32_t n_bands, const int32_t *channel, int32_t scale) {
    if (!channel) return "null argument";
    if (n_bands < 1 || n_bands > AWPU_SPECTRAL_MAX_BANDS) return "n_bands outside [1, 4]";
    for (int c = 0; c < 3; c++)
        if (channel[c] < -1 || channel[c] >= n_bands) return "channel outside [-1, n_bands)";
    if (scale != AWPU_SPECTRAL_SCALE_COMMON && scale != AWPU_SPECTRAL_SCALE_PER_BAND) return "unknown scale";
    return nullptr;
}

// what is wrong with a set of bands, or null: counts, taps, finite coefficients, channels, scale
inline const char *spectral_refusal(const awpu_spectral_t *sp) {
    if (!sp) return "null argument";
    if (sp->n_bands < 1 || sp->n_bands > AWPU_SPECTRAL_MAX_BANDS) return "n_bands outside [1, 4]";
    for (int b = 0; b < sp->n_bands; b++)
        if (const char *why = band_refusal(sp->coef[b], sp->taps[b])) return why;
    return spectral_display_refusal(sp->n_bands, sp->channel, sp->scale);
}

}  // namespace awpu
