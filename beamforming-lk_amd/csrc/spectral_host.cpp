// spectral_host.cpp -- awpu_hip_spectral_compose: the display rule of include/awpu_hip_spectral.h as executable C++, pure host code
// with no handle (like awpu_hip_heatmap_u8, whose maximum and level it restates through spectral_rule.h).  Written for reading,
// not for speed.  The kernels (spectral_kernels.hip) take the same steps out of spectral_rule.h.  A host compiler alone takes
// this file.
#include "spectral_rule.h"

extern "C" int awpu_hip_spectral_compose(const float *power, int64_t band_pitch, int32_t n_bands, int32_t n, const int32_t *channel,
                                         int32_t scale, uint8_t *image, uint8_t *dominant) {
    if (!power || (!image && !dominant) || n < 1) return AWPU_ERR_INVALID;
    if (awpu::spectral_display_refusal(n_bands, channel, scale)) return AWPU_ERR_INVALID;
    const auto plane = [&](int b) { return power + (int64_t) b * band_pitch; };
    if (image) {
        float max_of[AWPU_SPECTRAL_MAX_BANDS], common = 0.0f;
        for (int b = 0; b < n_bands; b++) {
            max_of[b] = 0.0f;
            for (int32_t i = 0; i < n; i++) max_of[b] = awpu::spectral_max_step(max_of[b], plane(b)[i]);
        }
        for (int c = 0; c < 3; c++)
            if (channel[c] >= 0) common = awpu::spectral_max_step(common, max_of[channel[c]]);
        for (int32_t i = 0; i < n; i++)
            for (int c = 0; c < 3; c++) {
                const int b = channel[c];
                image[(size_t) i * 3 + c] = b < 0 ? 0 : awpu::spectral_level(plane(b)[i], scale == AWPU_SPECTRAL_SCALE_COMMON ? common : max_of[b]);
            }
    }
    if (dominant)
        for (int32_t i = 0; i < n; i++) {
            uint32_t bits[AWPU_SPECTRAL_MAX_BANDS];
            for (int b = 0; b < n_bands; b++) bits[b] = awpu::spectral_bits(plane(b)[i]);
            dominant[i] = (uint8_t) awpu::spectral_dominant(bits, n_bands);
        }
    return AWPU_OK;
}
