// spectral_kernels.h -- the device side of include/awpu_hip_spectral.h: the pre-pass that writes the filtered windows of up to
// four bands from one read of the samples, the display step that composes a frame's band powers into a three-byte image and
// names the dominant band of every pixel, and the large three-byte image.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "awpu_hip_spectral.h"
#include "band_kernels.h"
#include "das_kernels.h"

namespace awpu {

// band_kernels.h's BandArgs for several bands: `in` and the outputs' layout are the same for all of them, band b's outputs are
// out_plane floats behind band b-1's, and in_first = the window's start in an input row less max_b taps[b] - 1 -- every band
// reads the same staged segment, a shorter one only its last taps[b] - 1 + n samples.
struct SpectralBandArgs {
    const float *in;
    long long in_frame, in_row;
    int in_first;
    float *out;
    long long out_frame, out_row, out_plane;
    int out_first;
    int n;
    const int32_t *index;
    int usable;
    int n_frames;
    int n_bands;
    int max_taps;
    int taps[AWPU_SPECTRAL_MAX_BANDS];
    float coef[AWPU_SPECTRAL_MAX_BANDS][AWPU_BAND_MAX_TAPS];  // kernel arguments, as BandArgs::coef: a launch in flight keeps its own
};

// hipErrorInvalidValue for n_bands outside [1, 4], a taps[b] outside [1, max_taps], max_taps above 128, and what launch_band_filter refuses
hipError_t launch_spectral_filter(const SpectralBandArgs &a, hipStream_t stream);

// What is shown of the powers.  Band b's frame f is d_power + b * plane + f * n.
struct SpectralShow {
    int n_bands;
    int channel[3];
    int scale;
};

// awpu_hip_spectral_compose for n_frames frames: d_image [n_frames][n][3] and d_dominant [n_frames][n], either may be null, not
// both; d_peaks [n_frames][4] floats of scratch (every band's maximum; needed only with an image).  n_frames in [1, 65535]
hipError_t launch_spectral_compose(const float *d_power, long long plane, int n, int n_frames, const SpectralShow &show, float *d_peaks,
                                   uint8_t *d_image, uint8_t *d_dominant, hipStream_t stream);

// d_src [batch][srows][scols][3] -> d_dst [batch][drows][dcols][3]: every byte plane through the taps of launch_upscale (d_taps =
// dcols column taps, then drows row taps) with its arithmetic, mirrored left-right when flip
hipError_t launch_spectral_upscale(const uint8_t *d_src, int srows, int scols, int batch, const ResizeTap *d_taps, bool flip,
                                   uint8_t *d_dst, int drows, int dcols, hipStream_t stream);

}  // namespace awpu
