// csm_kernels.h -- the device side of include/awpu_hip_csm.h: block spectra, the cross-spectral sum and the quadratic-form map
// (csm_kernels.hip).  Internal to libawpu_hip.so.
#pragma once

#include <hip/hip_runtime.h>

#include "awpu_hip_csm.h"
#include "das_kernels.h"

namespace awpu {

// Step 1.  samples [n_streams][pitch]; index [usable], gain [usable] or null; window [256] and twiddles [128][2] are the rule's
// tables as the host functions make them; spectra [n_blocks][n_bins][usable][2] is written.
// REACH: samples[index[a] * pitch + 256 * n_blocks - 1]; window[255]; twiddles[255]; every entry of spectra.
struct CsmSpectraArgs {
    const float *samples;
    long long pitch;
    const int32_t *index;
    const float *gain;
    const float *window;
    const float *twiddles;
    float *spectra;
    int32_t usable, n_blocks, n_bins;
    int32_t bin[AWPU_CSM_MAX_BINS];
};
hipError_t launch_csm_spectra(const CsmSpectraArgs &a, hipStream_t stream);

// Step 2.  spectra as above is added, block by block, into matrix [n_bins][usable][usable][2].
struct CsmAccumulateArgs {
    const float *spectra;
    float *matrix;
    int32_t usable, n_blocks, n_bins;
};
hipError_t launch_csm_accumulate(const CsmAccumulateArgs &a, hipStream_t stream);

// Steps 3 to 5.  matrix [n_bins][usable][usable][2]; lut [pixel_count][usable] in active-mic order with off_rel = off - wstart;
// map and q [n_bins][pixel_count], each or null; scale is step 5's divisor (csm_rule.h).
// REACH: every entry of matrix and lut; twiddles[255]; LDS: csm_map_lds_bytes below, at most 144 KiB.
struct CsmMapArgs {
    const float *matrix;
    const LutEntry *lut;
    const float *twiddles;
    float *map;
    float *q;
    int32_t usable, pixel_count, wstart, n_bins, kind;
    float scale;
    int32_t bin[AWPU_CSM_MAX_BINS];
};
constexpr int kCsmMapLdsBytes = 144 * 1024;
constexpr int kCsmMapMaxUsable = 2048;
// LDS of a workgroup that maps ppw pixels: the steering vectors [usable][ppw] and the ring of a round's y [2][16][ppw], 8 bytes each
inline int csm_map_lds_bytes(int usable, int ppw) { return (usable + 32) * ppw * 8; }
// pixels a workgroup maps: 64, or fewer where 64 steering vectors do not fit the LDS; 0 = too many mics
inline int csm_map_pixels_per_wave(int usable) {
    if (usable > kCsmMapMaxUsable) return 0;
    for (int ppw = 64; ppw >= 8; ppw /= 2)
        if (csm_map_lds_bytes(usable, ppw) <= kCsmMapLdsBytes) return ppw;
    return 0;
}
hipError_t launch_csm_map(const CsmMapArgs &a, hipStream_t stream);  // hipErrorInvalidValue where the mics do not fit


// The row a run shows of one frame's planes [n_bins][pixel_count] (csm_show_kernels.hip): the plane of bin `show`, or with show
// < 0 the planes added in ascending bin order with plain additions, from +0.
hipError_t launch_csm_show(const float *planes, int n_bins, int pixel_count, int show, float *row, hipStream_t stream);

}  // namespace awpu
