// csm_clean_kernels.h -- the device side of include/awpu_hip_csm_clean.h: what runs between two dirty maps of a CLEAN-SC loop
// (csm_clean_kernels.hip).  The maps themselves are launch_csm_map's (csm_kernels.h), unchanged.  Internal to libawpu_hip.so.
#pragma once

#include <hip/hip_runtime.h>

#include "awpu_hip_csm.h"
#include "das_kernels.h"

namespace awpu {

constexpr int kCsmCleanThreads = 256;  // the component kernel's workgroup: the rows it covers in one pass
constexpr int kCsmCleanMaxUsable = 2048;  // the map's bound: s and v of one bin, 8 bytes a mic each, stay in 32 KiB of LDS

// A bin's bookkeeping, in device memory from launch to launch.  `pixel` and `r` are what the component kernel leaves for the
// update kernel behind it: the pixel whose component is in v (-1: this iteration updates nothing) and gain / qs.
struct CsmCleanState {
    int32_t done;
    int32_t pixel;
    float first;
    float r;
    awpu_csm_clean_step_t step[AWPU_CSM_CLEAN_MAX_STEPS];
};

// Load: the entries b <= a of src [n_bins][usable][usable][2] into dst as D keeps them -- (re, +0) on the diagonal --, and their
// exact conjugates above the diagonal.  src == dst is taken: a thread reads its own entry alone.
// REACH: every entry of src on and below the diagonal; every entry of dst.
hipError_t launch_csm_clean_load(const float *src, float *dst, int usable, int n_bins, hipStream_t stream);

// What the component kernel reads and writes; one workgroup a bin.
//   matrix     a loaded D [n_bins][usable][usable][2]
//   lut        [n_pixels][usable] in active-mic order with off_rel = off - wstart; twiddles [128][2]
//   v          [n_bins][usable][2], written: the bin's component, zeros where the bin does not step
//   state      [n_bins], read and written
// REACH: every entry of matrix; lut row of the picked pixel (a pixel outside [0, n_pixels) is never used as an index);
// twiddles[255]; v[n_bins * usable * 2 - 1]; state[n_bins - 1]; LDS: 32 KiB + 128 bytes, static.
struct CsmCleanArgs {
    const float *matrix;
    const LutEntry *lut;
    const float *twiddles;
    float *v;
    CsmCleanState *state;
    int32_t usable, n_pixels, wstart, n_bins;
    float gain;
    int32_t bin[AWPU_CSM_MAX_BINS];
};

// The step form's: the pixels come from d_pixel [n_bins]; component [n_bins][usable][2] and qs [n_bins], each or null, are the
// caller's copies of v and qs (zeros for a skipped bin).  REACH as above, and pixel[n_bins - 1], qs[n_bins - 1].
hipError_t launch_csm_clean_component(const CsmCleanArgs &a, const int32_t *pixel, float *component, float *qs, hipStream_t stream);

// The loop form's, iteration i: pick over plane [n_bins][n_pixels] (the dirty rows P_i), the stop tests, the component, qs, the
// record.  A done bin leaves at once.  REACH as above, and every entry of plane.
hipError_t launch_csm_clean_iteration(const CsmCleanArgs &a, const float *plane, int i, float stop_ratio, hipStream_t stream);

// Update: one thread per entry b <= a of every bin whose state says it steps (pixel >= 0), writing the entry and its mirror.
// REACH: every entry of matrix; v and state as above.
hipError_t launch_csm_clean_update(float *matrix, const float *v, const CsmCleanState *state, int usable, int n_bins, hipStream_t stream);

// Finish: plane is the residual row of every bin.  steps [n_bins][n_steps], clean, residual, map [n_bins][n_pixels], each or null.
// REACH: every entry of plane and of each output given; state[n_bins - 1].
hipError_t launch_csm_clean_finish(const float *plane, const CsmCleanState *state, int n_steps, int n_pixels, int n_bins,
                                   awpu_csm_clean_step_t *steps, float *clean, float *residual, float *map, hipStream_t stream);

}  // namespace awpu
