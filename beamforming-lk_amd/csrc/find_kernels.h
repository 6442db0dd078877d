// find_kernels.h -- the device side of include/awpu_hip_find.h: the strongest peaks of every frame of a batch of power rows.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "awpu_hip_find.h"

namespace awpu {

constexpr int kFindThreads = 1024;  // one workgroup of sixteen waves per frame

// awpu_hip_find_peaks of d_power [n_frames][rows * cols] into d_sources [n_frames][max_sources] and d_count [n_frames], on
// `stream`.  LDS plan: a bit per pixel rounded up to whole waves of 64 pixels (AWPU_FIND_MAX_PIXELS: 32 KB), beside 0.5 KB of
// reduction slots.  hipErrorInvalidValue for what awpu_hip_find.h refuses (the bitmap would not fit) and for n_frames < 1.
hipError_t launch_find_peaks(const float *d_power, int n_frames, const awpu_find_t &f, awpu_source_t *d_sources, int32_t *d_count,
                             hipStream_t stream);

}  // namespace awpu
