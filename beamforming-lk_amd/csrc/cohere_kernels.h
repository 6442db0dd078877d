// cohere_kernels.h -- the device side of include/awpu_hip_cohere.h: the coherence sweep (cohere_kernels.hip).  Internal to
// libawpu_hip.so.
#pragma once

#include "das_kernels.h"

namespace awpu {

// The sweep takes what das_exact_kernel takes (SweepArgs: the frames in the layout launch() is given, the LutEntry table in
// active-mic order, the staged window) and writes, each where it is asked for: sweep.power, coherence and weighted
// [batch][pixel_count]; sweep.sums and energy [batch][pixel_count][256], out[] and e[] of the rule (energy[0] = energy[255] = 0).
struct CohereArgs {
    SweepArgs sweep;
    float *coherence;
    float *weighted;
    float *energy;
};

// REACH: the kernel stages history samples [wstart, wstart + window) of every active stream and reads nothing else of the frames;
// in LDS it reads x[off_rel .. off_rel + 256] of a staged row (off_rel + 256 <= window - 1 by prepare()'s window), the reach of
// das_exact_kernel.  hipErrorInvalidValue where the window does not fit das_exact_kernel's LDS budget.
hipError_t launch_cohere_sweep(const CohereArgs &a, hipStream_t stream);

}  // namespace awpu
