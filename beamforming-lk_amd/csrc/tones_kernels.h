// tones_kernels.h -- the device side of include/awpu_hip_tones.h: the tone sweep (tones_kernels.hip).  Internal to
// libawpu_hip.so.
#pragma once

#include "awpu_hip_tones.h"
#include "das_kernels.h"

namespace awpu {

// The sweep takes what das_exact_kernel takes (SweepArgs: the frames in the layout launch() is given, the LutEntry table in
// active-mic order, the staged window; sweep.power and sweep.sums are not used) and the rule's two tables as the host functions
// made them: window [256] of t.window, twiddles [128][2].  It writes, each where it is asked for: tone [batch][t.n_groups]
// [pixel_count], pitch [batch][pixel_count], pitch_row [batch][pixel_count] = (float) pitch (what a run shows),
// bins [batch][pixel_count][129], spectrum [batch][pixel_count][129][2].
struct TonesArgs {
    SweepArgs sweep;
    const float *window;
    const float *twiddles;
    float wss;  // the sum of the window's squares: 256 or 96
    float *tone;
    int32_t *pitch;
    float *pitch_row;
    float *bins;
    float *spectrum;
    awpu_tones_t t;  // edge[] travels as a kernel argument
};

// REACH: that of launch_cohere_sweep -- history samples [wstart, wstart + window) of every active stream, x[off_rel .. off_rel + 256]
// of a staged row -- plus window[0 .. 255] and twiddles[0 .. 255].  No LDS beyond the staged chunk: the transform's exchanges are
// cross-lane moves, so the chunk rule is das_exact_lds_bytes.  hipErrorInvalidValue where the window does not fit that budget.
hipError_t launch_tones_sweep(const TonesArgs &a, hipStream_t stream);

}  // namespace awpu
