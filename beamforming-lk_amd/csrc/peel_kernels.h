// peel_kernels.h -- the device side of include/awpu_hip_peel.h: the step, the loop's iteration (pick, bookkeeping, step) and
// the loop's finish (peel_kernels.hip).  Internal to libawpu_hip.so.
#pragma once

#include "das_kernels.h"

#include "awpu_hip_peel.h"

namespace awpu {

// One step of every frame of a batch.  frames [batch][n_streams][hist] are updated in place; lut [n_pixels][usable] holds
// {off - wstart, frac} in active-mic order (the coherence sweep's table); u [usable] is the rule's u[].
// REACH: of frame b with pixel p the kernel reads and writes history samples [off + lo, off + lo + len] of every active stream,
// off = lut[p][s].off_rel + wstart -- inside [0, hist) where the caller has checked the rule's range (peel_in_range) -- and nothing
// else of the frames; a pixel outside [0, n_pixels) skips the frame.  b[] takes len floats of LDS.
struct PeelArgs {
    float *frames;
    const LutEntry *lut;
    const int32_t *index;  // [usable] stream id per active mic
    const float *gain;     // [usable] or null
    float *beams;          // [batch][len] or null
    int32_t n_streams, hist, usable, n_pixels, wstart, lo, len, batch;
    float norm;            // 1.0f / (float) usable
    float u[AWPU_PEEL_MAX_MICS];
};

// The loop's bookkeeping of one frame, on the device from iteration to iteration
struct PeelState {
    int32_t done;
    float first;
    awpu_peel_step_t step[AWPU_PEEL_MAX_STEPS];
};

// the step with the pixels given: pixel [batch] device memory
hipError_t launch_peel_step(const PeelArgs &a, const int32_t *pixel, hipStream_t stream);

// iteration k of the loop: power [batch][n_pixels] is P_k.  Closes step k-1, picks, tests, records in state [batch], steps.
hipError_t launch_peel_iteration(const PeelArgs &a, const float *power, PeelState *state, int32_t k, float stop_ratio, hipStream_t stream);

// behind the last sweep: power is P_steps.  Closes the last step and writes, each where it is asked for, steps [batch][n_steps]
// and clean, residual, map [batch][n_pixels].
hipError_t launch_peel_finish(const float *power, PeelState *state, int32_t n_steps, int32_t n_pixels, int32_t batch, awpu_peel_step_t *steps,
                              float *clean, float *residual, float *map, hipStream_t stream);

}  // namespace awpu
