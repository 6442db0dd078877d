// band_kernels.h -- the device side of include/awpu_hip_band.h: the pre-pass that writes the filtered window of every frame and
// active stream in front of a sweep.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace awpu {

constexpr int kBandWaves = 4;      // streams per workgroup: one wave each
constexpr int kBandChunk = 512;    // outputs of a row a wave forms per pass: eight per lane
constexpr int kBandRowFloats = 640;  // LDS per wave: the chunk and the 127 samples in front of it (2.5 KB; 10 KB per workgroup)

// Where the samples are and where the filtered ones go.  Sample j of (frame f, stream id) is in[f * in_frame + id * in_row + j],
// the filtered one out[f * out_frame + id * out_row + j].  Outputs [out_first, out_first + n) of every frame and stream
// index[0 .. usable-1] are written; output out_first + i reads the inputs in_first + i .. in_first + i + taps - 1 (the caller
// has made sure they are there: in_first = the window's start in an input row less taps - 1).
struct BandArgs {
    const float *in;
    long long in_frame, in_row;
    int in_first;
    float *out;
    long long out_frame, out_row;
    int out_first;
    int n;
    const int32_t *index;
    int usable;
    int n_frames;
    int taps;
    float coef[128];  // [taps]: kernel arguments, so a handle's launches in flight keep theirs when its band is replaced
};

// hipErrorInvalidValue for taps outside [1, 128], n < 1, negative firsts, usable < 1 and n_frames outside [1, 65535]
hipError_t launch_band_filter(const BandArgs &a, hipStream_t stream);

}  // namespace awpu
