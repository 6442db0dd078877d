// band_kernels.hip -- the band's pre-pass (include/awpu_hip_band.h): for every frame and active stream, the window the sweeps
// read, filtered by the steps of band_rule.h, written where launch() expects a frame.  One wave per (frame, stream): the row
// segment [window start - (taps - 1), window end) goes through LDS in chunks of 512 outputs, lane l owns outputs l + 64 j of a
// chunk (consecutive lanes read consecutive LDS words: no bank conflicts), the coefficients are wave-uniform loads out of the kernel's arguments, the taps
// run in ascending order with the eight accumulators of a lane in registers.  Plain vector loads and stores, nothing else.
#include "band_kernels.h"

#include "band_rule.h"

namespace awpu {

namespace {

constexpr int kPerLane = kBandChunk / 64;
static_assert(sizeof(BandArgs{}.coef) == AWPU_BAND_MAX_TAPS * sizeof(float), "room for every tap");
static_assert(kBandChunk + AWPU_BAND_MAX_TAPS - 1 <= kBandRowFloats, "a chunk and its history fit a wave's LDS row");

__global__ __launch_bounds__(64 * kBandWaves) void band_filter_kernel(const BandArgs a) {
#pragma clang fp contract(off)
    __shared__ float rows[kBandWaves][kBandRowFloats];
    const int wave = __builtin_amdgcn_readfirstlane((int) threadIdx.x >> 6), lane = (int) threadIdx.x & 63;
    const int slot = (int) blockIdx.x * kBandWaves + wave;
    const bool live = slot < a.usable;  // (wave-uniform; the last workgroup's spare waves only keep the barriers' company)
    const long long id = live ? a.index[slot] : 0;
    const long long f = blockIdx.y;
    const float *in = a.in + f * a.in_frame + id * a.in_row + a.in_first;
    float *out = a.out + f * a.out_frame + id * a.out_row + a.out_first;
    float *seg = rows[wave];
    const int pre = a.taps - 1;
    for (int o0 = 0; o0 < a.n; o0 += kBandChunk) {
        const int cn = min(kBandChunk, a.n - o0);  // outputs of this chunk; it reads inputs [o0, o0 + pre + cn)
        for (int i = lane; i < pre + kBandChunk; i += 64) seg[i] = live && i < pre + cn ? in[o0 + i] : 0.0f;
        __syncthreads();
        float acc[kPerLane];
#pragma unroll
        for (int j = 0; j < kPerLane; j++) acc[j] = 0.0f;
        const float *at = seg + pre + lane;  // output lane + 64 j reads at[64 j - k] at tap k
#pragma unroll 4
        for (int k = 0; k < a.taps; k++) {
            const float ck = a.coef[k];
#pragma unroll
            for (int j = 0; j < kPerLane; j++) acc[j] = band_step(ck, at[64 * j - k], acc[j]);
        }
        if (live) {
#pragma unroll
            for (int j = 0; j < kPerLane; j++)
                if (lane + 64 * j < cn) out[o0 + lane + 64 * j] = acc[j];
        }
        __syncthreads();  // (the next chunk overwrites the row)
    }
}

}  // namespace

hipError_t launch_band_filter(const BandArgs &a, hipStream_t stream) {
    if (!a.in || !a.out || !a.index) return hipErrorInvalidValue;
    if (a.taps < 1 || a.taps > AWPU_BAND_MAX_TAPS || a.n < 1 || a.in_first < 0 || a.out_first < 0) return hipErrorInvalidValue;
    if (a.usable < 1 || a.n_frames < 1 || a.n_frames > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(band_filter_kernel, dim3((a.usable + kBandWaves - 1) / kBandWaves, a.n_frames), dim3(64 * kBandWaves), 0, stream, a);
    return hipGetLastError();
}

}  // namespace awpu
