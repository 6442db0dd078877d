// csm_show_kernels.hip -- gfx950: the row a cross-spectral run shows of a frame's planes (include/awpu_hip_csm_watch.h): one bin's
// plane, or the planes added in ascending bin order -- plain additions from +0, one thread a pixel.
#include "csm_kernels.h"

#pragma clang fp contract(off)

namespace awpu {

__global__ __launch_bounds__(256) void csm_show_kernel(const float *planes, int n_bins, int pixel_count, int show, float *row) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= pixel_count) return;
    if (show >= 0) {
        row[p] = planes[(size_t) show * pixel_count + p];
        return;
    }
    float sum = 0.0f;
    for (int k = 0; k < n_bins; k++) sum = sum + planes[(size_t) k * pixel_count + p];
    row[p] = sum;
}

hipError_t launch_csm_show(const float *planes, int n_bins, int pixel_count, int show, float *row, hipStream_t stream) {
    if (n_bins < 1 || n_bins > AWPU_CSM_MAX_BINS || pixel_count < 1 || show >= n_bins) return hipErrorInvalidValue;
    hipLaunchKernelGGL(csm_show_kernel, dim3((pixel_count + 255) / 256), dim3(256), 0, stream, planes, n_bins, pixel_count, show, row);
    return hipGetLastError();
}

}  // namespace awpu
