// block_kernels.hip -- runs of consecutive blocks (include/awpu_hip_blocks.h): the reference's one snapshot per block
// (Worker::loop, src/dsp/worker.h:212-224; Streams::read_stream, src/fpga/streams.hpp:113-116) formed for a whole chunk of
// blocks on the device.  Every new sample crosses PCIe once; consecutive snapshots share 768 samples and are cut out of one
// history per chunk.  Plain copies and the unpack of unpack_block_kernel (das_kernels.hip), nothing else.
#include "block_kernels.h"

#include <cstdint>

namespace awpu {

namespace {
constexpr int kDatagramBytes = 1032;  // AWPU_DATAGRAM_BYTES: 8-byte header + 256 x i32 (src/fpga/receiver.h:24-30)
}

// Pipeline::receive_exposure (src/fpga/pipeline.cpp:260-297) for n blocks at once.  A 64 x 64 tile (64 sensors x 64 samples)
// goes through LDS so that the datagram reads (along s) and the history writes (along i) are both coalesced; every input byte
// past the headers is read once.
__global__ void unpack_blocks_kernel(const unsigned char *datagrams, int n_sensors, float *hist, int hist_pitch, int first) {
    __shared__ float tile[64][65];
    const int i0 = blockIdx.x * 64, s0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;  // 256 threads: 4 rows per pass
    for (int r = ty; r < 64; r += 4) {
        const int s = s0 + tx, i = i0 + r;
        float v = 0.0f;
        if (s < n_sensors) {
            // pipeline.cpp:277-287: `inverted` toggles at every multiple of 8, starting inverted
            const bool inverted = ((s >> 3) & 1) == 0;
            const int idx = inverted ? 8 * (1 + (s >> 3)) - 1 - (s & 7) : s;
            const int32_t raw = *(const int32_t *) (datagrams + (size_t) i * kDatagramBytes + 8 + 4 * idx);
            v = (float) raw / 8388608.0f;  // MAX_VALUE_FLOAT, src/fpga/pipeline.h:25
        }
        tile[r][tx] = v;
    }
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        const int s = s0 + r, i = i0 + tx;
        if (s < n_sensors) hist[(size_t) s * hist_pitch + first + i] = tile[tx][r];
    }
}

hipError_t launch_unpack_blocks(const void *d_datagrams, int n_blocks, int n_sensors, float *d_hist, int hist_pitch, int first,
                                hipStream_t stream) {
    if (n_blocks < 1 || n_sensors < 1 || n_sensors > 256) return hipErrorInvalidValue;
    dim3 grid(n_blocks * 4, (n_sensors + 63) / 64);  // 256 samples per block = 4 tiles of 64
    hipLaunchKernelGGL(unpack_blocks_kernel, grid, dim3(256), 0, stream, (const unsigned char *) d_datagrams, n_sensors, d_hist,
                       hist_pitch, first);
    return hipGetLastError();
}

__global__ void copy_rows_kernel(const float *src, long long src_pitch, float *dst, long long dst_pitch, int n) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < n) dst[blockIdx.y * dst_pitch + j] = src[blockIdx.y * src_pitch + j];
}

hipError_t launch_copy_rows(const float *d_src, long long src_pitch, float *d_dst, long long dst_pitch, int n, int rows,
                            hipStream_t stream) {
    if (n < 1 || rows < 1 || rows > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(copy_rows_kernel, dim3((n + 255) / 256, rows), dim3(256), 0, stream, d_src, src_pitch, d_dst, dst_pitch, n);
    return hipGetLastError();
}

__global__ void cut_windows_kernel(const float *hist, int hist_pitch, int n_streams, int lo, int width, float *frames) {
    const int j = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y, k = blockIdx.z;
    if (j < width)
        frames[((size_t) k * n_streams + s) * width + j] = hist[(size_t) s * hist_pitch + 256 * (size_t) k + lo + j];
}

hipError_t launch_cut_windows(const float *d_hist, int hist_pitch, int n_streams, int n_frames, int lo, int width, float *d_frames,
                              hipStream_t stream) {
    // a snapshot is 1024 samples: the last window of the chunk ends inside its history [0, 768 + 256 * n_frames)
    if (n_streams < 1 || n_streams > 65535 || n_frames < 1 || n_frames > 65535 || width < 1 || lo < 0 || lo + width > 1024)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(cut_windows_kernel, dim3((width + 255) / 256, n_streams, n_frames), dim3(256), 0, stream, d_hist, hist_pitch,
                       n_streams, lo, width, d_frames);
    return hipGetLastError();
}

// the state n ingests leave (unpack_block_kernel): every sample twice, 1024 floats apart, the snapshot at column pos
__global__ void ring_write_kernel(const float *hist, int hist_pitch, int last, float *ring, int pos) {
    const int j = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    const float v = hist[(size_t) s * hist_pitch + last + j];
    float *row = ring + (size_t) s * 2048;
    const int q = (pos + j) & 1023;
    row[q] = v;
    row[q + 1024] = v;
}

hipError_t launch_ring_write(const float *d_hist, int hist_pitch, int last, int n_streams, float *d_ring, int pos, hipStream_t stream) {
    if (n_streams < 1 || n_streams > 65535 || last < 0 || last + 1024 > hist_pitch || pos < 0 || pos >= 1024) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ring_write_kernel, dim3(4, n_streams), dim3(256), 0, stream, d_hist, hist_pitch, last, d_ring, pos);
    return hipGetLastError();
}

}  // namespace awpu
