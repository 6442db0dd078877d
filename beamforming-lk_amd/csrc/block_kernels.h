// block_kernels.h -- the device side of include/awpu_hip_blocks.h: a run of consecutive blocks becomes a staging history
// [n_streams][768 + 256 * chunk] per chunk, and the history the overlapping snapshots' windows in the layout the sweeps read.
#pragma once

#include <hip/hip_runtime.h>

namespace awpu {

constexpr int kBlockPrefix = 768;  // samples of the snapshot before a chunk that its first snapshots still see (1024 - 256)

// n_blocks x 256 tight wire datagrams (AWPU_DATAGRAM_BYTES apart) -> hist[s * hist_pitch + first + i], i < 256 * n_blocks,
// with the arithmetic and the column flip of unpack_block_kernel
hipError_t launch_unpack_blocks(const void *d_datagrams, int n_blocks, int n_sensors, float *d_hist, int hist_pitch, int first,
                                hipStream_t stream);

// dst[r * dst_pitch + j] = src[r * src_pitch + j] for r < rows, j < n (rows of the samples form, the prefix of a history)
hipError_t launch_copy_rows(const float *d_src, long long src_pitch, float *d_dst, long long dst_pitch, int n, int rows,
                            hipStream_t stream);

// snapshot k of the chunk starts at history sample 256 * k: frames[k][s][j] = hist[s * hist_pitch + 256 * k + lo + j], j < width
hipError_t launch_cut_windows(const float *d_hist, int hist_pitch, int n_streams, int n_frames, int lo, int width, float *d_frames,
                              hipStream_t stream);

// the ingest ring [n_streams][2048] (both copies) set to the 1024 history samples from `last` on, its snapshot starting at `pos`
hipError_t launch_ring_write(const float *d_hist, int hist_pitch, int last, int n_streams, float *d_ring, int pos, hipStream_t stream);

}  // namespace awpu
