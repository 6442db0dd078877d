// watch_kernels.h -- the device side of include/awpu_hip_watch.h: the history of a sweep piece that shows every Nth block, its
// snapshots' windows, and the large display image of a whole piece written 16 bytes per lane.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "das_kernels.h"

namespace awpu {

// A piece shows blocks b0, b0 + every, ... (nf of them).  Its history holds, 256 samples per slot, only the blocks those
// snapshots read: slots 0..3 = blocks b0-3 .. b0, then m = min(every, 4) slots per further frame k = blocks b_k-m+1 .. b_k.
// Snapshot k starts at history sample 256 * m * k (consecutive blocks while every <= 4; four blocks of its own beyond).
inline int watch_slots(int every, int nf) { return 4 + (every < 4 ? every : 4) * (nf - 1); }
// the block of the call that slot `slot` holds (negative: a block the ring held before the call, -1 the newest)
inline __host__ __device__ int watch_slot_block(int slot, int b0, int every, int m) {
    return slot < 4 ? b0 - 3 + slot : b0 + every * (1 + (slot - 4) / m) - m + 1 + (slot - 4) % m;
}

// hist[s * hist_pitch + 256 * slot + i] for slots [slot0, slot0 + n_slots): blocks >= 0 out of d_src [n_streams][src_pitch]
// (block b at column 256 * b), blocks < 0 out of the ring's snapshot d_snapshot (pitch 2048: block -4 at column 0).  d_src may
// be null when every slot asked for holds a block < 0.
hipError_t launch_watch_gather(const float *d_src, long long src_pitch, const float *d_snapshot, int b0, int every, int n_streams,
                               float *d_hist, int hist_pitch, int slot0, int n_slots, hipStream_t stream);

// frames[k][s][j] = hist[s * hist_pitch + step * k + lo + j], j < width, k < n_frames: launch_cut_windows with a step
hipError_t launch_watch_cut(const float *d_hist, int hist_pitch, int n_streams, int n_frames, int step, int lo, int width,
                            float *d_frames, hipStream_t stream);

constexpr int kWatchTileRows = 16;  // output rows per workgroup of the large-image kernel
// the most source rows one such tile reads (row_taps: the drows row taps of resize_taps, host memory)
int watch_band_rows(const ResizeTap *row_taps, int srows, int drows);

// launch_upscale for a piece of frames, written wide: d_src [batch][srows][scols] -> d_dst [batch][drows][dcols] (x 3 through
// d_colormap [256][3] when it is not null), mirrored left-right when flip.  Same taps, same arithmetic, same bytes.
// band_rows = watch_band_rows of the row taps.  hipErrorInvalidValue when a tile's source rows do not fit LDS.
hipError_t launch_watch_upscale(const uint8_t *d_src, int srows, int scols, int batch, const ResizeTap *d_taps, int band_rows,
                                const uint8_t *d_colormap, bool flip, uint8_t *d_dst, int drows, int dcols, hipStream_t stream);

}  // namespace awpu
