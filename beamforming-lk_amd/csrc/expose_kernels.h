// expose_kernels.h -- the device side of include/awpu_hip_expose.h: the exposure pass over power rows, and the history of a
// sweep piece of an exposed run, which holds the blocks of whole windows rather than of single shown blocks.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "expose_rule.h"

namespace awpu {

// The rule over d_rows [win.n_rows][n_pixels], window by window (expose_rule.h): window w's rows here are added up in row order
// by the one thread that owns the pixel; a window that began before these rows starts from d_carry, one that closes writes row w
// of d_frames, one that does not leaves acc in d_carry.  d_carry may be null where no window needs it, d_frames where none
// closes.  Nothing is launched where the rows hold no window.
hipError_t launch_expose(const float *d_rows, long long n_pixels, const ExposeWindows &win, int mode, float *d_carry, float *d_frames,
                         hipStream_t stream);

// A piece of an exposed run sweeps n consecutive items of the run's swept blocks, starting with block k0: the last n0 blocks of
// k0's window (all n of the piece when it ends inside that window), then whole windows of `length` blocks whose first blocks are
// w1, w1 + every, ..., the last of them cut short where the piece ends.  Its history holds, 256 samples per slot, only the
// blocks those items' snapshots read, each item's four consecutive:
//   own == false (every - length < 3: the snapshots of neighbouring windows overlap): consecutive blocks, slot s = block k0 - 3 + s
//   own == true:  n0 + 3 slots = blocks k0 - 3 .. k0 + n0 - 1, then length + 3 slots per further window = its blocks and the three
//                 in front of them
// Item i's snapshot starts at history sample 256 * item_slot(i).
struct ExposeSlots {
    int k0, n0, w1, every, length;
    bool own;
    __host__ __device__ int per_window() const { return length + 3; }
    // the block of the call that slot `slot` holds (negative: a block the ring held before the call, -1 the newest)
    __host__ __device__ int slot_block(int slot) const {
        if (!own || slot < n0 + 3) return k0 - 3 + slot;
        const int s = slot - (n0 + 3);
        return w1 + every * (s / per_window()) - 3 + s % per_window();
    }
    __host__ __device__ int item_block(int i) const { return i < n0 ? k0 + i : w1 + every * ((i - n0) / length) + (i - n0) % length; }
    __host__ __device__ int item_slot(int i) const {
        if (!own) return item_block(i) - k0;
        return i < n0 ? i : n0 + 3 + (i - n0) / length * per_window() + (i - n0) % length;
    }
    __host__ __device__ int slots(int n) const { return item_slot(n - 1) + 4; }
};

// hist[s * hist_pitch + 256 * slot + i] for slots [slot0, slot0 + n_slots): blocks >= 0 out of d_src [n_streams][src_pitch]
// (block b at column 256 * b), blocks < 0 out of the ring's snapshot d_snapshot (pitch 2048: block -4 at column 0), exactly as
// launch_watch_gather (watch_kernels.h) does with its own slot map.
hipError_t launch_expose_gather(const float *d_src, long long src_pitch, const float *d_snapshot, const ExposeSlots &map, int n_streams,
                                float *d_hist, int hist_pitch, int slot0, int n_slots, hipStream_t stream);

}  // namespace awpu
