// find_kernels.hip -- finding sources (include/awpu_hip_find.h): the strongest peaks of every frame of a batch of power rows,
// one workgroup per frame, behind the sweep that wrote them (the frame -- 64 KB at 128 x 128 -- comes out of the L2).
//   1. the frame's maximum: a block-wide maximum of the order's 64-bit key (find_rule.h: power bits, then lower index);
//   2. the peak flags: a wave takes 64 consecutive pixels at a time, a lane tests its pixel against the thresholds, then against
//      its 3 x 3 window and -- only where it beats that -- against the whole (2 * radius + 1)^2 window; the wave's ballot goes
//      into an LDS bitmap as two plain stores of lane 0;
//   3. max_sources rounds of a block-wide maximum of the key over the flagged pixels, each below the winner of the round before
//      (a round that finds nothing leaves key 0, and so do all after it);
//   4. the first max_sources lanes describe one winner each in fp64 (find_rule.h: the host definition's own expressions).
// Every loop's trip count follows from the shape alone; keys are distinct, so no maximum depends on the order it is taken in;
// nothing is written with atomics.  Frames are independent.
#include "find_kernels.h"

#include "find_rule.h"

namespace awpu {

namespace {

constexpr int kFindWaves = kFindThreads / 64;

// the maximum over the workgroup, in every thread; `slots` [kFindWaves] must not be in use by a maximum still being read
__device__ inline unsigned long long block_max(unsigned long long v, unsigned long long *slots) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long best = 0;
#pragma unroll
    for (int w = 0; w < kFindWaves; w++) best = slots[w] > best ? slots[w] : best;
    return best;
}

// Does pixel i = (r, c), of power bits `bi`, beat every other pixel of its window of radius R?  Offsets that leave the grid are
// clamped onto its edge -- a pixel of the window again, or the pixel itself -- so the trip counts are the same for every lane
// and the loads of a row of the window are in flight together.
__device__ inline bool loses_to(const uint32_t *p, int rows, int cols, int r, int c, int dr, int dc, uint32_t bi, int i) {
    const int j = min(max(r + dr, 0), rows - 1) * cols + min(max(c + dc, 0), cols - 1);
    const uint32_t bj = p[j];
    return bj > bi || (bj == bi && j < i);
}
__device__ inline bool beats_3x3(const uint32_t *p, int rows, int cols, int r, int c, uint32_t bi, int i) {
    bool lost = false;
#pragma unroll
    for (int dr = -1; dr <= 1; dr++)
#pragma unroll
        for (int dc = -1; dc <= 1; dc++) lost |= loses_to(p, rows, cols, r, c, dr, dc, bi, i);
    return !lost;
}
__device__ inline bool beats_window(const uint32_t *p, int rows, int cols, int r, int c, int R, uint32_t bi, int i) {
    bool lost = false;
    for (int dr = -R; dr <= R; dr++) {
#pragma unroll 5
        for (int dc = -R; dc <= R; dc++) lost |= loses_to(p, rows, cols, r, c, dr, dc, bi, i);
    }
    return !lost;
}

}  // namespace

__global__ __launch_bounds__(kFindThreads) void find_peaks_kernel(const float *power, int rows, int cols, int radius, int max_sources,
                                                                   float min_power, float min_ratio, double sep_rows, double sep_cols,
                                                                   awpu_source_t *sources, int32_t *count) {
    extern __shared__ uint32_t flags[];  // [2 * ceil(n / 64)]: bit (i & 31) of word i >> 5 = pixel i is a peak
    __shared__ unsigned long long slots[2][kFindWaves];
    __shared__ unsigned long long winners[AWPU_FIND_MAX_SOURCES];
    const int n = rows * cols, tid = threadIdx.x, lane = tid & 63;
    const float *frame = power + (size_t) blockIdx.x * n;
    const uint32_t *p = reinterpret_cast<const uint32_t *>(frame);

    unsigned long long best = 0;
    for (int i = tid; i < n; i += kFindThreads) {
        const unsigned long long key = find_key(p[i], i);
        best = key > best ? key : best;
    }
    best = block_max(best, slots[0]);
    const float floor_ratio = find_floor_ratio(min_ratio, __uint_as_float((uint32_t) (best >> 32)));

    for (int base = (tid >> 6) * 64; base < n; base += kFindThreads) {  // (the same for every lane of a wave)
        const int i = base + lane;
        bool peak = false;
        if (i < n) {
            const uint32_t bi = p[i];
            const float v = __uint_as_float(bi);
            const int r = i / cols, c = i - r * cols;
            peak = v > 0.0f && v >= min_power && v >= floor_ratio;
            if (peak) peak = beats_3x3(p, rows, cols, r, c, bi, i);
            if (peak && radius > 1) peak = beats_window(p, rows, cols, r, c, radius, bi, i);
        }
        const unsigned long long mask = __ballot(peak);
        if (lane == 0) {
            flags[base >> 5] = (uint32_t) mask;
            flags[(base >> 5) + 1] = (uint32_t) (mask >> 32);
        }
    }
    __syncthreads();

    unsigned long long below = ~0ull;
    for (int k = 0; k < max_sources; k++) {
        unsigned long long pick = 0;
        for (int i = tid; i < n; i += kFindThreads) {
            if (flags[i >> 5] >> (i & 31) & 1) {
                const unsigned long long key = find_key(p[i], i);
                pick = key < below && key > pick ? key : pick;
            }
        }
        pick = block_max(pick, slots[k & 1]);  // (round k + 1 writes the other slots; round k + 2 comes behind round k + 1's barrier)
        if (tid == 0) winners[k] = pick;
        below = pick;  // 0: nothing is below it
    }
    __syncthreads();

    if (tid < 64) {
        const unsigned long long key = tid < max_sources ? winners[tid] : 0;
        const unsigned long long found = __ballot(key != 0);
        if (tid == 0) count[blockIdx.x] = __popcll(found);
        if (tid < max_sources) {
            awpu_source_t *out = sources + (size_t) blockIdx.x * max_sources + tid;
            if (key != 0) {
                const int i = (int) find_key_pixel(key);
                find_describe(frame, rows, cols, i / cols, i - (i / cols) * cols, sep_rows, sep_cols, out);
            } else {
                find_unused(out);
            }
        }
    }
}

hipError_t launch_find_peaks(const float *d_power, int n_frames, const awpu_find_t &f, awpu_source_t *d_sources, int32_t *d_count,
                             hipStream_t stream) {
    if (!d_power || !d_sources || !d_count || n_frames < 1 || find_refusal(&f)) return hipErrorInvalidValue;
    const int n = f.rows * f.cols;
    const size_t lds = (size_t) (n + 63) / 64 * 8;
    if (lds > AWPU_FIND_MAX_PIXELS / 8) return hipErrorInvalidValue;
    hipLaunchKernelGGL(find_peaks_kernel, dim3(n_frames), dim3(kFindThreads), lds, stream, d_power, f.rows, f.cols, f.radius, f.max_sources,
                       f.min_power, f.min_ratio, find_separation(f.fov_deg, f.rows), find_separation(f.fov_deg, f.cols), d_sources, d_count);
    return hipGetLastError();
}

}  // namespace awpu
