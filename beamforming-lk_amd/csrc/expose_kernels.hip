// expose_kernels.hip -- exposure (include/awpu_hip_expose.h): the power rows of a window of blocks added up, or their maximum
// taken, per pixel in block order.  A thread owns four consecutive pixels (the last n_pixels % 4 of a row: one pixel each) through
// all rows of a window, with acc in registers, so the add order is the rule's by construction: no atomics, no cross-lane sums.
// Rows are read with 16-byte loads at 4-byte alignment (a row of n_pixels % 4 != 0 floats starts at no better), consecutive lanes
// reading consecutive 16 bytes; frames and the carry row are written the same way.  The grid is pixel tiles x windows.  Only the
// first window of the rows can start from the carry row and only the last can end in it: the workgroups of grid row 0 take both,
// one after the other, so the thread that reads a pixel's carry is the thread that writes it.
// The step and the closing divide are expose_rule.h's, the host definition's own: contraction is off there (there is nothing to
// contract in an add or a compare, and it stays that way), and the divide is hipcc's correctly rounded fp32 division, which this
// file's build never trades for a reciprocal (no fast-math flag, no __fdividef).
#include "expose_kernels.h"

#include <algorithm>

namespace awpu {

namespace {

typedef float Floats4 __attribute__((ext_vector_type(4), aligned(4)));

struct ExposeArgs {
    const float *rows;
    float *carry, *frames;
    long long n_pixels;
    ExposeWindows win;
    int mode;
    float length_f;
};

__device__ inline float stepped(float acc, float p, int mode) { return expose_step(acc, p, mode); }
__device__ inline Floats4 stepped(Floats4 acc, Floats4 p, int mode) {
    return Floats4{expose_step(acc.x, p.x, mode), expose_step(acc.y, p.y, mode), expose_step(acc.z, p.z, mode),
                   expose_step(acc.w, p.w, mode)};
}
__device__ inline float closed(float acc, float length_f, int mode) { return expose_close(acc, length_f, mode); }
__device__ inline Floats4 closed(Floats4 acc, float length_f, int mode) {
    return Floats4{expose_close(acc.x, length_f, mode), expose_close(acc.y, length_f, mode),
                   expose_close(acc.z, length_f, mode), expose_close(acc.w, length_f, mode)};
}

// window w for the pixels at float offset `at` of a row, T = one pixel or four
template <class T>
__device__ inline void expose_window(const ExposeArgs &a, int w, long long at) {
    const int lo = a.win.lo(w), hi = a.win.hi(w);
    const float *p = a.rows + (long long) lo * a.n_pixels + at;
    T acc;
    int r = lo;
    if (a.win.carried(w)) {
        acc = *reinterpret_cast<const T *>(a.carry + at);
    } else {
        acc = *reinterpret_cast<const T *>(p);  // q == 0: acc = p_k
        r++, p += a.n_pixels;
    }
    for (; r < hi; r++, p += a.n_pixels) acc = stepped(acc, *reinterpret_cast<const T *>(p), a.mode);
    if (a.win.closes(w))
        *reinterpret_cast<T *>(a.frames + (long long) w * a.n_pixels + at) = closed(acc, a.length_f, a.mode);
    else
        *reinterpret_cast<T *>(a.carry + at) = acc;
}

__device__ inline void expose_unit(const ExposeArgs &a, int w, long long unit, long long n_vec) {
    if (unit < n_vec)
        expose_window<Floats4>(a, w, 4 * unit);
    else
        expose_window<float>(a, w, 4 * n_vec + (unit - n_vec));
}

__global__ __launch_bounds__(256) void expose_kernel(const ExposeArgs a) {
    const long long n_vec = a.n_pixels / 4, units = n_vec + a.n_pixels % 4;
    const long long unit = (long long) blockIdx.x * 256 + threadIdx.x;
    if (unit >= units) return;
    const int n_win = a.win.count();
    if (blockIdx.y == 0) {
        expose_unit(a, 0, unit, n_vec);
        if (n_win > 1) expose_unit(a, n_win - 1, unit, n_vec);
    }
    for (int w = 1 + (int) blockIdx.y; w < n_win - 1; w += (int) gridDim.y) expose_unit(a, w, unit, n_vec);
}

__global__ void expose_gather_kernel(const float *src, long long src_pitch, const float *snapshot, const ExposeSlots map, float *hist,
                                     int hist_pitch, int slot0) {
    const int slot = slot0 + blockIdx.x, s = blockIdx.y, i = threadIdx.x;
    const int blk = map.slot_block(slot);
    const float v = blk < 0 ? snapshot[(size_t) s * 2048 + 256 * (4 + blk) + i] : src[(size_t) s * src_pitch + 256 * (size_t) blk + i];
    hist[(size_t) s * hist_pitch + 256 * (size_t) slot + i] = v;
}

}  // namespace

hipError_t launch_expose(const float *d_rows, long long n_pixels, const ExposeWindows &win, int mode, float *d_carry, float *d_frames,
                         hipStream_t stream) {
    if (!d_rows || n_pixels < 1 || win.n_rows < 1 || win.length < 1 || win.stride < win.length || win.base < -(win.length - 1))
        return hipErrorInvalidValue;
    if (mode != AWPU_EXPOSE_MEAN && mode != AWPU_EXPOSE_PEAK) return hipErrorInvalidValue;
    const int n_win = win.count();
    if (n_win == 0) return hipSuccess;
    // who reads or writes the carry row, and whether any frame is written: each needs its buffer
    if ((win.carried(0) || !win.closes(n_win - 1)) && !d_carry) return hipErrorInvalidValue;
    if (win.closes(0) && !d_frames) return hipErrorInvalidValue;
    const long long units = n_pixels / 4 + n_pixels % 4, tiles = (units + 255) / 256;
    if (tiles > 0x7FFFFFFF) return hipErrorInvalidValue;
    const ExposeArgs a{d_rows, d_carry, d_frames, n_pixels, win, mode, (float) win.length};
    hipLaunchKernelGGL(expose_kernel, dim3((unsigned) tiles, (unsigned) std::min(std::max(n_win - 1, 1), 1024)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_expose_gather(const float *d_src, long long src_pitch, const float *d_snapshot, const ExposeSlots &map, int n_streams,
                                float *d_hist, int hist_pitch, int slot0, int n_slots, hipStream_t stream) {
    // (a block below -4 is not in the ring: slot 0 holds block k0 - 3 >= -3)
    if (map.k0 < 0 || map.n0 < 1 || map.length < 1 || map.every < map.length || n_streams < 1 || n_streams > 65535 || slot0 < 0 || n_slots < 1 ||
        256 * (slot0 + n_slots) > hist_pitch)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(expose_gather_kernel, dim3(n_slots, n_streams), dim3(256), 0, stream, d_src, src_pitch, d_snapshot, map, d_hist,
                       hist_pitch, slot0);
    return hipGetLastError();
}

}  // namespace awpu
