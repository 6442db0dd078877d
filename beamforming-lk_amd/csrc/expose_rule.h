// expose_rule.h -- the arithmetic of include/awpu_hip_expose.h that the host definition (expose_host.cpp), the kernel
// (expose_kernels.hip) and the run (awpu_runs.cpp) share: the argument checks, the counts, the plan of a block (t, q, j), the
// same plan seen window by window, and the per-pixel step.  No HIP types: a host compiler alone takes it.
#pragma once

#include <cstdint>

#include "awpu_hip_expose.h"

#if defined(__HIPCC__)
#define AWPU_EXPOSE_HD __host__ __device__
#else
#define AWPU_EXPOSE_HD
#endif

namespace awpu {

// what is wrong with a request, or null
inline const char *expose_refusal(const awpu_expose_t *e, int32_t every) {
    if (!e) return "null argument";
    if (e->length < 1 || e->length > every) return "length outside [1, every]";
    if (e->mode != AWPU_EXPOSE_MEAN && e->mode != AWPU_EXPOSE_PEAK) return "mode is AWPU_EXPOSE_MEAN or AWPU_EXPOSE_PEAK";
    return nullptr;
}

// what awpu_hip_expose_count answers (its arguments checked: n_blocks >= 1, first >= 0, 1 <= length <= every)
struct ExposeCount {
    int32_t n_frames, next_first, carry_in, carry_out, n_swept;
};
inline ExposeCount expose_count(int32_t n_blocks, int32_t first, int32_t every, int32_t length) {
    const int64_t L = length, E = every;
    const int64_t shown = first >= n_blocks ? 0 : ((int64_t) n_blocks - first + E - 1) / E;
    const int64_t next = first + shown * E - n_blocks;
    // t = k - first + L - 1 runs over [t0, t1]; below(T) = how many t in [0, T) have t % every < L
    const int64_t t0 = L - 1 - first, t1 = t0 + n_blocks - 1;
    const auto below = [&](int64_t T) { return T / E * L + (T % E < L ? T % E : L); };
    const int64_t swept = t1 < 0 ? 0 : below(t1 + 1) - below(t0 > 0 ? t0 : 0);
    return {(int32_t) shown, (int32_t) next, (int32_t) (t0 > 0 ? t0 : 0), (int32_t) (L - 1 - next > 0 ? L - 1 - next : 0), (int32_t) swept};
}

// the plan of block k of a call: false = skipped; else q = its place in its window and j = the window's frame
AWPU_EXPOSE_HD inline bool expose_block(int64_t k, int32_t first, int32_t every, int32_t length, int32_t *q, int32_t *j) {
    const int64_t t = k - first + length - 1;
    if (t < 0 || t % every >= length) return false;
    *q = (int32_t) (t % every), *j = (int32_t) (t / every);
    return true;
}

// The same plan window by window, over n_rows rows of which window w's q = 0 row is row base + w * stride (rows outside
// [0, n_rows) belong to other calls): a whole call's rows have base = first - (L - 1) and stride = every; the swept rows of a
// piece of a run, which hold no skipped block, have base = -(the first row's q) and stride = L.  base >= -(L - 1).
struct ExposeWindows {
    int32_t n_rows, base, stride, length;
    AWPU_EXPOSE_HD int64_t start(int32_t w) const { return base + (int64_t) w * stride; }
    AWPU_EXPOSE_HD int32_t count() const { return base >= n_rows ? 0 : (int32_t) (((int64_t) n_rows - base + stride - 1) / stride); }
    AWPU_EXPOSE_HD int32_t lo(int32_t w) const { return (int32_t) (start(w) > 0 ? start(w) : 0); }                    // its rows here: [lo, hi)
    AWPU_EXPOSE_HD int32_t hi(int32_t w) const { return (int32_t) (start(w) + length < n_rows ? start(w) + length : n_rows); }
    AWPU_EXPOSE_HD bool carried(int32_t w) const { return start(w) < 0; }                  // acc comes out of the carry row (window 0 only)
    AWPU_EXPOSE_HD bool closes(int32_t w) const { return start(w) + length <= n_rows; }    // frame w; else acc goes into the carry row (the last only)
};

AWPU_EXPOSE_HD inline uint32_t expose_bits(float v) {
    uint32_t u;
    __builtin_memcpy(&u, &v, sizeof u);
    return u;
}

// acc after a block that is not its window's first
AWPU_EXPOSE_HD inline float expose_step(float acc, float p, int32_t mode) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (mode == AWPU_EXPOSE_MEAN) return acc + p;
    return expose_bits(p) > expose_bits(acc) ? p : acc;
}

// the frame's value out of acc after its window's last block; length_f = (float) L
AWPU_EXPOSE_HD inline float expose_close(float acc, float length_f, int32_t mode) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return mode == AWPU_EXPOSE_MEAN ? acc / length_f : acc;
}

}  // namespace awpu
