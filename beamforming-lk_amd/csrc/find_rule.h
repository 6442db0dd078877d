// find_rule.h -- the arithmetic of include/awpu_hip_find.h that the host definition (find_host.cpp) and the kernel
// (find_kernels.hip) share, so that both evaluate the same expressions in the same order: the order's key, the argument checks,
// the refinement and the direction.  No HIP types: a host compiler alone takes it.
#pragma once

#include <cmath>
#include <cstdint>

#include "awpu_hip_find.h"

#if defined(__HIPCC__)
#define AWPU_FIND_HD __host__ __device__
#else
#define AWPU_FIND_HD
#endif

namespace awpu {

// a beats b  <=>  find_key(bits a, a) > find_key(bits b, b); keys of different pixels differ; 0 is no pixel's key where p > 0
AWPU_FIND_HD inline unsigned long long find_key(uint32_t bits, uint32_t pixel) {
    return (unsigned long long) bits << 32 | (0xFFFFFFFFu - pixel);
}
AWPU_FIND_HD inline uint32_t find_key_pixel(unsigned long long key) { return 0xFFFFFFFFu - (uint32_t) key; }

// the ratio threshold below the frame's maximum m: min_ratio = 0 is no threshold whatever m is (0 * inf and 0 * NaN are NaN, and
// a NaN threshold lets no pixel through); otherwise one fp32 multiply
AWPU_FIND_HD inline float find_floor_ratio(float min_ratio, float m) { return min_ratio == 0.0f ? 0.0f : min_ratio * m; }

// what is wrong with a request, or null
inline const char *find_refusal(const awpu_find_t *f) {
    if (!f) return "null argument";
    if (f->rows < 1 || f->cols < 1) return "rows and cols must be positive";
    if ((long long) f->rows * f->cols > AWPU_FIND_MAX_PIXELS) return "rows x cols above AWPU_FIND_MAX_PIXELS";
    if (f->radius < 1 || f->radius > AWPU_FIND_MAX_RADIUS) return "radius outside [1, 8]";
    if (f->max_sources < 1 || f->max_sources > AWPU_FIND_MAX_SOURCES) return "max_sources outside [1, 32]";
    if (!(f->min_ratio >= 0.0f && f->min_ratio <= 1.0f)) return "min_ratio outside [0, 1]";
    if (!(f->min_power >= 0.0f && f->min_power <= 3.402823466e38f)) return "min_power negative or not finite";
    if (!(f->fov_deg > 0.0f && f->fov_deg <= 180.0f)) return "fov_deg outside (0, 180]";
    return nullptr;
}

// the pitch of the sine-space grid along an axis of n pixels (awpu_hip_build_delay_table's sep_rows / sep_cols); host only, so
// that the kernel gets the host's sine
inline double find_separation(float fov_deg, int n) {
    const double fov = static_cast<double>(fov_deg) * (M_PI / 180.0);
    return std::sin(fov / 2.0) / (static_cast<double>(n) / 2.0);
}

// the sub-pixel offset along one axis from the powers before, at and after the peak
AWPU_FIND_HD inline double find_offset(float before, float at, float after) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double a = before, b = at, c = after;
    const double den = a - 2.0 * b + c;
    double d = den < 0.0 ? 0.5 * (a - c) / den : 0.0;
    d = d > 0.5 ? 0.5 : d;
    return d < -0.5 ? -0.5 : d;
}

// entry `out` for the peak at pixel (r, c) of the frame p
AWPU_FIND_HD inline void find_describe(const float *p, int rows, int cols, int r, int c, double sep_rows, double sep_cols, awpu_source_t *out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int i = r * cols + c;
    const double d_row = r > 0 && r < rows - 1 ? find_offset(p[i - cols], p[i], p[i + cols]) : 0.0;
    const double d_col = c > 0 && c < cols - 1 ? find_offset(p[i - 1], p[i], p[i + 1]) : 0.0;
    const double row = r + d_row, col = c + d_col;
    const double y = row * sep_rows - rows * sep_rows / 2.0 + sep_rows / 2.0;
    const double x = col * sep_cols - cols * sep_cols / 2.0 + sep_cols / 2.0;
    double norm = sqrt(x * x + y * y);
    if (norm > 1.0) norm = 1.0;
    out->pixel = i;
    out->power = p[i];
    out->row = row;
    out->col = col;
    out->theta = asin(norm);
    out->phi = x == 0.0 && y == 0.0 ? 0.0 : atan2(y, x);
}

AWPU_FIND_HD inline void find_unused(awpu_source_t *out) {
    out->pixel = -1;
    out->power = 0.0f;
    out->row = out->col = out->theta = out->phi = 0.0;
}

}  // namespace awpu
