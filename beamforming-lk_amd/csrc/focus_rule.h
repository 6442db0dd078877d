// focus_rule.h -- the arithmetic of include/awpu_hip_focus.h that the host definitions (geometry_host.cpp, focus_host.cpp) and
// the kernels (das_kernels.hip, track_kernels.hip) share, so that both evaluate the same expressions in the same order: the
// focus direction, an element's path, its delay, and the pick of a ranged source.  No HIP types: a host compiler alone takes it.
#pragma once

#include <cmath>
#include <cstdint>

#include "awpu_hip_focus.h"

#if defined(__HIPCC__)
#define AWPU_FOCUS_HD __host__ __device__
#else
#define AWPU_FOCUS_HD
#endif

namespace awpu {

constexpr double kFocusSamplesPerMetre = 48828.0 / 340.0;  // src/geometry/antenna.h:16-17, in double

// the square root of the rule: correctly rounded on either side
AWPU_FOCUS_HD inline double focus_sqrt(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __dsqrt_rn(x);
#else
    return std::sqrt(x);
#endif
}

// w = row z of Ry(-theta) times Rz(phi), from the twelve floats of awpu::pixel_rotations: m[0..8] = Rz row-major, m[9..11] = ry2
AWPU_FOCUS_HD inline void focus_direction(const float *m, double (&w)[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    for (int j = 0; j < 3; j++) {
        const double a = (double) m[9] * (double) m[j], b = (double) m[10] * (double) m[3 + j], c = (double) m[11] * (double) m[6 + j];
        w[j] = a + b + c;
    }
}

// F = distance * w
AWPU_FOCUS_HD inline void focus_point(const double (&w)[3], double distance, double (&F)[3]) {
    for (int j = 0; j < 3; j++) F[j] = distance * w[j];
}

// d_m: from the focus to the element at (x, y, z)
AWPU_FOCUS_HD inline double focus_path(const double (&F)[3], float x, float y, float z) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double dx = F[0] - (double) x, dy = F[1] - (double) y, dz = F[2] - (double) z;
    const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const double sum = xx + yy + zz;
    return focus_sqrt(sum);
}

// tau_m from the farthest element's path and its own
AWPU_FOCUS_HD inline float focus_delay(double far, double d) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double lead = far - d;
    return (float) (lead * kFocusSamplesPerMetre);
}

// a distance a focus can be at: > 0, +INFINITY included, not NaN
AWPU_FOCUS_HD inline bool focus_distance_ok(double distance) { return distance > 0.0; }
AWPU_FOCUS_HD inline bool focus_is_plane_wave(double distance) { return distance > 1.7976931348623157e308; }

// awpu_hip_range_pick for one source: p [n_dist] powers, distance [n_dist]
AWPU_FOCUS_HD inline void range_pick_one(const float *p, const double *distance, int n_dist, awpu_range_t *out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    int j = 0;
    uint32_t best = 0;
    for (int k = 0; k < n_dist; k++) {
        const float v = p[k];
        uint32_t bits;
        __builtin_memcpy(&bits, &v, sizeof bits);
        if (k == 0 || bits > best) best = bits, j = k;
    }
    const double u = focus_is_plane_wave(distance[j]) ? 0.0 : 1.0 / distance[j];
    double at = u;
    if (j > 0 && j < n_dist - 1) {
        const double a = p[j - 1], b = p[j], c = p[j + 1];
        const double den = a - 2.0 * b + c;
        double delta = den < 0.0 ? 0.5 * (a - c) / den : 0.0;
        delta = delta > 0.5 ? 0.5 : delta;
        delta = delta < -0.5 ? -0.5 : delta;
        const double before = focus_is_plane_wave(distance[j - 1]) ? 0.0 : 1.0 / distance[j - 1];
        const double after = focus_is_plane_wave(distance[j + 1]) ? 0.0 : 1.0 / distance[j + 1];
        const double step = delta >= 0.0 ? after - u : u - before;
        at = u + delta * step;
    }
    out->index = j;
    out->power = p[j];
    out->distance = at > 0.0 ? 1.0 / at : (double) __builtin_inff();
}

AWPU_FOCUS_HD inline void range_unused(awpu_range_t *out) {
    out->index = -1;
    out->power = 0.0f;
    out->distance = 0.0;
}

}  // namespace awpu
