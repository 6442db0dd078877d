// band_host.cpp -- awpu_hip_band_filter and awpu_hip_band_design: the rule of include/awpu_hip_band.h as executable C++, pure
// host code with no handle (like awpu_hip_find_peaks).  Written for reading, not for speed.  The kernel (band_kernels.hip) takes
// the same steps out of band_rule.h.  A host compiler alone takes this file.
#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC optimize("fp-contract=off")
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#include <cmath>

#include "band_rule.h"

extern "C" int awpu_hip_band_filter(const float *x, int32_t n_rows, int64_t pitch, int32_t n, const float *c, int32_t taps, float *y) {
    if (!x || !y || x == y || awpu::band_refusal(c, taps)) return AWPU_ERR_INVALID;
    if (n_rows < 1 || n < 1 || pitch < n) return AWPU_ERR_INVALID;
    for (int32_t r = 0; r < n_rows; r++) {
        const float *row = x + (size_t) r * (size_t) pitch;
        float *out = y + (size_t) r * (size_t) pitch;
        for (int32_t t = 0; t < n; t++) out[t] = awpu::band_output(c, taps, row, t);
    }
    return AWPU_OK;
}

extern "C" int awpu_hip_band_design(double lo_hz, double hi_hz, double sample_rate, int32_t taps, float *c) {
    if (!c || taps < 3 || taps > 127 || taps % 2 == 0) return AWPU_ERR_INVALID;
    if (!(sample_rate > 0.0) || !std::isfinite(sample_rate)) return AWPU_ERR_INVALID;
    if (!(lo_hz >= 0.0 && lo_hz < hi_hz && hi_hz <= sample_rate / 2.0)) return AWPU_ERR_INVALID;
    const double pi = 3.14159265358979323846;
    const int M = (taps - 1) / 2;
    const double f1 = lo_hz / sample_rate, f2 = hi_hz / sample_rate, fc = (f1 + f2) / 2.0;
    const auto sinc = [pi](double u) { return u == 0.0 ? 1.0 : std::sin(pi * u) / (pi * u); };
    double h[AWPU_BAND_MAX_TAPS];
    double re = 0.0, im = 0.0;
    for (int k = 0; k < taps; k++) {
        const double ideal = 2.0 * f2 * sinc(2.0 * f2 * (k - M)) - 2.0 * f1 * sinc(2.0 * f1 * (k - M));
        const double w = 0.54 - 0.46 * std::cos(2.0 * pi * k / (taps - 1));
        h[k] = ideal * w;
        re += h[k] * std::cos(2.0 * pi * k * fc);
        im -= h[k] * std::sin(2.0 * pi * k * fc);
    }
    const double g = std::sqrt(re * re + im * im);
    if (!(g > 0.0) || !std::isfinite(g)) return AWPU_ERR_INVALID;
    for (int k = 0; k < taps; k++) c[k] = (float) (h[k] / g);
    return AWPU_OK;
}
