// band_rule_check.cpp -- awpu_hip_band_filter and awpu_hip_band_design (csrc/band_host.cpp) at their largest and smallest
// sizes, as a program of its own: tests/test_band_cpu.py builds it with -fsanitize=address,undefined and runs it.  The buffers
// are exactly as long as the calls may touch, so a read or write past them is the sanitizer's to report.  Exit status 0 = fine.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "awpu_hip_band.h"

static int fails = 0;
#define CHECK(what)                                                     \
    do {                                                                \
        if (!(what)) {                                                  \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #what);      \
            fails++;                                                    \
        }                                                               \
    } while (0)

int main() {
    // the largest filter: 128 taps over rows longer and shorter than the taps, with a pitch wider than the rows
    {
        const int rows = 3, n = 1024, pitch = 1031, taps = AWPU_BAND_MAX_TAPS;
        std::vector<float> x((size_t) (rows - 1) * pitch + n), y(x.size(), -7.0f), c(taps);
        for (size_t i = 0; i < x.size(); i++) x[i] = (float) ((int) (i * 2654435761u % 2001u) - 1000) / 1024.0f;
        for (int k = 0; k < taps; k++) c[k] = (k & 1 ? -1.0f : 1.0f) / (float) (k + 1);
        CHECK(awpu_hip_band_filter(x.data(), rows, pitch, n, c.data(), taps, y.data()) == AWPU_OK);
        CHECK(y[0] == c[0] * x[0]);                  // one tap has a sample; the others add +0
        CHECK(y[n] == -7.0f && y[pitch - 1] == -7.0f);  // between the rows: untouched
        CHECK(y[pitch] == c[0] * x[pitch]);          // a row starts from a zero history, not from the row before it
        std::vector<float> x40(40, 1.0f), y40(40);
        CHECK(awpu_hip_band_filter(x40.data(), 1, 40, 40, c.data(), taps, y40.data()) == AWPU_OK);
    }
    // the smallest: one tap, one sample
    {
        const float x = -0.0f, c = 1.0f;
        float y = 5.0f;
        CHECK(awpu_hip_band_filter(&x, 1, 1, 1, &c, 1, &y) == AWPU_OK);
        CHECK(y == 0.0f);
        const float xs[3] = {1.5f, -2.25f, 1e-40f};
        float ys[3];
        CHECK(awpu_hip_band_filter(xs, 3, 1, 1, &c, 1, ys) == AWPU_OK);
        CHECK(std::memcmp(xs, ys, sizeof xs) == 0);
    }
    // refusals write nothing
    {
        float x[4] = {1, 2, 3, 4}, y[4] = {9, 9, 9, 9}, c[2] = {1.0f, INFINITY};
        CHECK(awpu_hip_band_filter(x, 1, 4, 4, c, 2, y) == AWPU_ERR_INVALID);
        CHECK(awpu_hip_band_filter(x, 1, 4, 4, c, 0, y) == AWPU_ERR_INVALID);
        CHECK(awpu_hip_band_filter(x, 1, 4, 4, c, AWPU_BAND_MAX_TAPS + 1, y) == AWPU_ERR_INVALID);
        CHECK(awpu_hip_band_filter(x, 1, 4, 4, c, 1, x) == AWPU_ERR_INVALID);
        CHECK(awpu_hip_band_filter(nullptr, 1, 4, 4, c, 1, y) == AWPU_ERR_INVALID);
        CHECK(awpu_hip_band_filter(x, 1, 3, 4, c, 1, y) == AWPU_ERR_INVALID);
        CHECK(y[0] == 9 && y[3] == 9);
    }
    // the design at its smallest and largest, into buffers of exactly `taps` floats
    for (int taps : {3, 127}) {
        std::vector<float> c(taps, -7.0f);
        CHECK(awpu_hip_band_design(6375.0, 9000.0, 48828.125, taps, c.data()) == AWPU_OK);
        for (int k = 0; k < taps; k++) CHECK(std::isfinite(c[k]) && c[k] == c[taps - 1 - k]);  // linear phase
        CHECK(awpu_hip_band_design(0.0, 48828.125 / 2.0, 48828.125, taps, c.data()) == AWPU_OK);   // the whole band
    }
    {
        float c[130];
        for (float &v : c) v = -7.0f;
        CHECK(awpu_hip_band_design(1000.0, 2000.0, 48828.125, 129, c) == AWPU_ERR_INVALID);
        CHECK(awpu_hip_band_design(1000.0, 2000.0, 48828.125, 64, c) == AWPU_ERR_INVALID);
        CHECK(awpu_hip_band_design(1000.0, 2000.0, 48828.125, 1, c) == AWPU_ERR_INVALID);
        CHECK(awpu_hip_band_design(2000.0, 2000.0, 48828.125, 63, c) == AWPU_ERR_INVALID);
        CHECK(awpu_hip_band_design(1000.0, 30000.0, 48828.125, 63, c) == AWPU_ERR_INVALID);
        CHECK(awpu_hip_band_design(1000.0, 2000.0, 48828.125, 63, nullptr) == AWPU_ERR_INVALID);
        for (float v : c) CHECK(v == -7.0f);
    }
    if (fails) return 1;
    std::puts("band rule: ok");
    return 0;
}
