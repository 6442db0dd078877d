// spectral_rule_check.cpp -- awpu_hip_spectral_compose (csrc/spectral_host.cpp) and the checks of csrc/spectral_rule.h at their
// largest and smallest sizes, as a program of its own: tests/test_spectral_cpu.py builds it with -fsanitize=address,undefined and
// runs it.  The buffers are exactly as long as the calls may touch, so a read or write past them is the sanitizer's to report.
// Exit status 0 = fine.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "awpu_hip_spectral.h"
#include "spectral_rule.h"

static int fails = 0;
#define CHECK(what)                                                     \
    do {                                                                \
        if (!(what)) {                                                  \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #what);      \
            fails++;                                                    \
        }                                                               \
    } while (0)

int main() {
    // the largest: four bands of a 512 x 512 frame, planes a pitch wider than a frame apart, the last one ending with its last pixel
    {
        const int n = 512 * 512, bands = AWPU_SPECTRAL_MAX_BANDS;
        const int64_t pitch = n + 5;
        std::vector<float> power((size_t) (bands - 1) * pitch + n);
        for (size_t i = 0; i < power.size(); i++) power[i] = (float) (i * 2654435761u % 2001u) / 64.0f;
        std::vector<uint8_t> image((size_t) n * 3, 7), dominant(n, 7), flat((size_t) n * 3);
        const int32_t channel[3] = {3, 0, 2};
        for (int32_t scale : {AWPU_SPECTRAL_SCALE_COMMON, AWPU_SPECTRAL_SCALE_PER_BAND}) {
            CHECK(awpu_hip_spectral_compose(power.data(), pitch, bands, n, channel, scale, image.data(), dominant.data()) == AWPU_OK);
            // against awpu_hip_heatmap_u8's expression, restated: the shown planes end to end, or each on its own
            float max_of[3] = {0, 0, 0}, common = 0;
            for (int c = 0; c < 3; c++)
                for (int i = 0; i < n; i++) max_of[c] = std::fmax(max_of[c], power[channel[c] * pitch + i]);
            for (int c = 0; c < 3; c++) common = std::fmax(common, max_of[c]);
            bool same = true, dom = true;
            for (int i = 0; i < n; i++) {
                for (int c = 0; c < 3; c++) {
                    const double level = (double) (power[channel[c] * pitch + i] / (scale == AWPU_SPECTRAL_SCALE_COMMON ? common : max_of[c])) * 255.0;
                    same &= image[(size_t) i * 3 + c] == (uint8_t) (level > 255.0 ? 255.0 : level);
                }
                int best = 0;
                for (int b = 1; b < bands; b++)
                    if (power[b * pitch + i] > power[best * pitch + i]) best = b;
                dom &= dominant[i] == best;
            }
            CHECK(same);
            CHECK(dom);
        }
        // either output alone
        CHECK(awpu_hip_spectral_compose(power.data(), pitch, bands, n, channel, 0, image.data(), nullptr) == AWPU_OK);
        CHECK(awpu_hip_spectral_compose(power.data(), pitch, bands, n, channel, 0, nullptr, dominant.data()) == AWPU_OK);
    }
    // the smallest: one band, one pixel; nothing shown
    {
        const float p = 2.5f;
        uint8_t image[3] = {9, 9, 9}, dominant = 9;
        const int32_t only[3] = {0, -1, 0}, none[3] = {-1, -1, -1};
        CHECK(awpu_hip_spectral_compose(&p, 0, 1, 1, only, AWPU_SPECTRAL_SCALE_COMMON, image, &dominant) == AWPU_OK);
        CHECK(image[0] == 255 && image[1] == 0 && image[2] == 255 && dominant == 0);
        CHECK(awpu_hip_spectral_compose(&p, 0, 1, 1, none, AWPU_SPECTRAL_SCALE_PER_BAND, image, &dominant) == AWPU_OK);
        CHECK(image[0] == 0 && image[1] == 0 && image[2] == 0 && dominant == 0);
        const float zero = 0.0f;
        CHECK(awpu_hip_spectral_compose(&zero, 0, 1, 1, only, AWPU_SPECTRAL_SCALE_COMMON, image, &dominant) == AWPU_OK);
        CHECK(image[0] == 0 && image[2] == 0 && dominant == 0);  // 0 / 0: level 0
    }
    // refusals write nothing
    {
        const float p[8] = {1, 2, 3, 4, 5, 6, 7, 8};
        uint8_t image[12], dominant[4];
        std::memset(image, 9, sizeof image), std::memset(dominant, 9, sizeof dominant);
        const int32_t good[3] = {0, 1, -1}, high[3] = {0, 2, 1}, low[3] = {-2, 0, 1};
        CHECK(awpu_hip_spectral_compose(nullptr, 4, 2, 4, good, 0, image, dominant) == AWPU_ERR_INVALID);
        CHECK(awpu_hip_spectral_compose(p, 4, 2, 4, nullptr, 0, image, dominant) == AWPU_ERR_INVALID);
        CHECK(awpu_hip_spectral_compose(p, 4, 2, 4, good, 0, nullptr, nullptr) == AWPU_ERR_INVALID);
        CHECK(awpu_hip_spectral_compose(p, 4, 2, 0, good, 0, image, dominant) == AWPU_ERR_INVALID);
        CHECK(awpu_hip_spectral_compose(p, 4, 0, 4, good, 0, image, dominant) == AWPU_ERR_INVALID);
        CHECK(awpu_hip_spectral_compose(p, 4, 5, 4, good, 0, image, dominant) == AWPU_ERR_INVALID);
        CHECK(awpu_hip_spectral_compose(p, 4, 2, 4, high, 0, image, dominant) == AWPU_ERR_INVALID);
        CHECK(awpu_hip_spectral_compose(p, 4, 2, 4, low, 0, image, dominant) == AWPU_ERR_INVALID);
        CHECK(awpu_hip_spectral_compose(p, 4, 2, 4, good, 2, image, dominant) == AWPU_ERR_INVALID);
        for (uint8_t v : image) CHECK(v == 9);
        for (uint8_t v : dominant) CHECK(v == 9);
    }
    // the check of a set of bands reads exactly taps[b] coefficients of the n_bands bands, and nothing of the others
    {
        std::vector<float> longest(AWPU_BAND_MAX_TAPS, 0.5f), one(1, 1.0f), bad(3, 1.0f);
        bad[2] = INFINITY;
        awpu_spectral_t sp{};
        sp.n_bands = 2;
        sp.taps[0] = AWPU_BAND_MAX_TAPS, sp.coef[0] = longest.data();
        sp.taps[1] = 1, sp.coef[1] = one.data();
        sp.taps[2] = 1000, sp.coef[2] = nullptr;  // (not a band of the set)
        sp.channel[0] = 0, sp.channel[1] = 1, sp.channel[2] = -1;
        sp.scale = AWPU_SPECTRAL_SCALE_PER_BAND;
        CHECK(awpu::spectral_refusal(&sp) == nullptr);
        CHECK(awpu::spectral_refusal(nullptr) != nullptr);
        sp.coef[1] = bad.data(), sp.taps[1] = 2;
        CHECK(awpu::spectral_refusal(&sp) == nullptr);  // the infinite coefficient lies behind the band's taps
        sp.taps[1] = 3;
        CHECK(awpu::spectral_refusal(&sp) != nullptr);
        sp.taps[1] = AWPU_BAND_MAX_TAPS + 1;
        CHECK(awpu::spectral_refusal(&sp) != nullptr);
        sp.taps[1] = 2, sp.coef[1] = nullptr;
        CHECK(awpu::spectral_refusal(&sp) != nullptr);
        sp.coef[1] = one.data(), sp.taps[1] = 1;
        for (int32_t n_bands : {0, AWPU_SPECTRAL_MAX_BANDS + 1}) {
            sp.n_bands = n_bands;
            CHECK(awpu::spectral_refusal(&sp) != nullptr);
        }
        sp.n_bands = 2, sp.channel[2] = 2;
        CHECK(awpu::spectral_refusal(&sp) != nullptr);
        sp.channel[2] = 1, sp.scale = 7;
        CHECK(awpu::spectral_refusal(&sp) != nullptr);
    }
    if (fails) return 1;
    std::puts("spectral rule: ok");
    return 0;
}
