// cohere_rule_check.cpp -- awpu_hip_cohere_host (csrc/cohere_host.cpp, cohere_rule.h) as a program of its own, meant to be built
// with -fsanitize=address,undefined: every buffer exactly as long as the header says, entries at both ends of the history (off = 0
// and off = hist - 257: the rule reads x[0 .. 256] and not a float more), the smallest sizes (one pixel, one mic, hist 257), a
// ragged list with gains, null outputs, and the refusals -- which must leave the outputs as they were.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cohere_rule.h"

namespace {

int failures = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                              \
        }                                                            \
    } while (0)

float sample(int b, int s, int t) { return (float) (((b * 7 + s * 131 + t * 17) % 199) - 99) * 0.0078125f; }

struct Shape {
    int batch, n_streams, hist, stride, n_pixels;
    std::vector<int32_t> index;
    bool gains;
};

void run(const Shape &sh) {
    const int U = (int) sh.index.size();
    std::vector<float> frames((size_t) sh.batch * sh.n_streams * sh.hist);
    for (int b = 0; b < sh.batch; b++)
        for (int s = 0; s < sh.n_streams; s++)
            for (int t = 0; t < sh.hist; t++) frames[((size_t) b * sh.n_streams + s) * sh.hist + t] = sample(b, s, t);
    std::vector<int32_t> off((size_t) sh.n_pixels * sh.stride);
    std::vector<float> frac(off.size());
    const int last = sh.hist - 257;
    for (int p = 0; p < sh.n_pixels; p++)
        for (int m = 0; m < sh.stride; m++) {
            const int k = p * 5 + m * 3;
            off[(size_t) p * sh.stride + m] = k % 3 == 0 ? 0 : (k % 3 == 1 ? last : (k * 37) % (last + 1));
            frac[(size_t) p * sh.stride + m] = k % 4 == 0 ? 0.0f : (k % 4 == 1 ? 1.0f : (float) (k % 11) / 11.0f);
        }
    std::vector<float> gain(U);
    for (int s = 0; s < U; s++) gain[s] = 0.5f + 0.25f * (float) (s % 5);
    const size_t n = (size_t) sh.batch * sh.n_pixels;
    std::vector<float> power(n), coherence(n), weighted(n), sums(n * 256), energy(n * 256);
    const float *g = sh.gains ? gain.data() : nullptr;
    CHECK(awpu_hip_cohere_host(frames.data(), sh.batch, sh.n_streams, sh.hist, off.data(), frac.data(), sh.stride, sh.n_pixels, sh.index.data(), U, g,
                               power.data(), coherence.data(), weighted.data(), sums.data(), energy.data()) == AWPU_OK);
    for (size_t i = 0; i < n; i++) {
        CHECK(coherence[i] >= 0.0f && coherence[i] <= 1.0f);
        CHECK(weighted[i] == power[i] * coherence[i]);
        CHECK(energy[i * 256] == 0.0f && energy[i * 256 + 255] == 0.0f);
        if (U == 1) {  // num and den are the same 254 numbers
            float den = 0.0f;
            for (int k = 1; k < 255; k++) den = den + energy[i * 256 + k];
            CHECK(coherence[i] == (den > 0.0f ? 1.0f : 0.0f));
        }
    }
    // every output on its own gives the bits it gives beside the others
    std::vector<float> alone(n * 256);
    float *outs[5] = {power.data(), coherence.data(), weighted.data(), sums.data(), energy.data()};
    for (int k = 0; k < 5; k++) {
        float *o[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        o[k] = alone.data();
        CHECK(awpu_hip_cohere_host(frames.data(), sh.batch, sh.n_streams, sh.hist, off.data(), frac.data(), sh.stride, sh.n_pixels, sh.index.data(), U,
                                   g, o[0], o[1], o[2], o[3], o[4]) == AWPU_OK);
        CHECK(std::memcmp(alone.data(), outs[k], (k < 3 ? n : n * 256) * sizeof(float)) == 0);
    }
    // refusals write nothing
    std::vector<float> keep = power;
    std::vector<int32_t> bad_off = off;
    bad_off[(size_t) (sh.n_pixels - 1) * sh.stride + sh.index[U - 1]] = last + 1;
    CHECK(awpu_hip_cohere_host(frames.data(), sh.batch, sh.n_streams, sh.hist, bad_off.data(), frac.data(), sh.stride, sh.n_pixels, sh.index.data(), U,
                               g, power.data(), nullptr, nullptr, nullptr, nullptr) == AWPU_ERR_RANGE);
    bad_off[(size_t) (sh.n_pixels - 1) * sh.stride + sh.index[U - 1]] = -1;
    CHECK(awpu_hip_cohere_host(frames.data(), sh.batch, sh.n_streams, sh.hist, bad_off.data(), frac.data(), sh.stride, sh.n_pixels, sh.index.data(), U,
                               g, power.data(), nullptr, nullptr, nullptr, nullptr) == AWPU_ERR_RANGE);
    for (float f : {-0.25f, 1.5f, NAN}) {
        std::vector<float> bad_frac = frac;
        bad_frac[(size_t) (sh.n_pixels - 1) * sh.stride + sh.index[0]] = f;
        CHECK(awpu_hip_cohere_host(frames.data(), sh.batch, sh.n_streams, sh.hist, off.data(), bad_frac.data(), sh.stride, sh.n_pixels,
                                   sh.index.data(), U, g, power.data(), nullptr, nullptr, nullptr, nullptr) == AWPU_ERR_INVALID);
    }
    CHECK(awpu_hip_cohere_host(nullptr, sh.batch, sh.n_streams, sh.hist, off.data(), frac.data(), sh.stride, sh.n_pixels, sh.index.data(), U, g,
                               power.data(), nullptr, nullptr, nullptr, nullptr) == AWPU_ERR_INVALID);
    CHECK(awpu_hip_cohere_host(frames.data(), 0, sh.n_streams, sh.hist, off.data(), frac.data(), sh.stride, sh.n_pixels, sh.index.data(), U, g,
                               power.data(), nullptr, nullptr, nullptr, nullptr) == AWPU_ERR_INVALID);
    CHECK(awpu_hip_cohere_host(frames.data(), sh.batch, sh.n_streams, 256, off.data(), frac.data(), sh.stride, sh.n_pixels, sh.index.data(), U, g,
                               power.data(), nullptr, nullptr, nullptr, nullptr) == AWPU_ERR_INVALID);
    CHECK(keep == power);
}

}  // namespace

int main() {
    run({1, 1, 257, 1, 1, {0}, false});                         // the smallest: one stream, the history exactly one window
    run({2, 4, 300, 4, 3, {0, 1, 2, 3}, true});
    run({1, 8, 1024, 8, 5, {6, 1, 3}, true});                   // a ragged list, out of order
    run({3, 8, 1024, 11, 2, {7}, false});                       // one mic; a table wider than the frame has streams
    const awpu_cohere_t weighted{AWPU_COHERE_WEIGHTED}, factor{AWPU_COHERE_FACTOR}, neither{2}, negative{-1};
    CHECK(!awpu::cohere_refusal(&weighted) && !awpu::cohere_refusal(&factor));
    CHECK(awpu::cohere_refusal(&neither) && awpu::cohere_refusal(&negative) && awpu::cohere_refusal(nullptr));
    if (failures) return 1;
    std::printf("cohere rule: ok\n");
    return 0;
}
