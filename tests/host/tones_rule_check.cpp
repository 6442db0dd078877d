// tones_rule_check.cpp -- awpu_hip_tones_host and the tables (csrc/tones_host.cpp, tones_rule.h) as a program of its own, meant to
// be built with -fsanitize=address,undefined: every buffer exactly as long as the header says, entries at both ends of the history
// (off = 0 and off = hist - 257), the smallest sizes (one pixel, one mic, hist 257), a ragged list with gains, both windows, one
// group, 129 groups and uneven edges, null outputs, and the refusals -- which must leave the outputs as they were.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "tones_rule.h"

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

awpu_tones_t groups_of(int32_t window, const std::vector<int32_t> &edges) {
    awpu_tones_t t;
    std::memset(&t, 0, sizeof t);
    t.window = window;
    t.n_groups = (int32_t) edges.size() - 1;
    for (size_t g = 0; g < edges.size(); g++) t.edge[g] = edges[g];
    return t;
}

void run(const Shape &sh, const awpu_tones_t &t) {
    const int U = (int) sh.index.size(), G = t.n_groups, K = AWPU_TONES_BINS;
    std::vector<float> frames((size_t) sh.batch * sh.n_streams * sh.hist);
    for (int b = 0; b < sh.batch; b++)
        for (int s = 0; s < sh.n_streams; s++)
            for (int i = 0; i < sh.hist; i++) frames[((size_t) b * sh.n_streams + s) * sh.hist + i] = sample(b, s, i);
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
    std::vector<float> tone(n * G), bins(n * K), spectrum(n * K * 2);
    std::vector<int32_t> pitch(n);
    const float *g = sh.gains ? gain.data() : nullptr;
    const auto call = [&](const awpu_tones_t *tt, float *to, int32_t *pi, float *bi, float *sp) {
        return awpu_hip_tones_host(frames.data(), sh.batch, sh.n_streams, sh.hist, off.data(), frac.data(), sh.stride, sh.n_pixels, sh.index.data(), U, g,
                                   tt, to, pi, bi, sp);
    };
    CHECK(call(&t, tone.data(), pitch.data(), bins.data(), spectrum.data()) == AWPU_OK);
    for (int b = 0; b < sh.batch; b++)
        for (int p = 0; p < sh.n_pixels; p++) {
            const size_t at = (size_t) b * sh.n_pixels + p;
            const float *bn = bins.data() + at * K;
            CHECK(pitch[at] >= t.edge[0] && pitch[at] < t.edge[G]);
            for (int k = t.edge[0]; k < t.edge[G]; k++) CHECK(bn[k] <= bn[pitch[at]] && bn[k] >= 0.0f);
            for (int gi = 0; gi < G; gi++) {
                float sum = 0.0f;
                for (int k = t.edge[gi]; k < t.edge[gi + 1]; k++) sum = sum + bn[k];
                CHECK(tone[((size_t) b * G + gi) * sh.n_pixels + p] == sum);
            }
            CHECK(spectrum[at * K * 2 + 1] == 0.0f);  // a real signal: z[0] is real
        }
    // every output on its own gives the bits it gives beside the others
    {
        std::vector<float> alone(n * K * 2);
        std::vector<int32_t> alone_pitch(n);
        CHECK(call(&t, alone.data(), nullptr, nullptr, nullptr) == AWPU_OK && std::memcmp(alone.data(), tone.data(), tone.size() * sizeof(float)) == 0);
        CHECK(call(&t, nullptr, alone_pitch.data(), nullptr, nullptr) == AWPU_OK && alone_pitch == pitch);
        CHECK(call(&t, nullptr, nullptr, alone.data(), nullptr) == AWPU_OK && std::memcmp(alone.data(), bins.data(), bins.size() * sizeof(float)) == 0);
        CHECK(call(&t, nullptr, nullptr, nullptr, alone.data()) == AWPU_OK && std::memcmp(alone.data(), spectrum.data(), spectrum.size() * sizeof(float)) == 0);
    }
    // refusals write nothing
    const std::vector<float> keep = bins;
    const std::vector<int32_t> keep_pitch = pitch;
    CHECK(call(&t, nullptr, nullptr, nullptr, nullptr) == AWPU_ERR_INVALID);
    CHECK(call(nullptr, nullptr, pitch.data(), bins.data(), nullptr) == AWPU_ERR_INVALID);
    awpu_tones_t bad = t;
    bad.window = 2;
    CHECK(call(&bad, nullptr, pitch.data(), bins.data(), nullptr) == AWPU_ERR_INVALID);
    bad = t, bad.n_groups = 0;
    CHECK(call(&bad, nullptr, pitch.data(), bins.data(), nullptr) == AWPU_ERR_INVALID);
    bad = t, bad.n_groups = 130;
    CHECK(call(&bad, nullptr, pitch.data(), bins.data(), nullptr) == AWPU_ERR_INVALID);
    bad = t, bad.edge[G] = 130;
    CHECK(call(&bad, nullptr, pitch.data(), bins.data(), nullptr) == AWPU_ERR_INVALID);
    bad = t, bad.edge[0] = -1;
    CHECK(call(&bad, nullptr, pitch.data(), bins.data(), nullptr) == AWPU_ERR_INVALID);
    bad = t, bad.edge[G] = bad.edge[G - 1];
    CHECK(call(&bad, nullptr, pitch.data(), bins.data(), nullptr) == AWPU_ERR_INVALID);
    std::vector<int32_t> bad_off = off;
    bad_off[(size_t) (sh.n_pixels - 1) * sh.stride + sh.index[U - 1]] = last + 1;
    CHECK(awpu_hip_tones_host(frames.data(), sh.batch, sh.n_streams, sh.hist, bad_off.data(), frac.data(), sh.stride, sh.n_pixels, sh.index.data(), U, g,
                              &t, nullptr, pitch.data(), bins.data(), nullptr) == AWPU_ERR_RANGE);
    std::vector<float> bad_frac = frac;
    bad_frac[(size_t) (sh.n_pixels - 1) * sh.stride + sh.index[0]] = NAN;
    CHECK(awpu_hip_tones_host(frames.data(), sh.batch, sh.n_streams, sh.hist, off.data(), bad_frac.data(), sh.stride, sh.n_pixels, sh.index.data(), U, g,
                              &t, nullptr, pitch.data(), bins.data(), nullptr) == AWPU_ERR_INVALID);
    CHECK(awpu_hip_tones_host(frames.data(), sh.batch, sh.n_streams, 256, off.data(), frac.data(), sh.stride, sh.n_pixels, sh.index.data(), U, g, &t,
                              nullptr, pitch.data(), bins.data(), nullptr) == AWPU_ERR_INVALID);
    CHECK(keep == bins && keep_pitch == pitch);
}

}  // namespace

int main() {
    std::vector<int32_t> every(130);
    for (int k = 0; k < 130; k++) every[k] = k;
    const awpu_tones_t all = groups_of(AWPU_TONES_RECT, {0, 129}), each = groups_of(AWPU_TONES_HANN, every),
                       uneven = groups_of(AWPU_TONES_HANN, {3, 4, 40, 41, 127}), top = groups_of(AWPU_TONES_RECT, {128, 129});
    run({1, 1, 257, 1, 1, {0}, false}, all);                    // the smallest: one stream, the history exactly one window
    run({2, 4, 300, 4, 3, {0, 1, 2, 3}, true}, each);
    run({1, 8, 1024, 8, 5, {6, 1, 3}, true}, uneven);           // a ragged list, out of order
    run({3, 8, 1024, 11, 2, {7}, false}, top);                  // one mic; a table wider than the frame has streams
    // the tables: exactly 256 and 128 x 2 floats
    std::vector<float> w(256), tw(256);
    CHECK(awpu_hip_tones_window(AWPU_TONES_RECT, w.data()) == AWPU_OK && w[0] == 1.0f && w[255] == 1.0f);
    CHECK(awpu_hip_tones_window(AWPU_TONES_HANN, w.data()) == AWPU_OK && w[0] == 0.0f && w[128] == 1.0f && w[1] == w[255]);
    CHECK(awpu_hip_tones_window(2, w.data()) == AWPU_ERR_INVALID && awpu_hip_tones_window(0, nullptr) == AWPU_ERR_INVALID);
    CHECK(awpu_hip_tones_twiddles(reinterpret_cast<float(*)[2]>(tw.data())) == AWPU_OK && tw[0] == 1.0f && tw[2 * 64 + 1] == -1.0f);
    CHECK(awpu_hip_tones_twiddles(nullptr) == AWPU_ERR_INVALID);
    // tones_linear: bins 14 .. 18 have their centres in [2500, 3500) at the reference's rate
    awpu_tones_t t;
    std::memset(&t, 0, sizeof t);
    CHECK(awpu_hip_tones_linear(2500.0f, 3500.0f, 2, 48828.125f, &t) == AWPU_OK && t.n_groups == 2 && t.edge[0] == 14 && t.edge[1] == 17 && t.edge[2] == 19);
    CHECK(!awpu::tones_refusal(&t) && !awpu::tones_refusal(&t, 1) && !awpu::tones_refusal(&t, AWPU_TONES_SHOW_PITCH));
    CHECK(awpu::tones_refusal(&t, 2) && awpu::tones_refusal(&t, -2));
    CHECK(awpu_hip_tones_linear(0.0f, 1e9f, 129, 48828.125f, &t) == AWPU_OK && t.edge[0] == 0 && t.edge[129] == 129);
    const awpu_tones_t keep = t;
    CHECK(awpu_hip_tones_linear(2500.0f, 3500.0f, 6, 48828.125f, &t) == AWPU_ERR_INVALID);  // five bins, six groups
    CHECK(awpu_hip_tones_linear(2500.0f, 3500.0f, 0, 48828.125f, &t) == AWPU_ERR_INVALID);
    CHECK(awpu_hip_tones_linear(2500.0f, 3500.0f, 1, 0.0f, &t) == AWPU_ERR_INVALID);
    CHECK(awpu_hip_tones_linear(2500.0f, 3500.0f, 1, 48828.125f, nullptr) == AWPU_ERR_INVALID);
    CHECK(std::memcmp(&keep, &t, sizeof t) == 0);
    if (failures) return 1;
    std::printf("tones rule: ok\n");
    return 0;
}
