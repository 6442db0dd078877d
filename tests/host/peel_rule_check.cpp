// peel_rule_check.cpp -- awpu_hip_peel_step_host and awpu_hip_peel_host (csrc/peel_host.cpp, peel_rule.h) as a program of its own,
// meant to be built with -fsanitize=address,undefined: every buffer exactly as long as the header says; a table whose reach
// touches both ends of the history (min off - E - 1 = 0 and max off + 257 + E = hist - 1: the step reads those two samples and not
// a float more); the smallest table (one pixel, one mic, E = 0); a shuffled list with gains, one of them 0; a frame without a
// pixel, a silent frame and a NaN frame; null outputs; and the refusals -- which must leave frames and outputs as they were.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "peel_rule.h"

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
    int batch, n_streams, hist, stride, n_pixels, E;
    std::vector<int32_t> index;
    bool gains;
};

void run(const Shape &sh) {
    const int U = (int) sh.index.size();
    const size_t frame_floats = (size_t) sh.n_streams * sh.hist;
    std::vector<float> frames((size_t) sh.batch * frame_floats);
    for (int b = 0; b < sh.batch; b++)
        for (int s = 0; s < sh.n_streams; s++)
            for (int t = 0; t < sh.hist; t++) frames[(size_t) b * frame_floats + (size_t) s * sh.hist + t] = sample(b, s, t);
    if (sh.batch > 2) {
        std::fill(frames.begin() + (sh.batch - 1) * frame_floats, frames.end(), NAN);                              // the last frame: NaN
        std::fill(frames.begin() + (sh.batch - 2) * frame_floats, frames.begin() + (sh.batch - 1) * frame_floats, 0.0f);  // the one before: silent
    }
    // offsets in [E + 1, hist - 258 - E], both ends taken: the reach is exactly [0, hist)
    const int lowest = sh.E + 1, highest = sh.hist - 258 - sh.E;
    CHECK(highest - lowest == sh.E);
    std::vector<int32_t> off((size_t) sh.n_pixels * sh.stride);
    std::vector<float> frac(off.size());
    for (int p = 0; p < sh.n_pixels; p++)
        for (int m = 0; m < sh.stride; m++) {
            const int k = p * 5 + m * 3;
            off[(size_t) p * sh.stride + m] = k % 3 == 0 ? lowest : (k % 3 == 1 ? highest : lowest + (k * 37) % (sh.E + 1));
            frac[(size_t) p * sh.stride + m] = k % 4 == 0 ? 0.0f : (k % 4 == 1 ? 1.0f : (float) (k % 11) / 11.0f);
        }
    off[(size_t) sh.index[0]] = lowest;
    off[(size_t) (sh.n_pixels - 1) * sh.stride + sh.index[U - 1]] = highest;
    std::vector<float> gain(U);
    for (int s = 0; s < U; s++) gain[s] = s == 1 ? 0.0f : 0.5f + 0.25f * (float) (s % 5) * (s % 2 ? -1.0f : 1.0f);
    const float *g = sh.gains ? gain.data() : nullptr;
    const int32_t *idx = sh.index.data();

    const int32_t len = awpu_hip_peel_beam_length(sh.n_streams, sh.hist, off.data(), frac.data(), sh.stride, sh.n_pixels, idx, U);
    CHECK(len == 258 + 2 * sh.E);
    if (len < 0) return;

    // the step: the first and the last pixel, and a frame without one
    std::vector<int32_t> pixel(sh.batch);
    for (int b = 0; b < sh.batch; b++) pixel[b] = b == 0 ? 0 : (b == 1 ? sh.n_pixels - 1 : -1);
    std::vector<float> work = frames, beams((size_t) sh.batch * len, -3.0f);
    CHECK(awpu_hip_peel_step_host(work.data(), sh.batch, sh.n_streams, sh.hist, off.data(), frac.data(), sh.stride, sh.n_pixels, idx, U, g, pixel.data(),
                                  0.5f, beams.data()) == AWPU_OK);
    CHECK(std::memcmp(work.data(), frames.data(), frame_floats * sizeof(float)) != 0);
    for (int b = 2; b < sh.batch; b++) {
        CHECK(std::memcmp(work.data() + b * frame_floats, frames.data() + b * frame_floats, frame_floats * sizeof(float)) == 0);
        for (int j = 0; j < len; j++) CHECK(beams[(size_t) b * len + j] == 0.0f);
    }
    std::vector<float> again = frames;
    CHECK(awpu_hip_peel_step_host(again.data(), sh.batch, sh.n_streams, sh.hist, off.data(), frac.data(), sh.stride, sh.n_pixels, idx, U, g, pixel.data(),
                                  0.5f, nullptr) == AWPU_OK);
    CHECK(std::memcmp(again.data(), work.data(), work.size() * sizeof(float)) == 0);

    // the loop, with every output and with none but the steps
    const awpu_peel_t pe{3, 1.0f, 0.0f};
    const size_t n = (size_t) sh.batch * sh.n_pixels;
    std::vector<awpu_peel_step_t> steps((size_t) sh.batch * pe.steps), steps_only(steps.size());
    std::vector<float> clean(n), residual(n), map(n), left(frames.size());
    const std::vector<float> keep = frames;
    CHECK(awpu_hip_peel_host(frames.data(), sh.batch, sh.n_streams, sh.hist, off.data(), frac.data(), sh.stride, sh.n_pixels, idx, U, g, &pe, steps.data(),
                             clean.data(), residual.data(), map.data(), left.data()) == AWPU_OK);
    CHECK(awpu_hip_peel_host(frames.data(), sh.batch, sh.n_streams, sh.hist, off.data(), frac.data(), sh.stride, sh.n_pixels, idx, U, g, &pe,
                             steps_only.data(), nullptr, nullptr, nullptr, nullptr) == AWPU_OK);
    CHECK(std::memcmp(frames.data(), keep.data(), keep.size() * sizeof(float)) == 0);
    CHECK(std::memcmp(steps.data(), steps_only.data(), steps.size() * sizeof(awpu_peel_step_t)) == 0);
    CHECK(steps[0].pixel >= 0 && steps[0].before > 0.0f && steps[0].removed >= 0.0f);
    for (int b = 0; b < sh.batch; b++)
        for (int p = 0; p < sh.n_pixels; p++) {
            const size_t at = (size_t) b * sh.n_pixels + p;
            CHECK(clean[at] >= 0.0f);
            if (b < 2 || sh.batch <= 2) CHECK(map[at] == clean[at] + residual[at]);
        }
    if (sh.batch > 2) {
        for (int b = sh.batch - 2; b < sh.batch; b++) {  // silent and NaN: no pick, no step
            for (int k = 0; k < pe.steps; k++) CHECK(steps[(size_t) b * pe.steps + k].pixel == -1 && steps[(size_t) b * pe.steps + k].removed == 0.0f);
            CHECK(std::memcmp(left.data() + b * frame_floats, keep.data() + b * frame_floats, frame_floats * sizeof(float)) == 0);
        }
        CHECK(std::isnan(residual[n - 1]) && clean[n - 1] == 0.0f);
    }

    // refusals leave everything as it was
    std::vector<float> canary(n, -5.0f);
    std::vector<int32_t> shifted = off;
    for (auto &o : shifted) o -= 1;  // one sample too early
    work = keep;
    CHECK(awpu_hip_peel_step_host(work.data(), sh.batch, sh.n_streams, sh.hist, shifted.data(), frac.data(), sh.stride, sh.n_pixels, idx, U, g, pixel.data(),
                                  1.0f, beams.data()) == AWPU_ERR_RANGE);
    for (auto &o : shifted) o += 2;  // one sample too late
    CHECK(awpu_hip_peel_host(work.data(), sh.batch, sh.n_streams, sh.hist, shifted.data(), frac.data(), sh.stride, sh.n_pixels, idx, U, g, &pe, nullptr,
                             canary.data(), canary.data(), canary.data(), nullptr) == AWPU_ERR_RANGE);
    const awpu_peel_t bad{0, 1.0f, 0.0f};
    CHECK(awpu_hip_peel_host(work.data(), sh.batch, sh.n_streams, sh.hist, off.data(), frac.data(), sh.stride, sh.n_pixels, idx, U, g, &bad, nullptr,
                             canary.data(), canary.data(), canary.data(), nullptr) == AWPU_ERR_INVALID);
    CHECK(awpu_hip_peel_step_host(work.data(), sh.batch, sh.n_streams, sh.hist, off.data(), frac.data(), sh.stride, sh.n_pixels, idx, U, g, pixel.data(), 0.0f,
                                  nullptr) == AWPU_ERR_INVALID);
    CHECK(std::memcmp(work.data(), keep.data(), keep.size() * sizeof(float)) == 0);
    for (float c : canary) CHECK(c == -5.0f);
}

}  // namespace

int main() {
    run({4, 8, 1024, 8, 6, 255, {6, 1, 7, 3, 4}, true});  // hist = 3 E + 259: the widest reach a history of 1024 takes
    run({1, 1, 259, 1, 1, 0, {0}, false});                // the smallest: one sample either side of the block's 257
    run({3, 4, 343, 6, 3, 28, {3, 0, 2}, true});
    if (failures) {
        std::printf("peel rule: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("peel rule: ok\n");
    return 0;
}
