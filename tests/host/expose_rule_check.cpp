// expose_rule_check.cpp -- awpu_hip_expose_count and awpu_hip_expose_rows (csrc/expose_host.cpp, expose_rule.h) as a program of
// its own, meant to be built with -fsanitize=address,undefined: the smallest sizes (1 pixel, length 1) and the largest (every =
// length = 1024), every buffer exactly as long as the header says, the frames checked against sums written window by window,
// the window view of expose_rule.h against its block view, and a split call against the whole one.
#include <cstdio>
#include <cstring>
#include <vector>

#include "expose_rule.h"

namespace {

int failures = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                              \
        }                                                            \
    } while (0)

float value(int k, int i) { return (float) ((k * 131 + i * 17) % 97) * 0.125f + (float) i; }

// one call over rows [k0, k0 + n) of a recording whose frame j shows block first + j * every, with exact-size buffers
void run(int n_total, int n_pixels, int first, int every, int length, int mode, const std::vector<int> &cuts) {
    std::vector<float> power((size_t) n_total * n_pixels);
    for (int k = 0; k < n_total; k++)
        for (int i = 0; i < n_pixels; i++) power[(size_t) k * n_pixels + i] = value(k, i);
    const awpu_expose_t e{length, mode};
    // the expected frames, window by window, from a zero carry
    std::vector<std::vector<float>> want;
    for (int j = 0; first + (long long) j * every < n_total; j++) {
        std::vector<float> frame(n_pixels);
        for (int i = 0; i < n_pixels; i++) {
            float acc = 0.0f;
            bool started = false;
            for (int k = first + j * every - length + 1; k <= first + j * every; k++) {
                if (k < 0) {  // (the zero carry stands for these blocks; they can only come first)
                    started = true;
                    continue;
                }
                const float p = power[(size_t) k * n_pixels + i];
                if (!started) acc = p;
                else acc = mode == AWPU_EXPOSE_MEAN ? acc + p : (awpu::expose_bits(p) > awpu::expose_bits(acc) ? p : acc);
                started = true;
            }
            frame[i] = mode == AWPU_EXPOSE_MEAN ? acc / (float) length : acc;
        }
        want.push_back(frame);
    }
    std::vector<float> carry(n_pixels, 0.0f);
    size_t j = 0;
    int at = 0, f = first;
    for (size_t c = 0; c <= cuts.size(); c++) {
        const int end = c < cuts.size() ? cuts[c] : n_total, n = end - at;
        int32_t n_frames, next_first, carry_in, carry_out, n_swept;
        CHECK(awpu_hip_expose_count(n, f, every, length, &n_frames, &next_first, &carry_in, &carry_out, &n_swept) == AWPU_OK);
        // the block view and the window view of the same call agree
        int swept = 0, closed = 0;
        for (int k = 0; k < n; k++) {
            int32_t q, jj;
            if (!awpu::expose_block(k, f, every, length, &q, &jj)) continue;
            swept++;
            closed += q == length - 1;
            const awpu::ExposeWindows win{n, f - (length - 1), every, length};
            CHECK(jj < win.count() && k >= win.lo(jj) && k < win.hi(jj) && k - win.start(jj) == q);
        }
        CHECK(swept == n_swept && closed == n_frames);
        const awpu::ExposeWindows win{n, f - (length - 1), every, length};
        CHECK((win.count() > 0 && win.carried(0)) == (carry_in > 0));
        CHECK((win.count() > 0 && !win.closes(win.count() - 1)) == (carry_out > 0));
        std::vector<float> frames((size_t) n_frames * n_pixels);
        const bool needs_carry = carry_in > 0 || carry_out > 0;
        CHECK(awpu_hip_expose_rows(power.data() + (size_t) at * n_pixels, n, n_pixels, f, every, &e, needs_carry ? carry.data() : nullptr,
                                   n_frames ? frames.data() : nullptr) == AWPU_OK);
        for (int r = 0; r < n_frames; r++, j++) {
            CHECK(j < want.size());
            if (j < want.size()) CHECK(std::memcmp(frames.data() + (size_t) r * n_pixels, want[j].data(), n_pixels * sizeof(float)) == 0);
        }
        at = end, f = next_first;
    }
    CHECK(j == want.size());
}

}  // namespace

int main() {
    for (int mode : {AWPU_EXPOSE_MEAN, AWPU_EXPOSE_PEAK}) {
        run(1, 1, 0, 1, 1, mode, {});             // the smallest: one block, one pixel, length 1
        run(5, 1, 0, 1, 1, mode, {2});
        run(23, 7, 2, 3, 3, mode, {5, 6, 15});    // windows that straddle the cuts
        run(23, 7, 1, 3, 2, mode, {1, 2, 3});
        run(23, 5, 0, 7, 4, mode, {11});          // a dim first frame: three blocks of window 0 lie before the recording
        run(2100, 3, 1023, 1024, 1024, mode, {}); // the largest: every = length = 1024
        run(2100, 3, 1023, 1024, 1024, mode, {1000, 1024, 2047});
    }
    // refusals write nothing
    {
        float power[4] = {1, 2, 3, 4}, carry[2] = {7, 7}, frames[4] = {9, 9, 9, 9};
        awpu_expose_t e{1, AWPU_EXPOSE_MEAN};
        int32_t a = -5, b = -5, c = -5, d = -5, s = -5;
        CHECK(awpu_hip_expose_count(0, 0, 1, 1, &a, &b, &c, &d, &s) == AWPU_ERR_INVALID);
        CHECK(awpu_hip_expose_count(1, 0, 1, 2, &a, &b, &c, &d, &s) == AWPU_ERR_INVALID);
        CHECK(awpu_hip_expose_count(1, 0, 1, 1, &a, &b, &c, &d, nullptr) == AWPU_ERR_INVALID);
        CHECK(a == -5 && b == -5 && c == -5 && d == -5 && s == -5);
        e.length = 3;
        CHECK(awpu_hip_expose_rows(power, 2, 2, 0, 2, &e, carry, frames) == AWPU_ERR_INVALID);
        e.length = 2, e.mode = 2;
        CHECK(awpu_hip_expose_rows(power, 2, 2, 1, 2, &e, carry, frames) == AWPU_ERR_INVALID);
        e.mode = AWPU_EXPOSE_PEAK;
        CHECK(awpu_hip_expose_rows(power, 2, 2, 0, 2, &e, nullptr, frames) == AWPU_ERR_INVALID);  // carry_in = 1
        CHECK(awpu_hip_expose_rows(power, 2, 2, 1, 2, &e, nullptr, nullptr) == AWPU_ERR_INVALID);  // a frame and nowhere to put it
        CHECK(awpu_hip_expose_rows(nullptr, 2, 2, 1, 2, &e, carry, frames) == AWPU_ERR_INVALID);
        CHECK(carry[0] == 7 && carry[1] == 7 && frames[0] == 9 && frames[3] == 9);
        CHECK(awpu_hip_expose_rows(power, 2, 2, 1, 2, &e, nullptr, frames) == AWPU_OK);  // one whole window: no carry needed
        CHECK(frames[0] == 3 && frames[1] == 4 && frames[2] == 9);
    }
    if (failures) return 1;
    std::printf("expose rule: ok\n");
    return 0;
}
