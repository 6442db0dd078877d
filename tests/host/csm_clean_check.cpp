// csm_clean_check.cpp -- the host functions of include/awpu_hip_csm_clean.h (csrc/csm_clean_host.cpp, csm_clean_rule.h) as a program
// of its own, meant to be built with -fsanitize=address,undefined together with csm_host.cpp: every buffer exactly as long as the
// header says, the smallest sizes (one mic, one pixel, one bin, one step), a ragged list on a wider table, eight bins with 0 and
// 128, 32 steps, a skipped bin, each output alone, and the refusals -- which must leave the outputs as they were.
#include <cstdio>
#include <cstring>
#include <vector>

#include "csm_clean_rule.h"

namespace {

int failures = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                              \
        }                                                            \
    } while (0)

float sample(int s, int t) { return (float) (((s * 131 + t * 17 + (t * t) % 23) % 199) - 99) * 0.0078125f; }

awpu_csm_t csm_of(int32_t window, const std::vector<int32_t> &bins, int32_t kind) {
    awpu_csm_t c;
    std::memset(&c, 0, sizeof c);
    c.window = window, c.n_bins = (int32_t) bins.size(), c.kind = kind;
    for (size_t i = 0; i < bins.size() && i < AWPU_CSM_MAX_BINS; i++) c.bin[i] = bins[i];
    return c;
}

void run(int n_streams, const std::vector<int32_t> &index, int n_pixels, const std::vector<int32_t> &bins, int steps, float gain) {
    const int U = (int) index.size(), K = (int) bins.size(), n_blocks = U + 2, pitch = 256 * n_blocks;
    awpu_csm_t c = csm_of(AWPU_TONES_HANN, bins, AWPU_CSM_CONVENTIONAL);
    std::vector<float> samples((size_t) n_streams * pitch);
    for (int s = 0; s < n_streams; s++)
        for (int i = 0; i < pitch; i++) samples[(size_t) s * pitch + i] = sample(s, i);
    std::vector<int32_t> off((size_t) n_pixels * n_streams);
    std::vector<float> frac(off.size());
    for (size_t k = 0; k < off.size(); k++) off[k] = (int32_t) ((k * 37) % 768), frac[k] = k % 4 == 0 ? 0.0f : (k % 4 == 1 ? 1.0f : (float) (k % 11) / 11.0f);
    const size_t M = (size_t) K * U * U * 2, plane = (size_t) K * n_pixels;
    std::vector<float> C(M, 0.0f);
    int32_t count = 0;
    CHECK(awpu_hip_csm_accumulate_host(samples.data(), pitch, n_streams, n_blocks, index.data(), U, nullptr, &c, C.data(), &count) == AWPU_OK);
    const awpu_csm_clean_t cl{steps, gain, 0.01f};
    const std::vector<float> before = C;
    std::vector<awpu_csm_clean_step_t> st((size_t) K * steps);
    std::vector<float> clean(plane), residual(plane), map(plane), D(M);
    CHECK(awpu_hip_csm_clean_host(C.data(), count, off.data(), frac.data(), n_streams, n_pixels, index.data(), U, &c, &cl, st.data(), clean.data(),
                                  residual.data(), map.data(), D.data()) == AWPU_OK);
    CHECK(C == before);
    CHECK(st[0].pixel >= 0 && st[0].pixel < n_pixels && st[0].before > 0.0f);
    for (size_t i = 0; i < plane; i++) CHECK(map[i] == clean[i] + residual[i]);
    std::vector<float> alone(plane);  // each output alone
    CHECK(awpu_hip_csm_clean_host(C.data(), count, off.data(), frac.data(), n_streams, n_pixels, index.data(), U, &c, &cl, nullptr, nullptr, alone.data(),
                                  nullptr, nullptr) == AWPU_OK);
    CHECK(std::memcmp(alone.data(), residual.data(), plane * sizeof(float)) == 0);
    // one step by hand at the first picks, the last bin skipped: the loop's first step
    std::vector<int32_t> pixel((size_t) K);
    for (int kb = 0; kb < K; kb++) pixel[(size_t) kb] = kb == K - 1 && K > 1 ? -1 : st[(size_t) kb * steps].pixel;
    std::vector<float> work = C, v((size_t) K * U * 2), qs((size_t) K);
    CHECK(awpu_hip_csm_clean_step_host(work.data(), pixel.data(), gain, off.data(), frac.data(), n_streams, n_pixels, index.data(), U, &c, v.data(),
                                       qs.data()) == AWPU_OK);
    CHECK(qs[0] > 0.0f);
    if (K > 1) CHECK(qs[(size_t) K - 1] == 0.0f);
    CHECK(awpu_hip_csm_clean_step_host(work.data(), pixel.data(), gain, off.data(), frac.data(), n_streams, n_pixels, index.data(), U, &c, nullptr, nullptr) ==
          AWPU_OK);
    // refusals leave everything as it was
    const std::vector<float> kept = residual, kept_work = work;
    const awpu_csm_clean_t bad_cl{0, gain, 0.0f};
    awpu_csm_t removed = c;
    removed.kind = AWPU_CSM_DIAGONAL_REMOVED;
    CHECK(awpu_hip_csm_clean_host(C.data(), count, off.data(), frac.data(), n_streams, n_pixels, index.data(), U, &c, &bad_cl, st.data(), clean.data(),
                                  residual.data(), map.data(), D.data()) == AWPU_ERR_INVALID);
    CHECK(awpu_hip_csm_clean_host(C.data(), count, off.data(), frac.data(), n_streams, n_pixels, index.data(), U, &removed, &cl, st.data(), clean.data(),
                                  residual.data(), map.data(), D.data()) == AWPU_ERR_INVALID);
    CHECK(awpu_hip_csm_clean_host(C.data(), count, off.data(), frac.data(), n_streams, n_pixels, index.data(), U, &c, &cl, nullptr, nullptr, nullptr, nullptr,
                                  nullptr) == AWPU_ERR_INVALID);
    CHECK(awpu_hip_csm_clean_step_host(work.data(), pixel.data(), 0.0f, off.data(), frac.data(), n_streams, n_pixels, index.data(), U, &c, v.data(), qs.data()) ==
          AWPU_ERR_INVALID);
    CHECK(awpu_hip_csm_clean_step_host(work.data(), nullptr, gain, off.data(), frac.data(), n_streams, n_pixels, index.data(), U, &c, v.data(), qs.data()) ==
          AWPU_ERR_INVALID);
    CHECK(residual == kept && work == kept_work);
}

}  // namespace

int main() {
    run(1, {0}, 1, {3}, 1, 1.0f);
    run(8, {6, 1, 3, 0, 7}, 9, {0, 5, 17, 40, 64, 99, 127, 128}, 32, 0.5f);
    run(24, {23, 0, 2, 3, 5, 7, 8, 11, 12, 13, 14, 16, 17, 19, 20, 21, 22}, 16, {5, 128}, 4, 1.0f);
    if (failures) return 1;
    std::printf("csm clean rule: ok\n");
    return 0;
}
