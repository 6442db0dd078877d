// csm_rule_check.cpp -- the host functions of include/awpu_hip_csm.h (csrc/csm_host.cpp, csm_rule.h) as a program of its own, meant
// to be built with -fsanitize=address,undefined: every buffer exactly as long as the header says, the smallest sizes (one mic, one
// pixel, one block, one bin), a ragged list with gains and a pitch wider than the blocks, bins 0 and 128, offsets 0 and large,
// fractions 0 and 1, a recording split over two calls, the three maps, the inverse, and the refusals -- which must leave the
// outputs as they were.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "csm_rule.h"

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

awpu_csm_t csm_of(int32_t window, const std::vector<int32_t> &bins, int32_t kind, float loading) {
    awpu_csm_t c;
    std::memset(&c, 0, sizeof c);
    c.window = window, c.n_bins = (int32_t) bins.size(), c.kind = kind, c.loading = loading;
    for (size_t i = 0; i < bins.size() && i < AWPU_CSM_MAX_BINS; i++) c.bin[i] = bins[i];
    return c;
}

struct Shape {
    int n_streams, n_blocks, pitch, stride, n_pixels;
    std::vector<int32_t> index;
    bool gains;
};

bool same(const std::vector<float> &a, const std::vector<float> &b) { return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0; }

void run(const Shape &sh, awpu_csm_t c) {
    const int U = (int) sh.index.size(), K = c.n_bins;
    std::vector<float> samples((size_t) sh.n_streams * sh.pitch);
    for (int s = 0; s < sh.n_streams; s++)
        for (int i = 0; i < sh.pitch; i++) samples[(size_t) s * sh.pitch + i] = sample(s, i);
    std::vector<int32_t> off((size_t) sh.n_pixels * sh.stride);
    std::vector<float> frac(off.size());
    for (int p = 0; p < sh.n_pixels; p++)
        for (int m = 0; m < sh.stride; m++) {
            const int k = p * 5 + m * 3;
            off[(size_t) p * sh.stride + m] = k % 3 == 0 ? 0 : (k % 3 == 1 ? 767 : (k * 37) % 768);
            frac[(size_t) p * sh.stride + m] = k % 4 == 0 ? 0.0f : (k % 4 == 1 ? 1.0f : (float) (k % 11) / 11.0f);
        }
    std::vector<float> gain(U);
    for (int s = 0; s < U; s++) gain[s] = 0.5f + 0.25f * (float) (s % 5);
    const float *g = sh.gains ? gain.data() : nullptr;
    const size_t msize = (size_t) K * U * U * 2, psize = (size_t) K * sh.n_pixels;

    std::vector<float> spectra((size_t) sh.n_blocks * K * U * 2);
    CHECK(awpu_hip_csm_spectra_host(samples.data(), sh.pitch, sh.n_streams, sh.n_blocks, sh.index.data(), U, g, &c, spectra.data()) == AWPU_OK);
    if (c.bin[0] == 0)
        for (int b = 0; b < sh.n_blocks; b++)
            for (int a = 0; a < U; a++) CHECK(spectra[(((size_t) b * K) * U + a) * 2 + 1] == 0.0f);  // (bin 0: t_0 = (1, -0))

    // one call, and the same blocks over two calls
    std::vector<float> C(msize, 0.0f), C2(msize, 0.0f);
    int32_t count = 0, count2 = 0;
    CHECK(awpu_hip_csm_accumulate_host(samples.data(), sh.pitch, sh.n_streams, sh.n_blocks, sh.index.data(), U, g, &c, C.data(), &count) == AWPU_OK);
    CHECK(count == sh.n_blocks);
    if (sh.n_blocks > 1) {
        std::vector<float> tail((size_t) sh.n_streams * sh.pitch - 256);  // the view that starts at block 1 ends where the buffer ends
        std::memcpy(tail.data(), samples.data() + 256, tail.size() * sizeof(float));
        CHECK(awpu_hip_csm_accumulate_host(samples.data(), sh.pitch, sh.n_streams, 1, sh.index.data(), U, g, &c, C2.data(), &count2) == AWPU_OK);
        CHECK(awpu_hip_csm_accumulate_host(tail.data(), sh.pitch, sh.n_streams, sh.n_blocks - 1, sh.index.data(), U, g, &c, C2.data(), &count2) == AWPU_OK);
        CHECK(count2 == count && same(C, C2));
    }
    for (int k = 0; k < K; k++)
        for (int a = 0; a < U; a++) {
            CHECK(C[(((size_t) k * U + a) * U + a) * 2 + 1] == 0.0f && C[(((size_t) k * U + a) * U + a) * 2] >= 0.0f);
            for (int b = 0; b < a; b++) {
                const float *lo = &C[(((size_t) k * U + a) * U + b) * 2], *up = &C[(((size_t) k * U + b) * U + a) * 2];
                CHECK(lo[0] == up[0] && lo[1] == -up[1]);
            }
        }

    std::vector<float> steer((size_t) sh.n_pixels * K * U * 2);
    CHECK(awpu_hip_csm_steer_host(off.data(), frac.data(), sh.stride, sh.n_pixels, sh.index.data(), U, &c, steer.data()) == AWPU_OK);
    for (size_t i = 0; i < steer.size(); i += 2) CHECK(std::fabs(steer[i] * steer[i] + steer[i + 1] * steer[i + 1] - 1.0f) < 1e-5f);

    std::vector<float> map(psize), q(psize), alone(psize);
    const auto map_call = [&](const float *m, int32_t n, const awpu_csm_t *cc, float *mo, float *qo) {
        return awpu_hip_csm_map_host(m, n, off.data(), frac.data(), sh.stride, sh.n_pixels, sh.index.data(), U, cc, mo, qo);
    };
    for (int32_t kind : {AWPU_CSM_CONVENTIONAL, AWPU_CSM_DIAGONAL_REMOVED}) {
        c.kind = kind;
        if (kind == AWPU_CSM_DIAGONAL_REMOVED && U == 1) {
            CHECK(map_call(C.data(), count, &c, map.data(), q.data()) == AWPU_ERR_INVALID);
            continue;
        }
        CHECK(map_call(C.data(), count, &c, map.data(), q.data()) == AWPU_OK);
        CHECK(map_call(C.data(), count, &c, alone.data(), nullptr) == AWPU_OK && same(alone, map));
        CHECK(map_call(C.data(), count, &c, nullptr, alone.data()) == AWPU_OK && same(alone, q));
        for (float v : map) CHECK(v >= 0.0f || kind == AWPU_CSM_CONVENTIONAL);
    }
    c.kind = AWPU_CSM_CAPON, c.loading = 0.05f;
    std::vector<float> G(msize, -3.0f);
    CHECK(awpu_hip_csm_invert_host(C.data(), count, U, &c, G.data()) == AWPU_OK);
    CHECK(map_call(G.data(), count, &c, map.data(), q.data()) == AWPU_OK);
    for (float v : map) CHECK(v >= 0.0f && std::isfinite(v));

    // refusals write nothing
    const std::vector<float> keep_map = map, keep_q = q, keep_G = G, keep_C = C, keep_spectra = spectra, keep_steer = steer;
    const int32_t keep_count = count;
    awpu_csm_t bad = c;
    const auto refused_everywhere = [&](const awpu_csm_t *cc) {
        CHECK(awpu_hip_csm_spectra_host(samples.data(), sh.pitch, sh.n_streams, sh.n_blocks, sh.index.data(), U, g, cc, spectra.data()) == AWPU_ERR_INVALID);
        CHECK(awpu_hip_csm_accumulate_host(samples.data(), sh.pitch, sh.n_streams, sh.n_blocks, sh.index.data(), U, g, cc, C.data(), &count) == AWPU_ERR_INVALID);
        CHECK(awpu_hip_csm_steer_host(off.data(), frac.data(), sh.stride, sh.n_pixels, sh.index.data(), U, cc, steer.data()) == AWPU_ERR_INVALID);
        CHECK(map_call(G.data(), count, cc, map.data(), q.data()) == AWPU_ERR_INVALID);
        CHECK(awpu_hip_csm_invert_host(C.data(), count, U, cc, G.data()) == AWPU_ERR_INVALID);
    };
    refused_everywhere(nullptr);
    bad = c, bad.window = 2, refused_everywhere(&bad);
    bad = c, bad.n_bins = 0, refused_everywhere(&bad);
    bad = c, bad.n_bins = 9, refused_everywhere(&bad);
    bad = c, bad.bin[K - 1] = 129, refused_everywhere(&bad);
    bad = c, bad.bin[0] = -1, refused_everywhere(&bad);
    bad = c, bad.kind = 3, refused_everywhere(&bad);
    bad = c, bad.loading = -1.0f, refused_everywhere(&bad);
    bad = c, bad.loading = NAN, refused_everywhere(&bad);
    if (K > 1) bad = c, bad.bin[1] = bad.bin[0], refused_everywhere(&bad);
    CHECK(map_call(G.data(), count, &c, nullptr, nullptr) == AWPU_ERR_INVALID);
    CHECK(map_call(nullptr, count, &c, map.data(), q.data()) == AWPU_ERR_INVALID);
    CHECK(map_call(G.data(), 0, &c, map.data(), q.data()) == AWPU_ERR_INVALID);
    CHECK(awpu_hip_csm_invert_host(C.data(), 0, U, &c, G.data()) == AWPU_ERR_INVALID);
    CHECK(awpu_hip_csm_invert_host(nullptr, count, U, &c, G.data()) == AWPU_ERR_INVALID);
    CHECK(awpu_hip_csm_spectra_host(nullptr, sh.pitch, sh.n_streams, sh.n_blocks, sh.index.data(), U, g, &c, spectra.data()) == AWPU_ERR_INVALID);
    CHECK(awpu_hip_csm_spectra_host(samples.data(), 256 * sh.n_blocks - 1, sh.n_streams, sh.n_blocks, sh.index.data(), U, g, &c, spectra.data()) == AWPU_ERR_INVALID);
    CHECK(awpu_hip_csm_accumulate_host(samples.data(), sh.pitch, sh.n_streams, sh.n_blocks, sh.index.data(), U, g, &c, C.data(), nullptr) == AWPU_ERR_INVALID);
    int32_t full = INT32_MAX;
    CHECK(awpu_hip_csm_accumulate_host(samples.data(), sh.pitch, sh.n_streams, sh.n_blocks, sh.index.data(), U, g, &c, C.data(), &full) == AWPU_ERR_INVALID && full == INT32_MAX);
    std::vector<int32_t> bad_index = sh.index;
    bad_index[U - 1] = sh.n_streams;
    CHECK(awpu_hip_csm_accumulate_host(samples.data(), sh.pitch, sh.n_streams, sh.n_blocks, bad_index.data(), U, g, &c, C.data(), &count) == AWPU_ERR_INVALID);
    std::vector<float> bad_frac = frac;
    bad_frac[(size_t) (sh.n_pixels - 1) * sh.stride + sh.index[0]] = NAN;
    CHECK(awpu_hip_csm_map_host(G.data(), count, off.data(), bad_frac.data(), sh.stride, sh.n_pixels, sh.index.data(), U, &c, map.data(), q.data()) == AWPU_ERR_INVALID);
    std::vector<int32_t> bad_off = off;
    bad_off[(size_t) (sh.n_pixels - 1) * sh.stride + sh.index[U - 1]] = -1;
    CHECK(awpu_hip_csm_steer_host(bad_off.data(), frac.data(), sh.stride, sh.n_pixels, sh.index.data(), U, &c, steer.data()) == AWPU_ERR_INVALID);
    // a matrix that is not positive definite: a negative diagonal
    std::vector<float> indefinite = C;
    indefinite[0] = -1.0f - std::fabs(C[0]) * (float) (U + 1);
    for (int a = 1; a < U; a++) indefinite[((size_t) a * U + a) * 2] = 0.0f;
    CHECK(awpu_hip_csm_invert_host(indefinite.data(), count, U, &c, G.data()) == AWPU_ERR_RANGE);
    CHECK(same(keep_map, map) && same(keep_q, q) && same(keep_G, G) && same(keep_C, C) && same(keep_spectra, spectra) && same(keep_steer, steer) &&
          keep_count == count);
}

}  // namespace

int main() {
    run({1, 1, 256, 1, 1, {0}, false}, csm_of(AWPU_TONES_RECT, {0}, AWPU_CSM_CONVENTIONAL, 0.0f));  // the smallest
    run({4, 3, 768, 4, 3, {0, 1, 2, 3}, true}, csm_of(AWPU_TONES_HANN, {0, 1, 2, 3, 4, 5, 6, 7}, AWPU_CSM_CONVENTIONAL, 0.0f));
    run({8, 5, 1300, 8, 5, {6, 1, 3}, true}, csm_of(AWPU_TONES_HANN, {3, 47, 128}, AWPU_CSM_DIAGONAL_REMOVED, 0.0f));  // ragged, out of order, a wide pitch
    run({8, 2, 512, 11, 2, {7, 2}, false}, csm_of(AWPU_TONES_RECT, {128}, AWPU_CSM_CAPON, 1e-3f));  // a table wider than the streams
    if (failures) return 1;
    std::printf("csm rule: ok\n");
    return 0;
}
