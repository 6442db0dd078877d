// csm_invert_check.cpp -- awpu_hip_csm_invert_rule_host (csrc/csm_invert_host.cpp, csm_invert_rule.h) as a program of its own,
// meant to be built with -fsanitize=address,undefined: every buffer exactly as long as the header says, the smallest sizes (one
// mic, one bin), an odd size, eight bins, `solved` given and null, an unsolved bin among solved ones (all zeros without loading;
// a NaN entry), G A against the identity, G's structure, and the refusals -- which must leave the outputs as they were.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "csm_invert_rule.h"

namespace {

int failures = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                              \
        }                                                            \
    } while (0)

awpu_csm_t csm_of(int n_bins, float loading) {
    awpu_csm_t c;
    std::memset(&c, 0, sizeof c);
    c.window = AWPU_TONES_RECT, c.n_bins = n_bins, c.kind = AWPU_CSM_CAPON, c.loading = loading;
    for (int i = 0; i < n_bins && i < AWPU_CSM_MAX_BINS; i++) c.bin[i] = 3 + 5 * i;
    return c;
}

double value(int k, int a, int j, int part) { return (double) (((k * 53 + a * 131 + j * 17 + part * 7 + (a * j) % 23) % 199) - 99) / 64.0; }

// C = X X^H of n_blocks made-up spectra, as step 2 lays it out: Hermitian, positive semi-definite
std::vector<float> matrix_of(int K, int U, int n_blocks) {
    std::vector<float> C((size_t) K * U * U * 2, 0.0f);
    for (int k = 0; k < K; k++)
        for (int a = 0; a < U; a++)
            for (int b = 0; b < U; b++) {
                double re = 0.0, im = 0.0;
                for (int j = 0; j < n_blocks; j++) {
                    const double ar = value(k, a, j, 0), ai = value(k, a, j, 1), br = value(k, b, j, 0), bi = value(k, b, j, 1);
                    re += ar * br + ai * bi, im += ai * br - ar * bi;
                }
                float *e = &C[(((size_t) k * U + a) * U + b) * 2];
                e[0] = (float) re, e[1] = a == b ? 0.0f : (float) im;
            }
    return C;
}

void run(int K, int U, int n_blocks, float loading, int spoil) {
    const size_t per_bin = (size_t) U * U * 2;
    std::vector<float> C = matrix_of(K, U, n_blocks);
    const int dead = K > 1 ? 1 : 0;  // the bin that `spoil` makes unsolved
    if (spoil == 1) std::fill(C.begin() + dead * per_bin, C.begin() + (dead + 1) * per_bin, 0.0f);
    if (spoil == 2) C[dead * per_bin + ((size_t) (U - 1) * U) * 2] = NAN;  // entry (U-1, 0): read (or, with one mic, the diagonal)
    awpu_csm_t c = csm_of(K, spoil == 1 ? 0.0f : loading);
    if (spoil == 1)  // (the other bins must stay positive definite without loading)
        CHECK(n_blocks >= U);
    std::vector<float> G(K * per_bin, -3.0f), alone(K * per_bin, -3.0f);
    std::vector<int32_t> solved(K, -7);
    CHECK(awpu_hip_csm_invert_rule_host(C.data(), n_blocks, U, &c, G.data(), solved.data()) == AWPU_OK);
    CHECK(awpu_hip_csm_invert_rule_host(C.data(), n_blocks, U, &c, alone.data(), nullptr) == AWPU_OK);
    CHECK(std::memcmp(G.data(), alone.data(), G.size() * sizeof(float)) == 0);
    for (int k = 0; k < K; k++) {
        const float *g = &G[k * per_bin];
        if (spoil && k == dead) {
            CHECK(solved[k] == 0);
            for (size_t i = 0; i < per_bin; i++) CHECK(g[i] == 0.0f && !std::signbit(g[i]));
            continue;
        }
        CHECK(solved[k] == 1);
        for (int a = 0; a < U; a++) {
            CHECK(g[((size_t) a * U + a) * 2] > 0.0f && g[((size_t) a * U + a) * 2 + 1] == 0.0f && !std::signbit(g[((size_t) a * U + a) * 2 + 1]));
            for (int b = 0; b < a; b++) {
                const float *lo = &g[((size_t) a * U + b) * 2], *up = &g[((size_t) b * U + a) * 2];
                CHECK(lo[0] == up[0] && lo[1] == -up[1]);
            }
        }
        // G A = I, with A as the rule loads it
        const float *cm = &C[k * per_bin];
        double trace = 0.0, largest = 0.0, worst = 0.0;
        for (int a = 0; a < U; a++) trace += (double) cm[((size_t) a * U + a) * 2] / n_blocks;
        const double load = (double) c.loading * (trace / U);
        for (size_t i = 0; i < per_bin; i++) largest = std::fmax(largest, std::fabs((double) g[i]));
        for (int a = 0; a < U; a++)
            for (int b = 0; b < U; b++) {
                double re = 0.0, im = 0.0;
                for (int j = 0; j < U; j++) {
                    const double gr = g[((size_t) a * U + j) * 2], gi = g[((size_t) a * U + j) * 2 + 1];
                    const double ar = (double) cm[((size_t) j * U + b) * 2] / n_blocks + (j == b ? load : 0.0);
                    const double ai = j == b ? 0.0 : (double) cm[((size_t) j * U + b) * 2 + 1] / n_blocks;
                    re += gr * ar - gi * ai, im += gr * ai + gi * ar;
                }
                worst = std::fmax(worst, std::fmax(std::fabs(re - (a == b ? 1.0 : 0.0)), std::fabs(im)));
            }
        // G is A^-1 rounded to float: each of the U terms of an entry of G A is off by at most 2^-24 |G| |A|
        double a_largest = 0.0;
        for (size_t i = 0; i < per_bin; i++) a_largest = std::fmax(a_largest, std::fabs((double) cm[i]) / n_blocks);
        CHECK(worst <= 4.0 * U * std::ldexp(1.0, -24) * largest * (a_largest + load));
    }

    // refusals write nothing
    const std::vector<float> keep = G;
    const std::vector<int32_t> keep_solved = solved;
    const auto refused = [&](const float *m, int32_t n, int32_t u, const awpu_csm_t *cc, float *out) {
        CHECK(awpu_hip_csm_invert_rule_host(m, n, u, cc, out, solved.data()) == AWPU_ERR_INVALID);
    };
    awpu_csm_t bad = c;
    refused(nullptr, n_blocks, U, &c, G.data());
    refused(C.data(), n_blocks, U, &c, nullptr);
    refused(C.data(), 0, U, &c, G.data());
    refused(C.data(), n_blocks, 0, &c, G.data());
    refused(C.data(), n_blocks, U, nullptr, G.data());
    bad = c, bad.window = 2, refused(C.data(), n_blocks, U, &bad, G.data());
    bad = c, bad.n_bins = 0, refused(C.data(), n_blocks, U, &bad, G.data());
    bad = c, bad.n_bins = 9, refused(C.data(), n_blocks, U, &bad, G.data());
    bad = c, bad.bin[0] = -1, refused(C.data(), n_blocks, U, &bad, G.data());
    bad = c, bad.kind = 3, refused(C.data(), n_blocks, U, &bad, G.data());
    bad = c, bad.loading = -1.0f, refused(C.data(), n_blocks, U, &bad, G.data());
    bad = c, bad.loading = NAN, refused(C.data(), n_blocks, U, &bad, G.data());
    CHECK(keep == G && keep_solved == solved);
}

}  // namespace

int main() {
    run(1, 1, 1, 0.0f, 0);  // the smallest
    run(1, 1, 1, 0.0f, 1);
    run(1, 1, 1, 0.5f, 2);
    run(3, 2, 5, 1e-2f, 0);
    run(8, 5, 9, 1e-2f, 0);
    run(8, 5, 9, 1e-2f, 1);  // an all-zero bin, no loading
    run(2, 7, 3, 1e-2f, 0);  // fewer blocks than mics: the loading alone makes it definite
    run(3, 17, 40, 1e-3f, 2);  // a NaN entry
    if (failures) return 1;
    std::printf("csm invert rule: ok\n");
    return 0;
}
