// csm_eig_check.cpp -- awpu_hip_csm_eig_host, _eig_weigh_host and _eig_map_host (csrc/csm_eig_host.cpp, csm_eig_rule.h) as a
// program of its own, meant to be built with -fsanitize=address,undefined: every buffer exactly as long as the header says, the
// smallest sizes (one mic, one bin), odd sizes with the dummy that sits out, eight bins, `solved` and `sweeps` given and null, an
// unsolved bin among solved ones (all zeros; a NaN entry; an eigenvalue that fits no float), one bin of 129 mics, a matrix of equal
// entries whose eigenvalues tie, A v against lambda v, V's columns against the identity, H's structure,
// both maps on a small table, and the refusals -- which must leave the outputs as they were.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "csm_eig_rule.h"

namespace {

int failures = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                              \
        }                                                            \
    } while (0)

awpu_csm_t csm_of(int n_bins) {
    awpu_csm_t c;
    std::memset(&c, 0, sizeof c);
    c.window = AWPU_TONES_RECT, c.n_bins = n_bins, c.kind = AWPU_CSM_CONVENTIONAL, c.loading = 0.0f;
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

void run(int K, int U, int n_blocks, int spoil) {
    const size_t per_bin = (size_t) U * U * 2;
    std::vector<float> C = matrix_of(K, U, n_blocks);
    const int dead = K > 1 ? 1 : 0;  // the bin that `spoil` makes unsolved
    if (spoil == 1) std::fill(C.begin() + dead * per_bin, C.begin() + (dead + 1) * per_bin, 0.0f);
    if (spoil == 2) C[dead * per_bin + ((size_t) (U - 1) * U) * 2] = NAN;  // entry (U-1, 0): read (or, with one mic, the diagonal)
    if (spoil == 3)  // every entry (3e38, 0): finite entries, the eigenvalue U * 3e38 / n_blocks a finite double that no float holds
        for (size_t i = 0; i < per_bin; i++) C[dead * per_bin + i] = i % 2 ? 0.0f : 3e38f;
    const awpu_csm_t c = csm_of(K);
    std::vector<float> values((size_t) K * U, -3.0f), vectors(K * per_bin, -3.0f), values2((size_t) K * U, -3.0f), vectors2(K * per_bin, -3.0f);
    std::vector<int32_t> solved(K, -7), sweeps(K, -7);
    CHECK(awpu_hip_csm_eig_host(C.data(), n_blocks, U, &c, values.data(), vectors.data(), solved.data(), sweeps.data()) == AWPU_OK);
    CHECK(awpu_hip_csm_eig_host(C.data(), n_blocks, U, &c, values2.data(), vectors2.data(), nullptr, nullptr) == AWPU_OK);
    CHECK(std::memcmp(values.data(), values2.data(), values.size() * sizeof(float)) == 0);
    CHECK(std::memcmp(vectors.data(), vectors2.data(), vectors.size() * sizeof(float)) == 0);
    for (int k = 0; k < K; k++) {
        const float *val = &values[(size_t) k * U], *vec = &vectors[k * per_bin];
        if (spoil && k == dead) {
            CHECK(solved[k] == 0 && (spoil == 3 ? sweeps[k] >= 1 && sweeps[k] <= 16 : sweeps[k] == 0));  // (3 fails behind its sweeps)
            for (int i = 0; i < U; i++) CHECK(val[i] == 0.0f && !std::signbit(val[i]));
            for (size_t i = 0; i < per_bin; i++) CHECK(vec[i] == 0.0f && !std::signbit(vec[i]));
            continue;
        }
        CHECK(solved[k] == 1 && sweeps[k] >= 1 && sweeps[k] <= 16);
        for (int r = 1; r < U; r++) CHECK(val[r - 1] >= val[r]);
        // A v = lambda v and V^H V = I, with A as the rule loads it, within (U + 2) 2^-23 (of the largest eigenvalue)
        const float *cm = &C[k * per_bin];
        const double bound = (U + 2) * std::ldexp(1.0, -23);
        double worst = 0.0, gram = 0.0;
        for (int r = 0; r < U; r++) {
            const float *v = vec + (size_t) r * U * 2;
            for (int a = 0; a < U; a++) {
                double re = 0.0, im = 0.0;
                for (int b = 0; b < U; b++) {
                    const float *e = b <= a ? &cm[((size_t) a * U + b) * 2] : &cm[((size_t) b * U + a) * 2];
                    const double ar = (double) e[0] / n_blocks, ai = b == a ? 0.0 : (b < a ? 1.0 : -1.0) * (double) e[1] / n_blocks;
                    re += ar * v[2 * b] - ai * v[2 * b + 1], im += ar * v[2 * b + 1] + ai * v[2 * b];
                }
                worst = std::fmax(worst, std::fmax(std::fabs(re - (double) val[r] * v[2 * a]), std::fabs(im - (double) val[r] * v[2 * a + 1])));
            }
            for (int s = 0; s <= r; s++) {
                const float *u = vec + (size_t) s * U * 2;
                double re = 0.0, im = 0.0;
                for (int a = 0; a < U; a++) re += (double) u[2 * a] * v[2 * a] + (double) u[2 * a + 1] * v[2 * a + 1], im += (double) u[2 * a] * v[2 * a + 1] - (double) u[2 * a + 1] * v[2 * a];
                gram = std::fmax(gram, std::fmax(std::fabs(re - (s == r ? 1.0 : 0.0)), std::fabs(im)));
            }
        }
        CHECK(worst <= bound * std::fmax((double) val[0], 0.0));
        CHECK(gram <= bound);
    }

    // the weighed matrix, both kinds, and its structure
    for (int kind = 0; kind < 2; kind++) {
        awpu_csm_eig_t e{kind, U > 2 ? 2 : U - 1, kind ? 4 : 0, 0};
        std::vector<float> H(K * per_bin, -3.0f);
        CHECK(awpu_hip_csm_eig_weigh_host(values.data(), vectors.data(), U, &c, &e, H.data()) == AWPU_OK);
        for (int k = 0; k < K; k++) {
            const float *h = &H[k * per_bin];
            double trace = 0.0;
            for (int a = 0; a < U; a++) {
                trace += h[((size_t) a * U + a) * 2];
                CHECK(h[((size_t) a * U + a) * 2 + 1] == 0.0f && !std::signbit(h[((size_t) a * U + a) * 2 + 1]));
                for (int b = 0; b < a; b++) {
                    const float *lo = &h[((size_t) a * U + b) * 2], *up = &h[((size_t) b * U + a) * 2];
                    CHECK(lo[0] == up[0] && lo[1] == -up[1]);
                }
            }
            if (kind == AWPU_CSM_EIG_MUSIC && !(spoil && k == dead)) CHECK(std::fabs(trace - (U - e.n_sources)) <= (U + 2) * std::ldexp(1.0, -23) * U);
        }
        // the map on a table of three pixels, with and without the solved words
        std::vector<int32_t> off((size_t) 3 * U), index(U);
        std::vector<float> frac((size_t) 3 * U);
        for (int a = 0; a < U; a++) index[a] = U - 1 - a;
        for (size_t i = 0; i < off.size(); i++) off[i] = (int32_t) ((i * 37) % 200), frac[i] = (float) ((i * 11) % 16) / 16.0f;
        std::vector<float> map((size_t) K * 3, -3.0f), all((size_t) K * 3, -3.0f);
        CHECK(awpu_hip_csm_eig_map_host(H.data(), solved.data(), off.data(), frac.data(), U, 3, index.data(), U, &c, &e, map.data()) == AWPU_OK);
        CHECK(awpu_hip_csm_eig_map_host(H.data(), nullptr, off.data(), frac.data(), U, 3, index.data(), U, &c, &e, all.data()) == AWPU_OK);
        for (int k = 0; k < K; k++)
            for (int p = 0; p < 3; p++) {
                const float m = map[(size_t) k * 3 + p];
                if (spoil && k == dead) {
                    CHECK(m == 0.0f && !std::signbit(m));
                } else {
                    CHECK(std::isfinite(m) && m >= 0.0f && m == all[(size_t) k * 3 + p]);
                    if (kind == AWPU_CSM_EIG_MUSIC) CHECK(m <= 16777216.0f);
                }
            }
        // refusals write nothing
        const std::vector<float> keep_h = H, keep_map = map;
        awpu_csm_eig_t bad = e;
        awpu_csm_t badc = c;
        const auto refused = [&](const awpu_csm_t *cc, const awpu_csm_eig_t *ee) {
            CHECK(awpu_hip_csm_eig_weigh_host(values.data(), vectors.data(), U, cc, ee, H.data()) == AWPU_ERR_INVALID);
            CHECK(awpu_hip_csm_eig_map_host(H.data(), solved.data(), off.data(), frac.data(), U, 3, index.data(), U, cc, ee, map.data()) == AWPU_ERR_INVALID);
        };
        refused(nullptr, &e);
        refused(&c, nullptr);
        bad = e, bad.kind = 2, refused(&c, &bad);
        bad = e, bad.kind = -1, refused(&c, &bad);
        bad = e, bad.n_sources = U, refused(&c, &bad);
        bad = e, bad.n_sources = -1, refused(&c, &bad);
        bad = e, bad.root = 7, refused(&c, &bad);
        bad = e, bad.root = -1, refused(&c, &bad);
        bad = e, bad.reserved = 1, refused(&c, &bad);
        badc = c, badc.kind = AWPU_CSM_CAPON, refused(&badc, &e);
        badc = c, badc.n_bins = 9, refused(&badc, &e);
        CHECK(awpu_hip_csm_eig_weigh_host(nullptr, vectors.data(), U, &c, &e, H.data()) == AWPU_ERR_INVALID);
        CHECK(awpu_hip_csm_eig_weigh_host(values.data(), vectors.data(), 0, &c, &e, H.data()) == AWPU_ERR_INVALID);
        CHECK(awpu_hip_csm_eig_map_host(H.data(), solved.data(), off.data(), frac.data(), U, 0, index.data(), U, &c, &e, map.data()) == AWPU_ERR_INVALID);
        CHECK(awpu_hip_csm_eig_map_host(H.data(), solved.data(), off.data(), frac.data(), U, 3, index.data(), U, &c, &e, nullptr) == AWPU_ERR_INVALID);
        CHECK(keep_h == H && keep_map == map);
    }

    const std::vector<float> keep = values, keep_vec = vectors;
    const std::vector<int32_t> keep_solved = solved, keep_sweeps = sweeps;
    const auto refused = [&](const float *m, int32_t n, int32_t u, const awpu_csm_t *cc, float *val, float *vec) {
        CHECK(awpu_hip_csm_eig_host(m, n, u, cc, val, vec, solved.data(), sweeps.data()) == AWPU_ERR_INVALID);
    };
    awpu_csm_t bad = c;
    refused(nullptr, n_blocks, U, &c, values.data(), vectors.data());
    refused(C.data(), n_blocks, U, &c, nullptr, vectors.data());
    refused(C.data(), n_blocks, U, &c, values.data(), nullptr);
    refused(C.data(), 0, U, &c, values.data(), vectors.data());
    refused(C.data(), n_blocks, 0, &c, values.data(), vectors.data());
    refused(C.data(), n_blocks, U, nullptr, values.data(), vectors.data());
    bad = c, bad.window = 2, refused(C.data(), n_blocks, U, &bad, values.data(), vectors.data());
    bad = c, bad.n_bins = 0, refused(C.data(), n_blocks, U, &bad, values.data(), vectors.data());
    bad = c, bad.bin[0] = -1, refused(C.data(), n_blocks, U, &bad, values.data(), vectors.data());
    bad = c, bad.kind = 3, refused(C.data(), n_blocks, U, &bad, values.data(), vectors.data());
    CHECK(keep == values && keep_vec == vectors && keep_solved == solved && keep_sweeps == sweeps);
}

// every entry (2, 0), one block: rank one, eigenvalues that tie exactly behind rotations -- every row of vectors is written once
void equal_entries(int U) {
    const size_t per_bin = (size_t) U * U * 2;
    std::vector<float> C(per_bin), values(U, -3.0f), vectors(per_bin, -3.0f);
    for (size_t i = 0; i < per_bin; i++) C[i] = i % 2 ? 0.0f : 2.0f;
    const awpu_csm_t c = csm_of(1);
    int32_t solved = -7, sweeps = -7;
    CHECK(awpu_hip_csm_eig_host(C.data(), 1, U, &c, values.data(), vectors.data(), &solved, &sweeps) == AWPU_OK);
    CHECK(solved == 1 && sweeps >= 1 && sweeps <= 16);
    int ties = 0;
    for (int r = 1; r < U; r++) {
        CHECK(values[r - 1] >= values[r]);
        ties += values[r - 1] == values[r] ? 1 : 0;
    }
    CHECK(ties >= 1);
    CHECK(std::fabs((double) values[0] - 2.0 * U) <= 2.0 * U * std::ldexp(1.0, -22));
    for (int r = 0; r < U; r++) {  // a row that the sort left out would keep its -3 words: every row has norm 1
        double norm = 0.0;
        for (int a = 0; a < 2 * U; a++) norm += (double) vectors[(size_t) r * U * 2 + a] * vectors[(size_t) r * U * 2 + a];
        CHECK(std::fabs(norm - 1.0) <= (U + 2) * std::ldexp(1.0, -23));
    }
}

}  // namespace

int main() {
    run(1, 1, 1, 0);  // the smallest: one entry, no pair
    run(1, 1, 1, 1);
    run(1, 1, 1, 2);
    run(3, 2, 5, 0);   // one pair
    run(8, 5, 9, 0);   // an odd size: the dummy sits out
    run(8, 5, 9, 1);   // an all-zero bin
    run(2, 7, 3, 0);   // fewer blocks than mics: rank-deficient
    run(3, 17, 40, 2);  // a NaN entry
    run(1, 24, 6, 0);
    run(3, 17, 9, 3);     // an eigenvalue past FLT_MAX: unsolved behind its sweeps
    run(1, 129, 261, 0);  // above 64 mics, odd
    equal_entries(5);
    equal_entries(65);
    if (failures) return 1;
    std::printf("csm eig rule: ok\n");
    return 0;
}
