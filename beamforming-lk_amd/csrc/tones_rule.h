// tones_rule.h -- the rule of include/awpu_hip_tones.h as host C++: the argument checks, the two tables and one pixel of one
// frame, written for reading, in the rule's own order.  Host only (the kernel, tones_kernels.hip, takes the same operations on the
// same operands lane by lane and reads the same tables); shared by the host definition (tones_host.cpp) and the stand-alone
// checker (tests/host/tones_rule_check.cpp).  No HIP types: a host compiler alone takes it.  Its users switch contraction off for
// GCC (#pragma GCC optimize at their top); for clang the functions below do.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "awpu_hip_tones.h"
#include "cohere_rule.h"  // cohere_check_table: the table and the active list against the frame

namespace awpu {

constexpr int kTonesSamples = 256;  // a block, and the transform's length
constexpr int kTonesBins = AWPU_TONES_BINS;

// what is wrong with a request, or null
inline const char *tones_refusal(const awpu_tones_t *t) {
    if (!t) return "null argument";
    if (t->window != AWPU_TONES_RECT && t->window != AWPU_TONES_HANN) return "window is AWPU_TONES_RECT or AWPU_TONES_HANN";
    if (t->n_groups < 1 || t->n_groups > kTonesBins) return "n_groups lies in [1, 129]";
    if (t->edge[0] < 0 || t->edge[t->n_groups] > kTonesBins) return "the edges lie in [0, 129]";
    for (int g = 0; g < t->n_groups; g++)
        if (t->edge[g] >= t->edge[g + 1]) return "the edges are strictly ascending";
    return nullptr;
}
// ... with what a run shows
inline const char *tones_refusal(const awpu_tones_t *t, int32_t show) {
    if (const char *why = tones_refusal(t)) return why;
    if (show != AWPU_TONES_SHOW_PITCH && (show < 0 || show >= t->n_groups)) return "show is a group of t or AWPU_TONES_SHOW_PITCH";
    return nullptr;
}

inline float tones_wss(int32_t window) { return window == AWPU_TONES_HANN ? 96.0f : 256.0f; }

// the two tables, by the header's formulas in double: no contraction here either, so that 0.5 - 0.5 * cos(..) is a product, then a difference
inline void tones_window(int32_t window, float *w) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double two_pi = 6.283185307179586476925286766559;
    for (int i = 0; i < kTonesSamples; i++) w[i] = window == AWPU_TONES_HANN ? (float) (0.5 - 0.5 * std::cos(two_pi * i / kTonesSamples)) : 1.0f;
}

inline void tones_twiddles(float (*t)[2]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double two_pi = 6.283185307179586476925286766559;
    for (int k = 0; k < kTonesSamples / 2; k++) {
        t[k][0] = (float) std::cos(two_pi * k / kTonesSamples);
        t[k][1] = (float) (-std::sin(two_pi * k / kTonesSamples));
    }
}

// step 1: out[0..255] of one pixel, cohere_pixel's out[] operation for operation
inline void tones_sums(const float *frame, int32_t hist, const int32_t *off_row, const float *frac_row, const int32_t *index, int32_t usable,
                       const float *gain, float *out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    constexpr int N = kTonesSamples;
    float x[N + 1];
    for (int i = 0; i < N; i++) out[i] = 0.0f;
    for (int32_t s = 0; s < usable; s++) {
        const int32_t id = index[s];
        const float *src = frame + (size_t) id * (size_t) hist + off_row[id];
        const float f = frac_row[id];
        if (gain) {
            const float g = gain[s];
            for (int i = 0; i <= N; i++) x[i] = src[i] * g;
        } else {
            for (int i = 0; i <= N; i++) x[i] = src[i];
        }
        for (int i = 0; i < N; i++) {
            const float d = x[i] - x[i + 1];
            out[i] = out[i] + __builtin_fmaf(f, d, x[i + 1]);
        }
    }
}

// steps 2 to 4: out[256] -> z[0..128] (re, im) and bins[0..128]; w and tw are the two tables
inline void tones_transform(const float *out, const float *w, const float (*tw)[2], float wss, int32_t usable, float (*spectrum)[2], float *bins) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    constexpr int N = kTonesSamples;
    float y[N], re[N], im[N];
    y[0] = 0.0f, y[N - 1] = 0.0f;
    for (int i = 1; i < N - 1; i++) {
        const float ma = out[i] * 0.5f - 0.25f * (out[i + 1] + out[i - 1]);
        y[i] = ma * w[i];
    }
    for (int n = 0; n < N; n++) {
        int r = 0;
        for (int bit = 0; bit < 8; bit++) r |= ((n >> bit) & 1) << (7 - bit);
        re[n] = y[r], im[n] = 0.0f;
    }
    for (int h = 1; h < N; h *= 2)
        for (int base = 0; base < N; base += 2 * h)
            for (int j = 0; j < h; j++) {
                const float wr = tw[j * (N / 2 / h)][0], wi = tw[j * (N / 2 / h)][1];
                const int a = base + j, b = base + j + h;
                const float p0 = re[b] * wr, p1 = im[b] * wi, p2 = re[b] * wi, p3 = im[b] * wr;
                const float tr = p0 - p1, ti = p2 + p3;
                const float ar = re[a], ai = im[a];
                re[a] = ar + tr, im[a] = ai + ti;
                re[b] = ar - tr, im[b] = ai - ti;
            }
    const float scale = wss * (float) (N * usable);
    for (int k = 0; k < kTonesBins; k++) {
        spectrum[k][0] = re[k], spectrum[k][1] = im[k];
        const float q0 = re[k] * re[k], q1 = im[k] * im[k];
        const float s = q0 + q1;
        const float c = (k == 0 || k == kTonesBins - 1) ? 1.0f : 2.0f;
        bins[k] = (c * s) / scale;
    }
}

// step 5: the groups of t, k ascending from +0.0f
inline void tones_groups(const float *bins, const awpu_tones_t *t, float *tone) {
    for (int g = 0; g < t->n_groups; g++) {
        float sum = 0.0f;
        for (int k = t->edge[g]; k < t->edge[g + 1]; k++) sum = sum + bins[k];
        tone[g] = sum;
    }
}

// step 6: the greater bits win, equal bits go to the lower k
inline int32_t tones_pitch(const float *bins, const awpu_tones_t *t) {
    int32_t best = t->edge[0];
    uint32_t best_bits = 0;
    for (int k = t->edge[0]; k < t->edge[t->n_groups]; k++) {
        uint32_t u;
        __builtin_memcpy(&u, &bins[k], sizeof u);
        if (k == t->edge[0] || u > best_bits) best = k, best_bits = u;
    }
    return best;
}

}  // namespace awpu
