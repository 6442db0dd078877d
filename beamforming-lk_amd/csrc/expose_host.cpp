// expose_host.cpp -- awpu_hip_expose_count and awpu_hip_expose_rows: the rule of include/awpu_hip_expose.h as executable C++,
// pure host code with no handle (like awpu_hip_find_peaks).  It is written for reading: block by block in the call's order, as
// the rule states it.  The kernel (expose_kernels.hip) evaluates the same expressions out of expose_rule.h.
#include <cstring>
#include <vector>

#include "expose_rule.h"

extern "C" int awpu_hip_expose_count(int32_t n_blocks, int32_t first, int32_t every, int32_t length, int32_t *n_frames, int32_t *next_first,
                                     int32_t *carry_in, int32_t *carry_out, int32_t *n_swept) {
    if (!n_frames || !next_first || !carry_in || !carry_out || !n_swept) return AWPU_ERR_INVALID;
    if (n_blocks < 1 || first < 0 || every < 1 || length < 1 || length > every) return AWPU_ERR_INVALID;
    const awpu::ExposeCount c = awpu::expose_count(n_blocks, first, every, length);
    *n_frames = c.n_frames, *next_first = c.next_first, *carry_in = c.carry_in, *carry_out = c.carry_out, *n_swept = c.n_swept;
    return AWPU_OK;
}

extern "C" int awpu_hip_expose_rows(const float *power, int32_t n_blocks, int32_t n_pixels, int32_t first, int32_t every,
                                    const awpu_expose_t *e, float *carry, float *frames) {
    if (!power || n_blocks < 1 || n_pixels < 1 || first < 0 || every < 1 || awpu::expose_refusal(e, every)) return AWPU_ERR_INVALID;
    const awpu::ExposeCount c = awpu::expose_count(n_blocks, first, every, e->length);
    if (!carry && (c.carry_in > 0 || c.carry_out > 0)) return AWPU_ERR_INVALID;
    if (!frames && c.n_frames > 0) return AWPU_ERR_INVALID;
    const size_t n = (size_t) n_pixels;
    const float length_f = (float) e->length;
    std::vector<float> acc(n, 0.0f);
    if (c.carry_in > 0) std::memcpy(acc.data(), carry, n * sizeof(float));
    for (int32_t k = 0; k < n_blocks; k++) {
        int32_t q, j;
        if (!awpu::expose_block(k, first, every, e->length, &q, &j)) continue;
        const float *p = power + (size_t) k * n;
        for (size_t i = 0; i < n; i++) acc[i] = q == 0 ? p[i] : awpu::expose_step(acc[i], p[i], e->mode);
        if (q == e->length - 1)
            for (size_t i = 0; i < n; i++) frames[(size_t) j * n + i] = awpu::expose_close(acc[i], length_f, e->mode);
    }
    if (c.carry_out > 0) std::memcpy(carry, acc.data(), n * sizeof(float));
    return AWPU_OK;
}
