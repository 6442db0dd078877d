// peel_host.cpp -- awpu_hip_peel_step_host and awpu_hip_peel_host: the rule of include/awpu_hip_peel.h as executable C++, pure
// host code with no handle (like awpu_hip_cohere_host).  Written for reading, not for speed: frame by frame, sample by sample,
// as the rule states it (peel_rule.h); the loop's sweep is the power of the coherence rule (cohere_rule.h).  The kernels
// (peel_kernels.hip) take the same operations lane by lane.  A host compiler alone takes this file.
#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC optimize("fp-contract=off")
#endif

#include <vector>

#include "cohere_rule.h"
#include "peel_rule.h"

namespace {

// the refusals the two calls share; the reach where there is none
int check_peel_table(int32_t n_streams, int32_t hist, const int32_t *off, const float *frac, int32_t lut_stride, int32_t n_pixels,
                     const int32_t *index, int32_t usable, awpu::PeelReach *reach) {
    if (!off || !frac || !index) return AWPU_ERR_INVALID;
    if (const int rc = awpu::cohere_check_table(n_streams, hist, off, frac, lut_stride, n_pixels, index, usable)) return rc;
    if (awpu::peel_listed_twice(index, usable)) return AWPU_ERR_INVALID;
    *reach = awpu::peel_reach(off, lut_stride, n_pixels, index, usable);
    return awpu::peel_in_range(*reach, hist) ? AWPU_OK : AWPU_ERR_RANGE;
}

std::vector<float> u_of(float loop_gain, const float *gain, int32_t usable) {
    std::vector<float> u((size_t) usable);
    for (int32_t s = 0; s < usable; s++) u[(size_t) s] = awpu::peel_u(loop_gain, gain, s);
    return u;
}

}  // namespace

extern "C" int32_t awpu_hip_peel_beam_length(int32_t n_streams, int32_t hist, const int32_t *off, const float *frac, int32_t lut_stride,
                                             int32_t n_pixels, const int32_t *index, int32_t usable) {
    awpu::PeelReach reach;
    if (const int rc = check_peel_table(n_streams, hist, off, frac, lut_stride, n_pixels, index, usable, &reach)) return rc;
    return reach.len;
}

extern "C" int awpu_hip_peel_step_host(float *frames, int32_t batch, int32_t n_streams, int32_t hist, const int32_t *off, const float *frac,
                                       int32_t lut_stride, int32_t n_pixels, const int32_t *index, int32_t usable, const float *gain,
                                       const int32_t *pixel, float loop_gain, float *beams) {
    if (!frames || !pixel || batch < 1) return AWPU_ERR_INVALID;
    if (awpu::peel_gain_refusal(loop_gain)) return AWPU_ERR_INVALID;
    awpu::PeelReach reach;
    if (const int rc = check_peel_table(n_streams, hist, off, frac, lut_stride, n_pixels, index, usable, &reach)) return rc;
    for (int32_t b = 0; b < batch; b++)
        if (pixel[b] < -1 || pixel[b] >= n_pixels) return AWPU_ERR_INVALID;
    const std::vector<float> u = u_of(loop_gain, gain, usable);
    std::vector<float> beam((size_t) reach.len);
    for (int32_t b = 0; b < batch; b++) {
        float *out = beams ? beams + (size_t) b * (size_t) reach.len : nullptr;
        if (pixel[b] < 0) {
            if (out) std::memset(out, 0, (size_t) reach.len * sizeof(float));
            continue;
        }
        const size_t row = (size_t) pixel[b] * (size_t) lut_stride;
        awpu::peel_step_frame(frames + (size_t) b * (size_t) n_streams * (size_t) hist, hist, off + row, frac + row, index, usable, gain, u.data(), reach,
                              beam.data());
        if (out) std::memcpy(out, beam.data(), (size_t) reach.len * sizeof(float));
    }
    return AWPU_OK;
}

extern "C" int awpu_hip_peel_host(const float *frames, int32_t batch, int32_t n_streams, int32_t hist, const int32_t *off, const float *frac,
                                  int32_t lut_stride, int32_t n_pixels, const int32_t *index, int32_t usable, const float *gain,
                                  const awpu_peel_t *pe, awpu_peel_step_t *steps, float *clean, float *residual, float *map,
                                  float *residual_frames) {
    if (!frames || batch < 1) return AWPU_ERR_INVALID;
    if (awpu::peel_refusal(pe)) return AWPU_ERR_INVALID;
    awpu::PeelReach reach;
    if (const int rc = check_peel_table(n_streams, hist, off, frac, lut_stride, n_pixels, index, usable, &reach)) return rc;
    constexpr int N = awpu::kCohereSamples;
    const size_t frame_floats = (size_t) n_streams * (size_t) hist;
    const std::vector<float> u = u_of(pe->gain, gain, usable);
    std::vector<float> work(frame_floats), row((size_t) n_pixels), beam((size_t) reach.len);
    float out[N], e[N];
    const auto sweep = [&]() {
        for (int32_t p = 0; p < n_pixels; p++) {
            const size_t at = (size_t) p * (size_t) lut_stride;
            row[(size_t) p] = awpu::cohere_pixel(work.data(), hist, off + at, frac + at, index, usable, gain, out, e).power;
        }
    };
    for (int32_t b = 0; b < batch; b++) {
        std::memcpy(work.data(), frames + (size_t) b * frame_floats, frame_floats * sizeof(float));
        awpu_peel_step_t st[AWPU_PEEL_MAX_STEPS];
        for (auto &s : st) s = {-1, 0.0f, 0.0f};
        float first = 0.0f;
        bool done = false;
        sweep();  // P_0
        for (int32_t k = 0; k < pe->steps && !done; k++) {
            unsigned long long best = 0;
            for (int32_t p = 0; p < n_pixels; p++) {
                const unsigned long long key = awpu::peel_key(row[(size_t) p], (uint32_t) p);
                best = key > best ? key : best;
            }
            if (best == 0) break;
            const int32_t pick = (int32_t) awpu::find_key_pixel(best);
            const float before = row[(size_t) pick];
            if (k == 0) first = before;
            if (before < awpu::find_floor_ratio(pe->stop_ratio, first)) break;
            st[k].pixel = pick, st[k].before = before;
            const size_t at = (size_t) pick * (size_t) lut_stride;
            awpu::peel_step_frame(work.data(), hist, off + at, frac + at, index, usable, gain, u.data(), reach, beam.data());
            sweep();  // P_{k+1}
            st[k].removed = awpu::peel_removed(before, row[(size_t) pick]);
        }
        if (steps) std::memcpy(steps + (size_t) b * (size_t) pe->steps, st, (size_t) pe->steps * sizeof(awpu_peel_step_t));
        for (int32_t p = 0; p < n_pixels; p++) {
            const size_t at = (size_t) b * (size_t) n_pixels + (size_t) p;
            const float c = awpu::peel_clean_at(st, pe->steps, p);
            if (clean) clean[at] = c;
            if (residual) residual[at] = row[(size_t) p];
            if (map) map[at] = c + row[(size_t) p];
        }
        if (residual_frames) std::memcpy(residual_frames + (size_t) b * frame_floats, work.data(), frame_floats * sizeof(float));
    }
    return AWPU_OK;
}
