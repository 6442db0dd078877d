// find_host.cpp -- awpu_hip_find_peaks: the rule of include/awpu_hip_find.h as executable C++, pure host code with no handle
// (like awpu_hip_heatmap_u8).  It is written for reading, not for speed: every pixel that passes the thresholds looks at its
// whole window.  The kernel (find_kernels.hip) evaluates the same expressions out of find_rule.h.
#include <algorithm>
#include <cstring>
#include <functional>
#include <vector>

#include "find_rule.h"

extern "C" int awpu_hip_find_peaks(const float *power, int32_t n_frames, const awpu_find_t *f, awpu_source_t *sources, int32_t *count) {
    if (!power || !sources || !count || n_frames < 1 || awpu::find_refusal(f)) return AWPU_ERR_INVALID;
    const int rows = f->rows, cols = f->cols, R = f->radius, n = rows * cols;
    const double sep_rows = awpu::find_separation(f->fov_deg, rows), sep_cols = awpu::find_separation(f->fov_deg, cols);
    std::vector<uint32_t> bits(n);
    std::vector<unsigned long long> peaks;
    for (int32_t k = 0; k < n_frames; k++) {
        const float *p = power + (size_t) k * n;
        std::memcpy(bits.data(), p, (size_t) n * sizeof(float));
        unsigned long long best = 0;
        for (int i = 0; i < n; i++) best = std::max(best, awpu::find_key(bits[i], i));
        float m;
        const uint32_t m_bits = (uint32_t) (best >> 32);
        std::memcpy(&m, &m_bits, sizeof m);
        const float floor_ratio = awpu::find_floor_ratio(f->min_ratio, m);
        peaks.clear();
        for (int r = 0; r < rows; r++) {
            for (int c = 0; c < cols; c++) {
                const int i = r * cols + c;
                if (!(p[i] > 0.0f && p[i] >= f->min_power && p[i] >= floor_ratio)) continue;
                const unsigned long long key = awpu::find_key(bits[i], i);
                bool beats = true;
                for (int rr = std::max(r - R, 0); rr <= std::min(r + R, rows - 1); rr++)
                    for (int cc = std::max(c - R, 0); cc <= std::min(c + R, cols - 1); cc++)
                        beats &= awpu::find_key(bits[rr * cols + cc], rr * cols + cc) <= key;
                if (beats) peaks.push_back(key);
            }
        }
        const int found = (int) std::min<size_t>(peaks.size(), f->max_sources);
        std::partial_sort(peaks.begin(), peaks.begin() + found, peaks.end(), std::greater<unsigned long long>());
        awpu_source_t *out = sources + (size_t) k * f->max_sources;
        for (int s = 0; s < f->max_sources; s++) {
            if (s < found) {
                const int i = (int) awpu::find_key_pixel(peaks[s]);
                awpu::find_describe(p, rows, cols, i / cols, i % cols, sep_rows, sep_cols, out + s);
            } else {
                awpu::find_unused(out + s);
            }
        }
        count[k] = found;
    }
    return AWPU_OK;
}
