// SphericalGradientHip driver for tests/test_tracker_cpu.py (--nogpu: the constructor must throw without a device) and
// tests/test_gpu_tracker.py (frames file in, targets out, twice with the same seed).
//   test_spherical_gradient --nogpu
//   test_spherical_gradient FRAMES.bin BLOCKS SEED     FRAMES.bin = float32 [BLOCKS][64][1024]
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "spherical_gradient_hip.h"

using awpu_host::SphericalGradientHip;
using awpu_host::TargetHip;

static std::vector<TargetHip> run(const std::vector<float> &frames, int blocks, uint32_t seed, const float *xyz, FILE *log) {
    std::vector<int32_t> index(64);
    for (int i = 0; i < 64; i++) index[i] = i;
    SphericalGradientHip sg(0, xyz, 64, index.data(), 64, 16, 10, 180.0f, seed);  // aw_processing_unit.cpp:83: 16 seekers, 10 iterations
    float *d = nullptr;
    if (hipMalloc(&d, 64 * 1024 * sizeof(float)) != hipSuccess) throw std::runtime_error("hipMalloc");
    for (int b = 0; b < blocks; b++) {
        if (hipMemcpy(d, frames.data() + (size_t) b * 64 * 1024, 64 * 1024 * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
            throw std::runtime_error("hipMemcpy");
        sg.reset();
        const int rc = sg.update(d);
        if (rc != AWPU_OK) throw std::runtime_error("update failed");
        if (log)
            for (const TargetHip &t : sg.targets())
                std::fprintf(log, "block %d target %.17g %.17g %.9g %.9g %llu\n", b, t.theta, t.phi, t.power, t.probability,
                             (unsigned long long) t.start);
    }
    (void) hipFree(d);
    return sg.targets();
}

int main(int argc, char **argv) {
    std::vector<float> xyz(3 * 64);
    if (awpu_hip_create_antenna(8, 8, 0.02f, xyz.data()) != AWPU_OK) return 2;
    if (argc > 1 && std::strcmp(argv[1], "--nogpu") == 0) {
        std::vector<int32_t> index(64);
        for (int i = 0; i < 64; i++) index[i] = i;
        try {
            SphericalGradientHip sg(0, xyz.data(), 64, index.data(), 64, 16, 10, 180.0f, 1);
        } catch (const std::runtime_error &e) {
            std::printf("refused: %s\n", e.what());
            return 0;
        }
        std::printf("constructed without a device\n");
        return 1;
    }
    if (argc < 4) return 2;
    const int blocks = std::atoi(argv[2]);
    const uint32_t seed = (uint32_t) std::strtoul(argv[3], nullptr, 10);
    std::vector<float> frames((size_t) blocks * 64 * 1024);
    FILE *f = std::fopen(argv[1], "rb");
    if (!f || std::fread(frames.data(), sizeof(float), frames.size(), f) != frames.size()) return 2;
    std::fclose(f);
    try {
        const std::vector<TargetHip> a = run(frames, blocks, seed, xyz.data(), stdout);
        const std::vector<TargetHip> b = run(frames, blocks, seed, xyz.data(), nullptr);
        bool same = a.size() == b.size();
        for (size_t k = 0; same && k < a.size(); k++)
            same = std::memcmp(&a[k], &b[k], sizeof(TargetHip)) == 0;
        std::printf("repeat %s\n", same ? "identical" : "DIFFERENT");
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
