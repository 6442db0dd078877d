// spherical_gradient_hip.h -- C++ host mirror of the reference's --tracking worker, SphericalGradient
// (src/dsp/gradient_ascend.{h,cpp}), on top of awpu_hip_track (include/awpu_hip_track.h).
//
// SphericalGradient::update (gradient_ascend.cpp:295-409) steps up to TRACKER_MAX trackers TRACKER_STEPS times and
// SWARM seekers once per iteration, one beam at a time.  Here one iteration is ONE awpu_hip_track launch that carries
// both groups.  That is the reference's order because (1) particles do not interact while they step, (2) the absorb
// pass compares trackers only after all of them have stepped, and (3) a seeker checks its closeness against the
// PREVIOUS block's `tracking` list, not against this iteration's trackers.
//
// Two changes make the class deterministic (the reference's arithmetic is otherwise kept, quirks included):
//   - canContinue() polling (worker.h) is replaced by the iteration count the reference's constructor takes but
//     ignores (`iterations`, 10 at aw_processing_unit.cpp:83);
//   - rand() (drandom, worker.h:22-24) is replaced by a seeded std::mt19937, and the tracker start times
//     (high_resolution_clock) by an iteration counter.
// There is no CPU path: the constructor throws when the engine cannot be created (no gfx950 device).
#pragma once

#include <cstdint>
#include <random>
#include <vector>

#include "awpu_hip_track.h"

namespace awpu_host {

// gradient_ascend.h:19-33
constexpr int kSeekerResetCounter = 128;
constexpr double kSeekerSpreadDeg = 7.0;
constexpr int kTrackerSteps = 5;
constexpr double kTrackerSlowdown = 0.1;
constexpr double kTrackerClosenessDeg = 5.0;
constexpr double kTrackerErrorThreshold = 1.0;
constexpr int kTrackerMax = 10;
constexpr double kTrackerSpreadDeg = 2.0;
constexpr double kParticleRate = 5e-4;

// Target (src/dsp/worker.h:32-64) with the start time as an iteration count.
struct TargetHip {
    double theta, phi;
    float power;        // directionGradient.radius
    float probability;  // 1 / gradientError
    uint64_t start;     // iteration at which the tracker started
};

class SphericalGradientHip {
public:
    // src/dsp/gradient_ascend.cpp:121-133.  xyz [3][n] element positions by stream id (n <= 64 * arrays), index [usable]
    // the active mics (antenna.index); fov in degrees (particles are limited to theta <= fov / 2).
    SphericalGradientHip(int device, const float *xyz, int n, const int32_t *index, int usable, std::size_t swarm_size,
                         std::size_t iterations, float fov, uint32_t seed = 0);
    ~SphericalGradientHip();
    SphericalGradientHip(const SphericalGradientHip &) = delete;
    SphericalGradientHip &operator=(const SphericalGradientHip &) = delete;

    // Worker::loop (worker.h:215-223) calls reset() then update() once per block.  d_frame: the block's snapshot
    // [n_streams][1024] in device memory, or nullptr = the engine's ingest ring.  Returns an awpu_status.
    void reset();                            // gradient_ascend.cpp:289-293
    int update(const float *d_frame);        // gradient_ascend.cpp:295-409
    const std::vector<TargetHip> &targets() const { return tracking_; }  // Worker::getTargets
    awpu_hip_t *engine() { return engine_; }
    double reference() const { return reference_; }

private:
    struct Tracker {
        awpu_particle_t p;
        bool tracking = false;
        uint64_t start = 0;
    };
    double drandom();  // worker.h:22-24 on the seeded generator
    void randomize(awpu_particle_t &p);                    // Particle::random, particle.cpp:11-14
    void jump(awpu_particle_t &p);                         // GradientSeeker::jump, gradient_ascend.cpp:90-93
    void initialize_particles();                           // gradient_ascend.cpp:135-141
    bool is_close(const awpu_particle_t &a, double theta, double phi, double angle) const;

    awpu_hip_t *engine_ = nullptr;
    std::size_t swarm_size_, iterations_;
    double fov_;  // radians, fov / 2 as the reference keeps it
    std::mt19937 rng_;
    std::vector<Tracker> trackers_;
    std::vector<awpu_particle_t> seekers_;
    std::vector<awpu_particle_t> launch_;  // trackers then seekers, the one launch per iteration
    std::vector<TargetHip> tracking_;
    double mean_ = 0.0, reference_ = 0.0;
    int reset_count_ = 0;
    uint64_t clock_ = 0;  // iterations run so far: the tracker start times
};

}  // namespace awpu_host
