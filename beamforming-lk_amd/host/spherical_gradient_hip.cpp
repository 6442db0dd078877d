// spherical_gradient_hip.cpp -- SphericalGradient::update (src/dsp/gradient_ascend.cpp:295-409) with one awpu_hip_track
// launch per iteration.  See spherical_gradient_hip.h for why one mixed launch keeps the reference's order.
#include "spherical_gradient_hip.h"

#include <cmath>
#include <stdexcept>
#include <string>

namespace awpu_host {

namespace {

constexpr double kPi = 3.14159265358979323846;

double to_radians(double degree) { return degree * (kPi / 180.0); }  // geometry.h:18 TO_RADIANS

// normalizeSpherical, particle.h:24-27
void normalize(awpu_particle_t &p, double limit) {
    const double r = std::fmod(p.phi, 2.0 * kPi);
    p.phi = r < 0.0 ? 2.0 * kPi + r : r;
    p.theta = std::max(0.0, std::min(p.theta, limit));
}

void check(int status, const char *what) {
    if (status != AWPU_OK)
        throw std::runtime_error(std::string("SphericalGradientHip: ") + what + ": " + awpu_hip_strerror(status) + " (" +
                                 awpu_hip_last_error() + ")");
}

}  // namespace

SphericalGradientHip::SphericalGradientHip(int device, const float *xyz, int n, const int32_t *index, int usable,
                                           std::size_t swarm_size, std::size_t iterations, float fov, uint32_t seed)
    : swarm_size_(swarm_size), iterations_(iterations), fov_(to_radians(fov / 2.0)), rng_(seed) {
    awpu_hip_cfg cfg;
    awpu_hip_default_cfg(&cfg);
    cfg.device = device;
    cfg.n_streams = n;
    cfg.lut_stride = n;
    cfg.n_pixels = 1;
    check(awpu_hip_create(&engine_, &cfg), "awpu_hip_create (there is no CPU path)");
    try {
        check(awpu_hip_set_antenna(engine_, xyz, n), "awpu_hip_set_antenna");
        check(awpu_hip_set_active_mics(engine_, index, usable), "awpu_hip_set_active_mics");
    } catch (...) {
        awpu_hip_destroy(engine_);
        throw;
    }
    // gradient_ascend.cpp:125-130: the trackers (constructed through Particle, which places them at random) then the swarm
    trackers_.resize(kTrackerMax);
    for (Tracker &t : trackers_) {
        t.p = awpu_particle_t{};
        t.p.spread = to_radians(kTrackerSpreadDeg);
        t.p.rate = kParticleRate * kTrackerSlowdown;
        randomize(t.p);
    }
    initialize_particles();
}

SphericalGradientHip::~SphericalGradientHip() { awpu_hip_destroy(engine_); }

double SphericalGradientHip::drandom() { return static_cast<double>(rng_()) / 4294967296.0; }

void SphericalGradientHip::randomize(awpu_particle_t &p) {
    p.theta = drandom() * fov_;
    p.phi = drandom() * (2.0 * kPi);
}

void SphericalGradientHip::jump(awpu_particle_t &p) {  // Particle::jump(thetaLimit / 2), particle.cpp:16-20
    const double size = fov_ / 2;
    p.theta += (drandom() * 2.0 - 1.0) * size;
    p.phi += (drandom() * 2.0 - 1.0) * size;
    normalize(p, fov_);
}

void SphericalGradientHip::initialize_particles() {
    seekers_.assign(swarm_size_, awpu_particle_t{});
    for (awpu_particle_t &s : seekers_) {
        s.spread = to_radians(kSeekerSpreadDeg);
        s.rate = kParticleRate;
        s.steps = 1;
        randomize(s);
    }
}

bool SphericalGradientHip::is_close(const awpu_particle_t &a, double theta, double phi, double angle) const {
    // Spherical::angle, geometry.cpp:109-118
    const double s1 = std::sin(kPi / 2.0 - a.theta), s2 = std::sin(kPi / 2.0 - theta);
    const double c1 = std::cos(kPi / 2.0 - a.theta), c2 = std::cos(kPi / 2.0 - theta);
    return std::acos(s1 * s2 + c1 * c2 * std::cos(a.phi - phi)) < angle;
}

void SphericalGradientHip::reset() {
    if (reset_count_++ % kSeekerResetCounter == 0) initialize_particles();
}

int SphericalGradientHip::update(const float *d_frame) {
    const double closeness = to_radians(kTrackerClosenessDeg);
    const int T = kTrackerMax, S = static_cast<int>(swarm_size_);
    launch_.resize(T + S);
    double reference = 0.0;  // <= 0: the first launch computes it on the device (gradient_ascend.cpp:301-313)
    for (std::size_t it = 0; it < iterations_; it++, clock_++) {
        double max_power = 0.0, best_theta = 0.0, best_phi = 0.0;
        bool better = false;

        // trackers and seekers in one launch: an idle tracker takes no step (its state is left as it is)
        int n_tracking = 0;
        for (int m = 0; m < T; m++) {
            launch_[m] = trackers_[m].p;
            launch_[m].steps = trackers_[m].tracking ? kTrackerSteps : 0;
            n_tracking += trackers_[m].tracking;
        }
        for (int s = 0; s < S; s++) launch_[T + s] = seekers_[s];
        double used = 0.0;
        const int rc = awpu_hip_track(engine_, d_frame, launch_.data(), T + S, fov_, reference, &used, nullptr);
        if (rc != AWPU_OK) return rc;
        reference = used;
        for (int m = 0; m < T; m++) trackers_[m].p = launch_[m];
        for (int s = 0; s < S; s++) seekers_[s] = launch_[T + s];

        // stop trackers (gradient_ascend.cpp:328-348): of two close ones the later starter stops; operator> on the start
        // times is strict, so of two that started together the second one stops
        for (int m = 0; m < T; m++) {
            if (!trackers_[m].tracking) continue;
            for (int n = m + 1; n < T; n++) {
                if (!trackers_[n].tracking) continue;
                if (is_close(trackers_[m].p, trackers_[n].p.theta, trackers_[n].p.phi, closeness)) {
                    if (trackers_[m].start > trackers_[n].start)
                        trackers_[m].tracking = false;
                    else
                        trackers_[n].tracking = false;
                }
            }
        }

        // seekers (gradient_ascend.cpp:353-383): against the previous block's targets
        float tmp_mean = 0.0f;
        int valid = 0;
        for (awpu_particle_t &seeker : seekers_) {
            bool jumped = false;
            for (const TargetHip &t : tracking_) {
                if (is_close(seeker, t.theta, t.phi, closeness)) {
                    jump(seeker);
                    jumped = true;
                    break;
                }
            }
            if (jumped) continue;
            valid++;
            tmp_mean += seeker.radius;
            if (seeker.radius > max_power && seeker.error < kTrackerErrorThreshold) {
                max_power = seeker.radius;
                best_theta = seeker.theta;
                best_phi = seeker.phi;
                better = true;
            }
        }

        // dispatch (gradient_ascend.cpp:385-393): EVERY idle tracker starts on the same best direction; the next
        // iteration's absorb pass keeps the first of them
        if (better && n_tracking < T) {
            for (Tracker &t : trackers_) {
                if (!t.tracking) {
                    t.p.theta = best_theta;
                    t.p.phi = best_phi;
                    t.tracking = true;
                    t.start = clock_;
                }
            }
        }
        mean_ = tmp_mean / static_cast<double>(valid);
    }
    reference_ = reference;

    // gradient_ascend.cpp:397-408
    tracking_.clear();
    for (Tracker &t : trackers_) {
        if (t.p.radius < mean_ || t.p.radius < reference || t.p.error > kTrackerErrorThreshold) {
            t.tracking = false;
            continue;
        }
        if (t.tracking)
            tracking_.push_back(TargetHip{t.p.theta, t.p.phi, static_cast<float>(t.p.radius), static_cast<float>(1 / t.p.error), t.start});
    }
    return AWPU_OK;
}

}  // namespace awpu_host
