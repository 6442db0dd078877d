/*
 * awpu_hip_track.h -- particle tracking on the device: the steering, the four monopulse beams and the
 * gradient step of the reference's --tracking and --miso modes, fused into one launch.
 *
 * Replaces (file:line relative to the reference tree):
 *   GradientParticle::step      src/dsp/gradient_ascend.cpp:30-81  (quadrant monopulse, RELATIVE 1)
 *   Spherical::quadrant         src/geometry/geometry.cpp:120-142, :181-216
 *   Particle::steer / beam / das / step   src/dsp/particle.cpp:22-27, :37-103
 *   normalizeSpherical          src/dsp/particle.h:24-27, src/geometry/geometry.cpp:7-20
 *   the block's reference power src/dsp/gradient_ascend.cpp:301-313, src/dsp/miso.cpp:31-38
 *
 * The reference steps one particle at a time, and every step of a particle depends on the one before, so a
 * batch of host calls (awpu_hip_steer_table + awpu_hip_beams) costs one round trip per step.  Here the
 * directions stay on the device and one launch advances every particle by its own number of steps
 * ("Trackers", shows SphericalGradient::update and MISOWorker::update on top of it).
 *
 * Conventions are those of awpu_hip.h (status codes, host pointers owned by the caller, one thread per handle).
 * A device-group handle answers from its first device, as awpu_hip_beams does.
 */
#ifndef AWPU_HIP_TRACK_H
#define AWPU_HIP_TRACK_H

#include "awpu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One particle (GradientParticle, src/dsp/gradient_ascend.h:26-58).  80 bytes. */
typedef struct awpu_particle {
    double theta, phi;                   /* directionCurrent: in, out */
    double spread, rate;                 /* monopulse spread (rad) and step size: in */
    int32_t steps;                       /* steps this call (0 = untouched): in */
    float error;                         /* gradientError after the last step: out */
    double grad_theta, grad_phi, radius; /* directionGradient after the last step: out */
    float power[4];                      /* q1..q4 (the beam powers) of the last step: out */
} awpu_particle_t;

/* The element positions the particles steer with: xyz[3][n] by stream id (as from awpu_hip_create_antenna /
 * awpu_hip_create_tiled_antenna), n <= cfg.lut_stride.  Delays are taken over all n elements, as the
 * reference's steering_vector_spherical does (src/geometry/antenna.cpp:126-129).  AWPU_ERR_RANGE when the
 * geometry's aperture exceeds 256 samples: then every table a direction can form reads inside
 * [0, 2 * 256] of a snapshot and the kernels need no per-entry checks. */
int awpu_hip_set_antenna(awpu_hip_t *h, const float *xyz, int32_t n);

/* awpu_hip_steer_table for the handle's antenna, computed on the device: off/frac [n_dir][n], bit-identical
 * to the host function (the same fp32 products without contraction, the same float rounding of the angles'
 * cosines and sines).  Synchronous. */
int awpu_hip_steer_table_device(awpu_hip_t *h, const double *theta, const double *phi, int32_t n_dir, int32_t *off,
                                float *frac);

/* Advances particle k by p[k].steps gradient steps (GradientParticle::step with RELATIVE 1), every particle in
 * the same launch; the outputs of p[k] are those after its last step.  A particle whose theta + spread exceeds
 * pi/2 moves its own theta down by spread / 2 before a step, as Spherical::quadrant does.
 *   d_frame       one snapshot [n_streams][hist] in device memory (hist >= 513), or NULL = the ingest ring's
 *   theta_limit   the particles' thetaLimit: neighbours and steps are clipped to [0, theta_limit].  It is the
 *                 caller's value as is: SphericalGradient passes fov/2 in radians, while MISOWorker sets its
 *                 beamformer's thetaLimit to its fov in DEGREES (src/dsp/miso.cpp:6), so in that mode theta is
 *                 never clipped -- pass the same number to reproduce it.
 *   reference     the block's reference power the gradient is divided by; <= 0: computed on the device from
 *                 stream 0's zero-delay window (sum over i = 1..254 of MA^2 / 254, fp32 in sample order)
 *   reference_used  (may be NULL) the value used
 *   beams         (may be NULL) [n][256]: Particle::das at every particle's final direction (MISO's audio block)
 * Needs awpu_hip_set_antenna and awpu_hip_set_active_mics.  Synchronous: one upload of p, one launch, one
 * read-back. */
int awpu_hip_track(awpu_hip_t *h, const float *d_frame, awpu_particle_t *p, int32_t n, double theta_limit,
                   double reference, double *reference_used, float *beams);

#ifdef __cplusplus
}
#endif

#endif /* AWPU_HIP_TRACK_H */
