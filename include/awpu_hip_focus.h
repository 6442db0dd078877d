/*
 * awpu_hip_focus.h -- focus and range: delay tables focused on a point at a finite distance instead of a plane wave, a batched
 * sweep of the beam power over focus distance at given directions (the distance at which it peaks is the source's), and both of
 * them for every shown block of a run of blocks (awpu_hip_find.h) while its history is still on the device.
 *
 * The reference has no counterpart: MIMOWorker::computeDelayLUT (src/dsp/mimo.cpp:20-59) and Particle::steer
 * (src/dsp/particle.cpp:37-49) steer with plane waves, which is right for its 14 cm array from about 1 m outward and wrong for
 * a 64 cm tile of four, whose Fresnel distance at 9 kHz is about 20 m; and it ranges a source with two arrays
 * (src/algorithms/triangulate.cpp).  The rule below extends awpu_hip_steering_delays: same rotations, same precisions, same
 * split, and at distance = +INFINITY the very same function.  The sweeps take their table as input (awpu_hip_set_delay_table,
 * MIMOWorkerHip::setDelayLUT), so a focused table costs the hot path nothing.
 *
 * THE RULE.  Input: element positions xyz [3][n] (fp32), a direction (theta, phi) and a distance in metres.
 *   Rotations. rz = Rz((float) phi) and ry2 = row z of Ry(-(float) theta), their entries rounded to float, exactly as
 *              awpu_hip_steering_delays forms them.  Everything below is in double, products and sums rounded one by one (no
 *              contraction into FMAs), sums taken left to right.
 *   Direction. w[j] = ry2[0] * rz[0][j] + ry2[1] * rz[1][j] + ry2[2] * rz[2][j], j = 0..2: the unit vector for which the
 *              plane-wave delay of element m is (fs / c) * w . p_m.
 *   Focus.     F = distance * w.
 *   Path.      d_m = sqrt((F0 - x_m)^2 + (F1 - y_m)^2 + (F2 - z_m)^2), the correctly rounded square root.
 *   Delay.     far = the maximum of d_m over all n elements; tau_m = (float) ((far - d_m) * (48828.0 / 340.0)).
 *   Split.     frac = (float) modf((double) tau, &whole), off = 256 - (int) whole (src/dsp/mimo.cpp:46-54).
 * So min tau = 0 -- the farthest element is read undelayed, as the plane-wave table reads the last one the wave reaches -- and,
 * by the triangle inequality, tau <= aperture * fs / c: awpu_hip_set_antenna's aperture check keeps every read of a focused
 * table inside samples [0, 513) of a snapshot, as it does for a plane wave.
 * distance = +INFINITY: the plane-wave function is called as it is -- the same bits as awpu_hip_steering_delays,
 * awpu_hip_steer_table and awpu_hip_build_delay_table.  distance <= 0 or NaN: AWPU_ERR_INVALID, nothing written.
 *
 * Conventions are those of awpu_hip.h (status codes, host pointers owned by the caller, one thread per handle).
 */
#ifndef AWPU_HIP_FOCUS_H
#define AWPU_HIP_FOCUS_H

#include "awpu_hip_find.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the rule as executable C: pure host code, no handle.  Null pointers, n < 1 and n_dir < 1: AWPU_ERR_INVALID. ---- */

/* tau [n] of one focus point */
int awpu_hip_focus_delays(const float *xyz, int32_t n, double theta, double phi, double distance, float *tau);

/* awpu_hip_steer_table with a distance per direction: off / frac [n_dir][n] */
int awpu_hip_focus_steer_table(const float *xyz, int32_t n, const double *theta, const double *phi, const double *distance,
                               int32_t n_dir, int32_t *off, float *frac);

/* awpu_hip_build_delay_table with every pixel of the sine-space grid focused at `distance` along its own direction: the grid,
 * the row slices and the refusals are that call's */
int awpu_hip_build_focus_table(const float *xyz, int32_t n, int32_t rows, int32_t columns, float fov_deg, double distance,
                               int32_t row_begin, int32_t row_count, int32_t *off, float *frac);

/* The same with the rows x columns x n part on HIP device `device`, as awpu_hip_build_delay_table_device does it: the per-pixel
 * rotations on the host, the rule's doubles on the device without contraction.  off and frac are the host builder's bits.
 * AWPU_ERR_NO_DEVICE without a gfx950 device; it never falls back to the host builder. */
int awpu_hip_build_focus_table_device(int32_t device, const float *xyz, int32_t n, int32_t rows, int32_t columns, float fov_deg,
                                      double distance, int32_t row_begin, int32_t row_count, int32_t *off, float *frac);

/* ---- ranging ---- */

#define AWPU_RANGE_MAX_CANDIDATES 64

/* One ranged source: 16 bytes. */
typedef struct awpu_range {
    int32_t index;   /* the candidate distance that wins, or -1: unused entry */
    float power;     /* its beam power */
    double distance; /* refined between the candidates, metres; +INFINITY: a plane wave */
} awpu_range_t;

/* The beam power of n_src directions at n_dist candidate focus distances each, in one launch.  The result is defined by
 * composition: power[k][j] is, bit for bit, the power awpu_hip_beams returns for the entry
 * awpu_hip_focus_steer_table(the handle's antenna, theta[k], phi[k], distance[j]) -- the same active mics, and like
 * awpu_hip_beams and awpu_hip_track no gains and RAW samples: a band set on the handle (awpu_hip_band.h) does not apply.
 * d_frame: a snapshot [n_streams][hist] in device memory, or NULL = the ingest ring's.  Needs awpu_hip_set_antenna and
 * awpu_hip_set_active_mics (AWPU_ERR_STATE), hist >= 513 for a d_frame (AWPU_ERR_RANGE); n_src in [1, AWPU_FIND_MAX_SOURCES],
 * n_dist in [1, AWPU_RANGE_MAX_CANDIDATES], finite angles, distances > 0 (+INFINITY allowed): AWPU_ERR_INVALID otherwise, before
 * any work.  power [n_src][n_dist]; best [n_src], or NULL: awpu_hip_range_pick of `power`.  Synchronous, like awpu_hip_track; a
 * device-group handle answers from its first device.  The delays are generated on the device; results leave as plain vector
 * stores, no atomics. */
int awpu_hip_range(awpu_hip_t *h, const float *d_frame, const double *theta, const double *phi, int32_t n_src,
                   const double *distance, int32_t n_dist, float *power, awpu_range_t *best);

/* Which candidate wins, and where between the candidates the power peaks: pure host code, all in double.
 *   Order.      Candidate a BEATS candidate b when bits(power[a]) > bits(power[b]) as unsigned 32-bit patterns, or the bits are
 *               equal and a < b (awpu_hip_find.h's order).  index = the candidate j that beats all others, power = its power.
 *   Refinement. In u = 1 / d with 1 / INFINITY = 0.  For 0 < j < n_dist - 1, with a, b, c the powers at j - 1, j, j + 1:
 *               den = a - 2b + c; delta = den < 0 ? 0.5 * (a - c) / den clamped to [-0.5, 0.5] : 0;
 *               u* = u_j + delta * (u_{j+1} - u_j) for delta >= 0, u_j + delta * (u_j - u_{j-1}) otherwise.
 *               No refinement at j = 0 and j = n_dist - 1: u* = u_j.
 *   Distance.   1 / u*, and +INFINITY when u* <= 0.
 * Domain: finite, non-negative powers (what the sweep writes), where an interior winner always has den < 0.  Outside it the
 * rule applies as written -- a negative power's bits beat every positive one's, den >= 0 leaves the winner unrefined -- and the
 * call stays inside its buffers.
 * power [n_src][n_dist], distance [n_dist] (any order; the refinement means something where 1 / d is monotonic), best [n_src].
 * n_src >= 1, n_dist in [1, AWPU_RANGE_MAX_CANDIDATES], no null pointer, distances > 0: AWPU_ERR_INVALID otherwise. */
int awpu_hip_range_pick(const float *power, int32_t n_src, const double *distance, int32_t n_dist, awpu_range_t *best);

/* ---- locating in a run of blocks: the arguments of awpu_hip_find_blocks / _samples / _samples_device, then the candidates and
 * where the ranges go.  The result is defined by composition: the awpu_hip_find_* call of the same form; then, for every shown
 * block, awpu_hip_range on that block's RAW snapshot at the theta / phi the run itself reports for its `count` sources:
 * ranges [n_frames][f->max_sources], range_power [n_frames][f->max_sources][n_dist] or NULL.  Unused source entries get
 * index = -1 and zeros (their range_power rows too).  Needs what awpu_hip_range needs besides the find run's requirements; the
 * refusals, the ring, `next_first` and mixing with the other run calls are exactly the find run's.  The range pass runs behind
 * each piece's peak pass while the piece's history is on the device; the device form takes its directions from d_sources on
 * the same stream and writes d_ranges / d_range_power in place (`stream`: awpu_hip.h, "Streams"). */
int awpu_hip_locate_blocks(awpu_hip_t *h, const void *datagrams, int32_t stride_bytes, int32_t n_blocks, const awpu_watch_t *w,
                           const awpu_find_t *f, awpu_source_t *sources, int32_t *count, float *power, const double *distance,
                           int32_t n_dist, awpu_range_t *ranges, float *range_power);

int awpu_hip_locate_samples(awpu_hip_t *h, const float *samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                            const awpu_find_t *f, awpu_source_t *sources, int32_t *count, float *power, const double *distance,
                            int32_t n_dist, awpu_range_t *ranges, float *range_power);

int awpu_hip_locate_samples_device(awpu_hip_t *h, const float *d_samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                                   const awpu_find_t *f, awpu_source_t *d_sources, int32_t *d_count, float *d_power,
                                   const double *distance, int32_t n_dist, awpu_range_t *d_ranges, float *d_range_power,
                                   void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AWPU_HIP_FOCUS_H */
