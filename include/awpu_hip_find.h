/*
 * awpu_hip_find.h -- finding sources: the strongest local maxima of a heatmap, refined to a fraction of a pixel and turned into
 * directions, on the host, on the device, and for every shown block of a run of blocks (awpu_hip_watch.h) while its powers are
 * still on the device.  What comes back is a few hundred bytes per frame instead of the frame.
 *
 * The reference has no counterpart: its MIMO worker tracks nothing, and its only source finder is the per-block gradient loop
 * (awpu_hip_track.h).  The directions use the sine-space grid of MIMOWorker::computeDelayLUT (src/dsp/mimo.cpp:21-43) as
 * awpu_hip_build_delay_table evaluates it, so theta / phi of a source can be handed to awpu_hip_steering_delays, to
 * awpu_hip_steer_table or to the listeners of awpu_hip_listen.h as they are.
 *
 * THE RULE.  Input: one power row p[rows * cols] of fp32 values, row-major, pixel i = r * cols + c -- the order
 * awpu_hip_build_delay_table emits.  Domain: every bit pattern.  The sweeps write exact 0, subnormals, +inf and NaN besides
 * ordinary powers (a frame whose squares overflow, a frame holding a bad sample), and the run forms below hand those rows
 * straight to the peak pass: the rule applies to them as written, no loop's trip count depends on the data, and the host and
 * the device results are equal on all of them.
 *   Order.     Pixel a BEATS pixel b when bits(p[a]) > bits(p[b]) as unsigned 32-bit patterns, or the bits are equal and a < b.
 *              On finite, non-negative powers: larger power, then lower index; +inf beats them, a NaN beats +inf, and any
 *              pattern with the sign bit set (-0.0 included) beats all of those.  The order is total: no result depends on
 *              scheduling.
 *   Maximum.   m = the power of the pixel that beats all others of the frame.
 *   Peak.      Pixel (r, c) is a peak when it beats every other pixel (r', c') of the grid with |r' - r| <= radius and
 *              |c' - c| <= radius, and p > 0, and p >= min_power, and p >= floor_ratio, where floor_ratio = 0 when
 *              min_ratio == 0 -- no ratio threshold, whatever m is -- and min_ratio * m (one fp32 multiply) otherwise.
 *   Report.    The min(max_sources, number of peaks) peaks that beat the others, strongest first; `count` = how many.  The unused
 *              ones of a frame's max_sources entries hold pixel = -1 and zeros elsewhere.
 *   Refinement (all in double).  For 0 < r < rows - 1, with a, b, c the powers at rows r - 1, r, r + 1 of column c:
 *              den = a - 2b + c, d_row = den < 0 ? 0.5 * (a - c) / den : 0, clamped to [-0.5, 0.5] (a peak beats its
 *              4-neighbours, so |d_row| <= 0.5 already); d_row = 0 on the border rows.  The column axis likewise.
 *              row = r + d_row, col = c + d_col.
 *   Direction. With fov = fov_deg * (pi / 180), sep_rows = sin(fov / 2) / (rows / 2.0), sep_cols likewise:
 *              y = row * sep_rows - rows * sep_rows / 2 + sep_rows / 2, x from col likewise,
 *              theta = asin(min(sqrt(x * x + y * y), 1)), phi = atan2(y, x) of the unnormalised pair (the reference's x /= norm is
 *              0 / 0 at the centre of an odd grid; that pixel gets phi = 0).
 * So a constant positive frame -- a constant +inf frame too, at every min_ratio -- has exactly one peak, pixel 0, and an
 * all-zero frame has none.  Two consequences off the finite powers: a NaN pixel is never a peak (p > 0 is false) and beats its
 * whole window, so no pixel within `radius` of it is a peak either; and with min_ratio > 0 a frame holding a NaN has no sources
 * at all (m is that NaN, and so is floor_ratio; only a finite pixel with the sign bit set, which no sweep writes, beats a
 * positive NaN and takes its place as m).  With min_ratio == 0 the peaks away from the NaN are reported as usual.
 *
 * pixel, power, count, row and col are the same bits from the host and the device entry points; theta and phi may differ in
 * their last bits (asin and atan2 of two maths libraries).
 *
 * Conventions are those of awpu_hip.h (status codes, host pointers owned by the caller, one thread per handle).
 */
#ifndef AWPU_HIP_FIND_H
#define AWPU_HIP_FIND_H

#include "awpu_hip_watch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AWPU_FIND_MAX_RADIUS 8
#define AWPU_FIND_MAX_SOURCES 32
#define AWPU_FIND_MAX_PIXELS 262144 /* rows * cols, e.g. 512 x 512: one workgroup keeps a frame's peak flags, a bit a pixel, in 32 KB of LDS */

/* What is a source.  radius in [1, 8]; max_sources in [1, 32]; min_power >= 0 and min_ratio in [0, 1], both finite; fov_deg in
 * (0, 180]; rows, cols >= 1 and rows * cols <= AWPU_FIND_MAX_PIXELS.  Anything else: AWPU_ERR_INVALID before any work. */
typedef struct awpu_find {
    int32_t rows, cols;          /* the grid of a power row */
    int32_t radius;              /* a peak beats the (2 * radius + 1)^2 window around it */
    int32_t max_sources;         /* entries per frame */
    float min_power, min_ratio;  /* p >= min_power and p >= min_ratio * (the frame's maximum) */
    float fov_deg;               /* the fov_deg the delay table was built with */
} awpu_find_t;

/* One source: 40 bytes. */
typedef struct awpu_source {
    int32_t pixel;      /* r * cols + c of the peak, or -1: unused entry */
    float power;        /* p[pixel] */
    double row, col;    /* refined position, within half a pixel of (r, c) */
    double theta, phi;  /* its direction, radians */
} awpu_source_t;

/* The rule as executable C: pure host code, no handle.  power [n_frames][rows * cols] -> sources [n_frames][max_sources],
 * count [n_frames].  n_frames >= 1 and no null pointer: AWPU_ERR_INVALID otherwise, nothing written. */
int awpu_hip_find_peaks(const float *power, int32_t n_frames, const awpu_find_t *f, awpu_source_t *sources, int32_t *count);

/* The same on device buffers (d_power, d_sources, d_count in device memory), one workgroup per frame, enqueued on `stream` (a
 * hipStream_t, NULL = the handle's own; awpu_hip.h, "Streams"); asynchronous, like awpu_hip_heatmap_u8_device.  Needs no delay table: any power rows
 * will do, those of awpu_hip_process_device straight after it on the same stream for instance.  A device-group handle answers
 * from its first device.  Reads every frame (2 * radius + 1)^2 + max_sources times out of the cache; writes with plain vector
 * stores, no atomics. */
int awpu_hip_find_peaks_device(awpu_hip_t *h, const float *d_power, int32_t n_frames, const awpu_find_t *f, awpu_source_t *d_sources,
                               int32_t *d_count, void *stream);

/* Finding in a run of blocks.  The three calls take the arguments of awpu_hip_watch_blocks / _samples / _samples_device with
 * (image, big_image) replaced by (f, sources, count); of `w` they read first, every, rows and cols and ignore the rest;
 * f->rows == w->rows and f->cols == w->cols (AWPU_ERR_INVALID otherwise); `power` may be NULL.  every = 1 finds in every block.
 *
 * The result is defined by composition: the awpu_hip_watch_* call of the same form asked for `power` only, then
 * awpu_hip_find_peaks of each shown row: sources [n_frames][max_sources], count [n_frames], n_frames as awpu_hip_watch_count
 * gives it.  The ring, the stats, the requirements and refusals, splitting a recording with `next_first` and mixing with the
 * other run calls are therefore exactly the watch run's.  The peak pass runs behind each piece's sweep while its powers are on
 * the device; the host forms bring sources and count back through pinned memory with the piece's other results (the powers
 * only when `power` is asked for); the device form writes d_sources and d_count in place and brings nothing back. */
int awpu_hip_find_blocks(awpu_hip_t *h, const void *datagrams, int32_t stride_bytes, int32_t n_blocks, const awpu_watch_t *w,
                         const awpu_find_t *f, awpu_source_t *sources, int32_t *count, float *power);

int awpu_hip_find_samples(awpu_hip_t *h, const float *samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                          const awpu_find_t *f, awpu_source_t *sources, int32_t *count, float *power);

int awpu_hip_find_samples_device(awpu_hip_t *h, const float *d_samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                                 const awpu_find_t *f, awpu_source_t *d_sources, int32_t *d_count, float *d_power, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AWPU_HIP_FIND_H */
