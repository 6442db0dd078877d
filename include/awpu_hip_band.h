/*
 * awpu_hip_band.h -- band-limited heatmaps: a per-handle FIR band in front of every sweep.  "Show me 6.4 - 9 kHz" is how an
 * acoustic camera separates a weak high-frequency source from strong low-frequency noise.
 *
 * The reference anticipates it and does not build it: math_toolbox/filter_produce.m designs fir1(..., 'bandpass') filters for
 * 1950-3541, 3541-6375 and 6375-9000 Hz at 48 828.125 Hz, and src/dsp/particle.h:17 carries USE_BANDPASS.
 *
 * Delay-and-sum is linear: filtering every mic in front of the sweep is filtering the beam.  So a band changes nothing about a
 * sweep but its input, and what a call returns with a band is DEFINED BY COMPOSITION: bit for bit what the same call on a
 * band-less handle of the same configuration (table, active mics, gains, math mode, interpolation, FIR table, max_batch)
 * returns on input that awpu_hip_band_filter has filtered with the handle's coefficients -- every stream's snapshot row of
 * cfg.hist samples, or the recording for the runs of blocks (a fresh handle's ring is zeros, and a filtered zero history is zero).
 *
 *   Follow the band:  awpu_hip_process, _process_async + _wait, _process_device, _process_device_sums, _process_ring; the
 *                     heatmap side of the runs -- `power` of awpu_hip_process_* / _listen_* / _watch_*, `image` / `big_image` of
 *                     awpu_hip_watch_*, `sources` / `count` / `power` of awpu_hip_find_blocks / _samples / _samples_device.
 *                     Per-mic gains stay where they are, behind the filter.
 *   Read raw samples, as without a band:  awpu_hip_beams, awpu_hip_track, awpu_hip_steer_table*, `audio` and `trail` of the
 *                     listen calls, awpu_hip_range and `ranges` / `range_power` of awpu_hip_locate_* (awpu_hip_focus.h),
 *                     awpu_hip_calibrate_*, awpu_hip_ring_snapshot, awpu_hip_ingest_block, the ring's content.
 *   Refused while a band is set (AWPU_ERR_STATE, nothing enqueued, handle and ring untouched):  awpu_hip_live_block (its
 *                     captured step), awpu_hip_pack_frames / _process_packed / _packed_bytes (the exchange format stays raw).
 *
 * History.  A window sample at position t reads x[t - taps + 1 .. t]; the sweeps read the window from `lo` on, the smallest `off`
 * of the table over all pixels and active mics.  With taps - 1 > lo a snapshot does not hold the history the band needs:
 * AWPU_ERR_RANGE, from awpu_hip_set_band where a table and a mic list are set already, else from the call that would sweep,
 * before anything is enqueued.
 *
 * Value edges follow from the rule: a non-finite sample reaches the `taps` outputs behind it in its own row and frame, and
 * nothing else.
 *
 * Conventions are those of awpu_hip.h (status codes, host pointers owned by the caller, one thread per handle).
 */
#ifndef AWPU_HIP_BAND_H
#define AWPU_HIP_BAND_H

#include "awpu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AWPU_BAND_MAX_TAPS 128

/* THE RULE.  y[t] = the fp32 value of: acc = +0; for k = 0 .. taps-1 in this order: acc = fmaf(c[k], x[t-k], acc); with
 * x[t] = +0 for t < 0.  One rounding per step, no contraction beyond the fmaf, no re-ordering.  Pure host code, no handle:
 * x, y [n_rows][pitch] floats, the first n of every row filtered; y may not alias x.  taps in [1, AWPU_BAND_MAX_TAPS], every
 * c[k] finite, n_rows >= 1, 1 <= n <= pitch: AWPU_ERR_INVALID otherwise, nothing written. */
int awpu_hip_band_filter(const float *x, int32_t n_rows, int64_t pitch, int32_t n, const float *c, int32_t taps, float *y);

/* A linear-phase band by the window method (what fir1 does by default), all in double, rounded to float at the end:
 * taps odd in [3, 127]; 0 <= lo_hz < hi_hz <= sample_rate / 2; M = (taps-1)/2; f1 = lo/fs, f2 = hi/fs;
 * ideal[k] = 2 f2 sinc(2 f2 (k-M)) - 2 f1 sinc(2 f1 (k-M)), sinc(u) = sin(pi u)/(pi u), 1 at u = 0;
 * w[k] = 0.54 - 0.46 cos(2 pi k / (taps-1));  g = | sum_k ideal[k] w[k] exp(-2 pi i k (f1+f2)/2) |;
 * c[k] = (float)(ideal[k] w[k] / g).  lo = 0 gives a low-pass, hi = fs/2 a high-pass.  AWPU_ERR_INVALID otherwise, nothing
 * written. */
int awpu_hip_band_design(double lo_hz, double hi_hz, double sample_rate, int32_t taps, float *c);

/* The handle's band: c [taps] is copied.  taps in [1, AWPU_BAND_MAX_TAPS] with every c[k] finite (AWPU_ERR_INVALID otherwise).
 * c == NULL with taps == 0 clears it.  AWPU_ERR_RANGE where the table and mic list already set leave the band too little
 * history (see above); AWPU_ERR_STATE on a device-group handle and while an awpu_hip_process_async call is in flight.  A
 * refused call leaves the handle's band as it was. */
int awpu_hip_set_band(awpu_hip_t *h, const float *c, int32_t taps);

#ifdef __cplusplus
}
#endif

#endif /* AWPU_HIP_BAND_H */
