/*
 * awpu_hip_expose.h -- exposure: heatmaps, display images and sources integrated over the last `length` blocks in front of
 * every shown block of a run (awpu_hip_watch.h), the mean of their power rows or their per-pixel maximum, accumulated on the
 * device in a defined order.  One 256-sample block is 5.2 ms of sound; a delay-and-sum map of a noise-like source flickers from
 * block to block and the peaks awpu_hip_find.h reports jitter with it.  `length` is the integration-time knob every acoustic
 * camera has; with the handle's band set (awpu_hip_band.h) the exposed picture is the band's.
 *
 * The reference only sketches this: MIMOWorker::populateHeatmap keeps an unused prevPower = maxV * alpha + (1 - alpha) *
 * prevPower (src/dsp/mimo.cpp:75-76).  Nothing of the reference is replaced.
 *
 * THE RULE.  L = length, 1 <= L <= every: the windows of successive frames never overlap.  Frame j of a call shows block
 * b_j = first + j * every, exactly as awpu_hip_watch_count counts frames, and is exposed over the L blocks b_j - L + 1 .. b_j.
 * p_k is block k's power row as awpu_hip_process_blocks defines it.  For k = 0 .. n_blocks - 1 of the call, in this order, and
 * for every pixel independently:
 *
 *     t = k - first + L - 1;   if (t < 0) skip;      q = t % every;   if (q >= L) skip;      j = t / every;
 *     if (q == 0)  acc = p_k;
 *     else if (mode == AWPU_EXPOSE_MEAN)  acc = acc + p_k;                         // one fp32 add, block order, nothing re-associated
 *     else                                acc = bits(p_k) > bits(acc) ? p_k : acc;  // unsigned 32-bit patterns: awpu_hip_find.h's order
 *     if (q == L - 1)  frame[j] = mode == AWPU_EXPOSE_MEAN ? acc / (float) L : acc; // one fp32 divide, not a reciprocal multiply
 *
 * (On the domain of finite non-negative powers the PEAK order is the maximum.)  Non-finite values propagate by this arithmetic
 * and have no special cases.  Skipped blocks (t < 0 or q >= L) are ingested by the run calls but never swept.
 *   Blocks before the call.  `acc` before block 0 is the caller's `carry` row [n_pixels]; carry_in = max(0, L - 1 - first) blocks
 *     of window 0 lie before the call.
 *   Blocks after the call.   carry_out = max(0, L - 1 - next_first).  When carry_out > 0, carry = acc on return: the open window,
 *     which may include carried-in blocks when the call is shorter than a window.  When carry_out == 0, `carry` is not written.
 *   `carry` may be NULL exactly when carry_in == 0 and carry_out == 0; any other NULL is AWPU_ERR_INVALID before anything is touched.
 * Chaining calls -- each with first = next_first of the one before and the same `carry` buffer -- gives bit for bit the frames of
 * one call over the whole recording.  Start a recording with first = L - 1: a smaller `first` needs a `carry` row, and a zeroed
 * one stands for silent blocks before the recording, so the first frame comes out dim (MEAN divides by L all the same).
 * With length == 1 and MEAN the frames are the watch run's power bits, since p / 1.0f == p.
 *
 * Conventions are those of awpu_hip.h (status codes, host pointers owned by the caller, one thread per handle).
 */
#ifndef AWPU_HIP_EXPOSE_H
#define AWPU_HIP_EXPOSE_H

#include "awpu_hip_find.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AWPU_EXPOSE_MEAN 0
#define AWPU_EXPOSE_PEAK 1

/* How a frame is exposed: 8 bytes.  length in [1, every]; mode AWPU_EXPOSE_MEAN | AWPU_EXPOSE_PEAK.  Anything else:
 * AWPU_ERR_INVALID with nothing written. */
typedef struct awpu_expose {
    int32_t length; /* L: the blocks a frame integrates, the shown block the last of them */
    int32_t mode;
} awpu_expose_t;

/* Pure host arithmetic, no handle.  n_frames and next_first are awpu_hip_watch_count's; carry_in and carry_out as THE RULE
 * defines them; n_swept = the blocks of the call that are not skipped.  n_blocks >= 1, first >= 0, every >= 1, 1 <= length <=
 * every, no null output: AWPU_ERR_INVALID otherwise, nothing written. */
int awpu_hip_expose_count(int32_t n_blocks, int32_t first, int32_t every, int32_t length, int32_t *n_frames, int32_t *next_first,
                          int32_t *carry_in, int32_t *carry_out, int32_t *n_swept);

/* The rule as executable C: pure host code, no handle.  power [n_blocks][n_pixels] (every block's row, skipped ones included)
 * -> frames [n_frames][n_pixels]; carry [n_pixels] in / out as above.  n_pixels >= 1; `frames` may be NULL only when n_frames ==
 * 0.  AWPU_ERR_INVALID otherwise, nothing written. */
int awpu_hip_expose_rows(const float *power, int32_t n_blocks, int32_t n_pixels, int32_t first, int32_t every, const awpu_expose_t *e,
                         float *carry, float *frames);

/* The same on device buffers (d_power, d_carry, d_frames in device memory), enqueued on `stream` (a hipStream_t, NULL = the
 * handle's own; awpu_hip.h, "Streams"); asynchronous, like awpu_hip_find_peaks_device.  Needs no delay table: any power rows will do.  A device-group
 * handle answers from its first device.  One thread owns its pixels through all rows of a window, so the add order is the
 * rule's by construction; no atomics, no cross-lane sums; the same bits as awpu_hip_expose_rows. */
int awpu_hip_expose_rows_device(awpu_hip_t *h, const float *d_power, int32_t n_blocks, int32_t n_pixels, int32_t first, int32_t every,
                                const awpu_expose_t *e, float *d_carry, float *d_frames, void *stream);

/* Exposure in a run of blocks.  The three calls take the arguments of awpu_hip_watch_blocks / _samples / _samples_device plus
 * (e, f, carry) in front of the outputs and (sources, count) behind them.  Each output may be NULL, at least one is not:
 *   image      [n_frames][rows * cols] bytes
 *   big_image  [n_frames][out_rows][out_cols] bytes, x 3 with a colour table
 *   power      [n_frames][pixel_count] floats: the exposed rows
 *   sources    [n_frames][max_sources], count [n_frames]: both or neither; `f` is NULL exactly when they are
 * `carry` [pixel_count] is host memory in the host forms and device memory in the device form, like the outputs.
 *
 * The result is defined by composition.  P = awpu_hip_process_blocks of the same run (all n_blocks rows); frames =
 * awpu_hip_expose_rows(P, n_blocks, pixel_count, w->first, w->every, e, carry, ...).  `power` row j == frames row j, bit for bit
 * in AWPU_MATH_F32_EXACT (in the other modes: the same rule on the rows this run sweeps, which are those of awpu_hip_process on
 * the same snapshots); `image` and `big_image` row j == awpu_hip_heatmap_u8 and the upscale / colour / flip chain of
 * awpu_hip_watch.h on that row; sources and count == awpu_hip_find_peaks of that row (f->rows == w->rows, f->cols == w->cols).
 * The ring afterwards is where n_blocks ingests leave it; awpu_hip_get_stats counts swept blocks.  A call with n_frames == 0 is
 * valid: it ingests, sweeps what its open window holds, and writes only `carry`.
 *
 * Requirements and refusals: those of the watch run, plus THE RULE's.  Device groups are refused like every run.  Argument
 * errors are reported before the handle is touched; on any error the ring, the outputs and `carry` are left as they were.
 *
 * Pipeline and memory.  The swept blocks go through the pieces of every other run, at most cfg.max_batch of them a chunk; the
 * frames that close inside a piece are exposed, shown and searched behind its sweep while its powers are on the device, and only
 * they come back.  The open window lives in one device row of the handle from piece to piece; the host forms upload `carry`
 * before the first piece and download it behind the last.  A piece's history holds only the blocks its swept snapshots read:
 * consecutive blocks where every - length < 3, else length + 3 blocks per window.  Skipped blocks that no snapshot reads never
 * reach the device, except the last four of the call, which the ring needs.  Nothing grows with n_blocks or with every. */
int awpu_hip_expose_blocks(awpu_hip_t *h, const void *datagrams, int32_t stride_bytes, int32_t n_blocks, const awpu_watch_t *w,
                           const awpu_expose_t *e, const awpu_find_t *f, float *carry, uint8_t *image, uint8_t *big_image, float *power,
                           awpu_source_t *sources, int32_t *count);

int awpu_hip_expose_samples(awpu_hip_t *h, const float *samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                            const awpu_expose_t *e, const awpu_find_t *f, float *carry, uint8_t *image, uint8_t *big_image, float *power,
                            awpu_source_t *sources, int32_t *count);

int awpu_hip_expose_samples_device(awpu_hip_t *h, const float *d_samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                                   const awpu_expose_t *e, const awpu_find_t *f, float *d_carry, uint8_t *d_image, uint8_t *d_big_image,
                                   float *d_power, awpu_source_t *d_sources, int32_t *d_count, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AWPU_HIP_EXPOSE_H */
