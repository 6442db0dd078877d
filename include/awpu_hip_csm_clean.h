/*
 * awpu_hip_csm_clean.h -- step 7 of awpu_hip_csm.h: CLEAN-SC (Sijtsma 2007), deconvolution of the conventional cross-spectral
 * map, per bin and on the device.  awpu_hip_csm.h states steps 1 to 6a and includes this header; include that one.  The
 * conventional plane is a dirty map: every source carries the array's beam pattern, and a weaker source of the same bin sits
 * among the stronger one's side lobes.  CLEAN-SC maps the matrix, takes the strongest pixel, forms the part of the matrix that is
 * coherent with that pixel's beam and subtracts it, and maps again.  It needs no point-spread model, takes a source's side lobes
 * out wherever they fall -- they are coherent with the peak --, and leaves incoherent self-noise in the residual.  Its output is,
 * per bin, a list of source pixels with their powers.  It is to the cross-spectral path what awpu_hip_peel.h is to the sweep.  The
 * reference has nothing like it; nothing of it is replaced.
 *
 * THE RULE (step 7).  Plain fp32 with one arithmetic, independent of cfg.math; every fused operation is a written-out fmaf and
 * nothing else is contracted (csrc/csm_clean_rule.h is the rule as code).  c->kind must be AWPU_CSM_CONVENTIONAL.  The rule runs
 * per bin k, independently of every other bin, on a working matrix D [usable][usable]:
 *
 *   Load.  D is C as the rule reads it: the entries b < a as they are, the diagonal as (re, +0), and D[b][a] written as the exact
 *          conjugate (re, -im) of D[a][b].  The caller's upper triangle and the diagonal's imaginary parts are never read.
 *   For i = 0 .. steps-1:
 *     Dirty row.  P_i = steps 3 to 5 (conventional) of D with the call's block count.
 *     Pick.       Peel's pick (awpu_hip_peel.h): among pixels with a finite power > 0 the greatest by awpu_hip_find.h's order
 *                 (power bits, then the lower index).  None: the bin is done.  i == 0: first = P_0[pick].
 *                 P_i[pick] < (stop_ratio == 0 ? 0 : stop_ratio * first): the bin is done.
 *     Component.  s = step 3's steering entries of the picked pixel, e_b = conj(s_b), v = D e:
 *                     v_a = the sum over ALL b = 0 .. usable-1, ascending, from +0, of D[a][b] e_b, each term step 4's four fmaf:
 *                         v.re = fmaf(D.re, s_b.re, v.re);  v.re = fmaf(D.im, s_b.im, v.re);
 *                         v.im = fmaf(D.im, s_b.re, v.im);  v.im = fmaf(-D.re, s_b.im, v.im)
 *                     with D[a][a] taken as (re, +0) and D[a][b], b > a, as the exact conjugate of D[b][a]
 *                     qs = the sum over a ascending, from +0:   qs = fmaf(s_a.re, v_a.re, qs);   qs = fmaf(-s_a.im, v_a.im, qs)
 *                 (qs = e^H D e.)  !(qs > 0), or qs not finite: the bin is done and no step is recorded.  Otherwise
 *                     r = gain / qs                                                                              (one division)
 *     Update.     D = D - gain * v v^H / qs.  For every b <= a:
 *                     t = (v_a.re * r, v_a.im * r)                                                      (two rounded products)
 *                     D.re = fmaf(-t.re, v_b.re, D.re);   D.re = fmaf(-t.im, v_b.im, D.re)
 *                     b < a also:   D.im = fmaf(-t.im, v_b.re, D.im);   D.im = fmaf(t.re, v_b.im, D.im)
 *                 the diagonal's im stays +0, and D[b][a] is written as the exact conjugate.
 *     Record.     step[i] = {pixel = pick, before = P_i[pick], removed = gain * before}                           (one product)
 *   After the loop.  A done bin is no longer modified; unused steps are {-1, 0, 0}.  residual = the dirty row of the bin's final D
 *   (one more map closes the loop); clean[p] = the `removed` of the steps at p, added in step order from +0; map = clean + residual,
 *   one add.
 *
 * In exact arithmetic a step takes the picked pixel's power from q to (1 - gain) q; the rule promises no more than its operations
 * give.  Every entry's sum is serial in ascending b; the device spreads entries, rows and bins over its threads, so the bits do
 * not depend on the launch shape (the statement step 6a makes).  Non-finite values take the rule as written: host and device agree
 * on WHERE a NaN is, not on its sign and payload; a bin with no finite pick is done at once; no bin reaches another bin.
 *   With the diagonal kept, a weak source reads high by the diagonal's noise floor (about 2 dB at self-noise of 0.5 .. 2 rms of the
 * strong source, 15 dB down).  CLEAN-SC on a diagonal-removed matrix needs a fixed-point iteration for its component and is not
 * taken here: kinds 1 and 2 are AWPU_ERR_INVALID in these calls.  Clean entries are points, as in awpu_hip_peel.h.
 *
 * Conventions are those of awpu_hip.h (status codes, host pointers owned by the caller, one thread per handle).
 */
#ifndef AWPU_HIP_CSM_CLEAN_H
#define AWPU_HIP_CSM_CLEAN_H

#include "awpu_hip_csm.h"
#include "awpu_hip_csm_watch.h" /* the runs' arguments */

#ifdef __cplusplus
extern "C" {
#endif

#define AWPU_CSM_CLEAN_MAX_STEPS 32
#define AWPU_CSM_CLEAN_MAP 0      /* what a CLEAN-SC run shows: clean + residual, */
#define AWPU_CSM_CLEAN_CLEAN 1    /* the removed powers at their pixels, */
#define AWPU_CSM_CLEAN_RESIDUAL 2 /* the last map */

/* The loop's parameters: 12 bytes.  Outside their ranges: AWPU_ERR_INVALID with nothing written, before a handle is touched. */
typedef struct awpu_csm_clean {
    int32_t steps;    /* [1, AWPU_CSM_CLEAN_MAX_STEPS] */
    float gain;       /* (0, 1] */
    float stop_ratio; /* [0, 1) */
} awpu_csm_clean_t;

/* One step of one bin: 12 bytes.  Unused: {-1, 0, 0}. */
typedef struct awpu_csm_clean_step {
    int32_t pixel;
    float before;
    float removed;
} awpu_csm_clean_step_t;

/* One step as executable C: pure host code, no handle.  matrix [n_bins][usable][usable][2] is updated in place: every bin gets the
 * load's form (the conjugate upper triangle, the diagonal's +0 -- which changes nothing in a matrix the load or a step wrote); a
 * bin whose pixel [n_bins] lies in [0, n_pixels) then gets the component and, where qs passes its test, the update.  Any other
 * pixel (-1) leaves the bin at that.  component [n_bins][usable][2] (v) and qs [n_bins], each or NULL; a skipped bin's rows are
 * zeroed.  Refusals follow awpu_hip_csm_map_host (a null matrix or pixel, a bad c or table, usable < 1), plus a kind other than
 * AWPU_CSM_CONVENTIONAL and a gain outside (0, 1]: AWPU_ERR_INVALID, nothing written. */
int awpu_hip_csm_clean_step_host(float *matrix, const int32_t *pixel, float gain, const int32_t *off, const float *frac, int32_t lut_stride,
                                 int32_t n_pixels, const int32_t *index, int32_t usable, const awpu_csm_t *c, float *component, float *qs);

/* The loop as executable C: pure host code, no handle; `matrix` is not written.  Each output may be NULL, not all of them: steps
 * [n_bins][cl->steps]; clean, residual, map [n_bins][n_pixels]; residual_matrix [n_bins][usable][usable][2] (the final D).
 * Refusals as above, plus a bad cl and a block count below 1. */
int awpu_hip_csm_clean_host(const float *matrix, int32_t block_count, const int32_t *off, const float *frac, int32_t lut_stride,
                            int32_t n_pixels, const int32_t *index, int32_t usable, const awpu_csm_t *c, const awpu_csm_clean_t *cl,
                            awpu_csm_clean_step_t *steps, float *clean, float *residual, float *map, float *residual_matrix);

/* The handle forms use the handle's delay table and active mics.  Their state refusals are those of the cross-spectral calls
 * (AWPU_INTERP_FIR8, a band, a device group, a call while awpu_hip_process_async is in flight: AWPU_ERR_STATE), and a slab handle
 * (pixel_count < n_pixels) is refused with AWPU_ERR_STATE too: the pick needs the whole map.  More active mics than the map takes
 * (2048): AWPU_ERR_RANGE.  They leave awpu_hip_stats' kernel_variant alone.  The working matrix, v, the bins' bookkeeping and the
 * dirty planes are buffers of the handle's, allocated at the first call and again at a call with more mics or bins: allocation
 * waits for the device and happens before the call enqueues anything.  Make the first call outside a stream capture; every
 * later one of that size enqueues and returns.
 *
 * One step on device buffers: d_matrix [n_bins][usable][usable][2] updated in place as awpu_hip_csm_clean_step_host updates it;
 * d_pixel [n_bins] device memory (what it holds is not checked: the kernel skips a bin whose pixel is outside the table);
 * d_component [n_bins][usable][2] and d_qs [n_bins], each or NULL.  Enqueued on `stream` (a hipStream_t, NULL = the handle's own);
 * asynchronous.  *c is read before the call returns. */
int awpu_hip_csm_clean_step_device(awpu_hip_t *h, float *d_matrix, const int32_t *d_pixel, const awpu_csm_t *c, float gain,
                                   float *d_component, float *d_qs, void *stream);

/* The loop.  The result is defined by composition: it equals, bit for bit, what a caller gets by driving awpu_hip_csm_map_device,
 * the pick and awpu_hip_csm_clean_step_device by hand -- and every one of those equals the host rule bit for bit, so the loop
 * equals awpu_hip_csm_clean_host with no tolerance involved.
 *
 * awpu_hip_csm_clean: a host matrix and host outputs as awpu_hip_csm_clean_host takes them, each or NULL, not all; synchronous. */
int awpu_hip_csm_clean(awpu_hip_t *h, const float *matrix, int32_t block_count, const awpu_csm_t *c, const awpu_csm_clean_t *cl,
                       awpu_csm_clean_step_t *steps, float *clean, float *residual, float *map, float *residual_matrix);

/* ... on device buffers, enqueued on `stream`; asynchronous, and nothing inside the loop waits on the host: the picks, the stop
 * tests, `first`, the done flags and the steps' records stay on the device.  d_matrix is not written; the working D is
 * d_residual_matrix where that is given (it must not overlap d_matrix: AWPU_ERR_INVALID), else a buffer of the handle's. */
int awpu_hip_csm_clean_device(awpu_hip_t *h, const float *d_matrix, int32_t block_count, const awpu_csm_t *c, const awpu_csm_clean_t *cl,
                              awpu_csm_clean_step_t *d_steps, float *d_clean, float *d_residual, float *d_map, float *d_residual_matrix,
                              void *stream);

/* CLEAN-SC in a run of blocks.  The three calls take the arguments of awpu_hip_csm_watch_blocks / _samples / _samples_device
 * (awpu_hip_csm_watch.h) with (cl, what) in front of the outputs, steps [n_frames][n_bins][cl->steps] (or NULL) behind them and no
 * `solved`; at least one output is given.
 *
 * The result is defined by composition.  A frame's matrix and block count are the watch run's (length, carry, *carried, the
 * ring: awpu_hip_csm_watch.h); its planes [n_bins][pixel_count] are the map (what == AWPU_CSM_CLEAN_MAP), the clean
 * (AWPU_CSM_CLEAN_CLEAN) or the residual (AWPU_CSM_CLEAN_RESIDUAL) rows, and its steps the steps, that awpu_hip_csm_clean gives
 * for that matrix; the shown row is the plane of bin index `show`, or with AWPU_CSM_SHOW_SUM the planes added in ascending bin
 * order, and goes through the display step of every run.  So frame j equals, bit for bit, awpu_hip_csm_accumulate_host over the
 * window from zeros -> awpu_hip_csm_clean_host -> the shown row -> awpu_hip_heatmap_u8 / awpu_hip_find_peaks.
 *   Refusals: the watch run's, in its order, with a bad cl, a `what` outside the three above and a kind other than
 * AWPU_CSM_CONVENTIONAL behind those of `carried` (AWPU_ERR_INVALID, before the handle is touched), and a slab handle among the
 * state refusals (AWPU_ERR_STATE).  The loop's buffers are the handle's, as above: make the first call outside a stream capture. */
int awpu_hip_csm_clean_blocks(awpu_hip_t *h, const void *datagrams, int32_t stride_bytes, int32_t n_blocks, const awpu_watch_t *w,
                              const awpu_csm_t *c, int32_t length, int32_t show, const awpu_find_t *f, float *carry, int32_t *carried,
                              const awpu_csm_clean_t *cl, int32_t what, uint8_t *image, uint8_t *big_image, float *power, awpu_source_t *sources,
                              int32_t *count, float *planes, awpu_csm_clean_step_t *steps);

int awpu_hip_csm_clean_samples(awpu_hip_t *h, const float *samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                               const awpu_csm_t *c, int32_t length, int32_t show, const awpu_find_t *f, float *carry, int32_t *carried,
                               const awpu_csm_clean_t *cl, int32_t what, uint8_t *image, uint8_t *big_image, float *power, awpu_source_t *sources,
                               int32_t *count, float *planes, awpu_csm_clean_step_t *steps);

int awpu_hip_csm_clean_samples_device(awpu_hip_t *h, const float *d_samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                                      const awpu_csm_t *c, int32_t length, int32_t show, const awpu_find_t *f, float *d_carry,
                                      int32_t *carried, const awpu_csm_clean_t *cl, int32_t what, uint8_t *d_image, uint8_t *d_big_image,
                                      float *d_power, awpu_source_t *d_sources, int32_t *d_count, float *d_planes,
                                      awpu_csm_clean_step_t *d_steps, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AWPU_HIP_CSM_CLEAN_H */
