/*
 * awpu_hip_csm_watch.h -- cross-spectral runs: a map per shown block of a recording, with display images and found sources, as
 * the tone runs (awpu_hip_tones.h) give them for the tone sweep.  awpu_hip_csm.h states the arithmetic and includes this header;
 * include that one.
 *
 * THE RULE.  With n_frames and next_first as awpu_hip_watch_count gives them, frame j shows block t = first + j * every of the
 * call.  Its matrix is what steps 1 and 2 of awpu_hip_csm.h add, from zeros and in block order, out of the blocks
 * max(t - length + 1, start of the recording) .. t, and its block count is the number of those blocks.  Windows may overlap:
 * `length` is independent of `every`.  (Every frame's matrix is added up from zeros: a sliding update that subtracts the block
 * leaving the window would not give these bits.)  For AWPU_CSM_CAPON the matrix goes through step 6a; steps 3 to 5 give the
 * frame's planes [n_bins][pixel_count].  The shown row is the plane of bin index `show` in [0, n_bins), or with
 * AWPU_CSM_SHOW_SUM the planes added in ascending bin order with plain additions from +0.  The shown row goes through the display
 * step of every run: `power` row j is it, `image` row j == awpu_hip_heatmap_u8 of it, `big_image` the upscale of that, `sources` /
 * `count` awpu_hip_find_peaks of it.  So frame j equals, bit for bit, awpu_hip_csm_accumulate_host over the window from zeros ->
 * (Capon) awpu_hip_csm_invert_rule_host -> awpu_hip_csm_map_host -> the sum -> awpu_hip_heatmap_u8 / awpu_hip_find_peaks.
 * An unsolved bin (step 6a) is a +0 plane and a 0 in `solved`; it is no error.
 *
 * A SPLIT RECORDING.  carry [length - 1][n_bins][usable][2] holds the spectra (step 1) of the blocks before the call, the newest
 * last: its last *carried entries are valid.  *carried is 0 before the first call; the call reads both and updates both (the
 * recording "starts" *carried blocks before the call).  A recording split over calls -- each continuing with the next_first of
 * the one before and the same c, length, active list and gains -- gives one call's bits.  With length == 1 carry may be NULL.
 *
 * ALL n_blocks blocks are appended to the handle's ingest ring, as awpu_hip_watch_blocks appends them: after the call the ring is
 * where that call leaves it on the same blocks.
 *
 * Refusals, in this order: those of the block source (awpu_hip_watch.h), of awpu_watch_t, of c (awpu_hip_csm.h), length outside
 * [1, 1024], show outside the request, a null carried (or carry, with length > 1), *carried outside [0, length - 1], of the find
 * request: AWPU_ERR_INVALID; then the state refusals of the cross-spectral calls (AWPU_ERR_STATE), cfg.hist != AWPU_HIST, more
 * than 256 streams on the wire, a slab handle or a grid other than rows x cols (AWPU_ERR_INVALID), no table or no active list
 * (AWPU_ERR_STATE), diagonal removal with one active mic (AWPU_ERR_INVALID), more active mics than the map or -- for Capon -- the
 * inverse takes (AWPU_ERR_RANGE).  Argument errors are reported before the handle is touched.
 *
 * Memory.  A piece is at most cfg.max_batch shown frames and 256 new blocks.  The device holds the spectra of length - 1 + 256
 * blocks, ONE frame's matrix, inverse and inverse scratch (a frame's launches follow one another on one stream: 24 MiB at 256 mics
 * and 8 bins), and a piece's rows, planes and images.  None of it grows with n_blocks.
 *
 * Conventions are those of awpu_hip.h (status codes, host pointers owned by the caller, one thread per handle).
 */
#ifndef AWPU_HIP_CSM_WATCH_H
#define AWPU_HIP_CSM_WATCH_H

#include "awpu_hip_csm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AWPU_CSM_SHOW_SUM (-1)
#define AWPU_CSM_MAX_LENGTH 1024

/* n_blocks x 256 wire datagrams (host, as awpu_hip_watch_blocks takes them) -> each may be NULL, at least one is not:
 *   image [n_frames][rows * cols], big_image, power [n_frames][pixel_count], sources / count (with f) as awpu_hip_tones_blocks
 *   gives them; planes [n_frames][n_bins][pixel_count] floats; solved [n_frames][n_bins] (1 wherever nothing had to be solved).
 * Host memory throughout; synchronous. */
int awpu_hip_csm_watch_blocks(awpu_hip_t *h, const void *datagrams, int32_t stride_bytes, int32_t n_blocks, const awpu_watch_t *w,
                              const awpu_csm_t *c, int32_t length, int32_t show, const awpu_find_t *f, float *carry, int32_t *carried,
                              uint8_t *image, uint8_t *big_image, float *power, awpu_source_t *sources, int32_t *count, float *planes,
                              int32_t *solved);

/* The same from unpacked samples [n_streams][pitch] floats (host): pitch >= 256 * n_blocks.  Synchronous. */
int awpu_hip_csm_watch_samples(awpu_hip_t *h, const float *samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                               const awpu_csm_t *c, int32_t length, int32_t show, const awpu_find_t *f, float *carry, int32_t *carried,
                               uint8_t *image, uint8_t *big_image, float *power, awpu_source_t *sources, int32_t *count, float *planes,
                               int32_t *solved);

/* The same on device buffers (d_samples, d_carry and every output; carried stays a host pointer and is updated before the call
 * returns, as block_count in awpu_hip_csm_samples_device), enqueued on `stream` (a hipStream_t, NULL = the handle's own);
 * asynchronous: nothing in the run waits on the host.  *c and *w are read before the call returns. */
int awpu_hip_csm_watch_samples_device(awpu_hip_t *h, const float *d_samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                                      const awpu_csm_t *c, int32_t length, int32_t show, const awpu_find_t *f, float *d_carry,
                                      int32_t *carried, uint8_t *d_image, uint8_t *d_big_image, float *d_power, awpu_source_t *d_sources,
                                      int32_t *d_count, float *d_planes, int32_t *d_solved, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AWPU_HIP_CSM_WATCH_H */
