/*
 * awpu_hip_csm_invert.h -- step 6a of awpu_hip_csm.h: the loaded inverse of a cross-spectral matrix with a written arithmetic, on
 * the host and on the device.  awpu_hip_csm.h states the rule and includes this header; include that one.  What the device gives
 * equals awpu_hip_csm_invert_rule_host bit for bit, the solved words included.  awpu_hip_csm_invert_host (step 6) stays as it is:
 * the same mathematics, other bits.
 *
 * Conventions are those of awpu_hip.h (status codes, host pointers owned by the caller, one thread per handle).
 */
#ifndef AWPU_HIP_CSM_INVERT_H
#define AWPU_HIP_CSM_INVERT_H

#include "awpu_hip_csm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The most active mics the handle forms invert: above it AWPU_ERR_RANGE.  (L and M are 2 x 4 MiB of doubles a bin there.) */
#define AWPU_CSM_INVERT_MAX_MICS 512

/* Step 6a as executable C: pure host code, no handle.  inverse [n_bins][usable][usable][2] of matrix with its block count (>= 1);
 * solved [n_bins] or NULL.  Refusals as awpu_hip_csm_invert_host's (a null matrix or inverse, a bad c, counts below 1:
 * AWPU_ERR_INVALID, nothing written).  An unsolved bin is no error here: its inverse is +0 and its solved word 0. */
int awpu_hip_csm_invert_rule_host(const float *matrix, int32_t block_count, int32_t usable, const awpu_csm_t *c, float *inverse,
                                  int32_t *solved);

/* Step 6a on the device, of a host matrix into a host inverse, with the handle's active list (usable mics).  Synchronous.  The
 * handle refusals are those of awpu_hip_csm_map; more than AWPU_CSM_INVERT_MAX_MICS active mics: AWPU_ERR_RANGE.  Any unsolved
 * bin: AWPU_ERR_RANGE, and the caller's inverse stays as it was. */
int awpu_hip_csm_invert(awpu_hip_t *h, const float *matrix, int32_t block_count, const awpu_csm_t *c, float *inverse);

/* ... on device buffers, enqueued on `stream` (a hipStream_t, NULL = the handle's own); asynchronous.  d_solved [n_bins] or NULL;
 * an unsolved bin is no error here, as in awpu_hip_csm_invert_rule_host.  L and M live in scratch the handle owns; *c is read
 * before the call returns. */
int awpu_hip_csm_invert_device(awpu_hip_t *h, const float *d_matrix, int32_t block_count, const awpu_csm_t *c, float *d_inverse,
                               int32_t *d_solved, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AWPU_HIP_CSM_INVERT_H */
