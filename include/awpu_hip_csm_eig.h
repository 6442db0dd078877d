/*
 * awpu_hip_csm_eig.h -- step 8 of awpu_hip_csm.h: the Hermitian eigendecomposition C = V L V^H of a cross-spectral matrix with a
 * written arithmetic, on the host and on the device, and the two subspace maps built from it: MUSIC, 1 / (s^H P_n s) with P_n the
 * projector on the noise subspace, and functional beamforming, (s^H C^(1/nu) s)^nu.  awpu_hip_csm.h states the rule and includes
 * this header; include that one.  What the device gives equals the host functions bit for bit: the eigenvalues, the eigenvectors,
 * the solved and sweep words, the weighed matrix and the maps.
 *
 * Conventions are those of awpu_hip.h (status codes, host pointers owned by the caller, one thread per handle).
 */
#ifndef AWPU_HIP_CSM_EIG_H
#define AWPU_HIP_CSM_EIG_H

#include "awpu_hip_csm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The most active mics the handle forms decompose: above it AWPU_ERR_RANGE.  (A and V are 2 x 1 MiB of doubles a bin there.) */
#define AWPU_CSM_EIG_MAX_MICS 256
/* The most sweeps a bin is given (step 8a): a bin that still rotates in its 32nd sweep is unsolved. */
#define AWPU_CSM_EIG_MAX_SWEEPS 32
#define AWPU_CSM_EIG_MUSIC 0
#define AWPU_CSM_EIG_FUNCTIONAL 1
#define AWPU_CSM_EIG_MAX_ROOT 6

/* What to make of the decomposition: 16 bytes.  kind is one of the two above.  AWPU_CSM_EIG_MUSIC reads n_sources, the dimension
 * of the signal subspace, in [0, usable - 1]; AWPU_CSM_EIG_FUNCTIONAL reads root, in [0, 6]: the exponent is nu = 2^root.  The
 * field a kind does not read must still lie in its range ([0, usable - 1], [0, 6]); reserved is 0.  Anything else:
 * AWPU_ERR_INVALID with nothing written. */
typedef struct awpu_csm_eig {
    int32_t kind;
    int32_t n_sources;
    int32_t root;
    int32_t reserved;
} awpu_csm_eig_t;

/* Step 8a as executable C: pure host code, no handle.  Of matrix [n_bins][usable][usable][2] with its block count (>= 1) the
 * diagonal's real parts and the entries b < a are read.  values [n_bins][usable] descend; vectors [n_bins][usable][usable][2]:
 * vectors[k][r] is the eigenvector of values[k][r], one contiguous row; solved [n_bins] and sweeps [n_bins], each or NULL.
 * Refusals: a null matrix, values or vectors, a bad c, counts below 1: AWPU_ERR_INVALID, nothing written.  An unsolved bin is no
 * error: its values and vectors are +0 and its solved word 0.  A bin with an eigenvalue that does not fit a float ((float) of it
 * is not finite) is unsolved too: the values of a solved bin are finite. */
int awpu_hip_csm_eig_host(const float *matrix, int32_t block_count, int32_t usable, const awpu_csm_t *c, float *values, float *vectors,
                          int32_t *solved, int32_t *sweeps);

/* Step 8b: weighed [n_bins][usable][usable][2], the Hermitian H = sum over r of w_r v_r v_r^H of values and vectors as above.
 * c->kind must be AWPU_CSM_CONVENTIONAL; c->loading is not read.  Refusals as above, and a bad e. */
int awpu_hip_csm_eig_weigh_host(const float *values, const float *vectors, int32_t usable, const awpu_csm_t *c, const awpu_csm_eig_t *e,
                                float *weighed);

/* Step 8c: map [n_bins][n_pixels] of weighed (steps 3 and 4 on it, then the finish); solved [n_bins] or NULL (every bin solved).
 * The table and the active list are awpu_hip_csm_map_host's, and so are their refusals. */
int awpu_hip_csm_eig_map_host(const float *weighed, const int32_t *solved, const int32_t *off, const float *frac, int32_t lut_stride,
                              int32_t n_pixels, const int32_t *index, int32_t usable, const awpu_csm_t *c, const awpu_csm_eig_t *e, float *map);

/* Step 8a on the device, of a host matrix with the handle's active list (usable mics) into host values and vectors; solved and
 * sweeps [n_bins], each or NULL.  Synchronous.  The handle refusals are those of awpu_hip_csm_invert; more than
 * AWPU_CSM_EIG_MAX_MICS active mics: AWPU_ERR_RANGE.  An unsolved bin is no error, as in awpu_hip_csm_eig_host. */
int awpu_hip_csm_eig(awpu_hip_t *h, const float *matrix, int32_t block_count, const awpu_csm_t *c, float *values, float *vectors,
                     int32_t *solved, int32_t *sweeps);

/* ... on device buffers, enqueued on `stream` (a hipStream_t, NULL = the handle's own); asynchronous: nothing waits on the host.
 * d_solved and d_sweeps [n_bins], each or NULL.  A and V live in scratch the handle owns; *c is read before the call returns. */
int awpu_hip_csm_eig_device(awpu_hip_t *h, const float *d_matrix, int32_t block_count, const awpu_csm_t *c, float *d_values, float *d_vectors,
                            int32_t *d_solved, int32_t *d_sweeps, void *stream);

/* Step 8b on device buffers, enqueued on `stream`; asynchronous.  *c and *e are read before the call returns. */
int awpu_hip_csm_eig_weigh_device(awpu_hip_t *h, const float *d_values, const float *d_vectors, const awpu_csm_t *c, const awpu_csm_eig_t *e,
                                  float *d_weighed, void *stream);

/* Steps 8a to 8c of a host matrix with its block count: host map [n_bins][pixel_count] (a slab handle maps its own pixels);
 * values [n_bins][usable] and solved [n_bins], each or NULL.  Synchronous.  Bit for bit the composition of awpu_hip_csm_eig_device,
 * awpu_hip_csm_eig_weigh_device, the q of awpu_hip_csm_map_device on the weighed matrix and the finish of step 8c. */
int awpu_hip_csm_eig_map(awpu_hip_t *h, const float *matrix, int32_t block_count, const awpu_csm_t *c, const awpu_csm_eig_t *e, float *map,
                         float *values, int32_t *solved);

/* ... on device buffers, enqueued on `stream`; asynchronous.  The vectors, the weighed matrix and q live in scratch the handle
 * owns; *c and *e are read before the call returns. */
int awpu_hip_csm_eig_map_device(awpu_hip_t *h, const float *d_matrix, int32_t block_count, const awpu_csm_t *c, const awpu_csm_eig_t *e,
                                float *d_map, float *d_values, int32_t *d_solved, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AWPU_HIP_CSM_EIG_H */
