// csm_calls.h -- what the host files of the cross-spectral calls share: of awpu_csm.cpp the state refusals, what a map and an
// inverse need before anything is enqueued and the launches of steps 1, 3 to 5 and 6a (awpu_csm_clean.cpp's loop maps with the
// map's; awpu_csm_run.cpp's runs enqueue them all); of awpu_csm_clean.cpp what a CLEAN-SC loop needs before anything is enqueued
// and the loop (the runs turn a frame's matrix into planes with it).  Internal to libawpu_hip.so.
#pragma once

#include "awpu_handle.h"
#include "awpu_hip_csm.h"
#include "csm_rule.h"

namespace awpu::host {

// floats of the matrix [n_bins][usable][usable][2], of one block's spectra [n_bins][usable][2] and of the planes [n_bins][pixel_count]
inline size_t csm_matrix_floats(const awpu_hip *h, const awpu_csm_t &c) { return (size_t) c.n_bins * h->usable() * h->usable() * 2; }
inline size_t csm_spectra_floats(const awpu_hip *h, const awpu_csm_t &c) { return (size_t) c.n_bins * h->usable() * 2; }
inline size_t csm_plane_floats(const awpu_hip *h, const awpu_csm_t &c) { return (size_t) c.n_bins * h->cfg.pixel_count; }
// the steering table (prepare()'s, or ensure_cohere_table's where prepare() builds none) and the twiddles behind the two windows
inline const awpu::LutEntry *csm_lut(const awpu_hip *h) { return h->d_lut ? h->d_lut.get() : h->d_cohere_lut.get(); }
inline const float *csm_twiddles(const awpu_hip *h) { return h->d_tones_tables.get() + 2 * awpu::kCsmSamples; }

// the refusals of a cross-spectral call that come before the handle is made ready: a null handle, a bad c (AWPU_ERR_INVALID); a
// device group, a call in flight, AWPU_INTERP_FIR8, a band (AWPU_ERR_STATE)
int csm_check(awpu_hip *h, const awpu_csm_t *c);
// step 1 of n_blocks blocks on device buffers, enqueued on s, behind ensure_tones_tables
int csm_enqueue_spectra(awpu_hip *h, const float *d_samples, long long pitch, int n_blocks, const awpu_csm_t &c, float *d_spectra, hipStream_t s);
// behind check_ready: the map's refusals that read the active list, then the steps that may block, before anything is enqueued
int csm_ready_map(awpu_hip *h, const awpu_csm_t *c);
// steps 3 to 5 on device buffers, enqueued on s
int csm_enqueue_map(awpu_hip *h, const float *d_matrix, int block_count, const awpu_csm_t &c, float *d_map, float *d_q, hipStream_t s);
// behind check_ready: the inverse's refusal that reads the active list, then its scratch, before anything is enqueued
int csm_ready_invert(awpu_hip *h, const awpu_csm_t *c);
// step 6a on device buffers, enqueued on s
int csm_enqueue_invert(awpu_hip *h, const float *d_matrix, int block_count, const awpu_csm_t &c, float *d_inverse, int32_t *d_solved, hipStream_t s);

// what a CLEAN-SC loop writes, device memory, each or null: steps [n_bins][cl.steps]; clean, residual, map [n_bins][pixel_count]
struct CsmCleanOut {
    awpu_csm_clean_step_t *steps = nullptr;
    float *clean = nullptr, *residual = nullptr, *map = nullptr;
};
// a loop's refusals that read the handle and come before it is made ready: csm_check's, the kind, a slab handle (AWPU_ERR_STATE)
int csm_clean_check(awpu_hip *h, const awpu_csm_t *c);
// everything of a loop that may block -- the handle made ready, the map's tables, the loop's own buffers (the working matrix too
// where the caller keeps none) --, before the call enqueues anything
int csm_clean_ready(awpu_hip *h, const awpu_csm_t &c, bool own_matrix);
// the load of d_matrix into D (which must not overlap it) and the loop on D, all on s, behind csm_clean_ready: nothing here
// allocates or waits.  D is left holding the residual's matrix.
int csm_clean_enqueue(awpu_hip *h, const float *d_matrix, float *D, int block_count, const awpu_csm_t &c, const awpu_csm_clean_t &cl,
                      const CsmCleanOut &out, hipStream_t s);

}  // namespace awpu::host
