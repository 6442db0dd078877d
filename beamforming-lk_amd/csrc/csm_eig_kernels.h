// csm_eig_kernels.h -- the device side of step 8 of include/awpu_hip_csm.h: the eigendecomposition of a cross-spectral matrix by
// the arithmetic of csm_eig_rule.h, the weighed matrix and the subspace maps' finish (csm_eig_kernels.hip).  Internal to
// libawpu_hip.so.
#pragma once

#include <hip/hip_runtime.h>

#include "csm_eig_rule.h"

namespace awpu {

// Step 8a.  matrix [n_bins][usable][usable][2] floats; values [n_bins][usable] and vectors [n_bins][usable][usable][2] floats;
// solved and sweeps [n_bins], each or null.  scratch: csm_eig_scratch_doubles(usable, n_bins) doubles, 16-byte aligned -- A, then
// V, [n_bins][usable][usable] CsmZ each, then the eigenvalues [n_bins][usable] doubles, then two state words a bin.
// REACH: of matrix the diagonal's real parts and the entries b < a; every entry of values and vectors; nothing outside the scratch.
struct CsmEigArgs {
    const float *matrix;
    float *values;
    float *vectors;
    int32_t *solved;
    int32_t *sweeps;
    double *scratch;
    int32_t usable, n_bins, block_count;
};
inline size_t csm_eig_scratch_doubles(int usable, int n_bins) {
    return (size_t) n_bins * ((size_t) usable * (size_t) usable * 4 + (size_t) usable + 1);  // (two int32 state words are one double)
}
constexpr int kCsmEigLdsBytes = 144 * 1024;
constexpr int kCsmEigResidentUsable = 64;  // up to here A and V live in LDS; above, in the scratch, which L2 holds
constexpr int kCsmEigFlagWords = 40;       // a sweep's "some pair rotated" words [kCsmEigMaxSweeps], the load's "not finite" word; padded
// LDS of the Jacobi kernel: a round's rotations (six doubles and two int32 a pair, M / 2 pairs), the loaded diagonal [usable]
// doubles (padded to an even count), the flag words, and -- where they fit -- A and V, rows of (usable | 1) CsmZ each (an odd
// pitch of 16-byte entries: a column's entries, and a row's, fall on different banks)
inline int csm_eig_lds_bytes(int usable, bool resident) {
    const int pairs = (usable + (usable & 1)) / 2;
    return 64 * pairs + 8 * (usable + (usable & 1)) + 4 * kCsmEigFlagWords + (resident ? 2 * 16 * usable * (usable | 1) : 0);
}
inline bool csm_eig_resident(int usable) { return usable <= kCsmEigResidentUsable; }
static_assert(64 * 32 + 8 * 64 + 4 * kCsmEigFlagWords + 2 * 16 * 64 * 65 <= kCsmEigLdsBytes, "64 mics fit the LDS");
// threads of the Jacobi kernel's one workgroup a bin
inline int csm_eig_threads(int usable) { return usable <= 8 ? 64 : usable <= 32 ? 256 : 1024; }
hipError_t launch_csm_eig(const CsmEigArgs &a, hipStream_t stream);  // hipErrorInvalidValue above kCsmEigMaxUsable

// Step 8b.  values and vectors as above; weighed [n_bins][usable][usable][2] is written, every entry.
struct CsmEigWeighArgs {
    const float *values;
    const float *vectors;
    float *weighed;
    int32_t usable, n_bins, kind, n_sources, root;
};
hipError_t launch_csm_eig_weigh(const CsmEigWeighArgs &a, hipStream_t stream);  // hipErrorInvalidValue above kCsmEigMaxUsable

// Step 8c's finish.  q and map [n_bins][pixel_count]; solved [n_bins] or null (every bin solved); scale = wss * 256.0f.
struct CsmEigFinishArgs {
    const float *q;
    const int32_t *solved;
    float *map;
    int32_t usable, pixel_count, n_bins, kind, root;
    float scale;
    int32_t bin[AWPU_CSM_MAX_BINS];
};
hipError_t launch_csm_eig_finish(const CsmEigFinishArgs &a, hipStream_t stream);

}  // namespace awpu
