// csm_invert_kernels.h -- the device side of step 6a of include/awpu_hip_csm.h: the loaded inverse of a cross-spectral matrix by
// the arithmetic of csm_invert_rule.h (csm_invert_kernels.hip).  Internal to libawpu_hip.so.
#pragma once

#include <hip/hip_runtime.h>

#include "csm_invert_rule.h"

namespace awpu {

// matrix and inverse [n_bins][usable][usable][2] floats; solved [n_bins] or null.  scratch: csm_invert_scratch_doubles(usable,
// n_bins) doubles, 16-byte aligned -- L, then M, [n_bins][usable][usable] CsmZ each, then two state words a bin.
// REACH: of matrix the diagonal's real parts and the entries b < a; every entry of inverse; nothing outside the scratch.
struct CsmInvertArgs {
    const float *matrix;
    float *inverse;
    int32_t *solved;
    double *scratch;
    int32_t usable, n_bins, block_count;
    float loading;
};
inline size_t csm_invert_scratch_doubles(int usable, int n_bins) {
    return (size_t) n_bins * (size_t) usable * (size_t) usable * 4 + (size_t) n_bins;  // (two int32 state words are one double)
}
constexpr int kCsmInvertLdsBytes = 144 * 1024;
// LDS of the factor kernel: column j [usable] CsmZ, the unloaded diagonal [usable] doubles, and -- where it fits -- the working
// triangle, rows of (usable | 1) CsmZ (an odd pitch: a column's entries fall on different banks)
inline int csm_invert_lds_bytes(int usable, bool resident) {
    return 16 * usable + 8 * (usable + (usable & 1)) + (resident ? 16 * usable * (usable | 1) : 0);
}
inline bool csm_invert_resident(int usable) { return csm_invert_lds_bytes(usable, true) <= kCsmInvertLdsBytes; }  // up to 95 mics
hipError_t launch_csm_invert(const CsmInvertArgs &a, hipStream_t stream);  // hipErrorInvalidValue above kCsmInvertMaxUsable

}  // namespace awpu
