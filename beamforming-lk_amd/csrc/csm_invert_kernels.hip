// csm_invert_kernels.hip -- gfx950 (MI355X, CDNA4): step 6a of include/awpu_hip_csm.h, the loaded inverse G of a cross-spectral
// matrix, per bin, in double.  Every arithmetic step is a function of csm_invert_rule.h, which the host rule compiles too; each
// entry's sum runs serially in ascending j inside ONE thread, so the bits do not depend on the launch shape.  Four launches:
//
// FACTOR (load and A = L L^H): a chain of `usable` dependent steps, one workgroup a bin, right-looking: step j finishes column j
// (the pivot's sqrt, the column's divisions), a barrier, then every entry (a, b), j < b <= a, of the trailing triangle takes its
// step j -- the same j-ascending sum an entry has in the rule, spread over 16 x 16 or 32 x 32 threads --, a barrier.  Column j is
// kept contiguous in LDS beside the triangle: the update's two operands are conflict-free reads.  The triangle is 16 bytes an
// entry: up to 95 mics it lives in LDS (rows of usable | 1 entries; 144 KiB), above that in the scratch, which L2 holds (4 MiB a
// bin at 512 mics).  The kernel leaves L's diagonal in the scratch and L's columns TRANSPOSED in the unused upper triangle of M,
// where the next kernel reads them coalesced.
//
// SOLVE (M = L^-1): column-parallel, one workgroup per (column, bin), one thread per row a: at step j the thread of row j divides
// its sum and hands M[j][col] on through LDS (two slots deep, one barrier a step), and every row a > j takes its step j.
//
// GRAM (G = M^H M): entry-parallel, one thread per entry b <= a, 16 x 16 a workgroup as the accumulate kernel's; the float entry
// and its exact conjugate are written.  A sum that is not finite raises the bin's second state word.
//
// FINISH: a bin whose factorisation stopped or whose state word is raised becomes +0 everywhere; the solved words.
//   Contraction is off in this file; no fast-math flag may be added to its build (`/` and sqrt are the IEEE double operations).
#include "csm_invert_kernels.h"

#include <atomic>

#pragma clang fp contract(off)

namespace awpu {

namespace {

struct CsmInvertScratch {
    CsmZ *L, *M;
    int32_t *state;  // [2]: the factorisation went through; a sum of G was not finite
};
__device__ inline CsmInvertScratch csm_invert_scratch(const CsmInvertArgs &a, int kb) {
    const size_t UU = (size_t) a.usable * a.usable;
    CsmZ *base = reinterpret_cast<CsmZ *>(a.scratch);
    return {base + (size_t) kb * UU, base + ((size_t) a.n_bins + kb) * UU, reinterpret_cast<int32_t *>(base + 2 * (size_t) a.n_bins * UU) + 2 * kb};
}

}  // namespace

template <bool kResident>
__global__ __launch_bounds__(1024) void csm_invert_factor_kernel(CsmInvertArgs a) {
    extern __shared__ __attribute__((aligned(16))) double csm_invert_lds[];
    const int U = a.usable, kb = blockIdx.x;
    const int T = blockDim.x, tx = threadIdx.x, ty = threadIdx.y, tid = ty * T + tx, nt = T * T;
    const CsmInvertScratch sc = csm_invert_scratch(a, kb);
    CsmZ *col = reinterpret_cast<CsmZ *>(csm_invert_lds);  // [U]: column j of L
    double *diag = csm_invert_lds + 2 * U;                 // [U]: the diagonal before loading
    const int pitch = kResident ? (U | 1) : U;
    CsmZ *W = kResident ? reinterpret_cast<CsmZ *>(diag + U + (U & 1)) : sc.L;  // the lower triangle, rows of `pitch`
    const float *C = a.matrix + (size_t) kb * U * U * 2;
    const double n = (double) a.block_count;

    // Load: every thread adds the trace itself, a ascending
    for (int r = tid; r < U; r += nt) diag[r] = csm_inv_load_diag(C[((size_t) r * U + r) * 2], n);
    __syncthreads();
    double trace = 0.0;
    for (int r = 0; r < U; r++) trace = trace + diag[r];
    const double load = csm_inv_loading(a.loading, trace, U);
    for (int r = ty; r < U; r += T)
        for (int b = tx; b <= r; b += T) {
            const size_t at = ((size_t) r * U + b) * 2;
            W[(size_t) r * pitch + b] = b < r ? csm_inv_load(C[at], C[at + 1], n) : CsmZ{csm_inv_loaded(diag[r], load), 0.0};
        }
    __syncthreads();

    bool ok = true;
    for (int j = 0; j < U; j++) {
        const double d = W[(size_t) j * pitch + j].re;  // (every thread reads the same word: the branch is uniform)
        ok = csm_inv_pivot_ok(d);
        if (!ok) break;
        const double ljj = csm_inv_pivot(d);
        for (int r = j + 1 + tid; r < U; r += nt) {
            const CsmZ l = csm_inv_over(W[(size_t) r * pitch + j], ljj);
            col[r] = l;
            sc.M[(size_t) j * U + r] = l;  // L^T, in the upper triangle that M leaves free
        }
        __syncthreads();
        // (behind the barrier: above 95 mics W is sc.L, and every thread has read the pivot there by now; in LDS the pivot stays
        // as it was, nobody reads it again)
        if (tid == 0) sc.L[(size_t) j * U + j] = {ljj, 0.0};
        for (int r = j + 1 + ty; r < U; r += T) {
            const CsmZ l = col[r];
            for (int b = j + 1 + tx; b <= r; b += T) {
                CsmZ &e = W[(size_t) r * pitch + b];
                if (b < r) {
                    CsmZ s = e;
                    csm_inv_factor_step(s, l, col[b]);
                    e = s;
                } else {
                    e.re = csm_inv_factor_step_diag(e.re, l);
                }
            }
        }
        __syncthreads();
    }
    if (tid == 0) sc.state[0] = ok ? 1 : 0, sc.state[1] = 0;
}

__global__ __launch_bounds__(512) void csm_invert_solve_kernel(CsmInvertArgs a) {
    __shared__ CsmZ handed[2];
    const int U = a.usable, c0 = blockIdx.x, kb = blockIdx.y, r = threadIdx.x;
    const CsmInvertScratch sc = csm_invert_scratch(a, kb);
    if (!sc.state[0]) return;  // (the whole workgroup)
    const bool mine = r >= c0 && r < U;
    const double lrr = mine ? sc.L[(size_t) r * U + r].re : 1.0;
    CsmZ s{r == c0 ? 1.0 : 0.0, 0.0};
    for (int j = c0; j < U; j++) {
        if (r == j) {
            const CsmZ m = csm_inv_over(s, lrr);
            sc.M[(size_t) j * U + c0] = m;
            handed[j & 1] = m;
        }
        __syncthreads();  // (slot j & 1 is written again two steps on, behind the next step's barrier)
        if (mine && r > j) csm_inv_solve_step(s, sc.M[(size_t) j * U + r], handed[j & 1]);  // L[r][j], from L^T
    }
}

__global__ __launch_bounds__(256) void csm_invert_gram_kernel(CsmInvertArgs a) {
    if (blockIdx.x > blockIdx.y) return;  // (a workgroup above the diagonal)
    const int U = a.usable, kb = blockIdx.z;
    const int r = blockIdx.y * 16 + threadIdx.y, b = blockIdx.x * 16 + threadIdx.x;
    const CsmInvertScratch sc = csm_invert_scratch(a, kb);
    if (!sc.state[0] || r >= U || b > r) return;
    CsmZ s{0.0, 0.0};
    for (int j = r; j < U; j++) csm_inv_gram_step(s, sc.M[(size_t) j * U + r], sc.M[(size_t) j * U + b]);
    if (!csm_inv_gram_ok(s)) sc.state[1] = 1;
    float *G = a.inverse + (size_t) kb * U * U * 2;
    const float re = (float) s.re, im = b < r ? (float) s.im : 0.0f;
    G[((size_t) r * U + b) * 2] = re, G[((size_t) r * U + b) * 2 + 1] = im;
    if (b < r) G[((size_t) b * U + r) * 2] = re, G[((size_t) b * U + r) * 2 + 1] = -im;
}

__global__ __launch_bounds__(256) void csm_invert_finish_kernel(CsmInvertArgs a) {
    const int kb = blockIdx.y;
    const CsmInvertScratch sc = csm_invert_scratch(a, kb);
    const bool solved = sc.state[0] && !sc.state[1];
    const size_t floats = (size_t) a.usable * a.usable * 2, i = (size_t) blockIdx.x * 256 + threadIdx.x;
    if (!solved && i < floats) a.inverse[(size_t) kb * floats + i] = 0.0f;
    if (a.solved && i == 0) a.solved[kb] = solved ? 1 : 0;
}

hipError_t launch_csm_invert(const CsmInvertArgs &a, hipStream_t stream) {
    const int U = a.usable;
    if (U < 1 || U > kCsmInvertMaxUsable || a.n_bins < 1 || a.n_bins > AWPU_CSM_MAX_BINS || a.block_count < 1) return hipErrorInvalidValue;
    const bool resident = csm_invert_resident(U);
    const int lds = csm_invert_lds_bytes(U, resident);
    // more than 64 KiB of dynamic LDS needs the limit raised once per device, as the map kernel's does
    static std::atomic<bool> raised[64] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (lds > 64 * 1024 && (dev < 0 || dev >= 64 || !raised[dev].load(std::memory_order_acquire))) {
        e = hipFuncSetAttribute((const void *) csm_invert_factor_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, kCsmInvertLdsBytes);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 64) raised[dev].store(true, std::memory_order_release);
    }
    const int T = U <= 64 ? 16 : 32;
    if (resident) {
        hipLaunchKernelGGL(csm_invert_factor_kernel<true>, dim3(a.n_bins), dim3(T, T), lds, stream, a);
    } else {
        hipLaunchKernelGGL(csm_invert_factor_kernel<false>, dim3(a.n_bins), dim3(T, T), lds, stream, a);
    }
    hipLaunchKernelGGL(csm_invert_solve_kernel, dim3(U, a.n_bins), dim3((U + 63) / 64 * 64), 0, stream, a);
    const int tiles = (U + 15) / 16;
    hipLaunchKernelGGL(csm_invert_gram_kernel, dim3(tiles, tiles, a.n_bins), dim3(16, 16), 0, stream, a);
    hipLaunchKernelGGL(csm_invert_finish_kernel, dim3((unsigned) (((size_t) U * U * 2 + 255) / 256), a.n_bins), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace awpu
