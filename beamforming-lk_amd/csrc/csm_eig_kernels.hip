// csm_eig_kernels.hip -- gfx950 (MI355X, CDNA4): step 8 of include/awpu_hip_csm.h, the Hermitian eigendecomposition of a
// cross-spectral matrix per bin, in double, and the subspace maps built on it.  Every arithmetic step is a function of
// csm_eig_rule.h, which the host rule compiles too; every stored word is produced by exactly one thread from operands the rule
// fixes, so the bits do not depend on the launch shape.  Four kernels:
//
// JACOBI (load and the sweeps): one workgroup a bin.  A and V are 16 bytes an entry: up to 64 mics they live in LDS (rows of
// usable | 1 entries, an odd pitch: the 16-lane groups of a 16-byte read fall on different banks along a row and along a column;
// 133 KiB), above that in the scratch, which L2 holds (2 x 1 MiB a bin at 256 mics).  A round: one thread per pair writes the
// rotation to LDS (and raises the sweep's flag where it rotates); a barrier; phase 1, the columns p and q of A and V, one item per
// (row, pair) with the lanes along the pairs -- a row's entries, read together --; a barrier; phase 2, the rows p and q of A, one
// item per (pair, column) with the lanes along the row, the pair's four entries in closed form; a barrier.  The flag of a sweep
// is a pure function of the matrix: every thread reads the same word behind the sweep's last barrier and the loop's exit is
// uniform.  The kernel leaves the eigenvalues (the diagonal, unsorted), V and the bin's state -- converged, sweeps -- in the scratch.
//
// SORT (sort and round): entry-parallel, one thread per (eigenvalue j, mic a): the rank of j from all eigenvalues, the float
// entry of eigenvector j in row `rank`; a bin that is unsolved (the Jacobi kernel's state, or an eigenvalue that does not fit a float)
// becomes +0 everywhere.  The solved and sweep words.
//
// WEIGH (step 8b): entry-parallel, one thread per entry b <= a, 16 x 16 a workgroup as the inverse's gram kernel; the weights of
// the bin are made once per workgroup, in LDS.  The entry and its exact conjugate are written.
//
// FINISH (step 8c): the map from q of the weighed matrix and the solved words.
//   Contraction is off in this file; no fast-math flag may be added to its build (`/` and sqrt are the IEEE operations).
#include "csm_eig_kernels.h"

#include <atomic>

#pragma clang fp contract(off)

namespace awpu {

namespace {

struct CsmEigScratch {
    CsmZ *A, *V;
    double *lambda;
    int32_t *state;  // [2]: the sweeps converged; how many ran
};
__device__ inline CsmEigScratch csm_eig_scratch(double *scratch, int usable, int n_bins, int kb) {
    const size_t UU = (size_t) usable * usable;
    CsmZ *base = reinterpret_cast<CsmZ *>(scratch);
    double *tail = scratch + 4 * (size_t) n_bins * UU;
    return {base + (size_t) kb * UU, base + ((size_t) n_bins + kb) * UU, tail + (size_t) kb * usable,
            reinterpret_cast<int32_t *>(tail + (size_t) n_bins * usable) + 2 * kb};
}

}  // namespace

template <bool kResident>
__global__ __launch_bounds__(1024) void csm_eig_jacobi_kernel(CsmEigArgs a) {
    extern __shared__ __attribute__((aligned(16))) double csm_eig_lds[];
    const int U = a.usable, kb = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int M = U + (U & 1), pairs = M / 2, Ue = U + (U & 1);
    const CsmEigScratch sc = csm_eig_scratch(a.scratch, U, a.n_bins, kb);
    // the round's rotations, one array a field
    double *rc = csm_eig_lds, *rs = rc + pairs, *rphr = rs + pairs, *rphi = rphr + pairs, *rnpp = rphi + pairs, *rnqq = rnpp + pairs;
    int32_t *rp = reinterpret_cast<int32_t *>(rnqq + pairs), *rq = rp + pairs;  // p < 0: the pair does not rotate
    double *diag = csm_eig_lds + 8 * pairs;                                     // [Ue]
    int32_t *flags = reinterpret_cast<int32_t *>(diag + Ue);                    // [kCsmEigFlagWords]
    const int pitch = kResident ? (U | 1) : U;
    CsmZ *A = kResident ? reinterpret_cast<CsmZ *>(diag + Ue + kCsmEigFlagWords / 2) : sc.A;
    CsmZ *V = kResident ? A + (size_t) U * pitch : sc.V;
    const float *C = a.matrix + (size_t) kb * U * U * 2;
    const double n = (double) a.block_count;

    // Load: every entry by one thread; every thread adds the trace itself, a ascending
    for (int i = tid; i < kCsmEigFlagWords; i += nt) flags[i] = 0;
    __syncthreads();
    for (int e = tid; e < U * U; e += nt) {
        const int r = e / U, b = e - r * U;
        if (b < r) {
            const CsmZ z = csm_inv_load(C[(size_t) e * 2], C[(size_t) e * 2 + 1], n);
            if (!csm_inv_finite(z.re) || !csm_inv_finite(z.im)) flags[kCsmEigMaxSweeps] = 1;
            A[(size_t) r * pitch + b] = z;
            A[(size_t) b * pitch + r] = CsmZ{z.re, -z.im};
        } else if (b == r) {
            const double d = csm_inv_load_diag(C[(size_t) e * 2], n);
            if (!csm_inv_finite(d)) flags[kCsmEigMaxSweeps] = 1;
            diag[r] = d;
            A[(size_t) r * pitch + r] = CsmZ{d, 0.0};
        }
        V[(size_t) r * pitch + b] = CsmZ{b == r ? 1.0 : 0.0, 0.0};
    }
    __syncthreads();
    double trace = 0.0;
    for (int r = 0; r < U; r++) trace = trace + diag[r];
    if (flags[kCsmEigMaxSweeps] || !csm_eig_trace_ok(trace)) {  // (every thread reads the same words: the whole workgroup leaves)
        if (tid == 0) sc.state[0] = 0, sc.state[1] = 0;
        return;
    }
    const double thr = csm_eig_threshold(trace, U);

    int sweeps = 0;
    bool converged = false;
    while (!converged && sweeps < kCsmEigMaxSweeps) {
        for (int round = 0; round < M - 1; round++) {
            if (tid < pairs) {
                int32_t p, q;
                bool rotates = false;
                if (csm_eig_pair(U, round, tid, p, q)) {
                    const CsmEigRotation o = csm_eig_rotation(A[(size_t) q * pitch + p], A[(size_t) p * pitch + p].re, A[(size_t) q * pitch + q].re, thr);
                    rotates = o.rotates;
                    if (rotates) {
                        rc[tid] = o.c, rs[tid] = o.s, rphr[tid] = o.phr, rphi[tid] = o.phi, rnpp[tid] = o.npp, rnqq[tid] = o.nqq;
                        rq[tid] = q;
                        flags[sweeps] = 1;
                    }
                }
                rp[tid] = rotates ? p : -1;
            }
            __syncthreads();
            // phase 1: the columns p and q of A (rows 0 .. U-1 of the items) and of V (rows U .. 2U-1)
            for (int it = tid; it < 2 * U * pairs; it += nt) {
                const int row2 = it / pairs, i = it - row2 * pairs;
                const int p = rp[i];
                if (p < 0) continue;
                const int q = rq[i];
                CsmZ *X = row2 < U ? A + (size_t) row2 * pitch : V + (size_t) (row2 - U) * pitch;
                CsmZ x = X[p], y = X[q];
                csm_eig_columns(rc[i], rs[i], rphr[i], rphi[i], x, y);
                X[p] = x, X[q] = y;
            }
            __syncthreads();
            // phase 2: the rows p and q of A
            for (int it = tid; it < pairs * U; it += nt) {
                const int i = it / U, j = it - i * U;
                const int p = rp[i];
                if (p < 0) continue;
                const int q = rq[i];
                CsmZ *xp = A + (size_t) p * pitch + j, *yq = A + (size_t) q * pitch + j;
                if (j == p) {
                    *xp = CsmZ{rnpp[i], 0.0}, *yq = CsmZ{0.0, 0.0};
                } else if (j == q) {
                    *xp = CsmZ{0.0, 0.0}, *yq = CsmZ{rnqq[i], 0.0};
                } else {
                    CsmZ x = *xp, y = *yq;
                    csm_eig_rows(rc[i], rs[i], rphr[i], rphi[i], x, y);
                    *xp = x, *yq = y;
                }
            }
            __syncthreads();
        }
        converged = !flags[sweeps];  // (written before this sweep's barriers, never after: every thread reads the same word)
        sweeps++;
    }
    for (int r = tid; r < U; r += nt) sc.lambda[r] = A[(size_t) r * pitch + r].re;
    if (kResident)
        for (int e = tid; e < U * U; e += nt) {
            const int r = e / U, b = e - r * U;
            sc.V[e] = V[(size_t) r * pitch + b];
        }
    if (tid == 0) sc.state[0] = converged ? 1 : 0, sc.state[1] = sweeps;
}

__global__ __launch_bounds__(256) void csm_eig_sort_kernel(CsmEigArgs a) {
    const int U = a.usable, kb = blockIdx.y;
    const int e = blockIdx.x * 256 + threadIdx.x;
    const CsmEigScratch sc = csm_eig_scratch(a.scratch, U, a.n_bins, kb);
    if (e >= U * U) return;
    const int j = e / U, m = e - j * U;  // eigenvalue j, mic m
    bool ok = sc.state[0] != 0;
    int rank = 0;
    if (ok) {
        const double lj = sc.lambda[j];
        for (int i = 0; i < U; i++) {
            const double li = sc.lambda[i];
            ok = ok && csm_eig_fits(li);
            rank += csm_eig_before(li, i, lj, j) ? 1 : 0;
        }
        if (ok) {
            const CsmZ v = sc.V[(size_t) m * U + j];
            float *dst = a.vectors + (((size_t) kb * U + rank) * U + m) * 2;
            dst[0] = (float) v.re, dst[1] = (float) v.im;
            if (m == 0) a.values[(size_t) kb * U + rank] = (float) lj;
        }
    }
    if (!ok) {  // an unsolved bin: +0 everywhere (every thread of the bin comes here)
        float *dst = a.vectors + ((size_t) kb * U * U + e) * 2;
        dst[0] = 0.0f, dst[1] = 0.0f;
        if (e < U) a.values[(size_t) kb * U + e] = 0.0f;
    }
    if (e == 0) {
        if (a.solved) a.solved[kb] = ok ? 1 : 0;
        if (a.sweeps) a.sweeps[kb] = sc.state[1];
    }
}

__global__ __launch_bounds__(256) void csm_eig_weigh_kernel(CsmEigWeighArgs a) {
    __shared__ float w[kCsmEigMaxUsable];
    if (blockIdx.x > blockIdx.y) return;  // (a workgroup above the diagonal)
    const int U = a.usable, kb = blockIdx.z;
    const int r = blockIdx.y * 16 + threadIdx.y, b = blockIdx.x * 16 + threadIdx.x;
    const float *val = a.values + (size_t) kb * U, *vec = a.vectors + (size_t) kb * U * U * 2;
    for (int i = threadIdx.y * 16 + threadIdx.x; i < U; i += 256) w[i] = csm_eig_weight(a.kind, a.n_sources, a.root, i, val[i]);
    __syncthreads();
    if (r >= U || b > r) return;
    CsmComplex h{0.0f, 0.0f};
    for (int i = 0; i < U; i++) {
        const float *row = vec + (size_t) i * U * 2;
        csm_eig_weigh_step(h, w[i], CsmComplex{row[2 * r], row[2 * r + 1]}, CsmComplex{row[2 * b], row[2 * b + 1]});
    }
    if (b == r) h.im = 0.0f;
    float *H = a.weighed + (size_t) kb * U * U * 2;
    H[((size_t) r * U + b) * 2] = h.re, H[((size_t) r * U + b) * 2 + 1] = h.im;
    if (b < r) H[((size_t) b * U + r) * 2] = h.re, H[((size_t) b * U + r) * 2 + 1] = -h.im;
}

__global__ __launch_bounds__(256) void csm_eig_finish_kernel(CsmEigFinishArgs a) {
    const int kb = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.pixel_count) return;
    const size_t at = (size_t) kb * a.pixel_count + p;
    const bool solved = !a.solved || a.solved[kb] != 0;
    a.map[at] = solved ? csm_eig_map_value(a.kind, a.root, a.bin[kb], a.q[at], (float) a.usable, a.scale) : 0.0f;
}

hipError_t launch_csm_eig(const CsmEigArgs &a, hipStream_t stream) {
    const int U = a.usable;
    if (U < 1 || U > kCsmEigMaxUsable || a.n_bins < 1 || a.n_bins > AWPU_CSM_MAX_BINS || a.block_count < 1) return hipErrorInvalidValue;
    const bool resident = csm_eig_resident(U);
    const int lds = csm_eig_lds_bytes(U, resident);
    // more than 64 KiB of dynamic LDS needs the limit raised once per device, as the inverse's factor kernel does
    static std::atomic<bool> raised[64] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (lds > 64 * 1024 && (dev < 0 || dev >= 64 || !raised[dev].load(std::memory_order_acquire))) {
        e = hipFuncSetAttribute((const void *) csm_eig_jacobi_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, kCsmEigLdsBytes);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 64) raised[dev].store(true, std::memory_order_release);
    }
    const int T = csm_eig_threads(U);
    if (resident) {
        hipLaunchKernelGGL(csm_eig_jacobi_kernel<true>, dim3(a.n_bins), dim3(T), lds, stream, a);
    } else {
        hipLaunchKernelGGL(csm_eig_jacobi_kernel<false>, dim3(a.n_bins), dim3(T), lds, stream, a);
    }
    hipLaunchKernelGGL(csm_eig_sort_kernel, dim3((unsigned) ((U * U + 255) / 256), a.n_bins), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_csm_eig_weigh(const CsmEigWeighArgs &a, hipStream_t stream) {
    const int U = a.usable;
    if (U < 1 || U > kCsmEigMaxUsable || a.n_bins < 1 || a.n_bins > AWPU_CSM_MAX_BINS) return hipErrorInvalidValue;
    const int tiles = (U + 15) / 16;
    hipLaunchKernelGGL(csm_eig_weigh_kernel, dim3(tiles, tiles, a.n_bins), dim3(16, 16), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_csm_eig_finish(const CsmEigFinishArgs &a, hipStream_t stream) {
    if (a.pixel_count < 1 || a.n_bins < 1 || a.n_bins > AWPU_CSM_MAX_BINS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(csm_eig_finish_kernel, dim3((unsigned) ((a.pixel_count + 255) / 256), a.n_bins), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace awpu
