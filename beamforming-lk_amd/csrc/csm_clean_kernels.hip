// csm_clean_kernels.hip -- gfx950 (MI355X, CDNA4): what a CLEAN-SC loop (include/awpu_hip_csm_clean.h) runs between two dirty maps.
// Every arithmetic step is a function of csm_clean_rule.h, which the host rule compiles too: the same operations on the same
// operands, in the rule's order.  The maps are launch_csm_map's; between two of them the loop launches TWO kernels.
//
// COMPONENT (pick + steering + v + qs + the record): one workgroup of four waves a bin.  The pick is peel's: a block-wide maximum
// of the order's key over the bin's dirty row, then lane 0's stop tests on the bin's state.  The workgroup forms the picked
// pixel's steering vector once, into LDS.  Lane a then owns row a of v = D conj(s): its chain walks b = 0 .. usable-1 in order,
// reading s_b from LDS (one address a wave: a broadcast) and D[a][b] as the conjugate of D[b][a .. a+63] -- the upper triangle is
// the exact conjugate and the diagonal's im +0, so these are the bits of the strided read of row a, and a wave's load is 512
// consecutive bytes.  The loads do not depend on the chain, so the compiler keeps eight of them in flight.  256 rows a pass;
// v goes to LDS and to device memory; lane 0 adds qs in row order (2 fmaf a row), divides once, and leaves the bin's verdict
// -- the pixel or -1, r, the step's record -- in its state for the update.  At 64 mics all of this is one wave's work of
// 64 x 64 terms: the launch is the cost, which is why the pick shares it.
//
// UPDATE: one thread per entry b <= a of a stepping bin, 16 x 16 entries a workgroup as csm_accumulate_kernel has them; workgroups
// above the diagonal, and every workgroup of a bin that does not step, leave at once.  The thread reads its entry, v_a and v_b,
// subtracts, writes the entry and its conjugate.
//
// LOAD puts a caller's matrix into D's form with the same thread layout; FINISH forms the three planes and the step list.
// No f32 MFMA anywhere: it does not keep the order.  Contraction is off in this file.
#include "csm_clean_kernels.h"

#include "csm_clean_rule.h"

#pragma clang fp contract(off)

namespace awpu {

namespace {

constexpr int kCleanWaves = kCsmCleanThreads / 64;

// the maximum over the workgroup, in every thread
__device__ __forceinline__ unsigned long long clean_block_max(unsigned long long v, unsigned long long *slots) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long best = 0;
#pragma unroll
    for (int w = 0; w < kCleanWaves; w++) best = slots[w] > best ? slots[w] : best;
    return best;
}

}  // namespace

__global__ __launch_bounds__(256) void csm_clean_load_kernel(const float *src, float *dst, int usable) {
    if (blockIdx.x > blockIdx.y) return;  // (a workgroup above the diagonal)
    const int a = blockIdx.y * 16 + threadIdx.y, b = blockIdx.x * 16 + threadIdx.x, kb = blockIdx.z;
    const size_t U = (size_t) usable;
    if (a >= usable || b > a) return;
    const float *C = src + (size_t) kb * U * U * 2;
    float *D = dst + (size_t) kb * U * U * 2;
    const CsmComplex d = csm_clean_load(C[(a * U + b) * 2], C[(a * U + b) * 2 + 1], a == b);
    D[(a * U + b) * 2] = d.re, D[(a * U + b) * 2 + 1] = d.im;
    if (b < a) {
        const CsmComplex m = csm_clean_mirror(d);
        D[(b * U + a) * 2] = m.re, D[(b * U + a) * 2 + 1] = m.im;
    }
}

// kLoop: iteration i of the loop (the pick from `plane`); otherwise the step form (the pixel from `pixel`)
template <bool kLoop>
__global__ __launch_bounds__(kCsmCleanThreads) void csm_clean_component_kernel(CsmCleanArgs c, const float *plane, int i, float stop_ratio,
                                                                             const int32_t *pixel, float *component, float *qs_out) {
    __shared__ float2 s[kCsmCleanMaxUsable];
    __shared__ float2 vl[kCsmCleanMaxUsable];
    __shared__ unsigned long long slots[kCleanWaves];
    __shared__ int shared_pick;
    const int tid = threadIdx.x, kb = blockIdx.x, U = c.usable;
    CsmCleanState &st = c.state[kb];
    float2 *v_out = reinterpret_cast<float2 *>(c.v) + (size_t) kb * U;
    float2 *comp = component ? reinterpret_cast<float2 *>(component) + (size_t) kb * U : nullptr;
    int p;
    float before = 0.0f;  // (lane 0's)
    if (kLoop) {
        const int was_done = i > 0 ? st.done : 0;  // (read in front of the first barrier, written behind it: the same word for every thread)
        if (was_done) return;
        const float *P = plane + (size_t) kb * c.n_pixels;
        unsigned long long best = 0;
#pragma unroll 4
        for (int q = tid; q < c.n_pixels; q += kCsmCleanThreads) {
            const unsigned long long key = peel_key(P[q], (uint32_t) q);
            best = key > best ? key : best;
        }
        best = clean_block_max(best, slots);
        if (tid == 0) {
            float first = 0.0f;
            if (i == 0) {
                st.done = 0;
                for (int j = 0; j < AWPU_CSM_CLEAN_MAX_STEPS; j++) st.step[j] = csm_clean_unused();
            } else {
                first = st.first;
            }
            const int32_t pick = csm_clean_pick(best, P, i, stop_ratio, &first);
            st.first = first;
            st.pixel = -1;  // (until qs has passed its test)
            if (pick < 0) st.done = 1;
            shared_pick = pick;
        }
        __syncthreads();
        p = shared_pick;
        if (p < 0) return;
        if (tid == 0) before = P[p];
    } else {
        p = pixel[kb];
        if (p < 0 || p >= c.n_pixels) {  // no step: the bin keeps its matrix, its rows are zero
            for (int a = tid; a < U; a += kCsmCleanThreads) {
                v_out[a] = make_float2(0.0f, 0.0f);
                if (comp) comp[a] = make_float2(0.0f, 0.0f);
            }
            if (tid == 0) {
                st.pixel = -1, st.r = 0.0f;
                if (qs_out) qs_out[kb] = 0.0f;
            }
            return;
        }
    }

    const int k = c.bin[kb];
    const LutEntry *lut_row = c.lut + (size_t) p * U;
    for (int b = tid; b < U; b += kCsmCleanThreads) {
        const LutEntry e = lut_row[b];
        const CsmComplex sv = csm_steer(c.twiddles, k, e.off_rel + c.wstart, e.frac);
        s[b] = make_float2(sv.re, sv.im);
    }
    __syncthreads();

    const float2 *__restrict__ D = reinterpret_cast<const float2 *>(c.matrix) + (size_t) kb * U * U;
    for (int a = tid; a < U; a += kCsmCleanThreads) {
        CsmComplex v{0.0f, 0.0f};
        const float2 *__restrict__ col = D + a;
#pragma unroll 8
        for (int b = 0; b < U; b++) {
            const float2 e = col[(size_t) b * U];  // D[b][a]
            const float2 sb = s[b];
            csm_clean_add_v(v, csm_clean_entry_from_column(e.x, e.y, b == a), {sb.x, sb.y});
        }
        const float2 out = make_float2(v.re, v.im);
        vl[a] = out, v_out[a] = out;
        if (comp) comp[a] = out;
    }
    __syncthreads();

    if (tid == 0) {
        float qs = 0.0f;
        for (int a = 0; a < U; a++) qs = csm_clean_add_qs(qs, {s[a].x, s[a].y}, {vl[a].x, vl[a].y});
        const bool ok = csm_clean_qs_ok(qs);
        st.r = ok ? csm_clean_r(c.gain, qs) : 0.0f;
        st.pixel = ok ? p : -1;
        if (kLoop) {
            if (ok) {
                st.step[i] = {p, before, csm_clean_removed(c.gain, before)};
            } else {
                st.done = 1;
            }
        } else if (qs_out) {
            qs_out[kb] = qs;
        }
    }
}

__global__ __launch_bounds__(256) void csm_clean_update_kernel(float *matrix, const float *v, const CsmCleanState *state, int usable) {
    if (blockIdx.x > blockIdx.y) return;  // (a workgroup above the diagonal)
    const int a = blockIdx.y * 16 + threadIdx.y, b = blockIdx.x * 16 + threadIdx.x, kb = blockIdx.z;
    if (state[kb].pixel < 0) return;  // (the bin does not step)
    const float r = state[kb].r;
    const size_t U = (size_t) usable;
    if (a >= usable || b > a) return;
    float *D = matrix + (size_t) kb * U * U * 2;
    const float2 *V = reinterpret_cast<const float2 *>(v) + (size_t) kb * U;
    const float2 va = V[a], vb = V[b];
    const CsmComplex t = csm_clean_t({va.x, va.y}, r);
    if (b < a) {
        CsmComplex d{D[(a * U + b) * 2], D[(a * U + b) * 2 + 1]};
        csm_clean_update(d, t, {vb.x, vb.y});
        const CsmComplex m = csm_clean_mirror(d);
        D[(a * U + b) * 2] = d.re, D[(a * U + b) * 2 + 1] = d.im;
        D[(b * U + a) * 2] = m.re, D[(b * U + a) * 2 + 1] = m.im;
    } else {
        D[(a * U + a) * 2] = csm_clean_update_diag(D[(a * U + a) * 2], t, {va.x, va.y});
        D[(a * U + a) * 2 + 1] = 0.0f;
    }
}

__global__ __launch_bounds__(kCsmCleanThreads) void csm_clean_finish_kernel(const float *plane, const CsmCleanState *state, int n_steps, int n_pixels,
                                                                          awpu_csm_clean_step_t *steps, float *clean, float *residual, float *map) {
    __shared__ awpu_csm_clean_step_t s_step[AWPU_CSM_CLEAN_MAX_STEPS];
    const int kb = blockIdx.y;
    if ((int) threadIdx.x < n_steps) {
        const awpu_csm_clean_step_t st = state[kb].step[threadIdx.x];
        s_step[threadIdx.x] = st;
        if (steps && blockIdx.x == 0) steps[(size_t) kb * n_steps + threadIdx.x] = st;
    }
    __syncthreads();
    const int p = blockIdx.x * kCsmCleanThreads + threadIdx.x;
    if (p >= n_pixels) return;
    const size_t at = (size_t) kb * n_pixels + p;
    const float cv = csm_clean_at(s_step, n_steps, p), r = plane[at];
    if (clean) clean[at] = cv;
    if (residual) residual[at] = r;
    if (map) map[at] = csm_clean_map(cv, r);
}

namespace {

bool clean_shape_ok(int usable, int n_bins) { return usable >= 1 && usable <= kCsmCleanMaxUsable && n_bins >= 1 && n_bins <= AWPU_CSM_MAX_BINS; }
bool clean_args_ok(const CsmCleanArgs &a) {
    return a.matrix && a.lut && a.twiddles && a.v && a.state && a.n_pixels >= 1 && clean_shape_ok(a.usable, a.n_bins) && a.gain > 0.0f && a.gain <= 1.0f;
}

}  // namespace

hipError_t launch_csm_clean_load(const float *src, float *dst, int usable, int n_bins, hipStream_t stream) {
    if (!src || !dst || !clean_shape_ok(usable, n_bins)) return hipErrorInvalidValue;
    const int tiles = (usable + 15) / 16;
    hipLaunchKernelGGL(csm_clean_load_kernel, dim3(tiles, tiles, n_bins), dim3(16, 16), 0, stream, src, dst, usable);
    return hipGetLastError();
}

hipError_t launch_csm_clean_component(const CsmCleanArgs &a, const int32_t *pixel, float *component, float *qs, hipStream_t stream) {
    if (!clean_args_ok(a) || !pixel) return hipErrorInvalidValue;
    hipLaunchKernelGGL(csm_clean_component_kernel<false>, dim3(a.n_bins), dim3(kCsmCleanThreads), 0, stream, a, nullptr, 0, 0.0f, pixel, component, qs);
    return hipGetLastError();
}

hipError_t launch_csm_clean_iteration(const CsmCleanArgs &a, const float *plane, int i, float stop_ratio, hipStream_t stream) {
    if (!clean_args_ok(a) || !plane || i < 0 || i >= AWPU_CSM_CLEAN_MAX_STEPS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(csm_clean_component_kernel<true>, dim3(a.n_bins), dim3(kCsmCleanThreads), 0, stream, a, plane, i, stop_ratio, nullptr, nullptr, nullptr);
    return hipGetLastError();
}

hipError_t launch_csm_clean_update(float *matrix, const float *v, const CsmCleanState *state, int usable, int n_bins, hipStream_t stream) {
    if (!matrix || !v || !state || !clean_shape_ok(usable, n_bins)) return hipErrorInvalidValue;
    const int tiles = (usable + 15) / 16;
    hipLaunchKernelGGL(csm_clean_update_kernel, dim3(tiles, tiles, n_bins), dim3(16, 16), 0, stream, matrix, v, state, usable);
    return hipGetLastError();
}

hipError_t launch_csm_clean_finish(const float *plane, const CsmCleanState *state, int n_steps, int n_pixels, int n_bins, awpu_csm_clean_step_t *steps,
                                   float *clean, float *residual, float *map, hipStream_t stream) {
    if (!plane || !state || n_steps < 1 || n_steps > AWPU_CSM_CLEAN_MAX_STEPS || n_pixels < 1 || n_bins < 1 || n_bins > AWPU_CSM_MAX_BINS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(csm_clean_finish_kernel, dim3((n_pixels + kCsmCleanThreads - 1) / kCsmCleanThreads, n_bins), dim3(kCsmCleanThreads), 0, stream, plane,
                       state, n_steps, n_pixels, steps, clean, residual, map);
    return hipGetLastError();
}

}  // namespace awpu
