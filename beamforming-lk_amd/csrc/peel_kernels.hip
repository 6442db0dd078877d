// peel_kernels.hip -- gfx950 (MI355X, CDNA4): the step and the loop of include/awpu_hip_peel.h.
//
//   step, frame b, pixel p, (o_s, f_s) = the pixel's table row:
//     b[i] = norm * sum_s lerp(f_s, g_s X_s[o_s+i], g_s X_s[o_s+i+1])       i = lo .. hi, the sum in list order, plain adds
//     X_s[o_s+i+1] = fma(-u_s, lerp(f_s, b[i+1], b[i]), X_s[o_s+i+1])       i = lo .. hi-1, every active s
//
// One workgroup of eight waves per frame; frames are independent, so a batch fills the chip and one frame is one workgroup's work
// (258 + 2 E beam samples of `usable` mics each: at the reference's shape 64 x 314 lerps -- DESIGN.md has the figures, and what a
// single frame costs this way).
//   The beam: a thread owns beam samples tid, tid + 512, ...; for each it walks the mics in the list's order, sixteen at a time
// -- the 32 loads of a group are issued before the group's add chain starts, so they are in flight together -- and a wave's
// loads of one mic are 64 consecutive floats.  The table row is read at wave-uniform addresses (scalar loads).  b[] goes to LDS.
//   The subtraction starts behind a barrier, when every beam sample of the frame is complete and every read of the beam pass has
// returned.  A wave takes mics wave, wave + 8, ..., two at a time and four runs of 64 samples of each: eight loads in flight
// before the first store.  Each sample of the frame is read and written once, by one lane; lanes walk i, so loads and stores
// are 64 consecutive floats again.  No atomics anywhere.
//   The loop's iteration kernel puts the pick (a block-wide maximum of the order's key, find_rule.h) and the bookkeeping (lane 0:
// close the step before, the stop tests, the record; PeelState in device memory) in front of the same step; the finish kernel
// closes the last step and forms the three maps.  Contraction is off in this file; the rule's fmaf are peel_rule.h's.
#include "peel_kernels.h"

#include "peel_rule.h"

#pragma clang fp contract(off)

namespace awpu {

namespace {

constexpr int kPeelThreads = 512;
constexpr int kPeelWaves = kPeelThreads / 64;
constexpr int kPeelGroup = 16;      // mics whose loads are in flight together
constexpr int kPeelLdsHead = 32;    // floats of LDS in front of b[]: the maximum's slots (8 x 8 bytes), the pick

__device__ __forceinline__ void peel_frame_step(const PeelArgs &a, int b, int p, float *beam) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int U = a.usable;
    const LutEntry *row = a.lut + (size_t) p * U;
    float *X = a.frames + (size_t) b * a.n_streams * a.hist;
    const int base = a.wstart + a.lo;  // sample o + i of a mic = off_rel + base + j, j = i - lo

    for (int j = tid; j < a.len; j += kPeelThreads) {
        float out = 0.0f;
        int s = 0;
        for (; s + kPeelGroup <= U; s += kPeelGroup) {
            float x0[kPeelGroup], x1[kPeelGroup], f[kPeelGroup];
#pragma unroll
            for (int q = 0; q < kPeelGroup; q++) {
                const LutEntry entry = row[s + q];
                const float *x = X + (size_t) a.index[s + q] * a.hist + entry.off_rel + base + j;
                x0[q] = x[0], x1[q] = x[1], f[q] = entry.frac;
            }
            if (a.gain) {
#pragma unroll
                for (int q = 0; q < kPeelGroup; q++) {
                    const float g = a.gain[s + q];
                    x0[q] = x0[q] * g, x1[q] = x1[q] * g;
                }
            }
#pragma unroll
            for (int q = 0; q < kPeelGroup; q++) out = out + peel_lerp(f[q], x0[q], x1[q]);
        }
        for (; s < U; s++) {
            const LutEntry entry = row[s];
            const float *x = X + (size_t) a.index[s] * a.hist + entry.off_rel + base + j;
            float x0 = x[0], x1 = x[1];
            if (a.gain) x0 = x0 * a.gain[s], x1 = x1 * a.gain[s];
            out = out + peel_lerp(entry.frac, x0, x1);
        }
        beam[j] = out * a.norm;
    }
    __syncthreads();  // b[] complete; every read of the beam pass has returned

    if (a.beams) {
        float *dst = a.beams + (size_t) b * a.len;
        for (int j = tid; j < a.len; j += kPeelThreads) dst[j] = beam[j];
    }
    // two mics and four runs of 64 samples at a time: eight loads in flight before the first store
    const int n = a.len - 1;
    for (int s0 = wave; s0 < U; s0 += 2 * kPeelWaves) {
        float *x[2];
        float u[2], f[2];
#pragma unroll
        for (int m = 0; m < 2; m++) {
            const int s = min(s0 + m * kPeelWaves, U - 1);  // (a second mic off the list: addresses of the last one, never used)
            const LutEntry entry = row[s];
            u[m] = a.u[s], f[m] = entry.frac;
            x[m] = X + (size_t) a.index[s] * a.hist + entry.off_rel + base + 1;  // sample o + i + 1 at x[j]
        }
        const bool second = s0 + kPeelWaves < U;
        for (int j0 = lane; j0 < n; j0 += 4 * 64) {
            float v[2][4];
#pragma unroll
            for (int m = 0; m < 2; m++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int j = j0 + 64 * q;
                    v[m][q] = j < n && (m == 0 || second) ? x[m][j] : 0.0f;
                }
#pragma unroll
            for (int m = 0; m < 2; m++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int j = j0 + 64 * q;
                    if (j < n && (m == 0 || second)) x[m][j] = peel_subtract(u[m], f[m], beam[j], beam[j + 1], v[m][q]);
                }
        }
    }
}

// the maximum over the workgroup, in every thread
__device__ __forceinline__ unsigned long long peel_block_max(unsigned long long v, unsigned long long *slots) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long best = 0;
#pragma unroll
    for (int w = 0; w < kPeelWaves; w++) best = slots[w] > best ? slots[w] : best;
    return best;
}

}  // namespace

__global__ __launch_bounds__(kPeelThreads) void peel_step_kernel(PeelArgs a, const int32_t *pixel) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int b = blockIdx.x;
    const int p = pixel[b];
    if (p < 0 || p >= a.n_pixels) {  // no step: the frame is untouched, its beam row zero
        if (a.beams)
            for (int j = threadIdx.x; j < a.len; j += kPeelThreads) a.beams[(size_t) b * a.len + j] = 0.0f;
        return;
    }
    peel_frame_step(a, b, p, lds + kPeelLdsHead);
}

__global__ __launch_bounds__(kPeelThreads) void peel_iteration_kernel(PeelArgs a, const float *power, PeelState *state, int k, float stop_ratio) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    unsigned long long *slots = reinterpret_cast<unsigned long long *>(lds);
    int *shared_pick = reinterpret_cast<int *>(lds + 2 * kPeelWaves);
    const int b = blockIdx.x;
    const float *P = power + (size_t) b * a.n_pixels;
    PeelState &st = state[b];
    if (k > 0 && st.done) return;  // (the same word for every thread: nobody passes a barrier alone)

    unsigned long long best = 0;
#pragma unroll 8
    for (int p = threadIdx.x; p < a.n_pixels; p += kPeelThreads) {
        const unsigned long long key = peel_key(P[p], (uint32_t) p);
        best = key > best ? key : best;
    }
    best = peel_block_max(best, slots);
    if (threadIdx.x == 0) {
        if (k == 0) {
            st.done = 0, st.first = 0.0f;
            for (int j = 0; j < AWPU_PEEL_MAX_STEPS; j++) st.step[j] = {-1, 0.0f, 0.0f};
        } else if (st.step[k - 1].pixel >= 0) {
            st.step[k - 1].removed = peel_removed(st.step[k - 1].before, P[st.step[k - 1].pixel]);
        }
        int pick = best ? (int) find_key_pixel(best) : -1;
        if (pick >= 0) {
            const float before = P[pick];
            if (k == 0) st.first = before;
            if (before < find_floor_ratio(stop_ratio, st.first)) {
                pick = -1;
            } else {
                st.step[k] = {pick, before, 0.0f};
            }
        }
        if (pick < 0) st.done = 1;
        *shared_pick = pick;
    }
    __syncthreads();
    const int p = *shared_pick;
    if (p < 0) return;
    peel_frame_step(a, b, p, lds + kPeelLdsHead);
}

__global__ __launch_bounds__(kPeelThreads) void peel_finish_kernel(const float *power, PeelState *state, int n_steps, int n_pixels, awpu_peel_step_t *steps,
                                                                   float *clean, float *residual, float *map) {
    __shared__ awpu_peel_step_t s_step[AWPU_PEEL_MAX_STEPS];
    const int b = blockIdx.x;
    const float *P = power + (size_t) b * n_pixels;
    PeelState &st = state[b];
    if ((int) threadIdx.x < n_steps) {
        awpu_peel_step_t s = st.step[threadIdx.x];
        if ((int) threadIdx.x == n_steps - 1 && s.pixel >= 0) s.removed = peel_removed(s.before, P[s.pixel]);  // the last sweep closes the last step
        s_step[threadIdx.x] = s;
        if (steps) steps[(size_t) b * n_steps + threadIdx.x] = s;
    }
    __syncthreads();
    for (int p = threadIdx.x; p < n_pixels; p += kPeelThreads) {
        const size_t at = (size_t) b * n_pixels + p;
        const float c = peel_clean_at(s_step, n_steps, p), r = P[p];
        if (clean) clean[at] = c;
        if (residual) residual[at] = r;
        if (map) map[at] = c + r;
    }
}

namespace {

// LDS of a step: the head, then b[]; 0 where it does not fit
size_t peel_lds_bytes(const PeelArgs &a) {
    const size_t bytes = ((size_t) kPeelLdsHead + (size_t) a.len) * sizeof(float);
    return a.len >= 2 && bytes <= 64 * 1024 ? bytes : 0;
}

bool peel_args_ok(const PeelArgs &a) {
    return a.frames && a.lut && a.index && a.batch >= 1 && a.usable >= 1 && a.usable <= AWPU_PEEL_MAX_MICS && a.n_pixels >= 1 && peel_lds_bytes(a) > 0;
}

}  // namespace

hipError_t launch_peel_step(const PeelArgs &a, const int32_t *pixel, hipStream_t stream) {
    if (!peel_args_ok(a) || !pixel) return hipErrorInvalidValue;
    hipLaunchKernelGGL(peel_step_kernel, dim3(a.batch), dim3(kPeelThreads), peel_lds_bytes(a), stream, a, pixel);
    return hipGetLastError();
}

hipError_t launch_peel_iteration(const PeelArgs &a, const float *power, PeelState *state, int32_t k, float stop_ratio, hipStream_t stream) {
    if (!peel_args_ok(a) || !power || !state || k < 0 || k >= AWPU_PEEL_MAX_STEPS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(peel_iteration_kernel, dim3(a.batch), dim3(kPeelThreads), peel_lds_bytes(a), stream, a, power, state, k, stop_ratio);
    return hipGetLastError();
}

hipError_t launch_peel_finish(const float *power, PeelState *state, int32_t n_steps, int32_t n_pixels, int32_t batch, awpu_peel_step_t *steps,
                              float *clean, float *residual, float *map, hipStream_t stream) {
    if (!power || !state || n_steps < 1 || n_steps > AWPU_PEEL_MAX_STEPS || n_pixels < 1 || batch < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(peel_finish_kernel, dim3(batch), dim3(kPeelThreads), 0, stream, power, state, n_steps, n_pixels, steps, clean, residual, map);
    return hipGetLastError();
}

}  // namespace awpu
