// cohere_kernels.hip -- gfx950 (MI355X, CDNA4): the coherence sweep of include/awpu_hip_cohere.h.
//
//   for pixel p:  out[0..255] = 0, e[1..254] = 0
//     for active mic s:  t[i] = fma(frac, X_s[off+i] - X_s[off+i+1], X_s[off+i+1])          (delay.cpp:19-25)
//                        out[i] += t[i];   ma = 0.5 t[i] - 0.25 (t[i+1] + t[i-1]);   e[i] = fma(ma, ma, e[i])
//     num = sum_{i=1..254} (0.5 out[i] - 0.25 (out[i+1] + out[i-1]))^2,   den = sum_{i=1..254} e[i]
//     power = num / (256 usable);  coherence = min(num / (usable den), 1), 0 unless den > 0;  weighted = power * coherence
//
// The shape is das_exact_kernel's (das_kernels.hip): one workgroup = 4 waves, a wave sweeps 4 consecutive pixels; the touched
// window of a chunk of mics is staged once in LDS ([chunk][W] fp32, gains applied); a table entry is wave-uniform, so (off, frac)
// travel in SGPRs; lane l owns samples l, l + 64, l + 128, l + 192, so every LDS read of a wave is 64 consecutive dwords
// (conflict-free); mics are visited in the list's order, so out[] has the reference's bits.
//   On top of that a lane needs t[i-1] and t[i+1] of the same mic.  It RECOMPUTES them from x[i-1 .. i+2]: four LDS reads and three
// lerps per sample, each the rule's own operation on the rule's own operands, so the neighbours a lane forms are bit for bit the
// t[] their owners form, and e[] has the rule's bits whatever the lane.  (The alternative, taking them from the neighbour lanes,
// saves two reads and two lerps and pays two cross-lane moves and the wrap between registers k and k +- 1: DESIGN.md has the
// figures.)  Sample 0 has no t[-1] and sample 255 no t[256]: their lanes clamp the address to the staged window -- x[0] and
// x[256], which the mic's own lerp reads anyway -- and what they add to e is thrown away behind the sweep.  No read, LDS or global,
// falls outside what das_exact_kernel reads.
//   Contraction is off in this file; the rule's two fmaf are written out.  The two 254-term sums are wave reductions in a fixed
// order; the division and the clamp happen once per pixel, in lane 0.
#include "cohere_kernels.h"

#pragma clang fp contract(off)

namespace awpu {

constexpr int kCohereThreads = 256;
constexpr int kCoherePPW = 4;

// num and den of one pixel, in every lane: lanes own samples {l, l+64, l+128, l+192}; e of samples 0 and 255 is zero already
__device__ __forceinline__ void cohere_sums(const float (&o)[4], const float (&e)[4], int lane, float *num_out, float *den_out) {
    float num = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        float prev = __shfl_up(o[k], 1);    // lane l-1, same k
        float next = __shfl_down(o[k], 1);  // lane l+1, same k
        // sample l+64k-1 of lane 0 lives in lane 63 of register k-1; likewise the far end
        const float wrap_prev = __shfl(o[k > 0 ? k - 1 : 0], 63);
        const float wrap_next = __shfl(o[k < 3 ? k + 1 : 3], 0);
        if (lane == 0) prev = wrap_prev;
        if (lane == 63) next = wrap_next;
        const int i = lane + 64 * k;
        const float ma = o[k] * 0.5f - 0.25f * (next + prev);
        if (i >= 1 && i <= kSamples - 2) num += ma * ma;
    }
    // den in num's order, lane by lane and across lanes: with one active mic e[] holds num's own squares, and then den is num, bit
    // for bit, and the coherence exactly 1 (adding the +0 of samples 0 and 255 changes no bits of a sum of squares)
    float den = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; k++) den += e[k];
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        num += __shfl_xor(num, s);
        den += __shfl_xor(den, s);
    }
    *num_out = num;
    *den_out = den;
}

__global__ __launch_bounds__(kCohereThreads) void cohere_sweep_kernel(CohereArgs c, int chunk) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const SweepArgs &a = c.sweep;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y;
    const int W = a.window;
    const int pix0 = (blockIdx.x * (kCohereThreads / 64) + wave) * kCoherePPW;
    const float *frame = a.frames + (size_t) b * a.n_streams * a.hist;
    // where a lane reads x[i-1] of its first sample and x[i+2] of its last: clamped to [0, 256] of the mic's window
    const int first_m1 = lane > 0 ? lane - 1 : 0;
    const int last_p2 = lane < 63 ? lane + 194 : kSamples;

    float acc[kCoherePPW][4], en[kCoherePPW][4];
#pragma unroll
    for (int pp = 0; pp < kCoherePPW; pp++)
#pragma unroll
        for (int k = 0; k < 4; k++) acc[pp][k] = 0.0f, en[pp][k] = 0.0f;

    for (int m0 = 0; m0 < a.usable; m0 += chunk) {
        const int mc = min(chunk, a.usable - m0);
        __syncthreads();  // previous chunk fully consumed
        for (int m = wave; m < mc; m += kCohereThreads / 64) {
            const float *src = frame + (size_t) a.index[m0 + m] * a.hist + a.wstart;
            if (a.gain) {  // optional per-mic gain (awpu_hip_set_mic_gains), one multiply per staged sample
                const float gm = a.gain[m0 + m];
                for (int t = lane; t < W; t += 64) lds[m * W + t] = src[t] * gm;
            } else {
                for (int t = lane; t < W; t += 64) lds[m * W + t] = src[t];
            }
        }
        __syncthreads();
#pragma unroll
        for (int pp = 0; pp < kCoherePPW; pp++) {
            const int p = pix0 + pp;
            if (p < a.pixel_count) {
                const LutEntry *row = a.lut + (size_t) p * a.usable + m0;
                for (int m = 0; m < mc; m++) {
                    const LutEntry entry = row[m];  // wave-uniform address: scalar load
                    const float f = entry.frac;
                    const float *x = lds + m * W + entry.off_rel;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const int i = lane + 64 * k;
                        const float xm = x[k == 0 ? first_m1 : i - 1];
                        const float x0 = x[i];
                        const float x1 = x[i + 1];
                        const float x2 = x[k == 3 ? last_p2 : i + 2];
                        const float tm = __builtin_fmaf(f, xm - x0, x0);  // t[i-1]
                        const float t = __builtin_fmaf(f, x0 - x1, x1);   // t[i]
                        const float tp = __builtin_fmaf(f, x1 - x2, x2);  // t[i+1]
                        acc[pp][k] = acc[pp][k] + t;
                        const float ma = t * 0.5f - 0.25f * (tp + tm);
                        en[pp][k] = __builtin_fmaf(ma, ma, en[pp][k]);
                    }
                }
            }
        }
    }

#pragma unroll
    for (int pp = 0; pp < kCoherePPW; pp++) {
        const int p = pix0 + pp;
        if (p < a.pixel_count) {
            // samples 0 and 255 are outside the stencil's range: what their lanes formed from the clamped reads is not e[]
            if (lane == 0) en[pp][0] = 0.0f;
            if (lane == 63) en[pp][3] = 0.0f;
            const size_t at = (size_t) b * a.pixel_count + p;
            if (a.sums) {
#pragma unroll
                for (int k = 0; k < 4; k++) a.sums[at * kSamples + lane + 64 * k] = acc[pp][k];
            }
            if (c.energy) {
#pragma unroll
                for (int k = 0; k < 4; k++) c.energy[at * kSamples + lane + 64 * k] = en[pp][k];
            }
            float num, den;
            cohere_sums(acc[pp], en[pp], lane, &num, &den);
            if (lane == 0) {
                const float power = num / (float) (kSamples * a.usable);
                float coh = den > 0.0f ? num / ((float) a.usable * den) : 0.0f;
                if (coh > 1.0f) coh = 1.0f;
                if (a.power) a.power[at] = power;
                if (c.coherence) c.coherence[at] = coh;
                if (c.weighted) c.weighted[at] = power * coh;
            }
        }
    }
}

hipError_t launch_cohere_sweep(const CohereArgs &a, hipStream_t stream) {
    int chunk = 0;
    const size_t lds = das_exact_lds_bytes(a.sweep.window, a.sweep.usable, &chunk);
    if (lds == 0) return hipErrorInvalidValue;
    const int pix_per_block = (kCohereThreads / 64) * kCoherePPW;
    dim3 grid((a.sweep.pixel_count + pix_per_block - 1) / pix_per_block, a.sweep.batch);
    if (grid.y > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cohere_sweep_kernel, grid, dim3(kCohereThreads), lds, stream, a, chunk);
    return hipGetLastError();
}

}  // namespace awpu
