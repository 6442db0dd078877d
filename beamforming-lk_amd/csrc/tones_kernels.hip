// tones_kernels.hip -- gfx950 (MI355X, CDNA4): the tone sweep of include/awpu_hip_tones.h.
//
//   for pixel p:  out[0..255] = sum over the active mics of fma(frac, X_s[off+i] - X_s[off+i+1], X_s[off+i+1])   (delay.cpp:19-25)
//     y[i] = (0.5 out[i] - 0.25 (out[i+1] + out[i-1])) w[i], y[0] = y[255] = 0;  z = FFT256(y);  bins[k] = c_k |z[k]|^2 / (wss 256 usable)
//     tone[g] = sum of bins over group g;  pitch = the strongest bin of the groups' range
//
// THE SWEEP is das_exact_kernel's (das_kernels.hip), as cohere_sweep_kernel took it over: one workgroup = 4 waves, a wave sweeps 4
// consecutive pixels; the touched window of a chunk of mics is staged once in LDS ([chunk][W] fp32, gains applied); a table entry
// is wave-uniform, so (off, frac) travel in SGPRs; lane l owns samples l, l + 64, l + 128, l + 192; one lerp per sample, mics in the
// list's order, so out[] has the reference's bits.
//
// THE EPILOGUE, once per pixel, in registers.  The stencil takes its neighbours from the neighbour lanes (cohere_sums' exchange).
// The transform is the rule's radix-2 decimation in time on bit-reversed input: position n of z starts as y[rev8(n)], so sample
// m = l + 64 k sits at position n = rev8(m), whose bit 0 is k >> 1, bit 1 is k & 1 and bits 2..7 are the lane's bits 5..0.  Stage h
// pairs positions that differ in bit log2(h):
//     h = 1:        registers k and k + 2 of the same lane (samples m and m + 128), tw = t[0]
//     h = 2:        registers 2 j and 2 j + 1               (samples m and m + 64),  tw = t[64 j]
//     h = 4 .. 128: lanes l and l ^ 32, 16, .., 1, the same register: one __shfl_xor per component; both lanes form the product
//                   tw * b from the same operands (the rule's operations, so the same bits) and the lower one keeps a + tw b, the
//                   upper one a - tw b.  tw = t[(n mod h) * (128 / h)]: 24 entries per lane, loaded once per wave.
// Behind the last stage position n <= 128 is bin n: bins 0..127 sit in the even lanes, bin 128 in lane 1.  The division happens per
// bin, in its lane.  A group of one bin is that bin, stored by its lane; a wider group is a lane partial over the lane's bins in
// register order, then a wave reduction (l ^ 32, .., 1): a fixed order, not the rule's (2e-5, awpu_hip_tones.h).  The pitch is a
// wave maximum of (bits << 32 | 255 - n): the greater bits win, equal bits go to the lower bin -- the rule's order exactly.
//   About 70 vector instructions per lane-stage and 48 cross-lane moves for the transform, a division per bin: some 600 vector
// instructions per pixel with one group, whatever the mic count ("Tone maps").
//   Contraction is off in this file; the lerp's fmaf is written out, nothing else is fused.
#include "tones_kernels.h"

#pragma clang fp contract(off)

namespace awpu {

constexpr int kTonesThreads = 256;
constexpr int kTonesPPW = 4;
constexpr int kTonesLaneStages = 6;  // h = 4 .. 128

// one butterfly of the rule between two registers of a lane
__device__ __forceinline__ void tones_butterfly(float &ar, float &ai, float &br, float &bi, float wr, float wi) {
    const float p0 = br * wr, p1 = bi * wi, p2 = br * wi, p3 = bi * wr;
    const float tr = p0 - p1, ti = p2 + p3;
    br = ar - tr, bi = ai - ti;
    ar = ar + tr, ai = ai + ti;
}

__global__ __launch_bounds__(kTonesThreads) void tones_sweep_kernel(TonesArgs c, int chunk) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const SweepArgs &a = c.sweep;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y;
    const int W = a.window;
    const int pix0 = (blockIdx.x * (kTonesThreads / 64) + wave) * kTonesPPW;
    const float *frame = a.frames + (size_t) b * a.n_streams * a.hist;

    float acc[kTonesPPW][4];
#pragma unroll
    for (int pp = 0; pp < kTonesPPW; pp++)
#pragma unroll
        for (int k = 0; k < 4; k++) acc[pp][k] = 0.0f;

    for (int m0 = 0; m0 < a.usable; m0 += chunk) {
        const int mc = min(chunk, a.usable - m0);
        __syncthreads();  // previous chunk fully consumed
        for (int m = wave; m < mc; m += kTonesThreads / 64) {
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
        for (int pp = 0; pp < kTonesPPW; pp++) {
            const int p = pix0 + pp;
            if (p < a.pixel_count) {
                const LutEntry *row = a.lut + (size_t) p * a.usable + m0;
                for (int m = 0; m < mc; m++) {
                    const LutEntry entry = row[m];  // wave-uniform address: scalar load
                    const float f = entry.frac;
                    const float *x = lds + m * W + entry.off_rel + lane;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const float x0 = x[64 * k];
                        const float x1 = x[64 * k + 1];
                        acc[pp][k] = acc[pp][k] + __builtin_fmaf(f, x0 - x1, x1);
                    }
                }
            }
        }
    }

    if (pix0 >= a.pixel_count) return;  // (wave-uniform; no barrier follows)

    // what the epilogue reads of the two tables, the same for the wave's four pixels
    int npos[4];  // where register k's value stands behind the last stage
    float win[4];
    const int lane_rev = (int) (__brev((unsigned) lane) >> 26) << 2;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        npos[k] = lane_rev | ((k & 1) << 1) | (k >> 1);
        win[k] = c.window[lane + 64 * k];
    }
    const float2 *tw = reinterpret_cast<const float2 *>(c.twiddles);
    const float2 tw0 = tw[0], tw64 = tw[64];
    float2 twl[kTonesLaneStages][4];
#pragma unroll
    for (int s = 0; s < kTonesLaneStages; s++)
#pragma unroll
        for (int k = 0; k < 4; k++) twl[s][k] = tw[(npos[k] & ((4 << s) - 1)) << (5 - s)];  // h = 4 << s, 128 / h = 32 >> s
    const float scale = c.wss * (float) (kSamples * a.usable);
    const int first_bin = c.t.edge[0], end_bin = c.t.edge[c.t.n_groups];

#pragma unroll
    for (int pp = 0; pp < kTonesPPW; pp++) {
        const int p = pix0 + pp;
        if (p >= a.pixel_count) break;  // (wave-uniform)
        const float(&o)[4] = acc[pp];
        float re[4], im[4];
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
            const float y = ma * win[k];
            re[k] = (i >= 1 && i <= kSamples - 2) ? y : 0.0f;
            im[k] = 0.0f;
        }
        // h = 1, h = 2: inside the lane
        tones_butterfly(re[0], im[0], re[2], im[2], tw0.x, tw0.y);
        tones_butterfly(re[1], im[1], re[3], im[3], tw0.x, tw0.y);
        tones_butterfly(re[0], im[0], re[1], im[1], tw0.x, tw0.y);
        tones_butterfly(re[2], im[2], re[3], im[3], tw64.x, tw64.y);
        // h = 4 .. 128: across lanes
#pragma unroll
        for (int s = 0; s < kTonesLaneStages; s++) {
            const int mask = 32 >> s;
            const bool upper = (lane & mask) != 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float other_re = __shfl_xor(re[k], mask), other_im = __shfl_xor(im[k], mask);
                const float ar = upper ? other_re : re[k], ai = upper ? other_im : im[k];
                const float br = upper ? re[k] : other_re, bi = upper ? im[k] : other_im;
                const float wr = twl[s][k].x, wi = twl[s][k].y;
                const float p0 = br * wr, p1 = bi * wi, p2 = br * wi, p3 = bi * wr;
                const float tr = p0 - p1, ti = p2 + p3;
                re[k] = upper ? ar - tr : ar + tr;
                im[k] = upper ? ai - ti : ai + ti;
            }
        }
        // bins, each in its lane
        const size_t at = (size_t) b * a.pixel_count + p;
        float bin[4];
        unsigned long long key = 0;  // (any bin of the range beats it: its low word is at least 127)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int n = npos[k];
            const float q0 = re[k] * re[k], q1 = im[k] * im[k];
            const float s = q0 + q1;
            const float ck = (n == 0 || n == AWPU_TONES_BINS - 1) ? 1.0f : 2.0f;
            bin[k] = (ck * s) / scale;
            if (n < AWPU_TONES_BINS) {
                if (c.bins) c.bins[at * AWPU_TONES_BINS + n] = bin[k];
                if (c.spectrum) {
                    c.spectrum[(at * AWPU_TONES_BINS + n) * 2] = re[k];
                    c.spectrum[(at * AWPU_TONES_BINS + n) * 2 + 1] = im[k];
                }
            }
            if (n >= first_bin && n < end_bin) {
                const unsigned long long mine = ((unsigned long long) __float_as_uint(bin[k]) << 32) | (unsigned) (255 - n);
                key = mine > key ? mine : key;
            }
        }
        if (c.pitch || c.pitch_row) {
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) {
                const unsigned long long other = __shfl_xor(key, s);
                key = other > key ? other : key;
            }
            const int pitch = 255 - (int) (unsigned) (key & 0xffffffffull);
            if (lane == 0) {
                if (c.pitch) c.pitch[at] = pitch;
                if (c.pitch_row) c.pitch_row[at] = (float) pitch;
            }
        }
        if (c.tone) {
            for (int g = 0; g < c.t.n_groups; g++) {  // (wave-uniform: the edges are kernel arguments)
                const int lo = c.t.edge[g], hi = c.t.edge[g + 1];
                float *dst = c.tone + ((size_t) b * c.t.n_groups + g) * a.pixel_count + p;
                if (hi - lo == 1) {  // the bin itself, from its lane
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        if (npos[k] == lo) *dst = bin[k];
                } else {
                    float sum = 0.0f;
#pragma unroll
                    for (int k = 0; k < 4; k++) sum += (npos[k] >= lo && npos[k] < hi) ? bin[k] : 0.0f;
#pragma unroll
                    for (int s = 32; s >= 1; s >>= 1) sum += __shfl_xor(sum, s);
                    if (lane == 0) *dst = sum;
                }
            }
        }
    }
}

hipError_t launch_tones_sweep(const TonesArgs &a, hipStream_t stream) {
    int chunk = 0;
    const size_t lds = das_exact_lds_bytes(a.sweep.window, a.sweep.usable, &chunk);
    if (lds == 0 || !a.window || !a.twiddles) return hipErrorInvalidValue;
    const int pix_per_block = (kTonesThreads / 64) * kTonesPPW;
    dim3 grid((a.sweep.pixel_count + pix_per_block - 1) / pix_per_block, a.sweep.batch);
    if (grid.y > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tones_sweep_kernel, grid, dim3(kTonesThreads), lds, stream, a, chunk);
    return hipGetLastError();
}

}  // namespace awpu
