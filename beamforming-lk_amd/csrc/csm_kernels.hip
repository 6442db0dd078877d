// csm_kernels.hip -- gfx950 (MI355X, CDNA4): the three kernels of include/awpu_hip_csm.h.  Every arithmetic step is a function of
// csm_rule.h, which the host rule compiles too: the same operations on the same operands, in the rule's order.
//
// SPECTRA (step 1): one wave per (block, active mic).  The wave stages the 256 windowed samples (coalesced) and the twiddles in
// LDS; lane l < n_bins then owns bin[l] and adds its 256 terms in order -- every lane reads the same sample (an LDS broadcast) and
// its own twiddle.  Eight lanes of 64 work: the step is 2 * 256 * n_bins fmaf per mic and block, next to nothing beside the map.
//
// ACCUMULATE (step 2): one thread per entry b <= a of a bin's matrix, 16 x 16 entries a workgroup, workgroups above the diagonal
// leave at once.  The thread reads its entry, adds the blocks in block order, writes the entry and its conjugate.
//
// THE MAP (steps 3 to 5): one lane per (pixel, bin); a workgroup is up to 64 consecutive pixels of ONE bin, so every matrix
// entry it reads is wave-uniform: it arrives through the scalar cache (s_load) and is an SGPR operand of the lanes' fmaf, as the
// fractions of the exact sweeps are.  conj(s_b) is per lane: the workgroup forms its pixels' steering vectors once, from off / frac
// and the twiddle table (a table of them would be pixels * bins * mics * 8 bytes: 268 MB at 256 mics, 128 x 128 pixels, 8 bins),
// and keeps them in LDS lane-major -- s[b][lane], 8 bytes a lane: one conflict-free ds_read_b64 a wave.  Four rows a are in flight
// in a wave: one read of s_b feeds sixteen fmaf in four independent chains.  (f32 MFMA runs at the vector rate here and does not
// keep the order.)  At 256 mics the 64 vectors are 128 KiB, one workgroup a compute unit -- so the workgroup is FOUR waves on the same
// pixels, one a SIMD: a round is 16 rows, wave w takes rows 4 w .. 4 w + 3 of it, each y_a is one wave's chain in the rule's order;
// the waves leave the round's y in a small LDS ring (two rounds deep, one barrier a round) and every wave then adds the round's
// sixteen rows to x and d, a ascending -- the rule's order again, 32 fmaf done four times over beside the thousands of a round.
// (usable + 32) * ppw * 8 bytes, the vectors and the ring, must fit 144 KiB: up to 256 mics a workgroup maps 64 pixels, up to 544
// mics 32, up to 1120 sixteen, up to 2048 eight.
//   Contraction is off in this file.
#include "csm_kernels.h"

#include <atomic>

#include "csm_rule.h"

#pragma clang fp contract(off)

namespace awpu {

__global__ __launch_bounds__(64) void csm_spectra_kernel(CsmSpectraArgs a) {
    __shared__ float v[kCsmSamples];
    __shared__ float tw[kCsmSamples];
    const int lane = threadIdx.x;
    const int mic = blockIdx.x, block = blockIdx.y;
    const float *x = a.samples + (size_t) a.index[mic] * (size_t) a.pitch + (size_t) block * kCsmSamples;
#pragma unroll
    for (int r = 0; r < kCsmSamples / 64; r++) {
        const int i = lane + 64 * r;
        v[i] = a.gain ? csm_stage(x[i], a.gain[mic], a.window[i]) : csm_stage(x[i], a.window[i]);
        tw[i] = a.twiddles[i];
    }
    __syncthreads();
    int k = -1;
#pragma unroll
    for (int j = 0; j < AWPU_CSM_MAX_BINS; j++)
        if (lane == j && j < a.n_bins) k = a.bin[j];
    if (k < 0) return;
    const CsmComplex X = csm_bin(v, tw, k);
    float *dst = a.spectra + (((size_t) block * a.n_bins + lane) * a.usable + mic) * 2;
    dst[0] = X.re, dst[1] = X.im;
}

__global__ __launch_bounds__(256) void csm_accumulate_kernel(CsmAccumulateArgs c) {
    if (blockIdx.x > blockIdx.y) return;  // (a workgroup above the diagonal)
    const int a = blockIdx.y * 16 + threadIdx.y, b = blockIdx.x * 16 + threadIdx.x, kb = blockIdx.z;
    const size_t U = (size_t) c.usable;
    if (a >= c.usable || b > a) return;
    float *C = c.matrix + (size_t) kb * U * U * 2;
    const float2 *X = reinterpret_cast<const float2 *>(c.spectra) + (size_t) kb * U;
    const size_t step = (size_t) c.n_bins * U;
    if (b < a) {
        CsmComplex e{C[(a * U + b) * 2], C[(a * U + b) * 2 + 1]};
        for (int blk = 0; blk < c.n_blocks; blk++) {
            const float2 xa = X[blk * step + a], xb = X[blk * step + b];
            csm_add_cross(e, {xa.x, xa.y}, {xb.x, xb.y});
        }
        C[(a * U + b) * 2] = e.re, C[(a * U + b) * 2 + 1] = e.im;
        C[(b * U + a) * 2] = e.re, C[(b * U + a) * 2 + 1] = -e.im;
    } else {
        float re = C[(a * U + a) * 2];
        for (int blk = 0; blk < c.n_blocks; blk++) {
            const float2 xa = X[blk * step + a];
            csm_add_auto(re, {xa.x, xa.y});
        }
        C[(a * U + a) * 2] = re, C[(a * U + a) * 2 + 1] = 0.0f;
    }
}

constexpr int kCsmRows = 4;   // rows a in flight in a wave
constexpr int kCsmWaves = 4;  // waves of a workgroup: they share the pixels' steering vectors and take a round's rows group by group
constexpr int kCsmRound = kCsmRows * kCsmWaves;

__global__ __launch_bounds__(64 * kCsmWaves) void csm_map_kernel(CsmMapArgs c, int ppw) {
    extern __shared__ __attribute__((aligned(16))) float csm_lds[];
    float2 *s = reinterpret_cast<float2 *>(csm_lds);  // [usable][ppw]
    float2 *ring = s + (size_t) c.usable * ppw;       // [2][kCsmRound][ppw]: the y of a round's rows, two rounds deep
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int kb = blockIdx.y;
    const int k = c.bin[kb];
    const int U = c.usable;
    // lanes past ppw (more than 256 mics) go along with the workgroup's last pixel and write nothing
    const int slot = lane < ppw ? lane : ppw - 1;
    const int p = blockIdx.x * ppw + slot;
    const int pc = p < c.pixel_count ? p : c.pixel_count - 1;

    const LutEntry *lut_row = c.lut + (size_t) pc * U;
    for (int b = wave; b < U; b += kCsmWaves) {  // each wave forms a quarter of the vector
        const LutEntry e = lut_row[b];
        const CsmComplex sv = csm_steer(c.twiddles, k, e.off_rel + c.wstart, e.frac);
        if (lane < ppw) s[b * ppw + lane] = make_float2(sv.re, sv.im);
    }
    __syncthreads();

    const float *__restrict__ H = c.matrix + (size_t) kb * U * U * 2;
    float d = 0.0f, x = 0.0f;
    const int rounds = (U + kCsmRound - 1) / kCsmRound;  // (the same for every wave: the barriers below are met by all)
    for (int r = 0; r < rounds; r++) {
        const int a0 = (r * kCsmWaves + wave) * kCsmRows;  // this wave's rows of the round
        CsmComplex y[kCsmRows];
#pragma unroll
        for (int j = 0; j < kCsmRows; j++) y[j] = {0.0f, 0.0f};
        if (a0 + kCsmRows <= U) {
            const float *__restrict__ row[kCsmRows];
#pragma unroll
            for (int j = 0; j < kCsmRows; j++) row[j] = H + (size_t) (a0 + j) * U * 2;
#pragma unroll 2
            for (int b = 0; b < a0; b++) {
                const float2 sv = s[b * ppw + slot];
#pragma unroll
                for (int j = 0; j < kCsmRows; j++) csm_add_y(y[j], row[j][2 * b], row[j][2 * b + 1], {sv.x, sv.y});  // (wave-uniform: scalar loads)
            }
#pragma unroll
            for (int j = 1; j < kCsmRows; j++) {
#pragma unroll
                for (int i = 0; i < j; i++) {  // the triangle inside the group: b = a0 .. a0 + j - 1
                    const float2 sv = s[(a0 + i) * ppw + slot];
                    csm_add_y(y[j], row[j][2 * (a0 + i)], row[j][2 * (a0 + i) + 1], {sv.x, sv.y});
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < kCsmRows; j++) {  // the last rows, one by one
                if (a0 + j < U) {
                    const float *__restrict__ row = H + (size_t) (a0 + j) * U * 2;
                    for (int b = 0; b < a0 + j; b++) {
                        const float2 sv = s[b * ppw + slot];
                        csm_add_y(y[j], row[2 * b], row[2 * b + 1], {sv.x, sv.y});
                    }
                }
            }
        }
        float2 *mine = ring + ((size_t) (r & 1) * kCsmRound + wave * kCsmRows) * ppw;
        if (lane < ppw) {
#pragma unroll
            for (int j = 0; j < kCsmRows; j++) mine[j * ppw + lane] = make_float2(y[j].re, y[j].im);
        }
        __syncthreads();
        // every wave adds the round's rows, a ascending: the same 2 fmaf a row in each of them.  (This half of the ring is written
        // again two rounds on, behind the next round's barrier, which no wave passes before it has read this one.)
        const float2 *round_y = ring + (size_t) (r & 1) * kCsmRound * ppw;
        for (int j = 0; j < kCsmRound; j++) {
            const int a = r * kCsmRound + j;
            if (a < U) {
                const float2 sa = s[a * ppw + slot], ya = round_y[j * ppw + slot];
                d = d + H[((size_t) a * U + a) * 2];
                x = csm_add_x(x, {sa.x, sa.y}, {ya.x, ya.y});
            }
        }
    }
    const float q = csm_q(c.kind, d, x);
    if (wave == 0 && lane < ppw && p < c.pixel_count) {
        const size_t at = (size_t) kb * c.pixel_count + p;
        if (c.q) c.q[at] = q;
        if (c.map) c.map[at] = csm_map_value(c.kind, k, q, c.scale);
    }
}

hipError_t launch_csm_spectra(const CsmSpectraArgs &a, hipStream_t stream) {
    if (a.usable < 1 || a.n_blocks < 1 || a.n_blocks > 65535 || a.n_bins < 1 || a.n_bins > AWPU_CSM_MAX_BINS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(csm_spectra_kernel, dim3(a.usable, a.n_blocks), dim3(64), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_csm_accumulate(const CsmAccumulateArgs &a, hipStream_t stream) {
    if (a.usable < 1 || a.n_blocks < 1 || a.n_bins < 1 || a.n_bins > AWPU_CSM_MAX_BINS) return hipErrorInvalidValue;
    const int tiles = (a.usable + 15) / 16;
    hipLaunchKernelGGL(csm_accumulate_kernel, dim3(tiles, tiles, a.n_bins), dim3(16, 16), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_csm_map(const CsmMapArgs &a, hipStream_t stream) {
    const int ppw = csm_map_pixels_per_wave(a.usable);
    if (a.usable < 1 || ppw == 0 || a.pixel_count < 1 || a.n_bins < 1 || a.n_bins > AWPU_CSM_MAX_BINS) return hipErrorInvalidValue;
    const int lds = csm_map_lds_bytes(a.usable, ppw);
    // more than 64 KiB of dynamic LDS needs the limit raised once per device (a process may hold handles on several GPUs)
    static std::atomic<bool> raised[64] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (lds > 64 * 1024 && (dev < 0 || dev >= 64 || !raised[dev].load(std::memory_order_acquire))) {
        e = hipFuncSetAttribute((const void *) csm_map_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kCsmMapLdsBytes);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 64) raised[dev].store(true, std::memory_order_release);
    }
    hipLaunchKernelGGL(csm_map_kernel, dim3((a.pixel_count + ppw - 1) / ppw, a.n_bins), dim3(64 * kCsmWaves), lds, stream, a, ppw);
    return hipGetLastError();
}

}  // namespace awpu
