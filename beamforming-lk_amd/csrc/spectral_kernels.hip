// spectral_kernels.hip -- the device side of include/awpu_hip_spectral.h.
//
// The pre-pass generalises band_filter_kernel (band_kernels.hip) to several bands: one wave per (frame, active stream); the row
// segment [window start - (longest taps - 1), window end) goes through LDS once per chunk of 512 outputs, and the bands are then
// run one after the other over that segment -- band_step of band_rule.h, ascending taps, lane l owning outputs l + 64 j of the
// chunk in eight accumulators (consecutive lanes read consecutive LDS words: no bank conflicts) -- each into its own plane of
// the output.  A band's steps are exactly those band_filter_kernel takes for it: the same bits.  The coefficients are
// wave-uniform loads out of the kernel's arguments.  Plain vector loads and stores, nothing else.
//
// The display step: every band's maximum of a frame by one workgroup (a reduction through registers and LDS, one plain store),
// then one pass over the frame's powers that forms the three levels and the dominant band of every pixel -- the steps of
// spectral_rule.h, which the host rule takes too.  The large image: every byte plane through launch_upscale's taps and arithmetic.
#include "spectral_kernels.h"

#include "band_rule.h"
#include "spectral_rule.h"

namespace awpu {

namespace {

constexpr int kPerLane = kBandChunk / 64;
static_assert(sizeof(SpectralBandArgs) <= 4096, "the bands' coefficients travel as kernel arguments");
static_assert(kBandChunk + AWPU_BAND_MAX_TAPS - 1 <= kBandRowFloats, "a chunk and its history fit a wave's LDS row");

__global__ __launch_bounds__(64 * kBandWaves) void spectral_filter_kernel(const SpectralBandArgs a) {
#pragma clang fp contract(off)
    __shared__ float rows[kBandWaves][kBandRowFloats];
    const int wave = __builtin_amdgcn_readfirstlane((int) threadIdx.x >> 6), lane = (int) threadIdx.x & 63;
    const int slot = (int) blockIdx.x * kBandWaves + wave;
    const bool live = slot < a.usable;  // (wave-uniform; the last workgroup's spare waves only keep the barriers' company)
    const long long id = live ? a.index[slot] : 0;
    const long long f = blockIdx.y;
    const float *in = a.in + f * a.in_frame + id * a.in_row + a.in_first;
    float *out = a.out + f * a.out_frame + id * a.out_row + a.out_first;
    float *seg = rows[wave];
    const int pre = a.max_taps - 1;
    for (int o0 = 0; o0 < a.n; o0 += kBandChunk) {
        const int cn = min(kBandChunk, a.n - o0);  // outputs of this chunk; it reads inputs [o0, o0 + pre + cn)
        for (int i = lane; i < pre + kBandChunk; i += 64) seg[i] = live && i < pre + cn ? in[o0 + i] : 0.0f;
        __syncthreads();
        const float *at = seg + pre + lane;  // output lane + 64 j reads at[64 j - k] at tap k
        for (int b = 0; b < a.n_bands; b++) {
            const int taps = a.taps[b];
            float acc[kPerLane];
#pragma unroll
            for (int j = 0; j < kPerLane; j++) acc[j] = 0.0f;
#pragma unroll 4
            for (int k = 0; k < taps; k++) {
                const float ck = a.coef[b][k];
#pragma unroll
                for (int j = 0; j < kPerLane; j++) acc[j] = band_step(ck, at[64 * j - k], acc[j]);
            }
            if (live) {
                float *plane = out + b * a.out_plane;
#pragma unroll
                for (int j = 0; j < kPerLane; j++)
                    if (lane + 64 * j < cn) plane[o0 + lane + 64 * j] = acc[j];
            }
        }
        __syncthreads();  // (the next chunk overwrites the row)
    }
}

// the maximum of band blockIdx.x's frame blockIdx.y into peaks[frame][band]
__global__ __launch_bounds__(256) void spectral_max_kernel(const float *power, long long plane, int n, float *peaks) {
    __shared__ float part[4];
    const float *p = power + (long long) blockIdx.x * plane + (long long) blockIdx.y * n;
    float m = 0.0f;
    for (int i = threadIdx.x; i < n; i += 256) m = spectral_max_step(m, p[i]);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) m = spectral_max_step(m, __shfl_xor(m, s));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++) m = spectral_max_step(m, part[w]);
        peaks[(size_t) blockIdx.y * AWPU_SPECTRAL_MAX_BANDS + blockIdx.x] = m;
    }
}

// v[b] without an address into the registers
__device__ inline float pick_band(const float (&v)[AWPU_SPECTRAL_MAX_BANDS], int b) { return b == 0 ? v[0] : (b == 1 ? v[1] : (b == 2 ? v[2] : v[3])); }

constexpr int kComposeUnit = 4;  // pixels per lane: 12 bytes of the image, 4 of the dominant bands

__global__ __launch_bounds__(256) void spectral_compose_kernel(const float *power, long long plane, int n, const SpectralShow show,
                                                               const float *peaks, uint8_t *image, uint8_t *dominant) {
    const long long f = blockIdx.y;
    const int i0 = ((int) blockIdx.x * 256 + (int) threadIdx.x) * kComposeUnit;
    if (i0 >= n) return;
    float max_of[AWPU_SPECTRAL_MAX_BANDS] = {0.0f, 0.0f, 0.0f, 0.0f}, scale_of[3] = {0.0f, 0.0f, 0.0f};
    if (image) {
#pragma unroll
        for (int b = 0; b < AWPU_SPECTRAL_MAX_BANDS; b++)
            if (b < show.n_bands) max_of[b] = peaks[f * AWPU_SPECTRAL_MAX_BANDS + b];
        float common = 0.0f;
#pragma unroll
        for (int c = 0; c < 3; c++)
            if (show.channel[c] >= 0) common = spectral_max_step(common, pick_band(max_of, show.channel[c]));
#pragma unroll
        for (int c = 0; c < 3; c++)
            if (show.channel[c] >= 0) scale_of[c] = show.scale == AWPU_SPECTRAL_SCALE_COMMON ? common : pick_band(max_of, show.channel[c]);
    }
    uint8_t level[kComposeUnit][3], best[kComposeUnit];
    const int valid = min(kComposeUnit, n - i0);
#pragma unroll
    for (int k = 0; k < kComposeUnit; k++) {
        float v[AWPU_SPECTRAL_MAX_BANDS] = {0.0f, 0.0f, 0.0f, 0.0f};
        uint32_t bits[AWPU_SPECTRAL_MAX_BANDS] = {0, 0, 0, 0};
#pragma unroll
        for (int b = 0; b < AWPU_SPECTRAL_MAX_BANDS; b++)
            if (k < valid && b < show.n_bands) {
                v[b] = power[b * plane + f * n + i0 + k];
                bits[b] = __float_as_uint(v[b]);
            }
        best[k] = (uint8_t) spectral_dominant(bits, AWPU_SPECTRAL_MAX_BANDS);  // (a band that is not there: bits 0, which beat nothing)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int b = show.channel[c];
            level[k][c] = b < 0 ? (uint8_t) 0 : spectral_level(pick_band(v, b), scale_of[c]);
        }
    }
    if (image) {
        uint8_t *o = image + ((size_t) f * n + i0) * 3;
        if (valid == kComposeUnit && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {  // 4 x 3 bytes = three dwords
            const uint8_t *l = &level[0][0];
            uint32_t w[3];
#pragma unroll
            for (int d = 0; d < 3; d++) w[d] = l[4 * d] | l[4 * d + 1] << 8 | l[4 * d + 2] << 16 | (uint32_t) l[4 * d + 3] << 24;
#pragma unroll
            for (int d = 0; d < 3; d++) reinterpret_cast<uint32_t *>(o)[d] = w[d];
        } else {
#pragma unroll
            for (int k = 0; k < kComposeUnit; k++)
#pragma unroll
                for (int c = 0; c < 3; c++)
                    if (k < valid) o[3 * k + c] = level[k][c];
        }
    }
    if (dominant) {
        uint8_t *o = dominant + (size_t) f * n + i0;
        if (valid == kComposeUnit && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
            *reinterpret_cast<uint32_t *>(o) = best[0] | best[1] << 8 | best[2] << 16 | (uint32_t) best[3] << 24;
        } else {
#pragma unroll
            for (int k = 0; k < kComposeUnit; k++)
                if (k < valid) o[k] = best[k];
        }
    }
}

constexpr int kBigUnit = 4;  // output pixels per lane: 12 bytes

// upscale_kernel's pixel (das_kernels.hip) for every byte of a three-byte one: the same taps, resize_combine, the same clamps
__global__ __launch_bounds__(256) void spectral_upscale_kernel(const uint8_t *src, int srows, int scols, const ResizeTap *taps, int flip,
                                                               uint8_t *dst, int drows, int dcols) {
    const int unit = (int) blockIdx.x * 256 + (int) threadIdx.x, dy = blockIdx.y;
    if (unit * kBigUnit >= dcols) return;
    const uint8_t *img = src + (size_t) blockIdx.z * srows * scols * 3;
    const int x0 = dcols < kBigUnit ? 0 : min(unit * kBigUnit, dcols - kBigUnit);  // (the row's last unit ends at its end)
    const int valid = min(kBigUnit, dcols);
    const ResizeTap ty = taps[dcols + dy];
    const uint8_t *row0 = img + (size_t) (min(max(ty.src, 0), srows - 1)) * scols * 3;
    const uint8_t *row1 = img + (size_t) (min(max(ty.src + 1, 0), srows - 1)) * scols * 3;
    uint8_t px[kBigUnit * 3];
#pragma unroll
    for (int k = 0; k < kBigUnit; k++) {
        const int x = min(x0 + k, dcols - 1);
        const ResizeTap tx = taps[flip ? dcols - 1 - x : x];
        const int c0 = tx.src, c1 = min(tx.src + 1, scols - 1);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int S0 = row0[3 * c0 + c] * tx.w0 + row0[3 * c1 + c] * tx.w1;
            const int S1 = row1[3 * c0 + c] * tx.w0 + row1[3 * c1 + c] * tx.w1;
            px[3 * k + c] = resize_combine(S0, S1, ty.w0, ty.w1);
        }
    }
    uint8_t *o = dst + (((size_t) blockIdx.z * drows + dy) * dcols + x0) * 3;
    if (valid == kBigUnit && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
#pragma unroll
        for (int d = 0; d < 3; d++)
            reinterpret_cast<uint32_t *>(o)[d] = px[4 * d] | px[4 * d + 1] << 8 | px[4 * d + 2] << 16 | (uint32_t) px[4 * d + 3] << 24;
    } else {
#pragma unroll
        for (int k = 0; k < 3 * kBigUnit; k++)
            if (k < 3 * valid) o[k] = px[k];
    }
}

}  // namespace

hipError_t launch_spectral_filter(const SpectralBandArgs &a, hipStream_t stream) {
    if (!a.in || !a.out || !a.index) return hipErrorInvalidValue;
    if (a.n_bands < 1 || a.n_bands > AWPU_SPECTRAL_MAX_BANDS || a.max_taps < 1 || a.max_taps > AWPU_BAND_MAX_TAPS) return hipErrorInvalidValue;
    for (int b = 0; b < a.n_bands; b++)
        if (a.taps[b] < 1 || a.taps[b] > a.max_taps) return hipErrorInvalidValue;
    if (a.n < 1 || a.in_first < 0 || a.out_first < 0 || a.out_plane < 0) return hipErrorInvalidValue;
    if (a.usable < 1 || a.n_frames < 1 || a.n_frames > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(spectral_filter_kernel, dim3((a.usable + kBandWaves - 1) / kBandWaves, a.n_frames), dim3(64 * kBandWaves), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_spectral_compose(const float *d_power, long long plane, int n, int n_frames, const SpectralShow &show, float *d_peaks,
                                   uint8_t *d_image, uint8_t *d_dominant, hipStream_t stream) {
    if (!d_power || (!d_image && !d_dominant) || (d_image && !d_peaks)) return hipErrorInvalidValue;
    if (n < 1 || n_frames < 1 || n_frames > 65535 || plane < 0) return hipErrorInvalidValue;
    if (spectral_display_refusal(show.n_bands, show.channel, show.scale)) return hipErrorInvalidValue;
    if (d_image) hipLaunchKernelGGL(spectral_max_kernel, dim3(show.n_bands, n_frames), dim3(256), 0, stream, d_power, plane, n, d_peaks);
    const int blocks = (n + 256 * kComposeUnit - 1) / (256 * kComposeUnit);
    hipLaunchKernelGGL(spectral_compose_kernel, dim3(blocks, n_frames), dim3(256), 0, stream, d_power, plane, n, show, d_peaks, d_image, d_dominant);
    return hipGetLastError();
}

hipError_t launch_spectral_upscale(const uint8_t *d_src, int srows, int scols, int batch, const ResizeTap *d_taps, bool flip,
                                   uint8_t *d_dst, int drows, int dcols, hipStream_t stream) {
    if (!d_src || !d_taps || !d_dst) return hipErrorInvalidValue;
    if (srows < 1 || scols < 1 || batch < 1 || batch > 65535 || drows < 1 || drows > 65535 || dcols < 1) return hipErrorInvalidValue;
    const int units = (dcols + kBigUnit - 1) / kBigUnit;
    hipLaunchKernelGGL(spectral_upscale_kernel, dim3((units + 255) / 256, drows, batch), dim3(256), 0, stream, d_src, srows, scols, d_taps,
                       flip ? 1 : 0, d_dst, drows, dcols);
    return hipGetLastError();
}

}  // namespace awpu
