// watch_kernels.hip -- watching a run of blocks (include/awpu_hip_watch.h): display images of every Nth block.  What the
// reference does per GUI frame on the host -- MIMOWorker::populateHeatmap (src/dsp/mimo.cpp:61-95), cv::resize in
// AWProcessingUnit::draw (aw_processing_unit.cpp:245-259), cv::applyColorMap and cv::flip of the GUI loop
// (src/aw_control_unit/aw_control_unit.cpp:293-378) -- for a whole sweep piece per launch.  The peak and the quantisation are
// launch_heatmap (das_kernels.hip: already one launch pair per batch); here are the history of a decimated piece, its cut, and
// the large image, which at recording rates is most of the bytes the call moves (1024 x 1024 x 3 = 3 MiB per frame).
#include "watch_kernels.h"

#include <algorithm>

namespace awpu {

__global__ void watch_gather_kernel(const float *src, long long src_pitch, const float *snapshot, int b0, int every, int m,
                                    float *hist, int hist_pitch, int slot0) {
    const int slot = slot0 + blockIdx.x, s = blockIdx.y, i = threadIdx.x;
    const int blk = watch_slot_block(slot, b0, every, m);
    const float v = blk < 0 ? snapshot[(size_t) s * 2048 + 256 * (4 + blk) + i] : src[(size_t) s * src_pitch + 256 * (size_t) blk + i];
    hist[(size_t) s * hist_pitch + 256 * (size_t) slot + i] = v;
}

hipError_t launch_watch_gather(const float *d_src, long long src_pitch, const float *d_snapshot, int b0, int every, int n_streams,
                               float *d_hist, int hist_pitch, int slot0, int n_slots, hipStream_t stream) {
    // (a block below -4 is not in the ring: slot 0 holds block b0 - 3 >= -3)
    if (b0 < 0 || every < 1 || n_streams < 1 || n_streams > 65535 || slot0 < 0 || n_slots < 1 || 256 * (slot0 + n_slots) > hist_pitch)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(watch_gather_kernel, dim3(n_slots, n_streams), dim3(256), 0, stream, d_src, src_pitch, d_snapshot, b0, every,
                       std::min(every, 4), d_hist, hist_pitch, slot0);
    return hipGetLastError();
}

__global__ void watch_cut_kernel(const float *hist, int hist_pitch, int n_streams, int step, int lo, int width, float *frames) {
    const int j = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y, k = blockIdx.z;
    if (j < width)
        frames[((size_t) k * n_streams + s) * width + j] = hist[(size_t) s * hist_pitch + (size_t) step * k + lo + j];
}

hipError_t launch_watch_cut(const float *d_hist, int hist_pitch, int n_streams, int n_frames, int step, int lo, int width,
                            float *d_frames, hipStream_t stream) {
    // a snapshot is 1024 samples: the last one of the piece ends inside its history
    if (n_streams < 1 || n_streams > 65535 || n_frames < 1 || n_frames > 65535 || width < 1 || lo < 0 || lo + width > 1024 || step < 256 ||
        (long long) step * (n_frames - 1) + 1024 > hist_pitch)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(watch_cut_kernel, dim3((width + 255) / 256, n_streams, n_frames), dim3(256), 0, stream, d_hist, hist_pitch,
                       n_streams, step, lo, width, d_frames);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// The large image.  upscale_kernel (das_kernels.hip) takes one thread per output pixel and stores its colour with three byte
// stores; right for one live frame, not for a recording.  Here a lane owns 16 consecutive pixels of an output row -- 48 bytes
// of a colour image, 16 of a grey one -- and stores them 16 bytes at a time; a wave covers 1024 pixels of a row, the four
// waves of a workgroup share the 16 rows of a tile, and a lane keeps its 16 column taps in registers over its four rows.
// The source rows a tile reads (a handful) and the colour table (one dword per level) are in LDS.  The arithmetic is
// upscale_kernel's: the same ResizeTap table, resize_combine, the same clamps.  flip mirrors the row: output pixel x shows
// what upscale_kernel computes for dcols - 1 - x (cv::flip(frame, frame, 1), aw_control_unit.cpp:376-378).
// A row's 16-byte stores need no more than the alignment of its first byte: where that is a multiple of 4 they are dwordx4
// stores, and in an image whose rows are not whole dwords (dcols % 4 != 0) the other rows go out as unaligned dword groups
// (global memory takes those at any address) -- never byte by byte.  The last dcols % 16 pixels of a row belong to a lane
// whose unit is moved left to end at the row's end: it stores some of its neighbour's pixels again, the same bytes.  Only an
// image narrower than one unit (dcols < 16) is written pixel by pixel.
// ---------------------------------------------------------------------------------------
namespace {
struct __attribute__((packed, aligned(1))) Bytes16 {
    uint32_t w[4];
};
typedef uint32_t Dwords4 __attribute__((ext_vector_type(4), aligned(4)));
constexpr int kUnit = 16;  // pixels per lane

__device__ inline void store16(uint8_t *out, bool dword_aligned, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    if (dword_aligned) {
        Dwords4 v = {a, b, c, d};
        *reinterpret_cast<Dwords4 *>(out) = v;
    } else {
        Bytes16 v = {{a, b, c, d}};
        *reinterpret_cast<Bytes16 *>(out) = v;
    }
}
}  // namespace

__global__ __launch_bounds__(256) void watch_upscale_kernel(const uint8_t *src, int srows, int scols, const ResizeTap *taps,
                                                            const uint8_t *colormap, int flip, uint8_t *dst, int drows, int dcols) {
    extern __shared__ uint32_t lds[];
    const bool colour = colormap != nullptr;
    uint32_t *table = lds;                                          // [256] b | g << 8 | r << 16 (as the bytes lie in memory)
    uint8_t *band = reinterpret_cast<uint8_t *>(lds + (colour ? 256 : 0));
    const int y0 = blockIdx.y * kWatchTileRows, y1 = min(y0 + kWatchTileRows, drows);
    const uint8_t *img = src + (size_t) blockIdx.z * srows * scols;
    const int first = min(max(taps[dcols + y0].src, 0), srows - 1);           // source rows [first, last] cover the tile
    const int last = min(max(taps[dcols + y1 - 1].src + 1, 0), srows - 1);
    for (int i = threadIdx.x; i < (last - first + 1) * scols; i += 256) band[i] = img[(size_t) first * scols + i];
    if (colour) table[threadIdx.x] = colormap[3 * threadIdx.x] | colormap[3 * threadIdx.x + 1] << 8 | colormap[3 * threadIdx.x + 2] << 16;
    __syncthreads();

    const int channels = colour ? 3 : 1;
    const auto pixel = [&](const ResizeTap tx, const ResizeTap ty) -> uint32_t {  // a pixel's bytes as they go to memory
        const uint8_t *row0 = band + (min(max(ty.src, 0), srows - 1) - first) * scols;
        const uint8_t *row1 = band + (min(max(ty.src + 1, 0), srows - 1) - first) * scols;
        const int c0 = tx.src, c1 = min(tx.src + 1, scols - 1);
        const int S0 = row0[c0] * tx.w0 + row0[c1] * tx.w1;
        const int S1 = row1[c0] * tx.w0 + row1[c1] * tx.w1;
        const uint8_t v = resize_combine(S0, S1, ty.w0, ty.w1);
        return colour ? table[v] : v;
    };
    const int unit = blockIdx.x * 64 + (threadIdx.x & 63);
    if (dcols < kUnit) {  // narrower than one unit: lane x of a wave writes pixel x of the wave's rows
        if (unit >= dcols) return;
        const ResizeTap tx = taps[flip ? dcols - 1 - unit : unit];
        for (int dy = y0 + (threadIdx.x >> 6); dy < y1; dy += 4) {
            uint32_t px = pixel(tx, taps[dcols + dy]);
            uint8_t *out = dst + (((size_t) blockIdx.z * drows + dy) * dcols + unit) * channels;
#pragma unroll 1
            for (int c = 0; c < channels; c++, px >>= 8) out[c] = (uint8_t) px;
        }
        return;
    }
    if (unit * kUnit >= dcols) return;
    const int x0 = min(unit * kUnit, dcols - kUnit);  // (the row's last unit ends at its end)
    ResizeTap tx[kUnit];  // the column taps of this lane's pixels (of the mirrored ones when flip), kept over its rows
#pragma unroll
    for (int k = 0; k < kUnit; k++) tx[k] = taps[flip ? dcols - 1 - (x0 + k) : x0 + k];
    for (int dy = y0 + (threadIdx.x >> 6); dy < y1; dy += 4) {
        const ResizeTap ty = taps[dcols + dy];
        uint32_t px[kUnit];
#pragma unroll
        for (int k = 0; k < kUnit; k++) px[k] = pixel(tx[k], ty);
        uint8_t *out = dst + (((size_t) blockIdx.z * drows + dy) * dcols + x0) * channels;
        const bool dword_aligned = (reinterpret_cast<uintptr_t>(out) & 3) == 0;
        if (colour) {  // 16 x 3 bytes = 12 dwords: four pixels fill three
            uint32_t o[12];
#pragma unroll
            for (int g = 0; g < 4; g++) {
                o[3 * g + 0] = px[4 * g] | px[4 * g + 1] << 24;
                o[3 * g + 1] = px[4 * g + 1] >> 8 | px[4 * g + 2] << 16;
                o[3 * g + 2] = px[4 * g + 2] >> 16 | px[4 * g + 3] << 8;
            }
#pragma unroll
            for (int q = 0; q < 3; q++) store16(out + 16 * q, dword_aligned, o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
        } else {
            uint32_t o[4];
#pragma unroll
            for (int d = 0; d < 4; d++) o[d] = px[4 * d] | px[4 * d + 1] << 8 | px[4 * d + 2] << 16 | px[4 * d + 3] << 24;
            store16(out, dword_aligned, o[0], o[1], o[2], o[3]);
        }
    }
}

int watch_band_rows(const ResizeTap *row_taps, int srows, int drows) {
    int most = 1;
    for (int y0 = 0; y0 < drows; y0 += kWatchTileRows) {
        const int y1 = std::min(y0 + kWatchTileRows, drows);
        const int first = std::min(std::max(row_taps[y0].src, 0), srows - 1);
        const int last = std::min(std::max(row_taps[y1 - 1].src + 1, 0), srows - 1);
        most = std::max(most, last - first + 1);
    }
    return most;
}

hipError_t launch_watch_upscale(const uint8_t *d_src, int srows, int scols, int batch, const ResizeTap *d_taps, int band_rows,
                                const uint8_t *d_colormap, bool flip, uint8_t *d_dst, int drows, int dcols, hipStream_t stream) {
    if (srows < 1 || scols < 1 || batch < 1 || batch > 65535 || drows < 1 || dcols < 1 || band_rows < 1) return hipErrorInvalidValue;
    const size_t lds = (d_colormap ? 1024 : 0) + (((size_t) band_rows * scols + 15) & ~(size_t) 15);
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    const dim3 grid((dcols + 64 * kUnit - 1) / (64 * kUnit), (drows + kWatchTileRows - 1) / kWatchTileRows, batch);
    if (grid.y > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(watch_upscale_kernel, grid, dim3(256), lds, stream, d_src, srows, scols, d_taps, d_colormap, flip ? 1 : 0, d_dst,
                       drows, dcols);
    return hipGetLastError();
}

}  // namespace awpu
