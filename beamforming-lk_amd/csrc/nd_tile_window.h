// The tile windows of das_exact_nd_kernel's staging (host only, no device: awpu_sweep.cpp's build_quad_lut, and the planner's CPU test).
// A workgroup sweeps one tile per item and reads, of every mic's packed row, only the elements its pixels' delays reach: for mic slot s
// the elements start .. start + 255 + spread, start = the smallest (off - wstart) of the tile's pixels, spread = the largest less the
// smallest.  The LDS row is therefore wq_tile = 256 + (the widest spread of any tile and mic) elements instead of the whole row's wq,
// and a refill copies a row from its start on.  A tile here is 16 columns x 8 rows (two quad rows) for both shapes of the kernel: the
// one-quad shape's 4-row tile lies inside one, so one table of LDS addresses serves both.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace awpu {

// mics of a chunk: rows of wq_tile 16-byte elements that one LDS image of `image_bytes` holds, a multiple of four, at most 16 -- a chunk's
// rows are dealt one to a wave (a row is 4 KiB at least, so no more than 19 would fit anyway); < 4: the image does not hold the window
inline int nd_chunk_mics(int wq_tile, int image_bytes) { return std::min(16, (int) ((size_t) image_bytes / ((size_t) wq_tile * 16)) & ~3); }

inline int nd_window_tiles(int rows, int cols) { return (((rows + 3) / 4 + 1) / 2) * ((cols + 15) / 16); }

// off[pixel * lut_stride + mic]: the grid's delay offsets (rows x cols pixels); index[s]: the mic of active slot s < usable.  The tile's
// pixels are the quad table's: rows and columns past the grid clamped to its last.  Fills start[tile * usable_pad + s] (elements;
// padding slots 0) with start + wq_tile <= wq, and returns wq_tile (= wq with every start 0 where some tile spans the whole window).
inline int nd_tile_windows(const int32_t *off, int lut_stride, const int32_t *index, int usable, int usable_pad, int rows, int cols, int wstart, int wq,
                           std::vector<uint16_t> *start) {
    const int tiles_per_row = (cols + 15) / 16, tiles = nd_window_tiles(rows, cols);
    std::vector<int32_t> lo((size_t) tiles * usable_pad, 0);
    int spread = 0;
    for (int t = 0; t < tiles; t++) {
        const int r0 = 8 * (t / tiles_per_row), c0 = 16 * (t % tiles_per_row);
        for (int s = 0; s < usable; s++) {
            int mn = INT32_MAX, mx = INT32_MIN;
            for (int r = r0; r < r0 + 8; r++)
                for (int c = c0; c < c0 + 16; c++) {
                    const size_t p = (size_t) std::min(r, rows - 1) * cols + std::min(c, cols - 1);
                    const int v = off[p * lut_stride + index[s]] - wstart;
                    mn = std::min(mn, v);
                    mx = std::max(mx, v);
                }
            lo[(size_t) t * usable_pad + s] = mn;
            spread = std::max(spread, mx - mn);
        }
    }
    const int wq_tile = std::min(wq, 256 + spread);
    start->assign((size_t) tiles * usable_pad, 0);
    if (wq_tile < wq && wq - wq_tile <= 0xffff)
        for (size_t i = 0; i < lo.size(); i++) (*start)[i] = (uint16_t) std::min(lo[i], wq - wq_tile);
    return wq_tile < wq && wq - wq_tile <= 0xffff ? wq_tile : wq;
}

}  // namespace awpu
