// The planner of das_exact_nd_kernel's tile windows (csrc/nd_tile_window.h) on a delay table read from a file, with no device:
//   nd_tile_window_check <file>      file = int32 { rows, cols, lut_stride, usable, wstart, wq, image_bytes }, then off[rows * cols * lut_stride],
//                                    then index[usable]
// Checks, for every pixel of every tile and every active mic, 0 <= off - wstart - start and off - wstart - start + 256 <= wq_tile, and
// start + wq_tile <= wq; prints "wq_tile=<n> chunk=<n> max_spread=<n> mean_spread=<x> ok" or the first violation.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nd_tile_window.h"

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[7];
    if (std::fread(head, sizeof(int32_t), 7, f) != 7) return 2;
    const int rows = head[0], cols = head[1], stride = head[2], usable = head[3], wstart = head[4], wq = head[5], image_bytes = head[6];
    std::vector<int32_t> off((size_t) rows * cols * stride), index(usable);
    if (std::fread(off.data(), sizeof(int32_t), off.size(), f) != off.size()) return 2;
    if (std::fread(index.data(), sizeof(int32_t), index.size(), f) != index.size()) return 2;
    std::fclose(f);
    const int usable_pad = (usable + 3) & ~3;
    std::vector<uint16_t> start;
    const int wq_tile = awpu::nd_tile_windows(off.data(), stride, index.data(), usable, usable_pad, rows, cols, wstart, wq, &start);
    const int tiles_per_row = (cols + 15) / 16, tiles = awpu::nd_window_tiles(rows, cols);
    if (start.size() != (size_t) tiles * usable_pad) return std::printf("start table: %zu entries\n", start.size()), 1;
    int max_spread = 0;
    double sum_spread = 0.0;
    for (int t = 0; t < tiles; t++)
        for (int s = 0; s < usable_pad; s++) {
            const int st = start[(size_t) t * usable_pad + s];
            if (s >= usable) {
                if (st != 0) return std::printf("padding slot %d of tile %d starts at %d\n", s, t, st), 1;
                continue;
            }
            if (st + wq_tile > wq) return std::printf("tile %d slot %d: start %d + %d > %d\n", t, s, st, wq_tile, wq), 1;
            int mn = 1 << 30, mx = -1;
            for (int r = 8 * (t / tiles_per_row); r < 8 * (t / tiles_per_row) + 8; r++)
                for (int c = 16 * (t % tiles_per_row); c < 16 * (t % tiles_per_row) + 16; c++) {
                    const size_t p = (size_t) (r < rows ? r : rows - 1) * cols + (c < cols ? c : cols - 1);
                    const int rel = off[p * stride + index[s]] - wstart - st;
                    if (rel < 0 || rel + 256 > wq_tile) return std::printf("tile %d slot %d pixel %zu: element %d of %d\n", t, s, p, rel, wq_tile), 1;
                    mn = rel < mn ? rel : mn;
                    mx = rel > mx ? rel : mx;
                }
            max_spread = mx - mn > max_spread ? mx - mn : max_spread;
            sum_spread += mx - mn;
        }
    std::printf("wq_tile=%d chunk=%d max_spread=%d mean_spread=%.2f ok\n", wq_tile, awpu::nd_chunk_mics(wq_tile, image_bytes), max_spread,
                sum_spread / ((double) tiles * usable));
    return 0;
}
