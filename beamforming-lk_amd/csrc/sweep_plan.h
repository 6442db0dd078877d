// The plans of the sweep kernels' LDS images (host only, no device: awpu_sweep.cpp, the launchers of das_fast.hip, and the planners' CPU
// test).  A planner takes the window (samples any table entry can touch) and the active mics, and says how a mic's row is laid out, how
// many rows a chunk holds and what the table rows are padded to -- or that the window does not fit.  Pure integer arithmetic.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

namespace awpu {

constexpr int kSamples = 256;  // N_SAMPLES, src/fpga/streams.hpp:28

constexpr int kFastLdsBytes = 78 * 1024;  // one staged image; a CU holds two (+ a 4 KiB side table)
constexpr int kFastSideBytes = 4 * 1024;
constexpr int kFastLdsBytesSmall = 38 * 1024;                          // image of the two-workgroups-per-CU double-buffered shape
constexpr int kQuadhsRowTableOffset = (2 * kFastLdsBytes - 4096) / 4;  // floats: the last 4 KiB hold the streams' row offsets (das_quadh_stationary_kernel)
constexpr uint32_t kFirStaticPlaneBytesHost = 768;                     // = kFirStaticPlaneBytes of das_fast_trip.inc (static_assert in das_fast.hip)

// what a mic's staged row holds; one member per planner (and form of it)
enum class PackLayout {
    kSingle,              // fast_plan: single frames, the window staged twice (copy q shifted by q floats)
    kPairs,               // pair_plan: (frame 2k, frame 2k+1) sample pairs, chunked
    kPairsStationary,     // pair_plan_stationary: the same with every mic resident
    kFir8Planes,          // fir8_plane_plan: the frame pairs in four planes
    kNd,                  // exact_nd_plan: {next, d} elements of a frame pair
    kNdHalves,            // exact_ndh_plan: {next, d} elements of the two halves of one frame, chunked
    kNdHalvesStationary,  // ... with every mic resident
    kHalvesStationary,    // quadh_stationary_plan: (sample t, sample t + 128) pairs, every mic resident
};

struct FastPlan {
    PackLayout layout;
    int fpi;          // frames per item (1 or 2)
    int wr;           // elements per staged row
    int chunk;        // mics staged per pass (multiple of 4, <= 64; stationary layouts: usable_pad)
    int usable_pad;   // table row length, usable rounded up to 4 (null entries at the end)
    int row_bytes;    // of a row in the LDS image
    int image_bytes;  // kSingle: LDS bytes of one staged image (fast_image_bytes); the other layouts: 0
};

inline int pad4(int n) { return (n + 3) & ~3; }

// the chunk rule: mics whose rows of `row_bytes` one image of `image_bytes` holds -- a multiple of four (whole entry groups), at most
// `cap`, at most usable_pad; -1: the image does not hold four rows
inline int chunk_mics(size_t image_bytes, size_t row_bytes, int usable_pad, int cap = 64) {
    const int fit = std::min(cap, (int) (image_bytes / row_bytes) & ~3);
    return fit < 4 ? -1 : std::min(fit, usable_pad);
}
// ... and the plan of a layout whose chunk is known (chunk_mics, or usable_pad: every mic has its own slot); false: it does not fit
inline bool fill_plan(FastPlan *plan, PackLayout layout, int fpi, int wr, size_t row_bytes, int chunk, int usable_pad, int image_bytes = 0) {
    if (chunk < 0) return false;
    *plan = FastPlan{layout, fpi, wr, chunk, usable_pad, (int) row_bytes, image_bytes};
    return true;
}

// single frames (das_fast_kernel / das_fast_db_kernel): fpi in {1, 2} frames share an image of `image_bytes`, a mic takes two rows
inline bool fast_plan(int window, int usable, int fpi, int image_bytes, FastPlan *plan) {
    if (fpi != 1 && fpi != 2) return false;
    const int wr = (window + 3) & ~3;  // rows are whole 16-byte pieces (and start 16-byte aligned)
    const size_t row_bytes = (size_t) wr * sizeof(float);
    return fill_plan(plan, PackLayout::kSingle, fpi, wr, row_bytes, chunk_mics((size_t) image_bytes / fpi, 2 * row_bytes, pad4(usable)), pad4(usable), image_bytes);
}
// nw: 8 = 8-wave workgroups, 32 = the double-buffered 16-wave shape, 24 = double-buffered 12-wave workgroups, two per CU
inline int fast_image_bytes(int nw) { return nw == 24 ? kFastLdsBytesSmall : kFastLdsBytes; }
inline bool fast_db_fits(const FastPlan &plan) { return (size_t) 2 * plan.usable_pad * sizeof(int) <= (size_t) kFastSideBytes; }

// frame pairs: rows of wp 8-byte elements, whole 16-byte pieces
inline bool pair_plan(int window, int usable, FastPlan *plan) {
    const int wp = (window + 1) & ~1;
    return fill_plan(plan, PackLayout::kPairs, 2, wp, (size_t) wp * 8, chunk_mics(kFastLdsBytes, (size_t) wp * 8, pad4(usable)), pad4(usable));
}
// ... every active mic's window of a frame pair in the LDS at once (addresses are not folded into chunks; the null entries of padding
// mics point at row 0)
inline bool pair_plan_stationary(int window, int usable, FastPlan *plan) {
    const int wp = (window + 1) & ~1;
    const bool fits = (size_t) usable * wp * 8 <= (size_t) 2 * kFastLdsBytes;
    return fill_plan(plan, PackLayout::kPairsStationary, 2, wp, (size_t) wp * 8, fits ? pad4(usable) : -1, pad4(usable));
}

// FIR8: four planes of wp / 4 elements.  Windows of 321..384 samples (every BASELINE shape but the single 8x8 array) are staged at the
// plane pitch the one-address block is generated for (sweep_fir8_planes_static: 33 instead of 36 VALU instructions per item);
// AWPU_FIR8_STATIC=0 (tuning builds; das_kernels.h turns a timing build into one before it includes this header) keeps the natural
// pitch for A/B runs
inline bool fir8_plane_plan(int window, int usable, FastPlan *plan) {
    int wp = (window + 3) & ~3;
#ifdef AWPU_TUNING_BUILD
    static const bool allow_static = !(std::getenv("AWPU_FIR8_STATIC") && std::atoi(std::getenv("AWPU_FIR8_STATIC")) == 0);
#else
    constexpr bool allow_static = true;
#endif
    const int wp_static = (int) (kFirStaticPlaneBytesHost / 2);
    if (allow_static && wp > wp_static - 64 && wp <= wp_static) wp = wp_static;
    return fill_plan(plan, PackLayout::kFir8Planes, 2, wp, (size_t) wp * 8, chunk_mics(kFastLdsBytes, (size_t) wp * 8, pad4(usable)), pad4(usable));
}

// {next, d} elements of a frame pair: plan->wr = elements per packed row (element t holds X[t+1] and X[t] - X[t+1]: one less than
// samples); row_bytes = 16 wq_tile, the LDS row -- the window a tile reads (nd_tile_window.h; wq_tile <= 0: not known yet, or no tile
// reads less: whole rows); chunk <= 16, a row per wave
inline bool exact_nd_plan(int window, int usable, int wq_tile, FastPlan *plan) {
    const int wq = window - 1;
    if (wq_tile <= 0 || wq_tile > wq) wq_tile = wq;
    if (wq_tile < kSamples) return false;
    return fill_plan(plan, PackLayout::kNd, 2, wq, (size_t) wq_tile * 16, chunk_mics(kFastLdsBytes, (size_t) wq_tile * 16, pad4(usable), 16), pad4(usable));
}
// ... of the two halves of one frame: element t holds samples t, t+1, t+128, t+129 of the window (plan->wr = wh, row_bytes = 16 wh)
inline bool exact_ndh_plan(int window, int usable, bool stationary, FastPlan *plan) {
    const int wh = window - 129, usable_pad = pad4(usable);
    if (wh < kSamples / 2) return false;
    const size_t row_bytes = (size_t) wh * 16;
    const bool all_fit = usable_pad * row_bytes <= (size_t) 2 * kFastLdsBytes;
    const int chunk = stationary ? (all_fit ? usable_pad : -1) : chunk_mics(kFastLdsBytes, row_bytes, usable_pad);
    return fill_plan(plan, stationary ? PackLayout::kNdHalvesStationary : PackLayout::kNdHalves, 1, wh, row_bytes, chunk, usable_pad);
}

// the halves layout with every mic resident: rows of (sample t, sample t + 128) elements; the LDS holds the halves image + the raw rows
// it is filtered from (at most wp + 136 floats each) + the row table
inline bool quadh_stationary_plan(int window, int usable, FastPlan *plan) {
    const int wp = (window - 128 + 1) & ~1, usable_pad = pad4(usable);
    if (wp < 130) return false;
    const bool fits = (size_t) usable_pad * wp * 8 + (size_t) usable * (wp + 130) * 4 <= (size_t) kQuadhsRowTableOffset * 4;
    return fill_plan(plan, PackLayout::kHalvesStationary, 1, wp, (size_t) wp * 8, fits ? usable_pad : -1, usable_pad);
}
// the raw rows a launch stages: history samples [raw_begin, raw_begin + raw_wr) of every active stream, whole 16-byte pieces;
// false if they do not fit beside the image (the caller then takes das_quadh_kernel)
inline bool quadh_stationary_raw(const FastPlan &plan, int usable, int wstart, int row_limit, int *raw_begin, int *raw_wr, int *image_offset) {
    const int begin = std::max(0, wstart - 1) & ~3;
    const int end = std::min(row_limit, (wstart + plan.wr + 128 + 1 + 3) & ~3);
    if (end <= begin || ((end - begin) & 3)) return false;
    const size_t image_off = ((size_t) usable * (end - begin) + 3) & ~(size_t) 3;
    if (image_off * 4 + (size_t) plan.usable_pad * plan.row_bytes > (size_t) kQuadhsRowTableOffset * 4) return false;
    if (usable > 1024) return false;  // (the row table)
    *raw_begin = begin;
    *raw_wr = end - begin;
    *image_offset = (int) image_off;
    return true;
}

// Frame pairs an XCD works on at a time: as many as keep their samples (pair_bytes each) in its 4 MiB L2 beside the table stream.
// (Eight pairs at the headline shape, 5.9 MB of samples, run 1.2 % faster than four -- fewer table passes --
// but the samples then stream from beyond the L2: 3.2 GB of L2 misses per launch instead of 0.72 GB.  Not taken.)
// `forced`: AWPU_FAST_PAIRGROUP of the tuning builds.
inline int xcd_pair_group(size_t pair_bytes, int n_pairs, int forced = 0) {
    int g = forced > 0 ? forced : (int) std::max<size_t>(1, (3u << 20) / pair_bytes);
    g = g >= 8 ? 8 : g >= 4 ? 4 : g >= 2 ? 2 : 1;
    while (g > 1 && g > n_pairs) g >>= 1;
    return g;
}

}  // namespace awpu
