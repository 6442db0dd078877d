// csm_run_plan.h -- the arithmetic of a cross-spectral run (awpu_csm_run.cpp), host only and over integers alone, so that a CPU
// test walks it (tests/host/csm_run_plan_check.cpp): how the run's scratch is laid out, which blocks a chunk takes and which
// frames it shows, and where in the spectra store a frame's window lies.
#pragma once
#include <algorithm>
#include <cstddef>

#include "sweep_plan.h"  // kSamples

namespace awpu {

constexpr int kBlocksPerLaunch = 1024;        // a recording is accumulated in pieces of so many blocks: what the spectra scratch holds
constexpr int kRunChunk = 256;                // a run takes at most so many NEW blocks a chunk
constexpr int kCsmRunDatagramBytes = 1032;    // AWPU_DATAGRAM_BYTES (awpu_csm_run.cpp asserts it)
constexpr int kCsmRunStepFloats = 3;          // sizeof(awpu_csm_clean_step_t) in floats (likewise)

inline int csm_run_chunk_blocks(int n_blocks) { return std::min(kRunChunk, n_blocks); }
// a piece: the frames of one display step, at most max_batch of them
inline int csm_run_piece(int n_frames, int max_batch) { return std::max(1, std::min(n_frames, max_batch)); }

// ---- the scratch: ten regions of one float buffer, in this order, each a multiple of 4 floats long ----------------------------
struct CsmRunRegion {
    size_t off, floats;
};
struct CsmRunShape {
    bool host, wire;  // the call's form: host memory (datagrams or samples) or the device form
    int n_streams, usable, n_bins, pixel_count, keep, chunk, piece;
    bool planes, solved, steps, power;  // the optional outputs asked for
    int clean_steps;                    // CLEAN-SC's steps, or 0
};
struct CsmRunLayout {
    CsmRunRegion spectra;  // the store: keep blocks in front of a chunk's
    CsmRunRegion carry;    // the host forms' carry (the device form's is the caller's)
    CsmRunRegion matrix, second;  // the frame's matrix; its inverse, or CLEAN-SC's working matrix
    CsmRunRegion rows;     // a piece's shown rows, where the caller's power does not take them
    CsmRunRegion planes;   // a piece's planes (host forms that ask), one frame's (nobody asked), none (the device form's are the caller's)
    CsmRunRegion solved, steps;  // a piece's solved words and step records on their way back (host forms)
    CsmRunRegion stage, wire;    // a chunk's samples [n_streams][256 * chunk] (host forms), and its datagrams
    size_t total;
};

inline CsmRunLayout csm_run_layout(const CsmRunShape &a) {
    const size_t K = (size_t) a.n_bins, U = (size_t) a.usable, P = (size_t) a.pixel_count, piece = (size_t) a.piece, chunk = (size_t) a.chunk;
    const size_t per_block = K * U * 2, matrix = K * U * U * 2;
    const size_t plane_frames = a.planes ? (a.host ? piece : 0) : 1;
    CsmRunLayout L{};
    size_t at = 0;
    const auto take = [&at](CsmRunRegion &r, size_t floats) { r.off = at, r.floats = (floats + 3) / 4 * 4, at += r.floats; };
    take(L.spectra, ((size_t) a.keep + chunk) * per_block);
    take(L.carry, a.host ? (size_t) a.keep * per_block : 0);
    take(L.matrix, matrix);
    take(L.second, matrix);
    take(L.rows, a.host || !a.power ? piece * P : 0);
    take(L.planes, plane_frames * K * P);
    take(L.solved, a.host && a.solved ? piece * K : 0);
    take(L.steps, a.host && a.steps ? piece * K * (size_t) a.clean_steps * kCsmRunStepFloats : 0);
    take(L.stage, a.host ? (size_t) a.n_streams * kSamples * chunk : 0);
    take(L.wire, a.wire ? (size_t) kSamples * chunk * kCsmRunDatagramBytes / sizeof(float) + 1 : 0);
    L.total = at;
    return L;
}

// ---- the walk: the chunk that starts at block c0 when j frames have been shown ends in front of block c1 and shows nf frames ---
struct CsmRunChunk {
    int c1, nf;
};
inline CsmRunChunk csm_run_chunk(int n_blocks, int first, int every, int n_frames, int piece, int c0, int j) {
    int c1 = std::min(c0 + csm_run_chunk_blocks(n_blocks), n_blocks), nf = 0;
    const auto shown = [&](int k) { return first + (j + k) * every; };
    while (j + nf < n_frames && nf < piece && shown(nf) < c1) nf++;
    if (j + nf < n_frames && shown(nf) < c1) c1 = shown(nf - 1) + 1;  // the piece is full: the chunk ends behind its last frame
    return {c1, nf};
}

// ---- a frame's window: blocks [lo, t] of the call (negative: carried in), n of them, from slot `slot` of the store on ---------
struct CsmRunWindow {
    int lo, n, slot;
};
inline CsmRunWindow csm_run_window(int t, int keep, int carried_in, int c0) {
    const int lo = std::max(t - keep, -carried_in);
    return {lo, t - lo + 1, keep + lo - c0};
}
// what the call leaves carried for the next one
inline int csm_run_carried(int carried_in, int n_blocks, int keep) { return (int) std::min<long long>((long long) carried_in + n_blocks, keep); }

}  // namespace awpu
