// run_pieces.h -- internal to libawpu_hip.so: the piece pipeline that every run of consecutive blocks goes through (run_pieces.cpp,
// where its protocol is described): where a run's samples come from, what a kind of run supplies as a Consumer, and the threaded
// copies of the host forms.  The kinds of run: awpu_runs.cpp, watch_run.h and the awpu_<feature>.cpp files.
#pragma once

#include "awpu_handle.h"

#include <algorithm>
#include <thread>
#include <vector>

namespace awpu::host {

// where a run's samples come from
struct BlockRun {
    const unsigned char *wire = nullptr;  // datagrams, `stride` bytes apart (host)
    int32_t stride = 0;
    const float *samples = nullptr;       // [n_streams][pitch] floats, host or (device) device memory
    int64_t pitch = 0;
    bool device = false;
};

// ... from a call's arguments, or what is wrong with them (none of these reads the handle)
int wire_source(const awpu_hip *h, const void *datagrams, int32_t stride_bytes, int32_t n_blocks, BlockRun *src);
int sample_source(const awpu_hip *h, const float *samples, int64_t pitch, int32_t n_blocks, bool device, BlockRun *src);

// fn(lo, hi) over [0, n) by up to 8 threads, each a contiguous share, when `bytes` (what the whole range copies) is 1 MB and
// more; where a thread cannot be started, the calling thread takes its share
template <class F>
void parallel_ranges(size_t n, size_t bytes, const F &fn) {
    const size_t n_threads = std::min<size_t>({8, n, bytes >> 20});
    if (n_threads < 2) {
        fn((size_t) 0, n);
        return;
    }
    std::vector<std::thread> pool;
    size_t k = 1;
    try {
        pool.reserve(n_threads - 1);
        for (; k < n_threads; k++) pool.emplace_back(fn, n * k / n_threads, n * (k + 1) / n_threads);
    } catch (...) {  // (std::system_error must not cross the C ABI)
    }
    fn((size_t) 0, n / n_threads);
    if (k < n_threads) fn(n * k / n_threads, n);
    for (auto &th : pool) th.join();
}

void parallel_copy(void *dst, const void *src, size_t bytes);

struct Piece {
    int i, b;      // i-th of the run, in the buffers b = i & 1
    int first, n;  // its items: blocks, or shown frames
    bool tail;     // the frameless last piece of a watch run: its history only feeds the ring
};

// what a consumer of a recording supplies to run_pieces
struct Consumer {
    int n_items = 0, n_blocks = 0;  // what is cut into pieces; the blocks the ring moves on by
    bool sweep = true;              // false: nothing is cut, swept or timed (listening without heatmaps)
    bool tail = false;              // a Piece::tail follows the last piece
    bool listens = false;           // steps 6, and 7 and 8 for what was heard
    bool whole_frames = false;      // the snapshots are cut whole (kFull) even where the window could be cut out: the sweep reads outside it (PeelPieces)
    float *power = nullptr;         // [n_items][pixel_count], per band: host memory in the host forms, device memory in the device form; or null
    BandSet bands;                  // in front of the sweeps: the handle's own band unless check() has set a spectral run's
    int pitch = 0;                  // floats per stream of a history (set by ensure)

    virtual int check() { return AWPU_OK; }  // refusals of its own, before the handle is made ready
    virtual int ensure(int piece_max, int lo, int width, hipStream_t sw) = 0;  // its buffers, for pieces of piece_max items
    virtual int begin(hipStream_t) { return AWPU_OK; }                         // on up, before the first history
    virtual int staged_blocks(const Piece &p) = 0;              // host forms: stages the input in blk_in.h[b]; the blocks to upload
    virtual int history(const Piece &p, hipStream_t s) = 0;     // blk_hist.d[b], out of blk_in.d[b] (host forms) or the caller's samples
    virtual int cut(const Piece &p, hipStream_t s) = 0;         // its snapshots' windows into d_blk_frames
    // the sweep of piece p's windows (one band's) into d_pow, untimed: launch(), unless the consumer sweeps otherwise (CoherePieces)
    virtual int sweep_frames(awpu_hip *h, const Piece &p, const float *d_frames, float *d_pow, hipStream_t s, int layout) {
        return launch(h, d_frames, p.n, d_pow, s, layout);
    }
    // behind the sweeps into d_pow (band b's powers `plane` floats behind band b-1's), before ev_blk_swept
    virtual int show(const Piece &, float *, long long, hipStream_t) { return AWPU_OK; }
    virtual int listen(const Piece &, hipStream_t) { return AWPU_OK; }
    virtual int fetch_shown(const Piece &, hipStream_t) { return AWPU_OK; }    // host forms: besides the powers, into pinned memory
    virtual int deliver_shown(const Piece &) { return AWPU_OK; }               // ... and on to the caller
    virtual int fetch_heard(const Piece &, hipStream_t) { return AWPU_OK; }
    virtual int deliver_heard(const Piece &) { return AWPU_OK; }
    virtual int ring_from(const Piece &last) = 0;               // the sample of the last history the ring's new snapshot starts at
    virtual int end(hipStream_t) { return AWPU_OK; }            // on li, behind the ring write

  protected:
    ~Consumer() = default;
};

inline float *hist_of(awpu_hip *h, int b) { return reinterpret_cast<float *>(h->blk_hist.d[b].get()); }

// the buffers every run needs for pieces of `piece` frames whose history and staging hold hist_blocks / in_blocks blocks (and,
// for the host forms, the second stream and the events)
int ensure_run_buffers(awpu_hip *h, const BlockRun &src, int piece, int width, bool sweep, int hist_blocks, int in_blocks, int planes);

// the run; the host forms are synchronous, the device form runs on `user` (NULL = h->stream)
int run_pieces(awpu_hip *h, const BlockRun &src, hipStream_t user, Consumer &c);

}  // namespace awpu::host
