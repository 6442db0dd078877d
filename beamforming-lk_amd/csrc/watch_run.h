// watch_run.h -- internal to libawpu_hip.so: what the runs that show every Nth block share (watch, find and locate runs in
// awpu_runs.cpp; spectral, exposed, coherence and peel runs in awpu_<feature>.cpp): the run structs, the display step, the
// staging and the history of a gathered piece, the watch run's consumer and the checks that read no handle.  Bodies: watch_run.cpp.
#pragma once

#include "run_pieces.h"

#include "awpu_hip_find.h"
#include "awpu_hip_focus.h"
#include "awpu_hip_watch.h"

#include <cstring>

#include "block_kernels.h"
#include "watch_kernels.h"

namespace awpu::host {

// ---- display images of every Nth block (kernels in watch_kernels.hip) ------------------------------------------------------------
// A piece is nf SHOWN frames, and its history holds only the blocks its snapshots read (watch_kernels.h: 4 + min(every, 4) *
// (nf - 1) slots of 256 samples), each piece's formed on its own: blocks from before the call out of the ring's snapshot, the
// rest staged and uploaded (host forms) or gathered out of the caller's samples (device form).  Behind a piece's sweep comes its
// display step: launch_heatmap for the whole piece, then the large image.  The ring's new snapshot is the last four blocks of
// the call: the tail of the last piece's history when the last block is shown, a four-slot history of its own (Piece::tail)
// otherwise.  A find run (awpu_hip_find.h) is a watch run whose display step is the peak pass: launch_find_peaks on the piece's
// powers, its counts and sources brought back (host forms) where the images would be.

// what a locate call (awpu_hip_focus.h) adds to a find run: behind a piece's peak pass, launch_range over every entry of its
// sources on the snapshots of the piece's history -- raw samples, whatever the sweep was given --, picked on the device.  ranges
// and range_power are host memory in the host forms, device memory in the device form
struct LocateRun {
    const double *distance = nullptr;  // [n_dist], host
    int32_t n_dist = 0;
    awpu_range_t *ranges = nullptr;    // [n_frames][max_sources]
    float *range_power = nullptr;      // [n_frames][max_sources][n_dist], or null
};

// what a find call adds to a watch run; sources and count are host memory in the host forms, device memory in the device form
struct FindRun {
    awpu_find_t f{};
    awpu_source_t *sources = nullptr;  // [n_frames][max_sources]
    int32_t *count = nullptr;          // [n_frames]
    const LocateRun *locate = nullptr;
};

struct WatchRun {
    awpu_watch_t w{};
    int n_frames = 0;
    uint8_t *image = nullptr, *big = nullptr;  // host memory in the host forms, device memory in the device form
    float *power = nullptr;
    const FindRun *find = nullptr;
};

// The display step: what happens to the nf rows of powers that a piece shows -- a watch piece's swept frames, the frames that
// closed inside an exposed piece --, for the outputs `wr` asks for.  The rows are on the device at d_rows, and j0 is the index of
// the first of them in the call's outputs.  The host forms write into scratch with a pinned twin and bring it back (fetch,
// deliver); the device form writes into the caller's arrays at j0 and keeps in scratch only what nobody asked for.  h->watch and
// h->find_out are laid out here and nowhere else.
struct Display {
    awpu_hip *const h;
    const WatchRun &wr;
    const awpu_watch_t &w;
    const FindRun *const fr;
    const LocateRun *const lr;
    const bool host, want_small;
    const size_t P, big_bytes;
    size_t small_off = 0, big_off = 0;  // in a watch buffer: the peaks, then the compact images, then the large ones
    size_t sources_off = 0;             // in a find buffer: the counts, then the sources
    size_t ranges_off = 0, rpower_off = 0;  // ... then (locate runs) the ranges and the candidates' powers; the device form keeps only the powers there, at 0

    Display(awpu_hip *h_, const WatchRun &wr_, bool host_);
    size_t source_bytes(int nf) const { return (size_t) nf * fr->f.max_sources * sizeof(awpu_source_t); }
    size_t rpower_bytes(int nf) const { return (size_t) nf * fr->f.max_sources * lr->n_dist * sizeof(float); }

    int check() const;
    // its buffers, for pieces that show at most piece_max rows
    int ensure(int piece_max, hipStream_t sw);
    // the range pass: launch_range over every entry of the rows' sources, picked on the device, on the rows' snapshots -- raw
    // samples, whatever the sweep was given --: row k's starts at hist + frame_step * k
    int range(int b, int j0, int nf, const awpu_source_t *d_sources, const float *hist, int hist_pitch, long long frame_step, hipStream_t s);
    // the peak pass, a locate run's range pass (a watch run's alone: its rows have snapshots, in `hist`), the compact image, the large one
    int show(int b, int j0, int nf, const float *d_rows, hipStream_t s, const float *hist = nullptr, int hist_pitch = 0, long long frame_step = 0);
    // host forms: into pinned memory, and on to the caller
    int fetch(int b, int nf, hipStream_t s);
    int deliver(int b, int j0, int nf);
};

// slots [q, slots) of a piece's history, slot s holding block block_of(s) of the call, into pinned blk_in.h[b]: tight datagrams,
// or rows of 256 * (slots - q)
template <class Map>
void stage_slots(awpu_hip *h, const BlockRun &src, const Map &block_of, int q, int slots, int b) {
    unsigned char *dst = h->blk_in.h[b];
    const int ns = slots - q;
    const size_t S = (size_t) h->cfg.n_streams, block_bytes = (size_t) awpu::kSamples * (src.wire ? (size_t) AWPU_DATAGRAM_BYTES : S * sizeof(float));
    parallel_ranges((size_t) ns, block_bytes * ns, [&](size_t lo, size_t hi) {
        for (size_t k = lo; k < hi; k++) {
            const size_t blk = (size_t) block_of(q + (int) k);
            if (src.wire) {
                const unsigned char *from = src.wire + blk * awpu::kSamples * src.stride;
                unsigned char *to = dst + k * awpu::kSamples * AWPU_DATAGRAM_BYTES;
                if (src.stride == AWPU_DATAGRAM_BYTES) {
                    std::memcpy(to, from, (size_t) awpu::kSamples * AWPU_DATAGRAM_BYTES);
                } else {
                    for (int i = 0; i < awpu::kSamples; i++) std::memcpy(to + (size_t) i * AWPU_DATAGRAM_BYTES, from + (size_t) i * src.stride, AWPU_DATAGRAM_BYTES);
                }
            } else {
                for (size_t s = 0; s < S; s++)
                    std::memcpy(dst + ((s * ns + k) * awpu::kSamples) * sizeof(float), src.samples + s * src.pitch + blk * awpu::kSamples,
                                awpu::kSamples * sizeof(float));
            }
        }
    });
}

// the history of a gathered piece (watch, exposure), whose slots [0, q) hold blocks from before the call: gather(src, src_pitch, n)
// fills slots [0, n) out of the ring's snapshot and src.  The device form: one gather out of the caller's samples; the host
// forms: [0, q) gathered, the rest -- staged and uploaded -- unpacked or copied in at slot q
template <class Gather>
int gathered_history(awpu_hip *h, const BlockRun &src, int b, int q, int slots, int pitch, hipStream_t s, const Gather &gather) {
    if (src.device) {
        AWPU_HIP_TRY(gather(src.samples, (long long) src.pitch, slots));
        return AWPU_OK;
    }
    const int S = h->cfg.n_streams;
    float *hist = hist_of(h, b);
    if (q > 0) AWPU_HIP_TRY(gather(nullptr, 0LL, q));
    if (src.wire) {
        AWPU_HIP_TRY(awpu::launch_unpack_blocks(h->blk_in.d[b], slots - q, S, hist, pitch, awpu::kSamples * q, s));
    } else {
        const long long n = (long long) awpu::kSamples * (slots - q);
        AWPU_HIP_TRY(awpu::launch_copy_rows(reinterpret_cast<const float *>(h->blk_in.d[b].get()), n, hist + awpu::kSamples * q, pitch, (int) n, S, s));
    }
    return AWPU_OK;
}

// what a run that forms no watch pieces ends with (the cross-spectral runs): the call's last four blocks into the ring, as a watch
// run's tail piece leaves them -- staged and uploaded (host forms), a history of four slots gathered, the ring written, ring_pos moved
int ring_tail(awpu_hip *h, const BlockRun &src, int n_blocks, hipStream_t s);

struct WatchPieces : Consumer {
    awpu_hip *const h;
    const BlockRun &src;
    const WatchRun &wr;
    const awpu_watch_t &w;
    const bool host;
    const int S, m;
    const size_t P;
    Display display;
    int lo = 0, width = 0;
    const float *snapshot = nullptr;    // blocks -4 .. -1 of the call

    WatchPieces(awpu_hip *h_, const BlockRun &src_, int n_blocks_, const WatchRun &wr_);
    // the blocks of a piece: its first shown block, the step, the slots of its history, and how many of them hold blocks from before the call
    struct Span {
        int b0, every, slots, q;
    };
    Span span(const Piece &p) const;

    int check() override { return display.check(); }
    int ensure(int piece_max, int lo_, int width_, hipStream_t sw) override;
    int staged_blocks(const Piece &p) override;
    int history(const Piece &p, hipStream_t s) override;
    int cut(const Piece &p, hipStream_t s) override;
    // shown frame j's snapshot starts at sample 256 * m * j of the history, as the cut reads it
    int show(const Piece &p, float *d_pow, long long, hipStream_t s) override {
        return display.show(p.b, p.first, p.n, d_pow, s, hist_of(h, p.b), pitch, (long long) awpu::kSamples * m);
    }
    int fetch_shown(const Piece &p, hipStream_t s) override { return display.fetch(p.b, p.n, s); }
    int deliver_shown(const Piece &p) override { return display.deliver(p.b, p.first, p.n); }
    int ring_from(const Piece &last) override { return last.tail ? 0 : awpu::kSamples * (awpu::watch_slots(w.every, last.n) - 4); }
};

// the find request of a call on the watch grid `w`: with sources and count or not at all, and then one find_peaks takes
int check_find_request(const awpu_watch_t *w, const awpu_find_t *f, const awpu_source_t *sources, const int32_t *count);

// the checks of a watch call that read no handle (any_output: something is asked for; big: a large image is), and what it shows
int check_watch(const awpu_watch_t *w, bool any_output, bool big, int n_blocks, WatchRun *wr);

// What exposed, coherence and peel runs open with: a watch run's outputs and an optional find request, refused in the order
// check_watch, the feature's own refusal() -- evaluated only once `w` has been checked --, check_find_request
struct ShownRun {
    WatchRun wr;
    FindRun find;
    template <class Refusal>
    int open(const awpu_watch_t *w, int n_blocks, const Refusal &refusal, const awpu_find_t *f, uint8_t *image, uint8_t *big, float *power,
             awpu_source_t *sources, int32_t *count, bool more_output = false) {
        if (int rc = check_watch(w, image || big || power || sources || count || more_output, big != nullptr, n_blocks, &wr)) return rc;
        if (const char *why = refusal()) return invalid(why);
        if (const int rc = check_find_request(w, f, sources, count)) return rc;
        if (f) find.f = *f, find.sources = sources, find.count = count;
        wr.image = image, wr.big = big, wr.power = power;
        wr.find = f ? &find : nullptr;
        return AWPU_OK;
    }
};

}  // namespace awpu::host
