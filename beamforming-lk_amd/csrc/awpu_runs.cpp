// awpu_runs.cpp -- runs of consecutive blocks of a recording through one pipeline of pieces: a heatmap of every block
// (include/awpu_hip_blocks.h), the beam audio of every block (awpu_hip_listen.h), display images of every Nth block
// (awpu_hip_watch.h) -- in up to four bands at once (awpu_hip_spectral.h) --, the sources in every Nth block (awpu_hip_find.h), their distances (awpu_hip_focus.h), and all of a watch run's exposed over the blocks in front of every Nth (awpu_hip_expose.h) or swept by the coherence sweep (awpu_hip_cohere.h).  The handle and what is called here out of awpu_hip.cpp and awpu_sweep.cpp: awpu_handle.h.
#include "awpu_handle.h"
#include "awpu_hip_blocks.h"
#include "awpu_hip_cohere.h"
#include "awpu_hip_expose.h"
#include "awpu_hip_find.h"
#include "awpu_hip_focus.h"
#include "awpu_hip_listen.h"
#include "awpu_hip_spectral.h"
#include "awpu_hip_watch.h"

#include <algorithm>
#include <cstring>
#include <thread>
#include <vector>

#include "block_kernels.h"
#include "cohere_rule.h"
#include "peel_rule.h"
#include "expose_kernels.h"
#include "find_kernels.h"
#include "find_rule.h"
#include "spectral_kernels.h"
#include "spectral_rule.h"
#include "watch_kernels.h"

using namespace awpu::host;

namespace {

// where a run's samples come from
struct BlockRun {
    const unsigned char *wire = nullptr;  // datagrams, `stride` bytes apart (host)
    int32_t stride = 0;
    const float *samples = nullptr;       // [n_streams][pitch] floats, host or (device) device memory
    int64_t pitch = 0;
    bool device = false;
};

// ... from a call's arguments, or what is wrong with them (none of these reads the handle)
int wire_source(const awpu_hip *h, const void *datagrams, int32_t stride_bytes, int32_t n_blocks, BlockRun *src) {
    if (!h) return invalid("null handle");
    if (!datagrams) return invalid("null argument");
    if (n_blocks < 1) return invalid("n_blocks below 1");
    if (stride_bytes < AWPU_DATAGRAM_BYTES) return invalid("datagram stride below 1032 bytes");
    src->wire = static_cast<const unsigned char *>(datagrams);
    src->stride = stride_bytes;
    return AWPU_OK;
}

int sample_source(const awpu_hip *h, const float *samples, int64_t pitch, int32_t n_blocks, bool device, BlockRun *src) {
    if (!h) return invalid("null handle");
    if (!samples) return invalid("null argument");
    if (n_blocks < 1) return invalid("n_blocks below 1");
    if (pitch < (int64_t) awpu::kSamples * n_blocks) return invalid("pitch below 256 * n_blocks");
    src->samples = samples;
    src->pitch = pitch;
    src->device = device;
    return AWPU_OK;
}

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

void parallel_copy(void *dst, const void *src, size_t bytes) {
    parallel_ranges(bytes >> 16, bytes, [&](size_t lo, size_t hi) {  // 64 KB grains, the rest with the last
        const size_t from = lo << 16, to = hi == (bytes >> 16) ? bytes : hi << 16;
        std::memcpy(static_cast<unsigned char *>(dst) + from, static_cast<const unsigned char *>(src) + from, to - from);
    });
    if ((bytes >> 16) == 0) std::memcpy(dst, src, bytes);
}

// ---- the pipeline -----------------------------------------------------------------------------------------------------------
// A run is cut into chunks of at most max_batch items -- blocks, or the shown frames of a watch run --, and every chunk into the
// pieces awpu_hip_process sweeps a batch of that size in (host_piece): the same launches as that call on the same snapshots, so
// the same bits.  Piece i, in the buffers b = i & 1, gets a history on the device (blk_hist.d[b]: the samples its snapshots
// read), the snapshots' windows are cut out of it into the layout awpu_hip_process uploads (kCompact; kFull without a compact
// window) and swept by launch().  (Pieces rather than whole chunks: the first piece's staging is the one nothing hides, and the
// buffers are a piece long.)  Three streams: `sw` cuts and sweeps, `up` uploads, forms histories and fetches results, `li` runs
// the listen kernels beside the sweep of the same piece.  The host forms (sw = the handle's stream, up = copy_stream, li =
// listen_stream where the handle has one and the run is swept, else sw), per piece:
//   1. the host waits ev_blk_in[b] (i >= 2: piece i-2's upload is over), then stages the piece's input in pinned blk_in.h[b]
//   2. upload to blk_in.d[b] on up, ev_blk_in[b] behind it
//   3. up waits ev_blk_cut[b] (i >= 2, swept runs) and ev_listened[b] (i >= 2, listened runs): piece i-2 has read blk_hist.d[b]
//   4. the history is formed on up, ev_blk_hist[b] behind it; sw waits it, and li where that is another stream
//   5. the cut on sw, then ev_blk_cut[b]; ev_begin at piece 0; the sweep, untimed (the run's bracket spans the pieces); what the
//      consumer shows of the powers; ev_blk_swept[b].  With bands -- the handle's own (awpu_hip_band.h) or a spectral run's
//      (awpu_hip_spectral.h) -- the cut is their pre-pass, which cuts and filters in one (band_cut) into a plane of d_blk_frames
//      per band, and ev_begin stands in front of it; then one sweep per band, each the launch() of the band-by-band run, into a
//      plane of the powers per band; nothing else of a run sees the bands
//   6. the listen kernels on li, ev_listened[b] behind them
//   7. piece i-1's results into pinned memory on up, behind ev_blk_swept / ev_listened, ev_blk_out / ev_listen_out behind them
//      (so piece i-2's way back is queued on up before piece i's history is formed: listen_out.d[b] is free when 6 writes it)
//   8. piece i-2's results to the caller, once hipEventSynchronize on those events returns
// and at the end: ev_end; the ring as n_blocks ingests leave it, written on sw; the remaining fetches and deliveries; up and li
// synchronised; wait_and_time.  An error synchronises every stream: nothing of the call may still read the caller's buffers.
// The device form is asynchronous on the caller's stream (null: the handle's), which is sw, up and li at once: steps 4 to 6
// without the events, results written in place, the handle's stream ordered behind the ring write through ev_blk_ring.  Either
// form starts behind what is queued on the handle's stream (ev_blk_ring again): the ring's zeroing, a device-form run not over.

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

float *hist_of(awpu_hip *h, int b) { return reinterpret_cast<float *>(h->blk_hist.d[b].get()); }

// the buffers every run needs for pieces of `piece` frames whose history and staging hold hist_blocks / in_blocks blocks (and,
// for the host forms, the second stream and the events)
int ensure_run_buffers(awpu_hip *h, const BlockRun &src, int piece, int width, bool sweep, int hist_blocks, int in_blocks, int planes) {
    const size_t S = (size_t) h->cfg.n_streams, P = (size_t) h->cfg.pixel_count;
    int rc = h->blk_hist.ensure(S * (awpu::kBlockPrefix + (size_t) awpu::kSamples * hist_blocks) * sizeof(float), false);
    if (rc != AWPU_OK) return rc;
    const size_t frames_floats = sweep ? S * width * (size_t) piece * planes : 0;  // (a listen run without heatmaps cuts no window)
    if (rc = h->d_blk_frames.ensure(frames_floats); rc != AWPU_OK) return rc;
    if (rc = h->ev_blk_ring.ensure(); rc != AWPU_OK) return rc;
    if (src.device) return AWPU_OK;
    rc = h->blk_in.ensure((size_t) awpu::kSamples * in_blocks * (src.wire ? (size_t) AWPU_DATAGRAM_BYTES : S * sizeof(float)), true);
    if (rc == AWPU_OK) rc = h->blk_out.ensure(sweep ? piece * P * planes * sizeof(float) : 0, true, false);
    if (rc == AWPU_OK) rc = h->copy_stream.ensure();
    for (auto *pair : {h->ev_blk_in, h->ev_blk_hist, h->ev_blk_cut, h->ev_blk_swept, h->ev_blk_out})
        for (int b = 0; b < 2 && rc == AWPU_OK; b++) rc = pair[b].ensure();
    if (rc != AWPU_OK) return rc;
    return sweep ? ensure_power(h, 2 * piece * P * planes) : AWPU_OK;  // two pieces' powers: one swept, one on its way back
}

// the run; the host forms are synchronous, the device form runs on `user` (NULL = h->stream)
int run_pieces(awpu_hip *h, const BlockRun &src, hipStream_t user, Consumer &c) {
    if (is_group(h)) return fail(AWPU_ERR_STATE, "a device group does not take runs of blocks");
    if (h->in_flight) return fail(AWPU_ERR_STATE, "an awpu_hip_process_async call is in flight on this handle: awpu_hip_wait first");
    const awpu_hip_cfg &cfg = h->cfg;
    if (cfg.hist != AWPU_HIST) return invalid("runs of blocks need hist 1024");
    if (src.wire && cfg.n_streams > 256) return invalid("the wire carries at most 256 streams");
    int rc = c.check();
    if (rc != AWPU_OK) return rc;
    const int chunk = std::max(1, std::min<int>(c.n_items, cfg.max_batch));
    if (c.bands.n == 0) c.bands = own_band(h);
    const int planes = c.bands.planes();
    if (c.sweep) {
        rc = check_ready(h, chunk);
        if (rc != AWPU_OK) return rc;
        if (c.bands.max_taps() - 1 > h->wstart) return fail(AWPU_ERR_RANGE, kBandHistory);
    } else {
        AWPU_HIP_TRY(hipSetDevice(cfg.device));
    }
    std::vector<Piece> pieces;
    int piece_max = 1;
    for (int c0 = 0; c0 < c.n_items; c0 += chunk) {
        const int nc = std::min(chunk, c.n_items - c0), piece = host_piece(nc);
        for (int k0 = 0; k0 < nc; k0 += piece) {
            const int i = (int) pieces.size();
            pieces.push_back({i, i & 1, c0 + k0, std::min(piece, nc - k0), false});
            piece_max = std::max(piece_max, pieces.back().n);
        }
    }
    const int n_pieces = (int) pieces.size();  // ... with results
    if (c.tail) pieces.push_back({n_pieces, n_pieces & 1, 0, 0, true});
    const bool compact = h->compact_hist > 0 && !c.whole_frames, host = !src.device;
    const int S = cfg.n_streams;
    const size_t P = (size_t) cfg.pixel_count;
    hipStream_t sw = host ? h->stream : (user ? user : h->stream);
    rc = enter_stream(h, sw);  // behind the handle's last call, whatever stream that was on (up and li follow sw: ev_blk_ring, ev_blk_hist)
    if (rc == AWPU_OK) rc = ensure_ring(h);
    if (rc == AWPU_OK) rc = c.ensure(piece_max, compact ? h->wstart : 0, compact ? h->compact_hist : AWPU_HIST, sw);
    if (rc != AWPU_OK) return rc;
    hipStream_t up = host ? h->copy_stream : sw;
    hipStream_t li = host && c.sweep && h->listen_stream && env().listen_stream ? h->listen_stream : sw;
    // the device form is asynchronous: the caller times its own stream; nothing swept, nothing timed.  (The bracket is body()'s.)
    const bool time_it = host && c.sweep && n_pieces > 0;
    const auto fetch = [&](const Piece &p) -> int {
        if (c.sweep) {
            AWPU_HIP_TRY(hipStreamWaitEvent(up, h->ev_blk_swept[p.b], 0));
            if (c.power)  // (a piece's band planes lie back to back: p.n * P floats each)
                AWPU_HIP_TRY(hipMemcpyAsync(h->blk_out.h[p.b], h->d_power + (size_t) p.b * piece_max * P * planes, (size_t) p.n * P * planes * sizeof(float),
                                            hipMemcpyDeviceToHost, up));
            if (const int frc = c.fetch_shown(p, up)) return frc;
            AWPU_HIP_TRY(hipEventRecord(h->ev_blk_out[p.b], up));
        }
        if (c.listens) {
            AWPU_HIP_TRY(hipStreamWaitEvent(up, h->ev_listened[p.b], 0));
            if (const int frc = c.fetch_heard(p, up)) return frc;
            AWPU_HIP_TRY(hipEventRecord(h->ev_listen_out[p.b], up));
        }
        return AWPU_OK;
    };
    const auto deliver = [&](const Piece &p) -> int {
        if (c.sweep) {
            AWPU_HIP_TRY(hipEventSynchronize(h->ev_blk_out[p.b]));
            for (int k = 0; c.power && k < planes; k++)
                std::memcpy(c.power + ((size_t) k * c.n_items + p.first) * P, reinterpret_cast<const float *>(h->blk_out.h[p.b].get()) + (size_t) k * p.n * P,
                            (size_t) p.n * P * sizeof(float));
            if (const int drc = c.deliver_shown(p)) return drc;
        }
        if (c.listens) {
            AWPU_HIP_TRY(hipEventSynchronize(h->ev_listen_out[p.b]));
            if (const int drc = c.deliver_heard(p)) return drc;
        }
        return AWPU_OK;
    };
    const auto body = [&]() -> int {
        if (up != h->stream) {
            AWPU_HIP_TRY(hipEventRecord(h->ev_blk_ring, h->stream));
            AWPU_HIP_TRY(hipStreamWaitEvent(up, h->ev_blk_ring, 0));
        }
        int brc = c.begin(up);
        if (brc != AWPU_OK) return brc;
        const size_t block_bytes = (size_t) awpu::kSamples * (src.wire ? (size_t) AWPU_DATAGRAM_BYTES : S * sizeof(float));
        int fetched = 0, delivered = 0;
        for (const Piece &p : pieces) {
            const int i = p.i, b = p.b;
            if (host) {
                if (i >= 2) AWPU_HIP_TRY(hipEventSynchronize(h->ev_blk_in[b]));
                const size_t bytes = block_bytes * c.staged_blocks(p);
                AWPU_HIP_TRY(hipMemcpyAsync(h->blk_in.d[b], h->blk_in.h[b], bytes, hipMemcpyHostToDevice, up));
                AWPU_HIP_TRY(hipEventRecord(h->ev_blk_in[b], up));
                if (i >= 2 && c.sweep) AWPU_HIP_TRY(hipStreamWaitEvent(up, h->ev_blk_cut[b], 0));
                if (i >= 2 && c.listens) AWPU_HIP_TRY(hipStreamWaitEvent(up, h->ev_listened[b], 0));
            }
            brc = c.history(p, up);
            if (brc != AWPU_OK) return brc;
            if (host) {
                AWPU_HIP_TRY(hipEventRecord(h->ev_blk_hist[b], up));
                AWPU_HIP_TRY(hipStreamWaitEvent(sw, h->ev_blk_hist[b], 0));
                if (li != sw) AWPU_HIP_TRY(hipStreamWaitEvent(li, h->ev_blk_hist[b], 0));
            }
            if (c.sweep && !p.tail) {
                const bool banded = c.bands.n > 0;  // the cut is then the bands' pre-pass, and inside the timed span
                if (time_it && i == 0 && banded) AWPU_HIP_TRY(hipEventRecord(h->ev_begin, sw));
                brc = c.cut(p, sw);
                if (brc != AWPU_OK) return brc;
                if (host) AWPU_HIP_TRY(hipEventRecord(h->ev_blk_cut[b], sw));
                if (time_it && i == 0 && !banded) AWPU_HIP_TRY(hipEventRecord(h->ev_begin, sw));
                // band k's powers: in the caller's plane k (device form with powers), else p.n * P floats behind band k-1's
                float *d_pow = host ? h->d_power + (size_t) b * piece_max * P * planes : (c.power ? c.power + (size_t) p.first * P : h->d_power);
                const long long pow_plane = !host && c.power ? (long long) c.n_items * P : (long long) p.n * P;
                const size_t frames_plane = (size_t) S * (compact ? h->compact_hist : AWPU_HIST) * p.n;
                for (int k = 0; k < planes && brc == AWPU_OK; k++)
                    brc = c.sweep_frames(h, p, h->d_blk_frames + k * frames_plane, d_pow + k * pow_plane, sw, compact ? kCompact : kFull);
                if (brc == AWPU_OK) brc = c.show(p, d_pow, pow_plane, sw);
                if (brc != AWPU_OK) return brc;
                if (host) AWPU_HIP_TRY(hipEventRecord(h->ev_blk_swept[b], sw));
            }
            if (c.listens) {
                brc = c.listen(p, li);
                if (brc != AWPU_OK) return brc;
                if (host) AWPU_HIP_TRY(hipEventRecord(h->ev_listened[b], li));
            }
            if (host) {
                if (i >= 1 && fetched < n_pieces && (brc = fetch(pieces[fetched++])) != AWPU_OK) return brc;
                if (i >= 2 && delivered < n_pieces && (brc = deliver(pieces[delivered++])) != AWPU_OK) return brc;
            }
        }
        if (time_it) AWPU_HIP_TRY(hipEventRecord(h->ev_end, sw));
        const Piece &last = pieces.back();
        const int pos = (int) ((h->ring_pos + (long long) awpu::kSamples * c.n_blocks) % AWPU_HIST);
        AWPU_HIP_TRY(awpu::launch_ring_write(hist_of(h, last.b), c.pitch, c.ring_from(last), S, h->d_ring, pos, sw));
        h->ring_pos = pos;
        brc = c.end(li);
        if (brc != AWPU_OK) return brc;
        if (!host) {
            if (sw != h->stream) {  // later calls on the ring (the handle's stream) come after this one
                AWPU_HIP_TRY(hipEventRecord(h->ev_blk_ring, sw));
                AWPU_HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_blk_ring, 0));
            }
            if (c.listens) AWPU_HIP_TRY(hipStreamSynchronize(sw));  // the listeners' state is host memory
            return AWPU_OK;
        }
        while (fetched < n_pieces)
            if ((brc = fetch(pieces[fetched++])) != AWPU_OK) return brc;
        while (delivered < n_pieces)
            if ((brc = deliver(pieces[delivered++])) != AWPU_OK) return brc;
        AWPU_HIP_TRY(hipStreamSynchronize(up));
        if (li != sw) AWPU_HIP_TRY(hipStreamSynchronize(li));
        return wait_and_time(h, time_it);
    };
    rc = body();
    if (rc != AWPU_OK && host) {
        (void) hipStreamSynchronize(h->copy_stream);
        if (h->listen_stream) (void) hipStreamSynchronize(h->listen_stream);
        (void) hipStreamSynchronize(h->stream);
    }
    return rc;
}

// ---- a heatmap of every block, and listening (kernels in block_kernels.hip, track_kernels.hip) ---------------------------------
// A piece is nb consecutive blocks.  Its history [n_streams][768 + 256 * piece] continues the one before it: the 768 samples
// before the piece (the ring's snapshot for the first piece, the tail of piece i-1's history after it), then its new samples.

// What a listen call adds to a run; audio and trail are host memory in the host forms, device memory in the device form.  Per
// piece, between its history and the ring write: the listen kernels on that history.
struct ListenRun {
    awpu_particle_t *listeners = nullptr;  // host, in/out
    int32_t n = 0;
    double theta_limit = 0.0, reference = 0.0;
    float *audio = nullptr;
    int64_t audio_pitch = 0;
    awpu_particle_t *trail = nullptr;
};

// blocks [g0, g0 + nb) of a host form into pinned staging blk_in.h[b]: tight datagrams, or rows of 256 * nb samples (the
// headline's 32-block pieces: 8.4 MB, 8 threads)
void stage_blocks(awpu_hip *h, const BlockRun &src, int g0, int nb, int b) {
    unsigned char *dst = h->blk_in.h[b];
    const size_t n = (size_t) awpu::kSamples * nb;
    const size_t rows = src.wire ? n : (size_t) h->cfg.n_streams;
    parallel_ranges(rows, n * (src.wire ? (size_t) AWPU_DATAGRAM_BYTES : rows * sizeof(float)), [&](size_t r0, size_t r1) {
        if (src.wire) {
            const unsigned char *from = src.wire + (size_t) g0 * awpu::kSamples * src.stride;
            if (src.stride == AWPU_DATAGRAM_BYTES) {
                std::memcpy(dst + r0 * AWPU_DATAGRAM_BYTES, from + r0 * AWPU_DATAGRAM_BYTES, (r1 - r0) * AWPU_DATAGRAM_BYTES);
            } else {
                for (size_t i = r0; i < r1; i++) std::memcpy(dst + i * AWPU_DATAGRAM_BYTES, from + i * src.stride, AWPU_DATAGRAM_BYTES);
            }
            return;
        }
        for (size_t s = r0; s < r1; s++)
            std::memcpy(dst + s * n * sizeof(float), src.samples + s * src.pitch + (size_t) g0 * awpu::kSamples, n * sizeof(float));
    });
}

struct BlockPieces final : Consumer {
    awpu_hip *const h;
    const BlockRun &src;
    const ListenRun *const ls;
    const bool host;
    const size_t state;  // bytes of the listeners
    bool tracking = false, fixed = false;
    std::vector<awpu_particle_t> heard;  // the listeners after the run
    int lo = 0, width = 0;
    const float *prev = nullptr;  // the 768 samples before the next piece
    long long prev_pitch = 2048;

    BlockPieces(awpu_hip *h_, const BlockRun &src_, int n_blocks_, float *power_, const ListenRun *ls_)
        : h(h_), src(src_), ls(ls_), host(!src_.device), state(ls_ ? (size_t) ls_->n * sizeof(awpu_particle_t) : 0), heard(ls_ ? ls_->n : 0) {
        n_items = n_blocks = n_blocks_;
        power = power_;
        listens = ls != nullptr;
        sweep = !ls || power;
        for (int l = 0; ls && l < ls->n; l++) (ls->listeners[l].steps > 0 ? tracking : fixed) = true;
    }
    size_t audio_bytes(int nb) const { return align16((size_t) ls->n * awpu::kSamples * nb * sizeof(float)); }

    int check() override { return ls ? check_antenna(h) : AWPU_OK; }
    int ensure(int piece_max, int lo_, int width_, hipStream_t) override {
        lo = lo_, width = width_;
        pitch = awpu::kBlockPrefix + awpu::kSamples * piece_max;
        prev = h->d_ring + h->ring_pos + awpu::kSamples;  // the last 768 samples of the current snapshot
        int rc = ensure_run_buffers(h, src, piece_max, width, sweep, piece_max, piece_max, bands.planes());
        if (rc != AWPU_OK || !ls) return rc;
        rc = ensure_track_index(h);
        if (rc != AWPU_OK) return rc;
        // the listeners' state, and for the host forms the way back of a piece's audio rows [n][256 * piece] and trail
        if (rc = h->d_listeners.ensure(state); rc != AWPU_OK) return rc;
        if (!host) return AWPU_OK;
        rc = h->listen_out.ensure(audio_bytes(piece_max) + (size_t) piece_max * state, true);
        if (rc != AWPU_OK) return rc;
        if (sweep && env().listen_stream) rc = h->listen_stream.ensure();
        for (auto *pair : {h->ev_listened, h->ev_listen_out})
            for (int b = 0; b < 2 && rc == AWPU_OK; b++) rc = pair[b].ensure();
        return rc;
    }
    int begin(hipStream_t s) override {
        if (ls) AWPU_HIP_TRY(hipMemcpyAsync(h->d_listeners, ls->listeners, state, hipMemcpyHostToDevice, s));
        return AWPU_OK;
    }
    int staged_blocks(const Piece &p) override {
        stage_blocks(h, src, p.first, p.n, p.b);
        return p.n;
    }
    int history(const Piece &p, hipStream_t s) override {
        const int S = h->cfg.n_streams;
        float *hist = hist_of(h, p.b);
        AWPU_HIP_TRY(awpu::launch_copy_rows(prev, prev_pitch, hist, pitch, awpu::kBlockPrefix, S, s));
        if (src.wire) {
            AWPU_HIP_TRY(awpu::launch_unpack_blocks(h->blk_in.d[p.b], p.n, S, hist, pitch, awpu::kBlockPrefix, s));
        } else {
            const float *rows = host ? reinterpret_cast<const float *>(h->blk_in.d[p.b].get()) : src.samples + (size_t) p.first * awpu::kSamples;
            AWPU_HIP_TRY(awpu::launch_copy_rows(rows, host ? (long long) awpu::kSamples * p.n : (long long) src.pitch,
                                                hist + awpu::kBlockPrefix, pitch, awpu::kSamples * p.n, S, s));
        }
        prev = hist + (size_t) awpu::kSamples * p.n;
        prev_pitch = pitch;
        return AWPU_OK;
    }
    int cut(const Piece &p, hipStream_t s) override {
        if (bands.n) return band_cut(h, bands, hist_of(h, p.b), awpu::kSamples, pitch, h->wstart, p.n, h->d_blk_frames, (long long) h->cfg.n_streams * width * p.n, h->compact_hist > 0 ? kCompact : kFull, s);
        AWPU_HIP_TRY(awpu::launch_cut_windows(hist_of(h, p.b), pitch, h->cfg.n_streams, p.n, lo, width, h->d_blk_frames, s));
        return AWPU_OK;
    }
    int listen(const Piece &p, hipStream_t s) override {
        awpu::ListenArgs a{};
        a.hist = hist_of(h, p.b);
        a.pitch = pitch;
        a.n_blocks = p.n;
        a.xyz = h->d_xyz;
        a.n = (int) (h->antenna.size() / 3);
        a.index = h->d_track_index;
        a.usable = h->usable();
        a.listeners = h->d_listeners;
        a.n_listeners = ls->n;
        a.theta_limit = ls->theta_limit;
        a.reference = ls->reference;
        if (host) {
            a.audio = reinterpret_cast<float *>(h->listen_out.d[p.b].get());
            a.audio_pitch = (long long) awpu::kSamples * p.n;
            a.trail = ls->trail ? h->listen_out.d[p.b] + audio_bytes(p.n) : nullptr;
        } else {
            a.audio = ls->audio + (size_t) awpu::kSamples * p.first;
            a.audio_pitch = ls->audio_pitch;
            a.trail = ls->trail ? ls->trail + (size_t) p.first * ls->n : nullptr;
        }
        AWPU_HIP_TRY(awpu::launch_listen(a, tracking, fixed, s));
        return AWPU_OK;
    }
    int fetch_heard(const Piece &p, hipStream_t s) override {
        AWPU_HIP_TRY(hipMemcpyAsync(h->listen_out.h[p.b], h->listen_out.d[p.b], audio_bytes(p.n) + (ls->trail ? (size_t) p.n * state : 0),
                                    hipMemcpyDeviceToHost, s));
        return AWPU_OK;
    }
    int deliver_heard(const Piece &p) override {
        const unsigned char *from = h->listen_out.h[p.b];
        const size_t row = (size_t) awpu::kSamples * p.n;
        for (int l = 0; l < ls->n; l++)
            std::memcpy(ls->audio + (size_t) l * ls->audio_pitch + (size_t) awpu::kSamples * p.first, from + l * row * sizeof(float), row * sizeof(float));
        if (ls->trail) std::memcpy(ls->trail + (size_t) p.first * ls->n, from + audio_bytes(p.n), (size_t) p.n * state);
        return AWPU_OK;
    }
    // the ring's snapshot = the last 1024 samples of the last history
    int ring_from(const Piece &last) override { return awpu::kSamples * (last.n - 1); }
    int end(hipStream_t s) override {
        if (ls) AWPU_HIP_TRY(hipMemcpyAsync(heard.data(), h->d_listeners, state, hipMemcpyDeviceToHost, s));
        return AWPU_OK;
    }
};

// `power`: [n_blocks][pixel_count], host memory in the host forms, device memory in the device form.  With `ls` the run is
// listened to as well, and swept only if powers are asked for.
int run_blocks(awpu_hip *h, const BlockRun &src, int n_blocks, float *power, hipStream_t user, const ListenRun *ls = nullptr) {
    BlockPieces c(h, src, n_blocks, power, ls);
    const int rc = run_pieces(h, src, user, c);
    if (rc == AWPU_OK && ls) std::memcpy(ls->listeners, c.heard.data(), c.state);
    return rc;
}

// the checks of a listen call that read no handle; then the run
int listen_run(awpu_hip *h, const BlockRun &src, int n_blocks, awpu_particle_t *listeners, int32_t n, double theta_limit, double reference,
               float *audio, int64_t audio_pitch, awpu_particle_t *trail, float *power, hipStream_t user) {
    if (!listeners || !audio) return invalid("null argument");
    if (int rc = check_particles(listeners, n, theta_limit, reference)) return rc;
    if (audio_pitch < (int64_t) awpu::kSamples * n_blocks) return invalid("audio_pitch below 256 * n_blocks");
    AWPU_CTX(h);
    const ListenRun ls{listeners, n, theta_limit, reference, audio, audio_pitch, trail};
    return run_blocks(h, src, n_blocks, power, user, &ls);
}

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

    Display(awpu_hip *h_, const WatchRun &wr_, bool host_)
        : h(h_), wr(wr_), w(wr_.w), fr(wr_.find), lr(wr_.find ? wr_.find->locate : nullptr), host(host_), want_small(wr_.image || wr_.big),
          P((size_t) h_->cfg.pixel_count), big_bytes((size_t) wr_.w.out_rows * wr_.w.out_cols * (wr_.w.d_colormap ? 3 : 1)) {}
    size_t source_bytes(int nf) const { return (size_t) nf * fr->f.max_sources * sizeof(awpu_source_t); }
    size_t rpower_bytes(int nf) const { return (size_t) nf * fr->f.max_sources * lr->n_dist * sizeof(float); }

    int check() const {
        if (h->cfg.pixel_count != h->cfg.n_pixels) return invalid("the display step needs the whole grid on this handle");
        if ((long long) w.rows * w.cols != h->cfg.n_pixels) return invalid("rows x cols must be the grid");
        return lr ? check_antenna(h) : (int) AWPU_OK;
    }
    // its buffers, for pieces that show at most piece_max rows
    int ensure(int piece_max, hipStream_t sw) {
        small_off = align16(sizeof(float) * piece_max), big_off = small_off + align16((size_t) piece_max * P);
        sources_off = align16(sizeof(int32_t) * piece_max);
        int rc = want_small ? h->watch.ensure(big_off + (host && wr.big ? (size_t) piece_max * big_bytes : 0), host) : (int) AWPU_OK;
        if (rc == AWPU_OK && wr.big) rc = ensure_taps(h, w.rows, w.cols, w.out_rows, w.out_cols, sw);
        if (rc != AWPU_OK || !fr) return rc;
        if (!lr) return host ? h->find_out.ensure(sources_off + source_bytes(piece_max), true) : (int) AWPU_OK;
        ranges_off = sources_off + align16(source_bytes(piece_max));
        rpower_off = host ? ranges_off + (size_t) piece_max * fr->f.max_sources * sizeof(awpu_range_t) : 0;
        rc = ensure_track_index(h);
        if (rc == AWPU_OK && (host || !lr->range_power)) rc = h->find_out.ensure(rpower_off + rpower_bytes(piece_max), host);
        return rc;
    }
    // the range pass: launch_range over every entry of the rows' sources, picked on the device, on the rows' snapshots -- raw
    // samples, whatever the sweep was given --: row k's starts at hist + frame_step * k
    int range(int b, int j0, int nf, const awpu_source_t *d_sources, const float *hist, int hist_pitch, long long frame_step, hipStream_t s) {
        const int ms = fr->f.max_sources;
        unsigned char *out = h->find_out.d[host ? b : 0];
        awpu::RangeArgs a{};
        a.frame_step = frame_step;
        a.per_frame = ms;
        a.pitch = hist_pitch;
        a.xyz = h->d_xyz;
        a.n = (int) (h->antenna.size() / 3);
        a.index = h->d_track_index;
        a.usable = h->usable();
        a.n_dist = lr->n_dist;
        for (int j = 0; j < lr->n_dist; j++) a.distance[j] = lr->distance[j];
        float *d_rpower = host || !lr->range_power ? reinterpret_cast<float *>(out + rpower_off) : lr->range_power + (size_t) j0 * ms * lr->n_dist;
        awpu_range_t *d_ranges = host ? reinterpret_cast<awpu_range_t *>(out + ranges_off) : lr->ranges + (size_t) j0 * ms;
        for (int k0 = 0; k0 < nf; k0 += 1024) {  // (a launch's grid: at most 65535 sources)
            a.frame = hist + (size_t) k0 * frame_step;
            a.sources = d_sources + (size_t) k0 * ms;
            a.n_src = std::min(1024, nf - k0) * ms;
            a.power = d_rpower + (size_t) k0 * ms * lr->n_dist;
            a.best = d_ranges + (size_t) k0 * ms;
            AWPU_HIP_TRY(awpu::launch_range(a, s));
        }
        return AWPU_OK;
    }
    // the peak pass, a locate run's range pass (a watch run's alone: its rows have snapshots, in `hist`), the compact image, the large one
    int show(int b, int j0, int nf, const float *d_rows, hipStream_t s, const float *hist = nullptr, int hist_pitch = 0, long long frame_step = 0) {
        if (nf == 0) return AWPU_OK;
        if (fr) {
            unsigned char *out = h->find_out.d[b];
            awpu_source_t *d_sources = host ? reinterpret_cast<awpu_source_t *>(out + sources_off) : fr->sources + (size_t) j0 * fr->f.max_sources;
            AWPU_HIP_TRY(awpu::launch_find_peaks(d_rows, nf, fr->f, d_sources, host ? reinterpret_cast<int32_t *>(out) : fr->count + j0, s));
            if (lr)
                if (const int rc = range(b, j0, nf, d_sources, hist, hist_pitch, frame_step, s)) return rc;
        }
        if (!want_small) return AWPU_OK;
        uint8_t *scratch = h->watch.d[host ? b : 0];
        uint8_t *d_small = host || !wr.image ? scratch + small_off : wr.image + (size_t) j0 * P;
        AWPU_HIP_TRY(awpu::launch_heatmap(d_rows, (int) P, nf, reinterpret_cast<float *>(scratch), false, d_small, s));
        if (wr.big)
            AWPU_HIP_TRY(awpu::launch_watch_upscale(d_small, w.rows, w.cols, nf, h->d_taps, h->taps_band_rows, w.d_colormap, w.flip != 0,
                                                    host ? scratch + big_off : wr.big + (size_t) j0 * big_bytes, w.out_rows, w.out_cols, s));
        return AWPU_OK;
    }
    // host forms: into pinned memory, and on to the caller
    int fetch(int b, int nf, hipStream_t s) {
        if (nf == 0) return AWPU_OK;
        if (fr)
            AWPU_HIP_TRY(hipMemcpyAsync(h->find_out.h[b], h->find_out.d[b], lr ? rpower_off + rpower_bytes(nf) : sources_off + source_bytes(nf),
                                        hipMemcpyDeviceToHost, s));
        uint8_t *to = h->watch.h[b], *from = h->watch.d[b];
        if (wr.image) AWPU_HIP_TRY(hipMemcpyAsync(to + small_off, from + small_off, (size_t) nf * P, hipMemcpyDeviceToHost, s));
        if (wr.big) AWPU_HIP_TRY(hipMemcpyAsync(to + big_off, from + big_off, (size_t) nf * big_bytes, hipMemcpyDeviceToHost, s));
        return AWPU_OK;
    }
    int deliver(int b, int j0, int nf) {
        if (nf == 0) return AWPU_OK;
        if (fr) {
            std::memcpy(fr->count + j0, h->find_out.h[b], sizeof(int32_t) * nf);
            std::memcpy(fr->sources + (size_t) j0 * fr->f.max_sources, h->find_out.h[b] + sources_off, source_bytes(nf));
        }
        if (lr) {
            const size_t entries = (size_t) j0 * fr->f.max_sources;
            std::memcpy(lr->ranges + entries, h->find_out.h[b] + ranges_off, (size_t) nf * fr->f.max_sources * sizeof(awpu_range_t));
            if (lr->range_power) std::memcpy(lr->range_power + entries * lr->n_dist, h->find_out.h[b] + rpower_off, rpower_bytes(nf));
        }
        if (wr.image) std::memcpy(wr.image + (size_t) j0 * P, h->watch.h[b] + small_off, (size_t) nf * P);
        if (wr.big) parallel_copy(wr.big + (size_t) j0 * big_bytes, h->watch.h[b] + big_off, (size_t) nf * big_bytes);
        return AWPU_OK;
    }
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

// ... of a watch piece (watch_kernels.h)
void stage_watch(awpu_hip *h, const BlockRun &src, int b0, int every, int q, int slots, int b) {
    const int m = std::min(every, 4);
    stage_slots(h, src, [=](int slot) { return awpu::watch_slot_block(slot, b0, every, m); }, q, slots, b);
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

    WatchPieces(awpu_hip *h_, const BlockRun &src_, int n_blocks_, const WatchRun &wr_)
        : h(h_), src(src_), wr(wr_), w(wr_.w), host(!src_.device), S(h_->cfg.n_streams), m(std::min(wr_.w.every, 4)), P((size_t) h_->cfg.pixel_count),
          display(h_, wr_, !src_.device) {
        n_items = wr.n_frames;
        n_blocks = n_blocks_;
        power = wr.power;
        // the last block of the call shown: the ring's new snapshot is the tail of the last piece's history
        tail = n_items == 0 || w.first + (n_items - 1) * w.every != n_blocks - 1;
    }
    // the blocks of a piece: its first shown block, the step, the slots of its history, and how many of them hold blocks from before the call
    struct Span {
        int b0, every, slots, q;
    };
    Span span(const Piece &p) const {
        const int b0 = p.tail ? n_blocks - 1 : w.first + p.first * w.every, every = p.tail ? 1 : w.every;
        return {b0, every, awpu::watch_slots(every, p.tail ? 1 : p.n), std::max(0, std::min(3 - b0, 4))};
    }

    int check() override { return display.check(); }
    int ensure(int piece_max, int lo_, int width_, hipStream_t sw) override {
        lo = lo_, width = width_;
        const int slots_max = awpu::watch_slots(w.every, piece_max);
        pitch = awpu::kSamples * slots_max;
        snapshot = h->d_ring + h->ring_pos;
        int rc = ensure_run_buffers(h, src, piece_max, width, true, slots_max - 3, slots_max, bands.planes());
        if (rc == AWPU_OK && !host && !wr.power) rc = ensure_power(h, (size_t) piece_max * P * bands.planes());
        return rc != AWPU_OK ? rc : display.ensure(piece_max, sw);
    }
    int staged_blocks(const Piece &p) override {
        const Span g = span(p);
        stage_watch(h, src, g.b0, g.every, g.q, g.slots, p.b);
        return g.slots - g.q;
    }
    int history(const Piece &p, hipStream_t s) override {
        const Span g = span(p);
        return gathered_history(h, src, p.b, g.q, g.slots, pitch, s, [&](const float *from, long long from_pitch, int n) {
            return awpu::launch_watch_gather(from, from_pitch, snapshot, g.b0, g.every, S, hist_of(h, p.b), pitch, 0, n, s);
        });
    }
    int cut(const Piece &p, hipStream_t s) override {
        if (bands.n) return band_cut(h, bands, hist_of(h, p.b), awpu::kSamples * m, pitch, h->wstart, p.n, h->d_blk_frames, (long long) S * width * p.n, h->compact_hist > 0 ? kCompact : kFull, s);
        AWPU_HIP_TRY(awpu::launch_watch_cut(hist_of(h, p.b), pitch, S, p.n, awpu::kSamples * m, lo, width, h->d_blk_frames, s));
        return AWPU_OK;
    }
    // shown frame j's snapshot starts at sample 256 * m * j of the history, as the cut reads it
    int show(const Piece &p, float *d_pow, long long, hipStream_t s) override {
        return display.show(p.b, p.first, p.n, d_pow, s, hist_of(h, p.b), pitch, (long long) awpu::kSamples * m);
    }
    int fetch_shown(const Piece &p, hipStream_t s) override { return display.fetch(p.b, p.n, s); }
    int deliver_shown(const Piece &p) override { return display.deliver(p.b, p.first, p.n); }
    int ring_from(const Piece &last) override { return last.tail ? 0 : awpu::kSamples * (awpu::watch_slots(w.every, last.n) - 4); }
};

// the find request of a call on the watch grid `w`: with sources and count or not at all, and then one find_peaks takes
int check_find_request(const awpu_watch_t *w, const awpu_find_t *f, const awpu_source_t *sources, const int32_t *count) {
    if (!sources != !count) return invalid("sources and count come together");
    if (!f != !sources) return invalid("a find request exactly when sources and count are asked for");
    if (!f) return AWPU_OK;
    if (const char *why = awpu::find_refusal(f)) return invalid(why);
    if (f->rows != w->rows || f->cols != w->cols) return invalid("the find grid must be the watch grid");
    return AWPU_OK;
}

// the checks of a watch call that read no handle (any_output: something is asked for; big: a large image is), and what it shows
int check_watch(const awpu_watch_t *w, bool any_output, bool big, int n_blocks, WatchRun *wr) {
    if (!w) return invalid("null argument");
    if (!any_output) return invalid("no output asked for");
    if (w->every < 1 || w->every > AWPU_WATCH_MAX_EVERY) return invalid("every outside [1, 1024]");
    if (w->first < 0) return invalid("first below 0");
    if (w->flip != 0 && w->flip != 1) return invalid("flip is 0 or 1");
    if (w->rows < 1 || w->cols < 1) return invalid("rows and cols must be positive");
    if (big && (w->out_rows < w->rows || w->out_cols < w->cols)) return invalid("upscale only: out >= in");
    if (big && w->cols > AWPU_WATCH_MAX_COLS) return invalid("compact image wider than AWPU_WATCH_MAX_COLS");
    wr->w = *w;
    int32_t next_first = 0;
    return awpu_hip_watch_count(n_blocks, w->first, w->every, &wr->n_frames, &next_first);
}

// those checks; then the run
int watch_run(awpu_hip *h, const BlockRun &src, int n_blocks, const awpu_watch_t *w, uint8_t *image, uint8_t *big, float *power, hipStream_t user,
              const FindRun *find = nullptr) {
    WatchRun wr;
    if (int rc = check_watch(w, image || big || power || find, big != nullptr, n_blocks, &wr)) return rc;
    wr.image = image;
    wr.big = big;
    wr.power = power;
    wr.find = find;
    AWPU_CTX(h);
    WatchPieces c(h, src, n_blocks, wr);
    return run_pieces(h, src, user, c);
}

// ---- spectral runs (awpu_hip_spectral.h; kernels in spectral_kernels.hip) ------------------------------------------------------
// A watch run with a set of bands of its own in front of the sweeps (run_pieces sweeps a piece once per band) and another display
// step: launch_spectral_compose on the piece's band powers, then the large three-byte image.  Pieces, histories, the ring: the
// watch run's.

// what a spectral call adds to a watch run; the outputs are host memory in the host forms, device memory in the device form
struct SpectralRun {
    awpu_spectral_t sp{};
    uint8_t *image = nullptr, *big = nullptr, *dominant = nullptr;
};

struct SpectralPieces final : WatchPieces {
    const SpectralRun &sr;
    const bool want_rgb;     // the three-byte image: asked for, or what the large one is made of
    const size_t big3_bytes;
    awpu::SpectralShow shown{};
    size_t image_off = 0, dominant_off = 0, big3_off = 0;  // in a spectral buffer: the band maxima, the images, the dominant bands, the large images

    SpectralPieces(awpu_hip *h_, const BlockRun &src_, int n_blocks_, const WatchRun &wr_, const SpectralRun &sr_)
        : WatchPieces(h_, src_, n_blocks_, wr_), sr(sr_), want_rgb(sr_.image || sr_.big), big3_bytes((size_t) wr_.w.out_rows * wr_.w.out_cols * 3) {
        shown.n_bands = sr.sp.n_bands, shown.scale = sr.sp.scale;
        for (int c = 0; c < 3; c++) shown.channel[c] = sr.sp.channel[c];
    }
    int check() override {
        if (const int rc = check_spectral(h, &sr.sp, &bands)) return rc;
        return WatchPieces::check();
    }
    int ensure(int piece_max, int lo_, int width_, hipStream_t sw) override {
        int rc = WatchPieces::ensure(piece_max, lo_, width_, sw);
        image_off = align16(sizeof(float) * AWPU_SPECTRAL_MAX_BANDS * piece_max);
        dominant_off = image_off + align16((size_t) piece_max * P * 3);
        big3_off = dominant_off + align16((size_t) piece_max * P);
        if (rc == AWPU_OK && (want_rgb || sr.dominant)) rc = h->spectral.ensure(big3_off + (host && sr.big ? (size_t) piece_max * big3_bytes : 0), host);
        if (rc == AWPU_OK && sr.big) rc = ensure_taps(h, w.rows, w.cols, w.out_rows, w.out_cols, sw);
        return rc;
    }
    int show(const Piece &p, float *d_pow, long long plane, hipStream_t s) override {
        if (!want_rgb && !sr.dominant) return AWPU_OK;
        uint8_t *scratch = h->spectral.d[host ? p.b : 0];
        uint8_t *d_image = !want_rgb ? nullptr : (host || !sr.image ? scratch + image_off : sr.image + (size_t) p.first * P * 3);
        uint8_t *d_dominant = !sr.dominant ? nullptr : (host ? scratch + dominant_off : sr.dominant + (size_t) p.first * P);
        AWPU_HIP_TRY(awpu::launch_spectral_compose(d_pow, plane, (int) P, p.n, shown, reinterpret_cast<float *>(scratch), d_image, d_dominant, s));
        if (sr.big)
            AWPU_HIP_TRY(awpu::launch_spectral_upscale(d_image, w.rows, w.cols, p.n, h->d_taps, w.flip != 0,
                                                       host ? scratch + big3_off : sr.big + (size_t) p.first * big3_bytes, w.out_rows, w.out_cols, s));
        return AWPU_OK;
    }
    int fetch_shown(const Piece &p, hipStream_t s) override {
        uint8_t *to = h->spectral.h[p.b], *from = h->spectral.d[p.b];
        if (sr.image) AWPU_HIP_TRY(hipMemcpyAsync(to + image_off, from + image_off, (size_t) p.n * P * 3, hipMemcpyDeviceToHost, s));
        if (sr.dominant) AWPU_HIP_TRY(hipMemcpyAsync(to + dominant_off, from + dominant_off, (size_t) p.n * P, hipMemcpyDeviceToHost, s));
        if (sr.big) AWPU_HIP_TRY(hipMemcpyAsync(to + big3_off, from + big3_off, (size_t) p.n * big3_bytes, hipMemcpyDeviceToHost, s));
        return AWPU_OK;
    }
    int deliver_shown(const Piece &p) override {
        const uint8_t *from = h->spectral.h[p.b];
        if (sr.image) std::memcpy(sr.image + (size_t) p.first * P * 3, from + image_off, (size_t) p.n * P * 3);
        if (sr.dominant) std::memcpy(sr.dominant + (size_t) p.first * P, from + dominant_off, (size_t) p.n * P);
        if (sr.big) parallel_copy(sr.big + (size_t) p.first * big3_bytes, from + big3_off, (size_t) p.n * big3_bytes);
        return AWPU_OK;
    }
};

// the checks of a spectral call that read no handle; then the run
int spectral_run(awpu_hip *h, const BlockRun &src, int n_blocks, const awpu_watch_t *w, const awpu_spectral_t *sp, uint8_t *image, uint8_t *big,
                 uint8_t *dominant, float *power, hipStream_t user) {
    if (const char *why = awpu::spectral_refusal(sp)) return invalid(why);
    WatchRun wr;
    if (int rc = check_watch(w, image || big || dominant || power, big != nullptr, n_blocks, &wr)) return rc;
    if (w->d_colormap) return invalid("a spectral image has its colours from the bands: no colour table");
    wr.power = power;
    SpectralRun sr;
    sr.sp = *sp;
    sr.image = image, sr.big = big, sr.dominant = dominant;
    AWPU_CTX(h);
    SpectralPieces c(h, src, n_blocks, wr, sr);
    return run_pieces(h, src, user, c);
}

// the checks of a find call that read no handle; then the watch run that finds: of `w` only first, every, rows and cols count
int find_run(awpu_hip *h, const BlockRun &src, int n_blocks, const awpu_watch_t *w, const awpu_find_t *f, awpu_source_t *sources, int32_t *count,
             float *power, hipStream_t user, const LocateRun *locate = nullptr) {
    if (!w || !sources || !count) return invalid("null argument");
    if (locate && !locate->ranges) return invalid("null argument");
    if (locate)
        if (const int rc = check_candidates(locate->distance, locate->n_dist)) return rc;
    if (!f) return invalid("null argument");
    if (const int rc = check_find_request(w, f, sources, count)) return rc;
    awpu_watch_t shown{};
    shown.first = w->first, shown.every = w->every, shown.rows = w->rows, shown.cols = w->cols;
    const FindRun find{*f, sources, count, locate};
    return watch_run(h, src, n_blocks, &shown, nullptr, nullptr, power, user, &find);
}

// ---- exposure (awpu_hip_expose.h; kernels in expose_kernels.hip) -----------------------------------------------------------------
// The items of an exposed run are its SWEPT blocks, in order: the blocks of every window that lie inside the call, the skipped
// ones between the windows left out.  With c = carry_in, item s is block q = (s + c) % L of window j = (s + c) / L, and (s + c) / L
// frames close in front of it.  A piece is n consecutive items, and its history holds only the blocks their snapshots read, by the
// slot map of expose_kernels.h: formed like a watch piece's, blocks from before the call out of the ring's snapshot, the rest
// staged and uploaded (host forms) or gathered out of the caller's samples (device form).  The windows are cut a window's items at
// a launch (consecutive blocks: launch_watch_cut, or the band's pre-pass, with a step of one block); where every == length the
// whole piece is one.  Behind the piece's sweep comes launch_expose on its powers -- the open window arrives and leaves in
// d_expose_carry --, and behind that the display step and the peak pass of a watch run on the frames that closed inside the
// piece.  Their number varies from piece to piece, so exposed powers, images and sources all travel through show / fetch_shown /
// deliver_shown and Consumer::power stays null.  The ring's new snapshot: as in a watch run.

struct ExposeRun {
    WatchRun shown;          // what it shows and where to: the outputs and the find request of a watch run, for the exposed frames
    awpu_expose_t e{};
    awpu::ExposeCount n{};
    float *carry = nullptr;  // host memory in the host forms, device memory in the device form, like the outputs
};

struct ExposePieces final : Consumer {
    awpu_hip *const h;
    const BlockRun &src;
    const ExposeRun &er;
    const awpu_watch_t &w;
    const bool host;
    const int S, L, E, c_in;
    const size_t P;
    Display display;
    float *const exposed;               // the exposed frames' powers, or null (Consumer::power, the swept blocks', stays null)
    int lo = 0, width = 0;
    const float *snapshot = nullptr;    // blocks -4 .. -1 of the call
    hipStream_t sw = nullptr;
    std::vector<float> carried;         // host forms: the open window after the run

    ExposePieces(awpu_hip *h_, const BlockRun &src_, int n_blocks_, const ExposeRun &er_)
        : h(h_), src(src_), er(er_), w(er_.shown.w), host(!src_.device), S(h_->cfg.n_streams), L(er_.e.length), E(er_.shown.w.every),
          c_in(er_.n.carry_in), P((size_t) h_->cfg.pixel_count), display(h_, er_.shown, !src_.device), exposed(er_.shown.power) {
        n_items = er.n.n_swept;
        n_blocks = n_blocks_;
        // the last block of the call swept: the ring's new snapshot is the tail of the last piece's history
        tail = n_items == 0 || item_block(n_items - 1) != n_blocks - 1;
    }
    int item_block(int s) const { return w.first + (s + c_in) / L * E - (L - 1) + (s + c_in) % L; }
    int frames_before(int s) const { return (s + c_in) / L; }
    int closed_in(const Piece &p) const { return frames_before(p.first + p.n) - frames_before(p.first); }  // the frames a piece shows
    // the slot map of a piece's history
    awpu::ExposeSlots map(const Piece &p) const {
        if (p.tail) return {n_blocks - 1, 1, n_blocks - 1 + E, E, L, false};
        const int q0 = (p.first + c_in) % L, k0 = item_block(p.first);
        return {k0, std::min(p.n, L - q0), k0 - q0 + E, E, L, E - L >= 3};
    }
    static int slots_of(const Piece &p, const awpu::ExposeSlots &m) { return m.slots(p.tail ? 1 : p.n); }
    // the most slots a piece of n items has: its items and, per window it touches, three blocks (own slots) or the gap (consecutive)
    int slots_max(int n) const {
        const int windows = (n + 2 * L - 2) / L;
        return E - L >= 3 ? n + 3 * windows : n + 3 + (windows - 1) * (E - L);
    }

    int check() override { return display.check(); }
    int ensure(int piece_max, int lo_, int width_, hipStream_t sw_) override {
        lo = lo_, width = width_, sw = sw_;
        const int most = std::max(slots_max(piece_max), 4);
        pitch = awpu::kSamples * most;
        snapshot = h->d_ring + h->ring_pos;
        int rc = ensure_run_buffers(h, src, piece_max, width, true, most - 3, most, bands.planes());
        if (rc == AWPU_OK && !host) rc = ensure_power(h, (size_t) piece_max * P * bands.planes());
        if (rc == AWPU_OK) rc = h->d_expose_carry.ensure(P);
        if (rc == AWPU_OK && (host || !exposed)) rc = h->expose.ensure((size_t) piece_max * P * sizeof(float), false);
        if (rc == AWPU_OK) rc = display.ensure(piece_max, sw);
        if (host && er.n.carry_out > 0) carried.resize(P);
        return rc;
    }
    int begin(hipStream_t s) override {
        if (c_in > 0)
            AWPU_HIP_TRY(hipMemcpyAsync(h->d_expose_carry, er.carry, P * sizeof(float), host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
        return AWPU_OK;
    }
    int staged_blocks(const Piece &p) override {
        const awpu::ExposeSlots m = map(p);
        const int slots = slots_of(p, m), q = std::max(0, 3 - m.k0);
        stage_slots(h, src, [&](int slot) { return m.slot_block(slot); }, q, slots, p.b);
        return slots - q;
    }
    int history(const Piece &p, hipStream_t s) override {
        const awpu::ExposeSlots m = map(p);
        return gathered_history(h, src, p.b, std::max(0, 3 - m.k0), slots_of(p, m), pitch, s, [&](const float *from, long long from_pitch, int n) {
            return awpu::launch_expose_gather(from, from_pitch, snapshot, m, S, hist_of(h, p.b), pitch, 0, n, s);
        });
    }
    int cut(const Piece &p, hipStream_t s) override {
        const awpu::ExposeSlots m = map(p);
        const size_t frame = (size_t) S * width;
        for (int i0 = 0, i1; i0 < p.n; i0 = i1) {  // items [i0, i1): consecutive blocks in consecutive slots
            i1 = E == L ? p.n : (i0 < m.n0 ? m.n0 : std::min(i0 + L, p.n));
            const float *from = hist_of(h, p.b) + (size_t) awpu::kSamples * m.item_slot(i0);
            float *to = h->d_blk_frames + i0 * frame;
            if (bands.n) {
                if (const int rc = band_cut(h, bands, from, awpu::kSamples, pitch, h->wstart, i1 - i0, to, (long long) frame * p.n, h->compact_hist > 0 ? kCompact : kFull, s)) return rc;
            } else {
                AWPU_HIP_TRY(awpu::launch_watch_cut(from, pitch, S, i1 - i0, awpu::kSamples, lo, width, to, s));
            }
        }
        return AWPU_OK;
    }
    int show(const Piece &p, float *d_pow, long long, hipStream_t s) override {
        const int j0 = frames_before(p.first);
        const awpu::ExposeWindows win{p.n, -((p.first + c_in) % L), L, L};
        float *d_frames = host || !exposed ?reinterpret_cast<float *>(h->expose.d[host ? p.b : 0].get()) : exposed + (size_t) j0 * P;
        AWPU_HIP_TRY(awpu::launch_expose(d_pow, (long long) P, win, er.e.mode, h->d_expose_carry, d_frames, s));  // (no frame closes: the carry still moves on)
        return display.show(p.b, j0, closed_in(p), d_frames, s);
    }
    int fetch_shown(const Piece &p, hipStream_t s) override {
        const int nf = closed_in(p);
        if (nf && exposed) AWPU_HIP_TRY(hipMemcpyAsync(h->blk_out.h[p.b], h->expose.d[p.b], (size_t) nf * P * sizeof(float), hipMemcpyDeviceToHost, s));
        return display.fetch(p.b, nf, s);
    }
    int deliver_shown(const Piece &p) override {
        const int j0 = frames_before(p.first), nf = closed_in(p);
        if (nf && exposed) std::memcpy(exposed + (size_t) j0 * P, h->blk_out.h[p.b], (size_t) nf * P * sizeof(float));
        return display.deliver(p.b, j0, nf);
    }
    int ring_from(const Piece &last) override { return awpu::kSamples * (slots_of(last, map(last)) - 4); }
    // the open window, behind the last piece's exposure on the sweep's stream (whatever stream the listen kernels of other runs have)
    int end(hipStream_t) override {
        if (er.n.carry_out == 0) return AWPU_OK;
        if (host)
            AWPU_HIP_TRY(hipMemcpyAsync(carried.data(), h->d_expose_carry, P * sizeof(float), hipMemcpyDeviceToHost, sw));
        else
            AWPU_HIP_TRY(hipMemcpyAsync(er.carry, h->d_expose_carry, P * sizeof(float), hipMemcpyDeviceToDevice, sw));
        return AWPU_OK;
    }
};

// the checks of an expose call that read no handle; then the run
int expose_run(awpu_hip *h, const BlockRun &src, int n_blocks, const awpu_watch_t *w, const awpu_expose_t *e, const awpu_find_t *f, float *carry,
               uint8_t *image, uint8_t *big, float *power, awpu_source_t *sources, int32_t *count, hipStream_t user) {
    WatchRun wr;
    if (int rc = check_watch(w, image || big || power || sources || count, big != nullptr, n_blocks, &wr)) return rc;
    if (const char *why = awpu::expose_refusal(e, w->every)) return invalid(why);
    if (const int rc = check_find_request(w, f, sources, count)) return rc;
    FindRun find;
    if (f) find.f = *f, find.sources = sources, find.count = count;
    wr.image = image, wr.big = big, wr.power = power;
    wr.find = f ? &find : nullptr;
    const ExposeRun er{wr, *e, awpu::expose_count(n_blocks, w->first, w->every, e->length), carry};
    if (!carry && (er.n.carry_in > 0 || er.n.carry_out > 0)) return invalid("null carry with a window open across the call's ends");
    AWPU_CTX(h);
    ExposePieces c(h, src, n_blocks, er);
    const int rc = run_pieces(h, src, user, c);
    if (rc == AWPU_OK && !src.device && er.n.carry_out > 0) std::memcpy(carry, c.carried.data(), c.carried.size() * sizeof(float));
    return rc;
}

// ---- coherence runs (awpu_hip_cohere.h; kernel in cohere_kernels.hip) -------------------------------------------------------------
// A watch run whose pieces are swept by the coherence sweep (launch_cohere) in place of launch(): the row a frame shows -- and
// everything behind it: the display step, the peak pass, the powers' way back -- is its weighted or its coherence row.  Pieces,
// histories, the band's pre-pass in the cut, the ring: the watch run's.
struct CoherePieces final : WatchPieces {
    const int show;
    CoherePieces(awpu_hip *h_, const BlockRun &src_, int n_blocks_, const WatchRun &wr_, int show_) : WatchPieces(h_, src_, n_blocks_, wr_), show(show_) {}
    int check() override {
        if (h->cfg.interp != AWPU_INTERP_LERP) return fail(AWPU_ERR_STATE, "the coherence sweep interpolates linearly: AWPU_INTERP_FIR8 is not taken");
        return WatchPieces::check();
    }
    int ensure(int piece_max, int lo_, int width_, hipStream_t sw) override {  // (the handle is ready; none of the run's work is enqueued yet)
        const int rc = ensure_cohere_table(h);
        return rc != AWPU_OK ? rc : WatchPieces::ensure(piece_max, lo_, width_, sw);
    }
    int sweep_frames(awpu_hip *, const Piece &p, const float *d_frames, float *d_pow, hipStream_t s, int layout) override {
        CohereOut out;
        (show == AWPU_COHERE_FACTOR ? out.coherence : out.weighted) = d_pow;
        return launch_cohere(h, d_frames, p.n, out, s, layout);
    }
};

// the checks of a coherence run that read no handle; then the run
int cohere_run(awpu_hip *h, const BlockRun &src, int n_blocks, const awpu_watch_t *w, const awpu_cohere_t *co, const awpu_find_t *f, uint8_t *image,
               uint8_t *big, float *power, awpu_source_t *sources, int32_t *count, hipStream_t user) {
    WatchRun wr;
    if (int rc = check_watch(w, image || big || power || sources || count, big != nullptr, n_blocks, &wr)) return rc;
    if (const char *why = awpu::cohere_refusal(co)) return invalid(why);
    if (const int rc = check_find_request(w, f, sources, count)) return rc;
    FindRun find;
    if (f) find.f = *f, find.sources = sources, find.count = count;
    wr.image = image, wr.big = big, wr.power = power;
    wr.find = f ? &find : nullptr;
    AWPU_CTX(h);
    CoherePieces c(h, src, n_blocks, wr, co->show);
    return run_pieces(h, src, user, c);
}

// ---- peel runs (awpu_hip_peel.h; the loop in awpu_peel.cpp) ------------------------------------------------------------------------
// A watch run whose pieces are peeled (peel_enqueue) in place of swept: a piece's snapshots are cut whole -- the step reads E + 1
// samples either side of the window -- into d_blk_frames, which the loop then turns into the residual, and the row a frame shows
// -- and everything behind it -- is its map, clean or residual row.  The steps go to the caller's array (device form) or come back
// with the piece's images through peel_steps (host forms).  Pieces, histories, the ring: the watch run's.
struct PeelPieces final : WatchPieces {
    const awpu_peel_t pe;
    const int show_row;
    awpu_peel_step_t *const steps;  // [n_frames][pe.steps], host or device memory as the run's other outputs, or null
    PeelPieces(awpu_hip *h_, const BlockRun &src_, int n_blocks_, const WatchRun &wr_, const awpu_peel_t &pe_, int show_, awpu_peel_step_t *steps_)
        : WatchPieces(h_, src_, n_blocks_, wr_), pe(pe_), show_row(show_), steps(steps_) {
        whole_frames = true;
    }
    size_t step_bytes(int n) const { return (size_t) n * pe.steps * sizeof(awpu_peel_step_t); }
    int check() override {
        const int rc = peel_handle_refusal(h);
        return rc != AWPU_OK ? rc : WatchPieces::check();
    }
    int ensure(int piece_max, int lo_, int width_, hipStream_t sw) override {  // (the handle is ready; none of the run's work is enqueued yet)
        int rc = peel_prepare(h, piece_max);
        if (rc == AWPU_OK && host && steps) rc = h->peel_steps.ensure(step_bytes(piece_max), true);
        return rc != AWPU_OK ? rc : WatchPieces::ensure(piece_max, lo_, width_, sw);
    }
    int sweep_frames(awpu_hip *, const Piece &p, const float *d_frames, float *d_pow, hipStream_t s, int layout) override {
        if (layout != kFull) return fail(AWPU_ERR_STATE, "a peel run cuts its snapshots whole");
        PeelOut out;
        (show_row == AWPU_PEEL_CLEAN ? out.clean : show_row == AWPU_PEEL_RESIDUAL ? out.residual : out.map) = d_pow;
        if (steps) out.steps = host ? reinterpret_cast<awpu_peel_step_t *>(h->peel_steps.d[p.b].get()) : steps + (size_t) p.first * pe.steps;
        return peel_enqueue(h, const_cast<float *>(d_frames), p.n, pe, out, s);  // (d_blk_frames: the run's own scratch, cut anew for every piece)
    }
    int fetch_shown(const Piece &p, hipStream_t s) override {
        if (steps) AWPU_HIP_TRY(hipMemcpyAsync(h->peel_steps.h[p.b], h->peel_steps.d[p.b], step_bytes(p.n), hipMemcpyDeviceToHost, s));
        return WatchPieces::fetch_shown(p, s);
    }
    int deliver_shown(const Piece &p) override {
        if (steps) std::memcpy(steps + (size_t) p.first * pe.steps, h->peel_steps.h[p.b], step_bytes(p.n));
        return WatchPieces::deliver_shown(p);
    }
};

// the checks of a peel run that read no handle; then the run
int peel_run(awpu_hip *h, const BlockRun &src, int n_blocks, const awpu_watch_t *w, const awpu_peel_t *pe, int32_t show, const awpu_find_t *f,
             uint8_t *image, uint8_t *big, float *power, awpu_peel_step_t *steps, awpu_source_t *sources, int32_t *count, hipStream_t user) {
    WatchRun wr;
    if (int rc = check_watch(w, image || big || power || steps || sources || count, big != nullptr, n_blocks, &wr)) return rc;
    if (const char *why = awpu::peel_refusal(pe)) return invalid(why);
    if (show != AWPU_PEEL_MAP && show != AWPU_PEEL_CLEAN && show != AWPU_PEEL_RESIDUAL) return invalid("show is AWPU_PEEL_MAP, AWPU_PEEL_CLEAN or AWPU_PEEL_RESIDUAL");
    if (const int rc = check_find_request(w, f, sources, count)) return rc;
    FindRun find;
    if (f) find.f = *f, find.sources = sources, find.count = count;
    wr.image = image, wr.big = big, wr.power = power;
    wr.find = f ? &find : nullptr;
    AWPU_CTX(h);
    PeelPieces c(h, src, n_blocks, wr, *pe, show, steps);
    return run_pieces(h, src, user, c);
}

}  // namespace

extern "C" {

int awpu_hip_peel_blocks(awpu_hip_t *h, const void *datagrams, int32_t stride_bytes, int32_t n_blocks, const awpu_watch_t *w,
                         const awpu_peel_t *pe, int32_t show, const awpu_find_t *f, uint8_t *image, uint8_t *big_image, float *power,
                         awpu_peel_step_t *steps, awpu_source_t *sources, int32_t *count) {
    BlockRun src;
    if (int rc = wire_source(h, datagrams, stride_bytes, n_blocks, &src)) return rc;
    return peel_run(h, src, n_blocks, w, pe, show, f, image, big_image, power, steps, sources, count, nullptr);
}

int awpu_hip_peel_samples(awpu_hip_t *h, const float *samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                          const awpu_peel_t *pe, int32_t show, const awpu_find_t *f, uint8_t *image, uint8_t *big_image, float *power,
                          awpu_peel_step_t *steps, awpu_source_t *sources, int32_t *count) {
    BlockRun src;
    if (int rc = sample_source(h, samples, pitch, n_blocks, false, &src)) return rc;
    return peel_run(h, src, n_blocks, w, pe, show, f, image, big_image, power, steps, sources, count, nullptr);
}

int awpu_hip_peel_samples_device(awpu_hip_t *h, const float *d_samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                                 const awpu_peel_t *pe, int32_t show, const awpu_find_t *f, uint8_t *d_image, uint8_t *d_big_image,
                                 float *d_power, awpu_peel_step_t *d_steps, awpu_source_t *d_sources, int32_t *d_count, void *stream) {
    BlockRun src;
    if (int rc = sample_source(h, d_samples, pitch, n_blocks, true, &src)) return rc;
    return peel_run(h, src, n_blocks, w, pe, show, f, d_image, d_big_image, d_power, d_steps, d_sources, d_count, static_cast<hipStream_t>(stream));
}

int awpu_hip_process_blocks(awpu_hip_t *h, const void *datagrams, int32_t stride_bytes, int32_t n_blocks, float *power) {
    BlockRun src;
    if (int rc = wire_source(h, datagrams, stride_bytes, n_blocks, &src)) return rc;
    if (!power) return invalid("null argument");
    AWPU_CTX(h);
    return run_blocks(h, src, n_blocks, power, nullptr);
}

int awpu_hip_process_samples(awpu_hip_t *h, const float *samples, int64_t pitch, int32_t n_blocks, float *power) {
    BlockRun src;
    if (int rc = sample_source(h, samples, pitch, n_blocks, false, &src)) return rc;
    if (!power) return invalid("null argument");
    AWPU_CTX(h);
    return run_blocks(h, src, n_blocks, power, nullptr);
}

int awpu_hip_process_samples_device(awpu_hip_t *h, const float *d_samples, int64_t pitch, int32_t n_blocks, float *d_power,
                                    void *stream) {
    BlockRun src;
    if (int rc = sample_source(h, d_samples, pitch, n_blocks, true, &src)) return rc;
    if (!d_power) return invalid("null argument");
    AWPU_CTX(h);
    return run_blocks(h, src, n_blocks, d_power, static_cast<hipStream_t>(stream));
}

int awpu_hip_listen_blocks(awpu_hip_t *h, const void *datagrams, int32_t stride_bytes, int32_t n_blocks, awpu_particle_t *listeners,
                           int32_t n, double theta_limit, double reference, float *audio, int64_t audio_pitch, awpu_particle_t *trail,
                           float *power) {
    BlockRun src;
    if (int rc = wire_source(h, datagrams, stride_bytes, n_blocks, &src)) return rc;
    return listen_run(h, src, n_blocks, listeners, n, theta_limit, reference, audio, audio_pitch, trail, power, nullptr);
}

int awpu_hip_listen_samples(awpu_hip_t *h, const float *samples, int64_t pitch, int32_t n_blocks, awpu_particle_t *listeners, int32_t n,
                            double theta_limit, double reference, float *audio, int64_t audio_pitch, awpu_particle_t *trail,
                            float *power) {
    BlockRun src;
    if (int rc = sample_source(h, samples, pitch, n_blocks, false, &src)) return rc;
    return listen_run(h, src, n_blocks, listeners, n, theta_limit, reference, audio, audio_pitch, trail, power, nullptr);
}

int awpu_hip_listen_samples_device(awpu_hip_t *h, const float *d_samples, int64_t pitch, int32_t n_blocks, awpu_particle_t *listeners,
                                   int32_t n, double theta_limit, double reference, float *d_audio, int64_t audio_pitch,
                                   awpu_particle_t *d_trail, float *d_power, void *stream) {
    BlockRun src;
    if (int rc = sample_source(h, d_samples, pitch, n_blocks, true, &src)) return rc;
    return listen_run(h, src, n_blocks, listeners, n, theta_limit, reference, d_audio, audio_pitch, d_trail, d_power,
                      static_cast<hipStream_t>(stream));
}

int awpu_hip_watch_count(int32_t n_blocks, int32_t first, int32_t every, int32_t *n_frames, int32_t *next_first) {
    if (!n_frames || !next_first) return invalid("null argument");
    if (n_blocks < 1) return invalid("n_blocks below 1");
    if (first < 0) return invalid("first below 0");
    if (every < 1) return invalid("every below 1");
    const int64_t shown = first >= n_blocks ? 0 : ((int64_t) n_blocks - first + every - 1) / every;
    *n_frames = (int32_t) shown;
    *next_first = (int32_t) (first + shown * every - n_blocks);
    return AWPU_OK;
}

int awpu_hip_watch_blocks(awpu_hip_t *h, const void *datagrams, int32_t stride_bytes, int32_t n_blocks, const awpu_watch_t *w,
                          uint8_t *image, uint8_t *big_image, float *power) {
    BlockRun src;
    if (int rc = wire_source(h, datagrams, stride_bytes, n_blocks, &src)) return rc;
    return watch_run(h, src, n_blocks, w, image, big_image, power, nullptr);
}

int awpu_hip_watch_samples(awpu_hip_t *h, const float *samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w, uint8_t *image,
                           uint8_t *big_image, float *power) {
    BlockRun src;
    if (int rc = sample_source(h, samples, pitch, n_blocks, false, &src)) return rc;
    return watch_run(h, src, n_blocks, w, image, big_image, power, nullptr);
}

int awpu_hip_watch_samples_device(awpu_hip_t *h, const float *d_samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                                  uint8_t *d_image, uint8_t *d_big_image, float *d_power, void *stream) {
    BlockRun src;
    if (int rc = sample_source(h, d_samples, pitch, n_blocks, true, &src)) return rc;
    return watch_run(h, src, n_blocks, w, d_image, d_big_image, d_power, static_cast<hipStream_t>(stream));
}

int awpu_hip_spectral_blocks(awpu_hip_t *h, const void *datagrams, int32_t stride_bytes, int32_t n_blocks, const awpu_watch_t *w,
                             const awpu_spectral_t *sp, uint8_t *image, uint8_t *big_image, uint8_t *dominant, float *power) {
    BlockRun src;
    if (int rc = wire_source(h, datagrams, stride_bytes, n_blocks, &src)) return rc;
    return spectral_run(h, src, n_blocks, w, sp, image, big_image, dominant, power, nullptr);
}

int awpu_hip_spectral_samples(awpu_hip_t *h, const float *samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                              const awpu_spectral_t *sp, uint8_t *image, uint8_t *big_image, uint8_t *dominant, float *power) {
    BlockRun src;
    if (int rc = sample_source(h, samples, pitch, n_blocks, false, &src)) return rc;
    return spectral_run(h, src, n_blocks, w, sp, image, big_image, dominant, power, nullptr);
}

int awpu_hip_spectral_samples_device(awpu_hip_t *h, const float *d_samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                                     const awpu_spectral_t *sp, uint8_t *d_image, uint8_t *d_big_image, uint8_t *d_dominant,
                                     float *d_power, void *stream) {
    BlockRun src;
    if (int rc = sample_source(h, d_samples, pitch, n_blocks, true, &src)) return rc;
    return spectral_run(h, src, n_blocks, w, sp, d_image, d_big_image, d_dominant, d_power, static_cast<hipStream_t>(stream));
}

int awpu_hip_find_peaks_device(awpu_hip_t *h, const float *d_power, int32_t n_frames, const awpu_find_t *f, awpu_source_t *d_sources,
                               int32_t *d_count, void *stream) {
    if (!h || !d_power || !d_sources || !d_count) return invalid("null argument");
    if (n_frames < 1) return invalid("n_frames below 1");
    if (const char *why = awpu::find_refusal(f)) return invalid(why);
    h = first_device(h);
    AWPU_CTX(h);
    AWPU_HIP_TRY(hipSetDevice(h->cfg.device));
    // (no enter_stream, here and in awpu_hip_expose_rows_device: nothing of the handle's is used)
    AWPU_HIP_TRY(awpu::launch_find_peaks(d_power, n_frames, *f, d_sources, d_count, stream_of(h, stream)));
    return AWPU_OK;
}

int awpu_hip_find_blocks(awpu_hip_t *h, const void *datagrams, int32_t stride_bytes, int32_t n_blocks, const awpu_watch_t *w,
                         const awpu_find_t *f, awpu_source_t *sources, int32_t *count, float *power) {
    BlockRun src;
    if (int rc = wire_source(h, datagrams, stride_bytes, n_blocks, &src)) return rc;
    return find_run(h, src, n_blocks, w, f, sources, count, power, nullptr);
}

int awpu_hip_find_samples(awpu_hip_t *h, const float *samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                          const awpu_find_t *f, awpu_source_t *sources, int32_t *count, float *power) {
    BlockRun src;
    if (int rc = sample_source(h, samples, pitch, n_blocks, false, &src)) return rc;
    return find_run(h, src, n_blocks, w, f, sources, count, power, nullptr);
}

int awpu_hip_find_samples_device(awpu_hip_t *h, const float *d_samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                                 const awpu_find_t *f, awpu_source_t *d_sources, int32_t *d_count, float *d_power, void *stream) {
    BlockRun src;
    if (int rc = sample_source(h, d_samples, pitch, n_blocks, true, &src)) return rc;
    return find_run(h, src, n_blocks, w, f, d_sources, d_count, d_power, static_cast<hipStream_t>(stream));
}

int awpu_hip_locate_blocks(awpu_hip_t *h, const void *datagrams, int32_t stride_bytes, int32_t n_blocks, const awpu_watch_t *w,
                           const awpu_find_t *f, awpu_source_t *sources, int32_t *count, float *power, const double *distance,
                           int32_t n_dist, awpu_range_t *ranges, float *range_power) {
    BlockRun src;
    if (int rc = wire_source(h, datagrams, stride_bytes, n_blocks, &src)) return rc;
    const LocateRun locate{distance, n_dist, ranges, range_power};
    return find_run(h, src, n_blocks, w, f, sources, count, power, nullptr, &locate);
}

int awpu_hip_locate_samples(awpu_hip_t *h, const float *samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                            const awpu_find_t *f, awpu_source_t *sources, int32_t *count, float *power, const double *distance,
                            int32_t n_dist, awpu_range_t *ranges, float *range_power) {
    BlockRun src;
    if (int rc = sample_source(h, samples, pitch, n_blocks, false, &src)) return rc;
    const LocateRun locate{distance, n_dist, ranges, range_power};
    return find_run(h, src, n_blocks, w, f, sources, count, power, nullptr, &locate);
}

int awpu_hip_locate_samples_device(awpu_hip_t *h, const float *d_samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                                   const awpu_find_t *f, awpu_source_t *d_sources, int32_t *d_count, float *d_power,
                                   const double *distance, int32_t n_dist, awpu_range_t *d_ranges, float *d_range_power,
                                   void *stream) {
    BlockRun src;
    if (int rc = sample_source(h, d_samples, pitch, n_blocks, true, &src)) return rc;
    const LocateRun locate{distance, n_dist, d_ranges, d_range_power};
    return find_run(h, src, n_blocks, w, f, d_sources, d_count, d_power, static_cast<hipStream_t>(stream), &locate);
}

int awpu_hip_expose_rows_device(awpu_hip_t *h, const float *d_power, int32_t n_blocks, int32_t n_pixels, int32_t first, int32_t every,
                                const awpu_expose_t *e, float *d_carry, float *d_frames, void *stream) {
    if (!h || !d_power) return invalid("null argument");
    if (n_blocks < 1 || n_pixels < 1 || first < 0 || every < 1) return invalid("n_blocks, n_pixels, every below 1 or first below 0");
    if (const char *why = awpu::expose_refusal(e, every)) return invalid(why);
    const awpu::ExposeCount n = awpu::expose_count(n_blocks, first, every, e->length);
    if (!d_carry && (n.carry_in > 0 || n.carry_out > 0)) return invalid("null carry with a window open across the call's ends");
    if (!d_frames && n.n_frames > 0) return invalid("null argument");
    h = first_device(h);
    AWPU_CTX(h);
    AWPU_HIP_TRY(hipSetDevice(h->cfg.device));
    const awpu::ExposeWindows win{n_blocks, first - (e->length - 1), every, e->length};
    AWPU_HIP_TRY(awpu::launch_expose(d_power, n_pixels, win, e->mode, d_carry, d_frames, stream_of(h, stream)));
    return AWPU_OK;
}

int awpu_hip_expose_blocks(awpu_hip_t *h, const void *datagrams, int32_t stride_bytes, int32_t n_blocks, const awpu_watch_t *w,
                           const awpu_expose_t *e, const awpu_find_t *f, float *carry, uint8_t *image, uint8_t *big_image, float *power,
                           awpu_source_t *sources, int32_t *count) {
    BlockRun src;
    if (int rc = wire_source(h, datagrams, stride_bytes, n_blocks, &src)) return rc;
    return expose_run(h, src, n_blocks, w, e, f, carry, image, big_image, power, sources, count, nullptr);
}

int awpu_hip_expose_samples(awpu_hip_t *h, const float *samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                            const awpu_expose_t *e, const awpu_find_t *f, float *carry, uint8_t *image, uint8_t *big_image, float *power,
                            awpu_source_t *sources, int32_t *count) {
    BlockRun src;
    if (int rc = sample_source(h, samples, pitch, n_blocks, false, &src)) return rc;
    return expose_run(h, src, n_blocks, w, e, f, carry, image, big_image, power, sources, count, nullptr);
}

int awpu_hip_expose_samples_device(awpu_hip_t *h, const float *d_samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                                   const awpu_expose_t *e, const awpu_find_t *f, float *d_carry, uint8_t *d_image, uint8_t *d_big_image,
                                   float *d_power, awpu_source_t *d_sources, int32_t *d_count, void *stream) {
    BlockRun src;
    if (int rc = sample_source(h, d_samples, pitch, n_blocks, true, &src)) return rc;
    return expose_run(h, src, n_blocks, w, e, f, d_carry, d_image, d_big_image, d_power, d_sources, d_count, static_cast<hipStream_t>(stream));
}

int awpu_hip_cohere_blocks(awpu_hip_t *h, const void *datagrams, int32_t stride_bytes, int32_t n_blocks, const awpu_watch_t *w,
                           const awpu_cohere_t *co, const awpu_find_t *f, uint8_t *image, uint8_t *big_image, float *power,
                           awpu_source_t *sources, int32_t *count) {
    BlockRun src;
    if (int rc = wire_source(h, datagrams, stride_bytes, n_blocks, &src)) return rc;
    return cohere_run(h, src, n_blocks, w, co, f, image, big_image, power, sources, count, nullptr);
}

int awpu_hip_cohere_samples(awpu_hip_t *h, const float *samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                            const awpu_cohere_t *co, const awpu_find_t *f, uint8_t *image, uint8_t *big_image, float *power,
                            awpu_source_t *sources, int32_t *count) {
    BlockRun src;
    if (int rc = sample_source(h, samples, pitch, n_blocks, false, &src)) return rc;
    return cohere_run(h, src, n_blocks, w, co, f, image, big_image, power, sources, count, nullptr);
}

int awpu_hip_cohere_samples_device(awpu_hip_t *h, const float *d_samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                                   const awpu_cohere_t *co, const awpu_find_t *f, uint8_t *d_image, uint8_t *d_big_image, float *d_power,
                                   awpu_source_t *d_sources, int32_t *d_count, void *stream) {
    BlockRun src;
    if (int rc = sample_source(h, d_samples, pitch, n_blocks, true, &src)) return rc;
    return cohere_run(h, src, n_blocks, w, co, f, d_image, d_big_image, d_power, d_sources, d_count, static_cast<hipStream_t>(stream));
}

}  // extern "C"
