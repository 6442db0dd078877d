// awpu_hip.cpp -- the C ABI of libawpu_hip.so (include/awpu_hip.h) and its call paths: handle lifetime, setters, frame upload,
// the single-call paths, the ring, display, tracking, the packed-frame entry points and the band in front of the sweeps.  The tables, the kernel launchers and
// the dispatch rule are the sweep layer (awpu_sweep.cpp); the runs of blocks are run_pieces.cpp and the files on it; a device group's handle is
// handed over to awpu_group.cpp.  No CPU fallback: every compute entry point ends in a gfx950 kernel launch or an error status.
#include "awpu_handle.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "awpu_hip_band.h"
#include "band_kernels.h"
#include "band_rule.h"
#include "spectral_kernels.h"
#include "das_kernels.h"
#include "focus_rule.h"
#include "watch_kernels.h"

using namespace awpu::host;

namespace {

thread_local std::string g_last_error;
thread_local awpu_hip *g_ctx = nullptr;  // the handle the calling thread is working on (CtxScope)

}  // namespace

namespace awpu::host {

void note_error(const std::string &text) {
    g_last_error = text;
    if (g_ctx) g_ctx->last_error = text;
}

CtxScope::CtxScope(awpu_hip *h) : saved(g_ctx) { g_ctx = h; }
CtxScope::~CtxScope() { g_ctx = saved; }

int hip_fail(hipError_t e, const char *what) {
    note_error(std::string(what) + ": " + hipGetErrorString(e));
    return AWPU_ERR_HIP;
}

int invalid(const char *why) {
    note_error(why);
    return AWPU_ERR_INVALID;
}

int fail(int status, const char *why) {
    note_error(why);
    return status;
}

}  // namespace awpu::host

awpu::host::EnvKnobs::EnvKnobs() {
    if (const char *v = std::getenv("AWPU_GROUP_FORCE_COPY")) group_copy = std::atoi(v);
    if (const char *v = std::getenv("AWPU_LIVE_GRAPH")) live_graph = std::atoi(v);
    if (const char *v = std::getenv("AWPU_SHAPE")) {
        const std::string shape(v);
        if (shape == "pair" || shape == "pair_vertical" || shape == "pair_horizontal") {
            pairs = 1, quads = 0, stationary = 0;
            if (shape != "pair") pair_cols = shape == "pair_vertical";
        } else if (shape == "quad") quads = 1;
        else if (shape == "noquad") quads = 0;
        else if (shape == "stationary") pairs = 1, quads = 0, stationary = 1;
        else if (shape == "quadh") quads = 1, pairs = 0, halves = 1;
        else if (shape == "quadh_chunked") quads = 1, pairs = 0, halves = 1, stationary = 0;  // never the resident-window variant
        else if (shape == "single_db") pairs = 0, quads = 0, fpi = 1, ppw = 8, nw = 32;
        else if (shape == "single_small") pairs = 0, quads = 0, fpi = 1, ppw = 2, nw = 8;
        else if (shape == "fir8_planes") fir_planes = 2;
        else if (shape == "exact_verify") exact_pairs = ExactShape::kVerify;
        else if (shape == "exact_pair") exact_pairs = ExactShape::kPair;
        else if (shape == "exact_quad") exact_pairs = ExactShape::kQuad;
        else if (shape == "exact_nd1") exact_pairs = ExactShape::kNd1;
        else if (shape == "exact_nd2") exact_pairs = ExactShape::kNd2;
        else if (shape == "exact_ndp") exact_pairs = ExactShape::kNdp;
        else std::fprintf(stderr, "libawpu_hip: AWPU_SHAPE=%s is not a shape of this build; ignored\n", v);
    }
#ifdef AWPU_TUNING_BUILD
    if (const char *v = std::getenv("AWPU_LISTEN_STREAM")) listen_stream = std::atoi(v);
    if (const char *v = std::getenv("AWPU_FAST_QUADS")) quads = std::atoi(v);
    if (const char *v = std::getenv("AWPU_FAST_PAIRGROUP")) pair_group = std::atoi(v);
    if (const char *v = std::getenv("AWPU_QUAD_VARIANT")) quad_variant = std::atoi(v);
    if (const char *v = std::getenv("AWPU_FAST_HALVES")) halves = std::atoi(v);
    if (const char *v = std::getenv("AWPU_EXACT_PAIRS")) exact_pairs = (ExactShape) std::atoi(v);
    if (const char *v = std::getenv("AWPU_FAST_WGS")) wgs = std::atoi(v);
    if (const char *v = std::getenv("AWPU_FIR8_PLANES")) fir_planes = std::atoi(v);
    if (const char *v = std::getenv("AWPU_FIR8_SHARE")) fir_share = std::atoi(v);
    if (const char *v = std::getenv("AWPU_FAST_STATIONARY")) stationary = std::atoi(v);
    if (const char *v = std::getenv("AWPU_FAST_PAIRCOLS")) pair_cols = std::atoi(v);
    if (const char *v = std::getenv("AWPU_FAST_VARIANT"))
        if (std::sscanf(v, "%d,%d,%d", &fpi, &ppw, &nw) < 2) fpi = ppw = nw = 0;
    if (const char *v = std::getenv("AWPU_FAST_PAIRS")) pairs = std::atoi(v);
    if (const char *v = std::getenv("AWPU_FAST_DEBUG")) debug = std::atoi(v);
#ifndef AWPU_TIMING_BUILD
    debug &= awpu::kDebugSafeBits;  // the wrong-result timing switches exist only with -DAWPU_TIMING_BUILD (das_kernels.h)
#endif
    if (const char *v = std::getenv("AWPU_FAST_FPW")) fpw = std::atoi(v);
#endif
}

const EnvKnobs &awpu::host::env() {
    static const EnvKnobs knobs;  // initialised once, thread-safe
    return knobs;
}

// The captured live-block graphs hold raw device pointers (d_power, d_display, d_taps, d_ring, tables, d_pack):
// whoever frees or reallocates one of those retires the graphs first (the buffers that grow: ensure_seen_by_live_graphs,
// awpu_handle.h).  The next live calls run step by step and capture again once the buffers have settled.
void awpu::host::retire_live_graphs(awpu_hip *h) {
    for (auto &g : h->live_graphs) (void) hipGraphExecDestroy(g.exec);
    h->live_graphs.clear();
    h->live_warm = 0;
}

namespace awpu::host {

extern const char *const kBandHistory = "the band reads taps - 1 samples in front of the window: the delay table leaves a snapshot fewer";

int check_ready(awpu_hip *h, int batch) {
    if (!h) return invalid("null handle");
    if (batch < 1 || batch > h->cfg.max_batch) return invalid("batch outside [1, max_batch]");
    if (!h->have_table || !h->have_mics) {
        return fail(AWPU_ERR_STATE, "delay table and active mics must be set before processing");
    }
    if (h->cfg.interp == AWPU_INTERP_FIR8 && !h->have_fir) {
        return fail(AWPU_ERR_STATE, "AWPU_INTERP_FIR8 needs awpu_hip_set_fir_table");
    }
    AWPU_HIP_TRY(hipSetDevice(h->cfg.device));
    if (!h->prepared) {
        const int rc = prepare(h);
        if (rc != AWPU_OK) return rc;
    }
    if (h->band_taps() - 1 > h->wstart) return fail(AWPU_ERR_RANGE, kBandHistory);
    return AWPU_OK;
}

// Call order across streams, (c) of the stream contract in awpu_hip.h: every entry point that enqueues work comes through here with
// the stream it resolved, the device current -- except the four that use nothing of the handle's but its tables (awpu_hip_pack_frames,
// _heatmap_u8_device, _find_peaks_device, _expose_rows_device: they may run beside the handle's other work).  The handle's scratch
// (d_pack, the item queues, d_band, d_power, the runs' buffers, the ring) has one owner at a time because a call on another stream
// than the last one starts behind an event recorded on that last stream.  The same stream again -- every loop that drives a handle
// from one stream -- records and awaits nothing.
int enter_stream(awpu_hip *h, hipStream_t s) {
    if (s == h->last_stream) return AWPU_OK;
    if (h->last_stream) {
        if (const int rc = h->ev_order.ensure(); rc != AWPU_OK) return rc;
        AWPU_HIP_TRY(hipEventRecord(h->ev_order, h->last_stream));
        AWPU_HIP_TRY(hipStreamWaitEvent(s, h->ev_order, 0));
    }
    h->last_stream = s;
    return AWPU_OK;
}

int ensure_power(awpu_hip *h, size_t need_power) { return ensure_seen_by_live_graphs(h, h->d_power, need_power); }

// frames per sweep launch of a host batch: large batches go up in pieces of whole frame pairs, so that piece k+1 crosses PCIe
// while piece k is swept (enqueue_host_process; a run of blocks sweeps its chunks the same way)
int host_piece(int batch) {
    const int n_pieces = batch >= 128 ? 4 : (batch >= 64 ? 2 : 1);
    return ((batch + n_pieces - 1) / n_pieces + 1) & ~1;
}

// upload of host frames + the sweep into h->d_power, all on h->stream, nothing waited for.  Timed: every caller ends in wait_and_time
int enqueue_host_process(awpu_hip *h, const float *frames, int batch, const BandSet *given) {
    int rc = check_ready(h, batch);
    if (rc == AWPU_OK) rc = enter_stream(h, h->stream);
    if (rc != AWPU_OK) return rc;
    const BandSet bands = given ? *given : own_band(h);  // several: band b's powers of the batch at d_power + b * batch * pixel_count
    if (bands.max_taps() - 1 > h->wstart) return fail(AWPU_ERR_RANGE, kBandHistory);
    const bool compact = h->compact_hist > 0;
    const int pre = compact ? std::max(bands.max_taps() - 1, 0) : 0;  // a band reads that many samples in front of the window: they travel too
    const int dev_hist = (compact ? h->compact_hist : h->cfg.hist) + pre;
    const size_t need_frames = (size_t) h->cfg.n_streams * dev_hist * batch;
    rc = h->d_frames.ensure(need_frames);
    if (rc == AWPU_OK) rc = ensure_power(h, (size_t) h->cfg.pixel_count * batch * bands.planes());
    if (rc != AWPU_OK) return rc;
    // Large batches go up in pieces on a second stream, so that piece k+1 crosses PCIe while piece k is swept (the
    // pieces are whole frame pairs: the same arithmetic as one launch).  last_kernel_ms then spans all the sweeps.
    const int piece = host_piece(batch);
    const int n_pieces = (batch + piece - 1) / piece;
    if (n_pieces > 1) {
        rc = h->copy_stream.ensure();
        for (awpu_hip::Event &ev : h->ev_copied)
            if (rc == AWPU_OK) rc = ev.ensure();
        if (rc != AWPU_OK) return rc;
    }
    int turn = 0;
    for (int b0 = 0; b0 < batch; b0 += piece, turn++) {
        const int nb = std::min(piece, batch - b0);
        hipStream_t up = n_pieces > 1 ? h->copy_stream : h->stream;
        float *dst = h->d_frames + (size_t) b0 * h->cfg.n_streams * dev_hist;
        const float *src = frames + (size_t) b0 * h->cfg.n_streams * h->cfg.hist;
        if (compact) {  // rows of compact_hist floats cut out of rows of hist floats: a third of the PCIe bytes
            AWPU_HIP_TRY(hipMemcpy2DAsync(dst, (size_t) dev_hist * sizeof(float), src + h->wstart - pre, (size_t) h->cfg.hist * sizeof(float),
                                          (size_t) dev_hist * sizeof(float), (size_t) nb * h->cfg.n_streams, hipMemcpyHostToDevice, up));
        } else {
            AWPU_HIP_TRY(hipMemcpyAsync(dst, src, (size_t) nb * h->cfg.n_streams * dev_hist * sizeof(float), hipMemcpyHostToDevice, up));
        }
        if (n_pieces > 1) {
            AWPU_HIP_TRY(hipEventRecord(h->ev_copied[turn & 1], up));
            AWPU_HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_copied[turn & 1], 0));
            if (b0 == 0) AWPU_HIP_TRY(hipEventRecord(h->ev_begin, h->stream));  // several pieces: the bracket spans them all, recorded here
        }
        rc = band_sweep(h, bands, dst, (long long) h->cfg.n_streams * dev_hist, dev_hist, compact ? pre : h->wstart, nb,
                        h->d_power + (size_t) b0 * h->cfg.pixel_count, (long long) batch * h->cfg.pixel_count, h->stream, compact ? kCompact : kFull,
                        n_pieces > 1 ? SweepOpts{} : kTimed);
        if (rc != AWPU_OK) return rc;
    }
    if (n_pieces > 1) AWPU_HIP_TRY(hipEventRecord(h->ev_end, h->stream));
    return AWPU_OK;
}

// h->d_power [batch][pixel_count] -> host image `power` [batch][pitch] (pitch = this handle's pixels, or the whole group's: a
// part's pixel ranges then land where they belong in the wider image), on h->stream
int enqueue_power_to_host(awpu_hip *h, int batch, float *power, size_t pitch) {
    const size_t row = (size_t) h->cfg.pixel_count * sizeof(float);
    if (h->member.ranges.empty()) {
        if (pitch == (size_t) h->cfg.pixel_count) {
            AWPU_HIP_TRY(hipMemcpyAsync(power, h->d_power, row * batch, hipMemcpyDeviceToHost, h->stream));
        } else {
            AWPU_HIP_TRY(hipMemcpy2DAsync(power, pitch * sizeof(float), h->d_power, row, row, (size_t) batch, hipMemcpyDeviceToHost, h->stream));
        }
        return AWPU_OK;
    }
    size_t done = 0;  // pixels of the part's own rows already sent
    for (const auto &r : h->member.ranges) {
        AWPU_HIP_TRY(hipMemcpy2DAsync(power + r.first, pitch * sizeof(float), h->d_power + done, row, (size_t) r.second * sizeof(float),
                                      (size_t) batch, hipMemcpyDeviceToHost, h->stream));
        done += (size_t) r.second;
    }
    return AWPU_OK;
}

// The bands' pre-pass (awpu_hip_band.h, awpu_hip_spectral.h; band_kernels.hip for one band, spectral_kernels.hip for several): the
// window of `batch` frames, filtered, into `out` in a layout launch() takes -- kCompact, kFull-shaped with only the window written,
// or kRing-shaped (one frame, rows 2048 floats apart, `out` standing for the snapshot's start) --, band b's out_plane floats
// behind band b-1's.  Sample j of (frame f, stream id) is in[f * in_frame + id * in_row + j]; in_lo = where history sample wstart
// is in such a row, with the longest band's taps - 1 samples in front of it (the caller has seen to that).  What is written is
// what a band-less call stages: the window rounded up as compact_hist is, cut at the end of the history.
int band_cut(awpu_hip *h, const BandSet &bands, const float *in, long long in_frame, long long in_row, int in_lo, int batch, float *out,
             long long out_plane, int layout, hipStream_t s) {
    const int S = h->cfg.n_streams;
    const long long out_row = layout == kCompact ? h->compact_hist : (layout == kRing ? 2048 : h->cfg.hist);
    const long long out_frame = layout == kRing ? 0 : out_row * S;
    const int out_first = layout == kCompact ? 0 : h->wstart;
    const int n = std::min(((h->window + 3) & ~3) + 4, h->cfg.hist - h->wstart);
    if (bands.n == 1) {
        awpu::BandArgs a{};
        a.in = in;
        a.in_frame = in_frame, a.in_row = in_row;
        a.in_first = in_lo - (bands.taps[0] - 1);
        a.out = out;
        a.out_row = out_row, a.out_frame = out_frame, a.out_first = out_first;
        a.n = n;
        a.index = h->d_index;
        a.usable = h->usable();
        a.n_frames = batch;
        a.taps = bands.taps[0];
        std::copy(bands.coef[0], bands.coef[0] + bands.taps[0], a.coef);
        AWPU_HIP_TRY(awpu::launch_band_filter(a, s));
        return AWPU_OK;
    }
    awpu::SpectralBandArgs a{};
    a.in = in;
    a.in_frame = in_frame, a.in_row = in_row;
    a.in_first = in_lo - (bands.max_taps() - 1);
    a.out = out;
    a.out_row = out_row, a.out_frame = out_frame, a.out_plane = out_plane, a.out_first = out_first;
    a.n = n;
    a.index = h->d_index;
    a.usable = h->usable();
    a.n_frames = batch;
    a.n_bands = bands.n;
    a.max_taps = bands.max_taps();
    for (int b = 0; b < bands.n; b++) {
        a.taps[b] = bands.taps[b];
        std::copy(bands.coef[b], bands.coef[b] + bands.taps[b], a.coef[b]);
    }
    AWPU_HIP_TRY(awpu::launch_spectral_filter(a, s));
    return AWPU_OK;
}

// launch() on frames of the caller's or the ring's (kFull, kRing), or on windows uploaded with the bands' history in front of them
// (kCompact: rows of max taps - 1 + compact_hist floats), through the bands where there are any: the pre-pass into d_band in
// `layout`, a plane per band, then for every band the launch() a band-less handle makes for the same call -- the same layout and
// batch, so the same kernel -- into d_power + b * power_plane.  A timed call's event bracket spans all of it: recorded here, the
// sweeps behind the pre-pass untimed.  With `own` the sweep behind the pre-pass is the caller's (the coherence sweep of
// awpu_hip_cohere.h, the tone sweep of awpu_hip_tones.h: at most one band, d_power unused)
int band_sweep(awpu_hip *h, const BandSet &bands, const float *in, long long in_frame, long long in_row, int in_lo, int batch, float *d_power,
               long long power_plane, hipStream_t s, int layout, const SweepOpts &o, const OwnSweep *own) {
    const auto sweep = [&](const float *frames, float *power, const SweepOpts &so) {
        return own ? (*own)(frames, so.timed) : launch(h, frames, batch, power, s, layout, so);
    };
    if (bands.n == 0) return sweep(in, d_power, o);
    const size_t S = (size_t) h->cfg.n_streams;
    const size_t plane = layout == kRing ? S * 2048 : S * (size_t) (layout == kCompact ? h->compact_hist : h->cfg.hist) * batch;
    const size_t need = plane * bands.n;
    if (!h->d_band.holds(need)) {  // (what no pre-pass writes and a sweep's wide loads may touch reads as zeros)
        if (const int rc = h->d_band.grow(need); rc != AWPU_OK) return rc;
        AWPU_HIP_TRY(hipMemsetAsync(h->d_band, 0, need * sizeof(float), s));
    }
    if (o.timed) AWPU_HIP_TRY(hipEventRecord(h->ev_begin, s));
    int rc = band_cut(h, bands, in, in_frame, in_row, in_lo, batch, h->d_band, (long long) plane, layout, s);
    const SweepOpts untimed{false, o.sums, o.flag};
    for (int b = 0; b < bands.n && rc == AWPU_OK; b++) rc = sweep(h->d_band + b * plane, d_power + b * power_plane, untimed);
    if (rc == AWPU_OK && o.timed) AWPU_HIP_TRY(hipEventRecord(h->ev_end, s));
    return rc;
}

}  // namespace awpu::host

namespace {

// One frame in, one heatmap out, synchronously: the call MIMOWorker::update makes once per 256-sample block (mimo.cpp:100-103 is the
// snapshot it replaces).  The caller's buffers are pageable (std::vector, mimo.h:83-88): a device copy straight out of / into them goes
// through the runtime's own bounce buffers in several synchronous steps (measured at the reference's default shape: 58-64 us per call
// around a 20 us sweep).  Here the touched window of every stream is gathered into a PINNED buffer of the handle by the CPU (64 rows x
// 1.2 KB), crosses PCIe in ONE piece read by a small kernel (a DMA-engine copy of 75 KB is mostly start-up), and the sweep stores its
// powers straight into a pinned buffer.  Measured at the reference's shape (C level; Python adds ~5 us): 53 -> 43 us exact, 48 -> 38 us
// fast, and -- with the event bracket around the sweep sampled instead of recorded on every call -- 42 / 37 us: gather 1.3, the two launches
// 2.8 + ~3, then ~33 us until the stream is idle (upload 3 + sweep 21.6 / 19.5 + dispatch latencies + the end-of-kernel release and its
// signal), copy out 2.0; and in the default mode at the reference's shape -- completion by a flag the resident kernel's last workgroup
// stores behind its powers (launch_exact_ndh: done_*) instead of by the stream's signal -- 36.5 us.  Measured and not kept: spinning on
// hipStreamQuery instead of hipStreamSynchronize (equal); a stream-written flag (hipStreamWriteValue32: 18 us slower); the workgroup flag
// with the powers written through as they are stored (10 000 acknowledged four-byte PCIe writes: +60 us; gathered into 64-byte lines
// first: what ships).
int live_host_call(awpu_hip *h, const float *frames, float *power) {
    int rc = check_ready(h, 1);
    if (rc == AWPU_OK) rc = enter_stream(h, h->stream);
    if (rc != AWPU_OK) return rc;
    const bool compact = h->compact_hist > 0;
    const int dev_hist = compact ? h->compact_hist : h->cfg.hist;
    const size_t need_frames = (size_t) h->cfg.n_streams * dev_hist;
    rc = h->d_frames.ensure(need_frames);
    if (rc == AWPU_OK) rc = ensure_power(h, (size_t) h->cfg.pixel_count);
    if (rc == AWPU_OK) rc = h->h_live_in.ensure(need_frames);
    if (rc == AWPU_OK) rc = h->h_live_out.ensure((size_t) h->cfg.pixel_count);
    if (rc != AWPU_OK) return rc;
#ifdef AWPU_TUNING_BUILD
    static const bool live_timing = std::getenv("AWPU_LIVE_TIMING") != nullptr;
    static double t_acc[5] = {0, 0, 0, 0, 0};
    static long t_calls = 0;
    const auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](int k, std::chrono::steady_clock::time_point &from) {
        const auto now = std::chrono::steady_clock::now();
        t_acc[k] += std::chrono::duration<double, std::micro>(now - from).count();
        from = now;
    };
    auto t = t0;
#endif
    if (compact) {  // rows of compact_hist floats cut out of rows of hist floats
        for (int s = 0; s < h->cfg.n_streams; s++)
            std::memcpy(h->h_live_in + (size_t) s * dev_hist, frames + (size_t) s * h->cfg.hist + h->wstart, (size_t) dev_hist * sizeof(float));
    } else {
        std::memcpy(h->h_live_in, frames, need_frames * sizeof(float));
    }
#ifdef AWPU_TUNING_BUILD
    if (live_timing) lap(0, t);
#endif
    // the upload: by a kernel that reads the pinned buffer over PCIe (a DMA-engine copy of 75 KB is mostly start-up: 8.6 us measured);
    // windows that are no whole number of 16-byte pieces (never, with compact rows) take the DMA copy
    if ((need_frames & 3) == 0) {
        AWPU_HIP_TRY(awpu::launch_upload_floats(h->h_live_in, h->d_frames, need_frames, h->stream));
    } else {
        AWPU_HIP_TRY(hipMemcpyAsync(h->d_frames, h->h_live_in, need_frames * sizeof(float), hipMemcpyHostToDevice, h->stream));
    }
#ifdef AWPU_TUNING_BUILD
    if (live_timing) lap(1, t);
#endif
    // (the sweep stores its powers straight into the pinned buffer -- one 4-byte store per pixel over PCIe, complete when the kernel
    // is: a device-to-host copy behind the sweep would be one more DMA start-up, ~10 us, for 40 KB)
    // the event bracket around the sweep (awpu_hip_stats.last_kernel_ms) is two more packets on the stream and two more runtime calls:
    // 3.3 us of a call of 50 (measured from Python, both modes).  This path brackets its first call and every 32nd after it; the other
    // calls leave last_kernel_ms / total_kernel_ms as they are
    {
        const bool timed = (h->live_calls++ & 31) == 0;
        bool flagged = false;  // this call's sweep will raise the completion flag (a timed call waits for the stream: its end event)
        rc = launch(h, h->d_frames, 1, h->h_live_out, h->stream, compact ? kCompact : kFull, {timed, nullptr, timed ? nullptr : &flagged});
        if (rc == AWPU_OK) {
#ifdef AWPU_TUNING_BUILD
            if (live_timing) lap(2, t);
#endif
            bool seen = false;
            if (flagged) {
                // the sweep's last workgroup stores the call's number behind its powers (das_fast.hip: store_tile_and_signal): ~7 us
                // sooner than the stream's completion signal.  Should it not arrive within 20 ms (it arrives within the sweep's ~25 us),
                // the stream's own completion decides
                const auto spin_from = std::chrono::steady_clock::now();
                for (unsigned spins = 0;; spins++) {
                    if (__atomic_load_n(h->h_done_flag.get(), __ATOMIC_ACQUIRE) == h->done_seq) {
                        seen = true;
                        break;
                    }
                    __builtin_ia32_pause();
                    if ((spins & 0xfff) == 0xfff && std::chrono::steady_clock::now() - spin_from > std::chrono::milliseconds(20)) break;
                }
            }
            if (!seen) rc = wait_and_time(h, timed);
        }
    }
    if (rc != AWPU_OK) return rc;
#ifdef AWPU_TUNING_BUILD
    if (live_timing) lap(3, t);
#endif
    std::memcpy(power, h->h_live_out, (size_t) h->cfg.pixel_count * sizeof(float));
#ifdef AWPU_TUNING_BUILD
    if (live_timing) {
        lap(4, t);
        if (++t_calls == 5) for (double &v : t_acc) v = 0;  // (the first calls build tables and raise limits)
        if (t_calls > 5 && (t_calls - 5) % 100 == 0) {
            std::fprintf(stderr, "[awpu live] per call us: gather %.1f | hipMemcpyAsync H2D %.1f | launch() %.1f | wait %.1f | copy out %.1f\n", t_acc[0] / 100,
                         t_acc[1] / 100, t_acc[2] / 100, t_acc[3] / 100, t_acc[4] / 100);
            for (double &v : t_acc) v = 0;
        }
    }
#endif
    return AWPU_OK;
}

}  // namespace

int awpu::host::wait_and_time(awpu_hip *h, bool timed) {
    AWPU_HIP_TRY(hipSetDevice(h->cfg.device));
    AWPU_HIP_TRY(hipStreamSynchronize(h->stream));
    if (timed) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, h->ev_begin, h->ev_end) == hipSuccess) {
            h->stats.last_kernel_ms = ms;
            h->stats.total_kernel_ms += ms;
        }
    }
    return AWPU_OK;
}

// what the runs of blocks (run_pieces.cpp) share with the calls below
namespace awpu::host {

size_t align16(size_t n) { return (n + 15) & ~(size_t) 15; }

static_assert(sizeof(awpu_particle_t) == 80, "awpu_particle_t is part of the ABI (include/awpu_hip_track.h)");

// what awpu_hip_track and the listen calls ask of their particles (none of it reads the handle)
int check_particles(const awpu_particle_t *p, int32_t n, double theta_limit, double reference) {
    if (n < 1 || n > 65535) return invalid("n outside [1, 65535]");
    if (!(theta_limit > 0.0) || !std::isfinite(theta_limit)) return invalid("theta_limit must be finite and > 0");
    if (!std::isfinite(reference)) return invalid("reference not finite");
    for (int k = 0; k < n; k++) {
        if (p[k].steps < 0 || p[k].steps > 4096) return invalid("steps outside [0, 4096]");
        if (!std::isfinite(p[k].theta) || !std::isfinite(p[k].phi) || !std::isfinite(p[k].spread) || !std::isfinite(p[k].rate))
            return invalid("particle direction, spread or rate not finite");
    }
    return AWPU_OK;
}

// ... and of the handle: the antenna, and the active mics inside it
int check_antenna(const awpu_hip *h) {
    if (h->antenna.empty()) return fail(AWPU_ERR_STATE, "antenna not set (awpu_hip_set_antenna)");
    if (!h->have_mics || h->index.empty()) return fail(AWPU_ERR_STATE, "active mics not set");
    const int n_el = (int) (h->antenna.size() / 3);
    for (int id : h->index)
        if (id >= n_el) return fail(AWPU_ERR_STATE, "an active mic is not an element of the antenna");
    return AWPU_OK;
}

// d_track_index = the active mics
int ensure_track_index(awpu_hip *h) {
    const int U = h->usable();
    if (h->track_index == h->index) return AWPU_OK;
    if (const int rc = h->d_track_index.ensure((size_t) U); rc != AWPU_OK) return rc;
    h->track_index.clear();
    AWPU_HIP_TRY(hipMemcpy(h->d_track_index, h->index.data(), (size_t) U * sizeof(int32_t), hipMemcpyHostToDevice));
    h->track_index = h->index;
    return AWPU_OK;
}

// the ingest ring and its one-block staging, allocated at first use: the ring starts zeroed (on h->stream)
int ensure_ring(awpu_hip *h) {
    if (h->d_ring) return AWPU_OK;
    const size_t ring_bytes = (size_t) h->cfg.n_streams * 2048 * sizeof(float);
    if (const int rc = h->d_ring.ensure((size_t) h->cfg.n_streams * 2048); rc != AWPU_OK) return rc;
    AWPU_HIP_TRY(hipMemsetAsync(h->d_ring, 0, ring_bytes, h->stream));
    if (const int rc = h->d_datagrams.ensure((size_t) awpu::kSamples * AWPU_DATAGRAM_BYTES); rc != AWPU_OK) return rc;
    h->ring_pos = 0;
    return AWPU_OK;
}

// H2D of one block of raw datagrams + the unpack launch, enqueued on the handle's stream (no wait)
int enqueue_ingest(awpu_hip *h, const void *datagrams, int32_t stride_bytes) {
    if (!h || !datagrams) return invalid("null argument");
    if (h->cfg.hist != AWPU_HIST || h->cfg.n_streams > 256) return invalid("ingest needs hist 1024 and <= 256 streams");
    if (stride_bytes < AWPU_DATAGRAM_BYTES) return invalid("datagram stride below 1032 bytes");
    AWPU_HIP_TRY(hipSetDevice(h->cfg.device));
    int rc = enter_stream(h, h->stream);
    if (rc == AWPU_OK) rc = ensure_ring(h);
    if (rc != AWPU_OK) return rc;
    // tight copy of the 256 datagrams (the header travels too: 8 bytes each, ignored like the
    // reference ignores msg.counter, pipeline.cpp:264-267)
    AWPU_HIP_TRY(hipMemcpy2DAsync(h->d_datagrams, AWPU_DATAGRAM_BYTES, datagrams, (size_t) stride_bytes,
                                  AWPU_DATAGRAM_BYTES, awpu::kSamples, hipMemcpyHostToDevice, h->stream));
    AWPU_HIP_TRY(awpu::launch_unpack_block(h->d_datagrams, AWPU_DATAGRAM_BYTES, h->cfg.n_streams, h->d_ring,
                                           h->ring_pos, h->stream));
    h->ring_pos = (h->ring_pos + awpu::kSamples) % AWPU_HIST;  // Streams::forward
    return AWPU_OK;
}

// h->d_taps = the column and row taps of rows x cols -> out_rows x out_cols, rebuilt when the shape changes
int ensure_taps(awpu_hip *h, int rows, int cols, int out_rows, int out_cols, hipStream_t s) {
    const int key[4] = {rows, cols, out_rows, out_cols};
    if (!h->d_taps || std::memcmp(key, h->taps_key, sizeof(key)) != 0) {
        std::vector<awpu::ResizeTap> taps((size_t) out_cols + out_rows);
        awpu::resize_taps(cols, out_cols, true, taps.data());
        awpu::resize_taps(rows, out_rows, false, taps.data() + out_cols);
        AWPU_HIP_TRY(hipStreamSynchronize(s));  // an earlier launch may still read the old taps
        retire_live_graphs(h);
        if (const int rc = h->d_taps.grow(taps.size()); rc != AWPU_OK) return rc;
        AWPU_HIP_TRY(hipMemcpy(h->d_taps, taps.data(), taps.size() * sizeof(awpu::ResizeTap), hipMemcpyHostToDevice));
        std::memcpy(h->taps_key, key, sizeof(key));
        h->taps_band_rows = awpu::watch_band_rows(taps.data() + out_cols, rows, out_rows);
    }
    return AWPU_OK;
}

}  // namespace awpu::host

extern "C" {

void awpu_hip_default_cfg(awpu_hip_cfg *cfg) {
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = (int32_t) sizeof(*cfg);
    cfg->device = 0;
    cfg->n_streams = AWPU_ELEMENTS;
    cfg->hist = AWPU_HIST;
    cfg->n_pixels = 0;
    cfg->lut_stride = AWPU_ELEMENTS;
    cfg->interp = AWPU_INTERP_LERP;
    cfg->math = AWPU_MATH_F32_EXACT;  // the reference has one arithmetic (delay.cpp:19-25 inside mimo.cpp:121-137): that one; FAST is an opt-in
    cfg->max_batch = 1;
    cfg->pixel_begin = 0;
    cfg->pixel_count = 0;
}

int awpu_hip_create(awpu_hip_t **out, const awpu_hip_cfg *cfg) {
    if (!out || !cfg) return invalid("null argument");
    *out = nullptr;
    if (cfg->struct_size != (int32_t) sizeof(awpu_hip_cfg)) return invalid("cfg.struct_size");
    if (cfg->n_streams < 1 || cfg->lut_stride < 1 || cfg->n_pixels < 1 || cfg->max_batch < 1)
        return invalid("n_streams, lut_stride, n_pixels and max_batch must be >= 1");
    if (cfg->hist < AWPU_N_SAMPLES + 1) return invalid("hist must hold at least 257 samples");
    if (cfg->max_batch > 65535) return invalid("max_batch above 65535");
    if (cfg->interp != AWPU_INTERP_LERP && cfg->interp != AWPU_INTERP_FIR8) return invalid("cfg.interp");
    if (cfg->math != AWPU_MATH_F32_EXACT && cfg->math != AWPU_MATH_F32_FAST && cfg->math != AWPU_MATH_BF16_ACC)
        return invalid("cfg.math");
    if (cfg->math == AWPU_MATH_BF16_ACC && cfg->interp != AWPU_INTERP_LERP)
        return invalid("the bf16 accumulator is built for the linear interpolation only");
    awpu_hip_cfg c = *cfg;
    if (c.pixel_count == 0) {
        c.pixel_begin = 0;
        c.pixel_count = c.n_pixels;
    }
    if (c.pixel_begin < 0 || c.pixel_count < 1 || c.pixel_begin + c.pixel_count > c.n_pixels)
        return invalid("pixel shard outside the grid");
    if (c.window_begin != 0 || c.window_end != 0) {
        const int reach = c.interp == AWPU_INTERP_FIR8 ? 263 : 257;
        if (c.window_begin < 0 || c.window_end > c.hist || c.window_end - c.window_begin < reach)
            return invalid("window_begin/window_end outside the history or narrower than one delay() read");
    }

    if (c.n_devices > 1) return create_group(out, c);
    c.n_devices = 1;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1 || c.device < 0 || c.device >= n_dev) {
        return fail(AWPU_ERR_NO_DEVICE, "no usable HIP device (this library has no CPU path)");
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c.device) != hipSuccess ||
        std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        return fail(AWPU_ERR_NO_DEVICE, "device is not gfx950 (MI355X); kernels are built for gfx950 only");
    }
    AWPU_HIP_TRY(hipSetDevice(c.device));

    awpu_hip *h = new (std::nothrow) awpu_hip();
    if (!h) return AWPU_ERR_NOMEM;
    h->cfg = c;
    const char *what = "stream/event creation";
    int rc = h->stream.ensure(what);
    if (rc == AWPU_OK) rc = h->ev_begin.ensure(hipEventDefault, what);
    if (rc == AWPU_OK) rc = h->ev_end.ensure(hipEventDefault, what);
    h->last_stream = h->stream;
    if (rc != AWPU_OK) {
        awpu_hip_destroy(h);
        return rc;
    }
    *out = h;
    return AWPU_OK;
}

int awpu_hip_destroy(awpu_hip_t *h) {
    if (!h) return AWPU_OK;
    for (awpu_hip *part : h->group.parts) awpu_hip_destroy(part);
    h->group.parts.clear();
    (void) hipSetDevice(h->cfg.device);
    if (h->stream) (void) hipStreamSynchronize(h->stream);
    if (h->copy_stream) (void) hipStreamSynchronize(h->copy_stream);
    if (h->listen_stream) (void) hipStreamSynchronize(h->listen_stream);
    retire_live_graphs(h);
    free_tables(h);
    delete h;  // buffers, events and streams go with their owners (awpu_handle.h)
    return AWPU_OK;
}

int awpu_hip_set_delay_table(awpu_hip_t *h, const int32_t *off, const float *frac) {
    AWPU_CTX(h);
    if (!h || !off || !frac) return invalid("null argument");
    if (is_group(h)) return group_set_delay_table(h, off, frac);
    const size_t n = (size_t) h->cfg.pixel_count * h->cfg.lut_stride;
    for (size_t i = 0; i < n; i++) {
        if (!(frac[i] >= 0.0f && frac[i] <= 1.0f)) return invalid("fraction outside [0, 1]");
    }
    h->off.assign(off, off + n);
    h->frac.assign(frac, frac + n);
    h->have_table = true;
    h->prepared = false;
    return AWPU_OK;
}

int awpu_hip_set_active_mics(awpu_hip_t *h, const int32_t *index, int32_t usable) {
    AWPU_CTX(h);
    if (!h) return invalid("null handle");
    if (is_group(h)) return group_set_active_mics(h, index, usable);
    const int limit = std::min(h->cfg.n_streams, h->cfg.lut_stride);
    if (usable < 1 || usable > limit) return invalid("usable outside [1, min(n_streams, lut_stride)]");
    std::vector<int32_t> idx(usable);
    for (int s = 0; s < usable; s++) {
        idx[s] = index ? index[s] : s;
        if (idx[s] < 0 || idx[s] >= limit) return invalid("mic id outside the streams / table");
    }
    h->index.swap(idx);
    h->have_mics = true;
    h->prepared = false;
    return AWPU_OK;
}

int awpu_hip_set_mic_gains(awpu_hip_t *h, const float *gains) {
    AWPU_CTX(h);
    if (!h) return invalid("null handle");
    if (is_group(h)) return group_set_mic_gains(h, gains);
    if (!gains) {
        h->gain.clear();
    } else {
        for (int s = 0; s < h->cfg.n_streams; s++)
            if (!std::isfinite(gains[s])) return invalid("gain not finite");
        h->gain.assign(gains, gains + h->cfg.n_streams);
    }
    h->prepared = false;
    return AWPU_OK;
}

namespace {

// aw_processing_unit.cpp:145-200 on the 64 mean squares of one array.  The reference sorts with operator<, which is no order
// once a mean square is NaN (a NaN sample in the stream): the median then depends on where the NaN stands, and the NaN stream
// passes both tests below (every comparison with NaN is false).  Defined here, and in oracle_calibrate alike: NaN sorts last
// -- finite values ascending, then +inf, then NaN --, and a mic is usable only if its mean square and the median are finite
// and the reference's two tests pass.  On all-finite mean squares these are the reference's bits.
int usable_from_power(const float *power, float reference_power_level, int32_t *index, float *correction,
                      float *median_out) {
    float sorted[AWPU_ELEMENTS];
    std::copy(power, power + AWPU_ELEMENTS, sorted);
    std::sort(sorted, sorted + AWPU_ELEMENTS, [](float a, float b) { return std::isnan(b) ? !std::isnan(a) : a < b; });
    // the reference averages elements 32 and 33 of the sorted list (.cpp:150), in double, then rounds
    const float median = (float) ((sorted[AWPU_ELEMENTS / 2] + sorted[AWPU_ELEMENTS / 2 + 1]) / 2.0);
    int count = 0;
    for (int s = 0; s < AWPU_ELEMENTS; s++) {
        const bool far_off = std::fabs(power[s] - median) > 1e-4;  // float promoted against a double bound
        const bool dead = power[s] < median * 1e-3;
        if (!std::isfinite(power[s]) || !std::isfinite(median) || far_off || dead) continue;
        index[count] = s;
        correction[count] = reference_power_level / power[s];
        count++;
    }
    if (median_out) *median_out = median;
    return count;
}

int calibrate_rows(awpu_hip *h, const float *d_rows, int pitch, int hist, float reference_power_level, int32_t *index,
                   float *correction, float *median, int32_t *usable, hipStream_t s) {
    if (const int rc = h->d_calib.ensure(AWPU_ELEMENTS); rc != AWPU_OK) return rc;
    AWPU_HIP_TRY(awpu::launch_stream_power(d_rows, pitch, hist, AWPU_ELEMENTS, h->d_calib, s));
    float power[AWPU_ELEMENTS];
    AWPU_HIP_TRY(hipMemcpyAsync(power, h->d_calib, sizeof(power), hipMemcpyDeviceToHost, s));
    AWPU_HIP_TRY(hipStreamSynchronize(s));
    *usable = usable_from_power(power, reference_power_level, index, correction, median);
    return AWPU_OK;
}

}  // namespace

int awpu_hip_calibrate_device(awpu_hip_t *h, const float *d_frame, int32_t array, float reference_power_level,
                              int32_t *index, float *correction, float *median, int32_t *usable, void *stream) {
    h = first_device(h);
    AWPU_CTX(h);
    if (!h || !d_frame || !index || !correction || !usable) return invalid("null argument");
    if (array < 0 || (array + 1) * AWPU_ELEMENTS > h->cfg.n_streams) return invalid("array outside the streams");
    if (h->cfg.hist > 16384) return invalid("history too long for the calibration kernel");
    AWPU_HIP_TRY(hipSetDevice(h->cfg.device));
    hipStream_t s = stream_of(h, stream);
    if (const int rc = enter_stream(h, s); rc != AWPU_OK) return rc;
    return calibrate_rows(h, d_frame + (size_t) array * AWPU_ELEMENTS * h->cfg.hist, h->cfg.hist, h->cfg.hist,
                          reference_power_level, index, correction, median, usable, s);
}

int awpu_hip_calibrate_host(awpu_hip_t *h, const float *frame, int32_t array, float reference_power_level,
                             int32_t *index, float *correction, float *median, int32_t *usable) {
    const bool busy = h && h->in_flight;  // (the staging buffer below is the one an asynchronous call uploads into)
    h = first_device(h);
    AWPU_CTX(h);
    if (!h || !frame || !index || !correction || !usable) return invalid("null argument");
    if (array < 0 || (array + 1) * AWPU_ELEMENTS > h->cfg.n_streams) return invalid("array outside the streams");
    if (h->cfg.hist > 16384) return invalid("history too long for the calibration kernel");
    if (busy) return fail(AWPU_ERR_STATE, "an awpu_hip_process_async call is in flight on this handle: awpu_hip_wait first");
    AWPU_HIP_TRY(hipSetDevice(h->cfg.device));
    if (const int rc = enter_stream(h, h->stream); rc != AWPU_OK) return rc;
    // only the array's 64 streams travel; they share the frame staging buffer of awpu_hip_process
    const size_t need = (size_t) AWPU_ELEMENTS * h->cfg.hist;
    if (const int rc = h->d_frames.ensure(need); rc != AWPU_OK) return rc;
    AWPU_HIP_TRY(hipMemcpyAsync(h->d_frames, frame + (size_t) array * AWPU_ELEMENTS * h->cfg.hist, need * sizeof(float),
                                hipMemcpyHostToDevice, h->stream));
    return calibrate_rows(h, h->d_frames, h->cfg.hist, h->cfg.hist, reference_power_level, index, correction, median,
                          usable, h->stream);
}

int awpu_hip_calibrate_ring(awpu_hip_t *h, int32_t array, float reference_power_level, int32_t *index,
                            float *correction, float *median, int32_t *usable) {
    h = first_device(h);
    AWPU_CTX(h);
    if (!h || !index || !correction || !usable) return invalid("null argument");
    if (array < 0 || (array + 1) * AWPU_ELEMENTS > h->cfg.n_streams) return invalid("array outside the streams");
    if (!h->d_ring) {
        return fail(AWPU_ERR_STATE, "no block ingested yet");
    }
    AWPU_HIP_TRY(hipSetDevice(h->cfg.device));
    if (const int rc = enter_stream(h, h->stream); rc != AWPU_OK) return rc;
    return calibrate_rows(h, h->d_ring + (size_t) array * AWPU_ELEMENTS * 2048 + h->ring_pos, 2048, AWPU_HIST,
                          reference_power_level, index, correction, median, usable, h->stream);
}

int awpu_hip_beams(awpu_hip_t *h, const float *d_frame, const int32_t *off, const float *frac, int32_t n_dir,
                   float *power, float *beams) {
    h = first_device(h);
    AWPU_CTX(h);
    if (!h || !off || !frac || (!power && !beams)) return invalid("null argument");
    if (n_dir < 1 || n_dir > 65535) return invalid("n_dir outside [1, 65535]");
    if (!h->have_mics) {
        return fail(AWPU_ERR_STATE, "active mics not set");
    }
    int pitch = h->cfg.hist;
    const float *frame = d_frame;
    if (!frame) {  // the current snapshot of the ingest ring
        if (!h->d_ring) {
            return fail(AWPU_ERR_STATE, "no block ingested yet");
        }
        frame = h->d_ring + h->ring_pos;
        pitch = 2048;
    }
    const int U = h->usable(), stride = h->cfg.lut_stride;
    std::vector<awpu::LutEntry> entries((size_t) n_dir * U);
    for (int d = 0; d < n_dir; d++) {
        for (int s = 0; s < U; s++) {
            const int id = h->index[s];
            const int o = off[(size_t) d * stride + id];
            const float f = frac[(size_t) d * stride + id];
            if (o < 0 || o + awpu::kSamples > h->cfg.hist - 1) {  // delay() reads X[off .. off+256]
                return fail(AWPU_ERR_RANGE, "delay table entry reads outside the frame history");
            }
            if (!(f >= 0.0f && f <= 1.0f)) return invalid("fraction outside [0, 1]");
            entries[(size_t) d * U + s] = awpu::LutEntry{id * pitch + o, f};
        }
    }
    AWPU_HIP_TRY(hipSetDevice(h->cfg.device));
    if (const int rc = enter_stream(h, h->stream); rc != AWPU_OK) return rc;
    if (const int rc = h->d_beam_lut.ensure(entries.size()); rc != AWPU_OK) return rc;
    if (const int rc = h->d_beam_out.ensure((size_t) n_dir * (1 + awpu::kSamples)); rc != AWPU_OK) return rc;
    // [n] powers then [n][256] beams, n = the directions the buffer was allocated for (its layout follows its allocation)
    float *d_power = h->d_beam_out, *d_beams = h->d_beam_out + h->d_beam_out.cap / (1 + awpu::kSamples);
    AWPU_HIP_TRY(hipMemcpyAsync(h->d_beam_lut, entries.data(), entries.size() * sizeof(awpu::LutEntry),
                                hipMemcpyHostToDevice, h->stream));
    AWPU_HIP_TRY(awpu::launch_das_beams(frame, h->d_beam_lut, U, n_dir, d_power, beams ? d_beams : nullptr, h->stream));
    if (power)
        AWPU_HIP_TRY(hipMemcpyAsync(power, d_power, (size_t) n_dir * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (beams)
        AWPU_HIP_TRY(hipMemcpyAsync(beams, d_beams, (size_t) n_dir * awpu::kSamples * sizeof(float),
                                    hipMemcpyDeviceToHost, h->stream));
    AWPU_HIP_TRY(hipStreamSynchronize(h->stream));  // `entries` must outlive the upload
    return AWPU_OK;
}

// ---- particle tracking (include/awpu_hip_track.h; kernels in track_kernels.hip) ---------------------------------------

int awpu_hip_set_antenna(awpu_hip_t *h, const float *xyz, int32_t n) {
    h = first_device(h);
    AWPU_CTX(h);
    if (!h || !xyz) return invalid("null argument");
    if (n < 1 || n > h->cfg.lut_stride) return invalid("n outside [1, lut_stride]");
    for (int k = 0; k < 3 * n; k++)
        if (!std::isfinite(xyz[k])) return invalid("element position not finite");
    // the aperture in samples bounds every delay a direction can form (tau = projection * scale - its minimum), so
    // with it at most 256 every table entry has off in [0, 256] and delay() reads inside [0, 512]
    double widest = 0.0;
    for (int a = 0; a < n; a++)
        for (int b = a + 1; b < n; b++) {
            const double dx = (double) xyz[a] - xyz[b], dy = (double) xyz[n + a] - xyz[n + b], dz = (double) xyz[2 * n + a] - xyz[2 * n + b];
            widest = std::max(widest, dx * dx + dy * dy + dz * dz);
        }
    if (std::sqrt(widest) * (48828.0 / 340.0) > (double) awpu::kSamples)
        return fail(AWPU_ERR_RANGE, "antenna aperture exceeds 256 samples: delays would read outside the frame history");
    AWPU_HIP_TRY(hipSetDevice(h->cfg.device));
    if (h->antenna.size() != (size_t) 3 * n) {
        h->antenna.clear();
        if (const int rc = h->d_xyz.grow((size_t) 3 * n); rc != AWPU_OK) return rc;
    }
    AWPU_HIP_TRY(hipMemcpy(h->d_xyz, xyz, (size_t) 3 * n * sizeof(float), hipMemcpyHostToDevice));
    h->antenna.assign(xyz, xyz + (size_t) 3 * n);
    return AWPU_OK;
}

int awpu_hip_steer_table_device(awpu_hip_t *h, const double *theta, const double *phi, int32_t n_dir, int32_t *off,
                                float *frac) {
    h = first_device(h);
    AWPU_CTX(h);
    if (!h || !theta || !phi || !off || !frac) return invalid("null argument");
    if (n_dir < 1 || n_dir > 65535) return invalid("n_dir outside [1, 65535]");
    if (h->antenna.empty()) return fail(AWPU_ERR_STATE, "antenna not set (awpu_hip_set_antenna)");
    const int n = (int) (h->antenna.size() / 3);
    AWPU_HIP_TRY(hipSetDevice(h->cfg.device));
    if (int rc = enter_stream(h, h->stream)) return rc;
    const size_t angles = align16((size_t) n_dir * sizeof(double)), table = (size_t) n_dir * n;
    if (int rc = h->d_track.ensure(2 * angles + table * (sizeof(int32_t) + sizeof(float)))) return rc;
    double *d_theta = (double *) h->d_track.get(), *d_phi = (double *) (h->d_track + angles);
    int32_t *d_off = (int32_t *) (h->d_track + 2 * angles);
    float *d_frac = (float *) (d_off + table);
    AWPU_HIP_TRY(hipMemcpyAsync(d_theta, theta, (size_t) n_dir * sizeof(double), hipMemcpyHostToDevice, h->stream));
    AWPU_HIP_TRY(hipMemcpyAsync(d_phi, phi, (size_t) n_dir * sizeof(double), hipMemcpyHostToDevice, h->stream));
    AWPU_HIP_TRY(awpu::launch_steer_table(h->d_xyz, n, d_theta, d_phi, n_dir, d_off, d_frac, h->stream));
    AWPU_HIP_TRY(hipMemcpyAsync(off, d_off, table * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    AWPU_HIP_TRY(hipMemcpyAsync(frac, d_frac, table * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    AWPU_HIP_TRY(hipStreamSynchronize(h->stream));
    return AWPU_OK;
}

int awpu_hip_track(awpu_hip_t *h, const float *d_frame, awpu_particle_t *p, int32_t n, double theta_limit,
                   double reference, double *reference_used, float *beams) {
    h = first_device(h);
    AWPU_CTX(h);
    if (!h || !p) return invalid("null argument");
    if (int rc = check_particles(p, n, theta_limit, reference)) return rc;
    if (int rc = check_antenna(h)) return rc;
    const int n_el = (int) (h->antenna.size() / 3);
    int pitch = h->cfg.hist;
    const float *frame = d_frame;
    if (!frame) {  // the current snapshot of the ingest ring
        if (!h->d_ring) return fail(AWPU_ERR_STATE, "no block ingested yet");
        frame = h->d_ring + h->ring_pos;
        pitch = 2048;
    } else if (h->cfg.hist < 2 * awpu::kSamples + 1) {
        return fail(AWPU_ERR_RANGE, "history shorter than 513 samples: a steered delay can read outside it");
    }
    AWPU_HIP_TRY(hipSetDevice(h->cfg.device));
    if (int rc = enter_stream(h, h->stream)) return rc;
    const int U = h->usable();
    if (int rc = ensure_track_index(h)) return rc;
    const size_t particles = (size_t) n * sizeof(awpu_particle_t), head = align16(particles + sizeof(double));
    if (int rc = h->d_track.ensure(head + (beams ? (size_t) n * awpu::kSamples * sizeof(float) : 0))) return rc;
    awpu::TrackArgs a{};
    a.frame = frame;
    a.pitch = pitch;
    a.xyz = h->d_xyz;
    a.n = n_el;
    a.index = h->d_track_index;
    a.usable = U;
    a.particles = h->d_track;
    a.n_particles = n;
    a.theta_limit = theta_limit;
    a.reference = reference;
    a.reference_out = (double *) (h->d_track + particles);
    a.beams = beams ? (float *) (h->d_track + head) : nullptr;
    AWPU_HIP_TRY(hipMemcpyAsync(h->d_track, p, particles, hipMemcpyHostToDevice, h->stream));
    AWPU_HIP_TRY(awpu::launch_track(a, h->stream));
    double used = 0.0;
    std::vector<unsigned char> back(particles + sizeof(double));
    AWPU_HIP_TRY(hipMemcpyAsync(back.data(), h->d_track, back.size(), hipMemcpyDeviceToHost, h->stream));
    if (beams)
        AWPU_HIP_TRY(hipMemcpyAsync(beams, a.beams, (size_t) n * awpu::kSamples * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    AWPU_HIP_TRY(hipStreamSynchronize(h->stream));
    std::memcpy(p, back.data(), particles);
    std::memcpy(&used, back.data() + particles, sizeof(double));
    if (reference_used) *reference_used = used;
    return AWPU_OK;
}

int awpu_hip_set_fir_table(awpu_hip_t *h, const float *coeffs) {
    AWPU_CTX(h);
    if (!h || !coeffs) return invalid("null argument");
    if (is_group(h)) return group_set_fir_table(h, coeffs);
    AWPU_HIP_TRY(hipSetDevice(h->cfg.device));
    // (on the device: the caller's 101 rows followed by zero rows up to kFir8CoeffRows -- the plane kernel's padding
    // entries name row 101, and its entry requests run a few items past a row's end, where any 7-bit row may stand)
    if (const int rc = h->d_fir.ensure(awpu::kFir8CoeffRows * 8); rc != AWPU_OK) return rc;
    if (const int rc = enter_stream(h, h->stream); rc != AWPU_OK) return rc;
    AWPU_HIP_TRY(hipStreamSynchronize(h->stream));  // (a sweep still reading the old coefficients)
    AWPU_HIP_TRY(hipMemset(h->d_fir, 0, awpu::kFir8CoeffRows * 8 * sizeof(float)));
    AWPU_HIP_TRY(hipMemcpy(h->d_fir, coeffs, 101 * 8 * sizeof(float), hipMemcpyHostToDevice));
    h->fir.assign(coeffs, coeffs + 101 * 8);
    h->have_fir = true;  // (the plane table names coefficient rows, it does not carry them: nothing to rebuild)
    return AWPU_OK;
}

// ---- the band (include/awpu_hip_band.h; the rule itself: band_host.cpp, the pre-pass: band_kernels.hip) ----------------------------

int awpu_hip_set_band(awpu_hip_t *h, const float *c, int32_t taps) {
    AWPU_CTX(h);
    if (!h) return invalid("null handle");
    if (is_group(h)) return fail(AWPU_ERR_STATE, "a device group takes no band");
    if (h->in_flight) return fail(AWPU_ERR_STATE, "an awpu_hip_process_async call is in flight on this handle: awpu_hip_wait first");
    if (!c && taps == 0) {
        h->band.clear();
        return AWPU_OK;
    }
    if (const char *why = awpu::band_refusal(c, taps)) return invalid(why);
    if (h->have_table && h->have_mics) {  // the window's start, as prepare() will find it
        int lo = h->cfg.hist;
        for (int p = 0; p < h->cfg.pixel_count; p++)
            for (int id : h->index) lo = std::min(lo, h->off[(size_t) p * h->cfg.lut_stride + id]);
        if (h->cfg.window_end > h->cfg.window_begin) lo = std::min(lo, h->cfg.window_begin);
        if (taps - 1 > lo) return fail(AWPU_ERR_RANGE, kBandHistory);
    }
    h->band.assign(c, c + taps);
    return AWPU_OK;
}

int awpu_hip_process(awpu_hip_t *h, const float *frames, int32_t batch, float *power) {
    AWPU_CTX(h);
    if (!h) return invalid("null handle");
    if (!frames || !power) return invalid("null argument");
    if (h->in_flight) return fail(AWPU_ERR_STATE, "an awpu_hip_process_async call is in flight on this handle: awpu_hip_wait first");
    if (is_group(h)) return group_process(h, frames, batch, power);
    // (a band-limited frame takes the batches' path: the live path's upload is the bare window, and its completion flag the sweep's)
    if (batch == 1 && h->member.ranges.empty() && h->band.empty()) return live_host_call(h, frames, power);
    int rc = enqueue_host_process(h, frames, batch);
    if (rc != AWPU_OK) return rc;
    rc = enqueue_power_to_host(h, batch, power, (size_t) h->cfg.pixel_count);
    if (rc != AWPU_OK) return rc;
    return wait_and_time(h, true);
}

int awpu_hip_process_async(awpu_hip_t *h, const float *frames, int32_t batch, float *power) {
    AWPU_CTX(h);
    if (!h) return invalid("null handle");
    if (!frames || !power) return invalid("null argument");
    if (h->in_flight) return fail(AWPU_ERR_STATE, "a call is in flight already: awpu_hip_wait first");
    int rc;
    if (is_group(h)) {
        rc = group_process_async(h, frames, batch, power);
    } else {
        rc = enqueue_host_process(h, frames, batch);
        if (rc == AWPU_OK) rc = enqueue_power_to_host(h, batch, power, (size_t) h->cfg.pixel_count);
    }
    h->in_flight = rc == AWPU_OK;
    return rc;
}

int awpu_hip_wait(awpu_hip_t *h) {
    AWPU_CTX(h);
    if (!h) return invalid("null handle");
    if (!h->in_flight) return AWPU_OK;  // nothing to wait for
    h->in_flight = false;
    return is_group(h) ? group_wait(h) : wait_and_time(h, true);
}

int awpu_hip_process_device(awpu_hip_t *h, const float *d_frames, int32_t batch, float *d_power,
                            void *stream) {
    AWPU_CTX(h);
    if (!h) return invalid("null handle");
    if (!d_frames || !d_power) return invalid("null argument");
    if (is_group(h)) return group_process_device(h, d_frames, batch, d_power, static_cast<hipStream_t>(stream));
    int rc = check_ready(h, batch);
    hipStream_t s = stream_of(h, stream);
    if (rc == AWPU_OK) rc = enter_stream(h, s);
    if (rc != AWPU_OK) return rc;
    return band_sweep(h, d_frames, (long long) h->cfg.n_streams * h->cfg.hist, h->cfg.hist, h->wstart, batch, d_power, s, kFull);
}

int awpu_hip_process_device_sums(awpu_hip_t *h, const float *d_frames, int32_t batch, float *d_power, float *d_sums, void *stream) {
    AWPU_CTX(h);
    if (!h) return invalid("null handle");
    if (!d_frames || !d_power || !d_sums) return invalid("null argument");
    if (is_group(h)) return invalid("the pre-epilogue sums are exported by single-device handles only");
    const int rc = check_ready(h, batch);
    if (rc != AWPU_OK) return rc;
    const bool exact_fir8 = h->cfg.math == AWPU_MATH_F32_EXACT && h->cfg.interp == AWPU_INTERP_FIR8;  // das_fir8_kernel, the reference's rounding
    if (!h->exact_pairs_ok && !exact_fir8) return fail(AWPU_ERR_STATE, "the pre-epilogue sums need AWPU_MATH_F32_EXACT");
    hipStream_t s = stream_of(h, stream);
    if (const int erc = enter_stream(h, s); erc != AWPU_OK) return erc;
    return band_sweep(h, d_frames, (long long) h->cfg.n_streams * h->cfg.hist, h->cfg.hist, h->wstart, batch, d_power, s, kFull, {false, d_sums});
}

int awpu_hip_ingest_block(awpu_hip_t *h, const void *datagrams, int32_t stride_bytes) {
    AWPU_CTX(h);
    if (h && is_group(h)) return group_ingest_block(h, datagrams, stride_bytes);
    const int rc = enqueue_ingest(h, datagrams, stride_bytes);
    if (rc != AWPU_OK) return rc;
    // the staging buffer is reused by the next call: finish the copy before returning
    AWPU_HIP_TRY(hipStreamSynchronize(h->stream));
    return AWPU_OK;
}

namespace {

// the steps of one live block on h->stream, without the final wait; `timed`: not inside a graph capture (event records there would
// not bracket anything)
int enqueue_live_block(awpu_hip *h, const void *datagrams, int32_t stride_bytes, float *power, int32_t rows, int32_t cols,
                       uint8_t *image, int32_t out_rows, int32_t out_cols, const uint8_t *d_colormap, uint8_t *big_image, bool timed) {
    const int n = h->cfg.n_pixels;
    int rc = enqueue_ingest(h, datagrams, stride_bytes);
    if (rc != AWPU_OK) return rc;
    rc = ensure_power(h, (size_t) n);
    if (rc != AWPU_OK) return rc;
    rc = launch(h, h->d_ring + h->ring_pos, 1, h->d_power, h->stream, kRing, {timed});
    if (rc != AWPU_OK) return rc;
    if (power) AWPU_HIP_TRY(hipMemcpyAsync(power, h->d_power, (size_t) n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (image || big_image) {
        const size_t channels = d_colormap ? 3 : 1;
        const size_t need = sizeof(float) + (size_t) n + (big_image ? (size_t) out_rows * out_cols * channels : 0);
        rc = ensure_seen_by_live_graphs(h, h->d_display, need);
        if (rc != AWPU_OK) return rc;
        float *d_peak = reinterpret_cast<float *>(h->d_display.get());
        uint8_t *d_small = h->d_display + sizeof(float), *d_big = d_small + n;
        AWPU_HIP_TRY(awpu::launch_heatmap(h->d_power, n, 1, d_peak, false, d_small, h->stream));
        if (image) AWPU_HIP_TRY(hipMemcpyAsync(image, d_small, (size_t) n, hipMemcpyDeviceToHost, h->stream));
        if (big_image) {
            rc = awpu_hip_upscale_u8_device(h, d_small, rows, cols, 1, d_colormap, d_big, out_rows, out_cols, h->stream);
            if (rc != AWPU_OK) return rc;
            AWPU_HIP_TRY(hipMemcpyAsync(big_image, d_big, (size_t) out_rows * out_cols * channels, hipMemcpyDeviceToHost,
                                        h->stream));
        }
    }
    return AWPU_OK;
}

}  // namespace

int awpu_hip_live_block(awpu_hip_t *h, const void *datagrams, int32_t stride_bytes, float *power, int32_t rows,
                        int32_t cols, uint8_t *image, int32_t out_rows, int32_t out_cols, const uint8_t *d_colormap,
                        uint8_t *big_image) {
    AWPU_CTX(h);
    if (h && is_group(h)) return invalid("the display step needs the whole grid on one device");
    if (h && h->in_flight) return fail(AWPU_ERR_STATE, "an awpu_hip_process_async call is in flight on this handle: awpu_hip_wait first");
    if (h && !h->band.empty()) return fail(AWPU_ERR_STATE, "the live block's captured step takes no band: clear it (awpu_hip_set_band) or ingest and sweep the ring");
    int rc = check_ready(h, 1);
    if (rc == AWPU_OK) rc = enter_stream(h, h->stream);  // (before a capture opens: the steps' own calls then find nothing to record)
    if (rc != AWPU_OK) return rc;
    const int n = h->cfg.n_pixels;
    if (h->cfg.pixel_count != n) return invalid("the display step needs the whole grid on this handle");
    if ((image || big_image) && (rows < 1 || cols < 1 || rows * cols != n)) return invalid("rows x cols must be the grid");
    if (big_image && (out_rows < rows || out_cols < cols || out_rows > 65535)) return invalid("upscale only: out >= in");
    if (!datagrams) return invalid("null argument");

    // A live block is eight small copies and launches: launch-latency bound.  Once every lazily allocated buffer
    // exists (after two plain calls) the sequence is captured into a HIP graph -- one per ring position and set of
    // caller buffers, a display loop reuses its own -- and replayed with a single launch.
    const bool graphs = env().live_graph != 0 && !h->live_graph_broken && h->d_ring != nullptr;
    // (a call of another shape allocates: upscale taps, a larger display buffer -- not while a capture is open)
    const unsigned long long shape = ((unsigned long long) (unsigned) rows << 48) ^ ((unsigned long long) (unsigned) cols << 36) ^
                                     ((unsigned long long) (unsigned) out_rows << 20) ^ ((unsigned long long) (unsigned) out_cols << 4) ^
                                     (power ? 1u : 0u) ^ (image ? 2u : 0u) ^ (big_image ? 4u : 0u) ^ (d_colormap ? 8u : 0u);
    // Only a caller that comes round with the SAME buffers gains from a graph: a call with other buffers than the
    // one before it (fresh arrays every block) starts the count again and is never captured.
    const void *bufs[5] = {datagrams, power, image, d_colormap, big_image};
    if (shape != h->live_shape || std::memcmp(bufs, h->live_bufs, sizeof(bufs)) != 0) {
        h->live_shape = shape;
        std::memcpy(h->live_bufs, bufs, sizeof(bufs));
        h->live_warm = 0;
    }
    if (graphs && h->live_warm >= 2) {
        awpu_hip::LiveGraph key{h->ring_pos, stride_bytes, rows, cols, out_rows, out_cols, datagrams, power, image, d_colormap,
                                big_image, h->table_gen, nullptr, 0};
        for (auto &g : h->live_graphs)
            if (g.ring_pos == key.ring_pos && g.stride == key.stride && g.rows == key.rows && g.cols == key.cols &&
                g.out_rows == key.out_rows && g.out_cols == key.out_cols && g.datagrams == key.datagrams && g.power == key.power &&
                g.image == key.image && g.colormap == key.colormap && g.big_image == key.big_image && g.gen == key.gen) {
                g.last_use = ++h->live_clock;
                AWPU_HIP_TRY(hipSetDevice(h->cfg.device));
                AWPU_HIP_TRY(hipGraphLaunch(g.exec, h->stream));
                h->ring_pos = (h->ring_pos + awpu::kSamples) % AWPU_HIST;  // (what enqueue_ingest does on the plain path)
                h->stats.launches += 1;
                h->stats.frames += 1;
                AWPU_HIP_TRY(hipStreamSynchronize(h->stream));
                return AWPU_OK;
            }
        if (h->live_graphs.size() >= 64) {  // full: the least recently replayed graph makes room
            auto lru = std::min_element(h->live_graphs.begin(), h->live_graphs.end(),
                                        [](const awpu_hip::LiveGraph &a, const awpu_hip::LiveGraph &b) { return a.last_use < b.last_use; });
            (void) hipGraphExecDestroy(lru->exec);
            h->live_graphs.erase(lru);
        }
        {   // capture this variant (the stream is idle: every call ends with a wait)
            AWPU_HIP_TRY(hipSetDevice(h->cfg.device));
            const int keep_pos = h->ring_pos;
            const auto keep_stats = h->stats;
            hipGraph_t graph = nullptr;
            hipError_t e = hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal);
            if (e == hipSuccess) {
                rc = enqueue_live_block(h, datagrams, stride_bytes, power, rows, cols, image, out_rows, out_cols, d_colormap, big_image, false);
                e = hipStreamEndCapture(h->stream, &graph);  // (also on failure: it takes the stream out of capture mode)
            } else {
                rc = AWPU_ERR_HIP;
            }
            h->ring_pos = keep_pos;  // nothing ran yet
            h->stats = keep_stats;
            hipGraphExec_t exec = nullptr;
            if (rc == AWPU_OK && e == hipSuccess && graph && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess) {
                key.exec = exec;
                key.last_use = ++h->live_clock;
                h->live_graphs.push_back(key);
            } else {
                hipStreamCaptureStatus status = hipStreamCaptureStatusNone;  // (an invalidated capture must not outlive this call)
                if (hipStreamIsCapturing(h->stream, &status) == hipSuccess && status != hipStreamCaptureStatusNone) {
                    hipGraph_t dead = nullptr;
                    (void) hipStreamEndCapture(h->stream, &dead);
                    if (dead) (void) hipGraphDestroy(dead);
                }
                (void) hipGetLastError();
                h->live_graph_broken = true;  // this runtime does not capture the sequence: stay on the plain path
            }
            if (graph) (void) hipGraphDestroy(graph);
            if (!h->live_graph_broken) return awpu_hip_live_block(h, datagrams, stride_bytes, power, rows, cols, image, out_rows, out_cols, d_colormap, big_image);
        }
    }
    // (the plain path records a bracket that nobody reads, as it always has: whether this call should be timed is a separate question)
    rc = enqueue_live_block(h, datagrams, stride_bytes, power, rows, cols, image, out_rows, out_cols, d_colormap, big_image, true);
    if (rc != AWPU_OK) return rc;
    AWPU_HIP_TRY(hipStreamSynchronize(h->stream));
    h->live_warm++;
    return AWPU_OK;
}

int awpu_hip_process_ring(awpu_hip_t *h, float *power) {
    AWPU_CTX(h);
    if (!h) return invalid("null handle");
    if (!power) return invalid("null argument");
    if (is_group(h)) return group_process_ring(h, power);
    int rc = check_ready(h, 1);
    if (rc == AWPU_OK) rc = enter_stream(h, h->stream);
    if (rc != AWPU_OK) return rc;
    if (!h->d_ring) {
        return fail(AWPU_ERR_STATE, "no block ingested yet");
    }
    const size_t need_power = (size_t) h->cfg.pixel_count;
    rc = ensure_power(h, need_power);
    if (rc != AWPU_OK) return rc;
    rc = band_sweep(h, h->d_ring + h->ring_pos, 0, 2048, h->wstart, 1, h->d_power, h->stream, kRing, kTimed);  // (a bracket nobody reads, as above)
    if (rc != AWPU_OK) return rc;
    AWPU_HIP_TRY(hipMemcpyAsync(power, h->d_power, need_power * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    AWPU_HIP_TRY(hipStreamSynchronize(h->stream));
    return AWPU_OK;
}

int awpu_hip_ring_snapshot(awpu_hip_t *h, float *frames) {
    h = first_device(h);
    AWPU_CTX(h);
    if (!h || !frames) return invalid("null argument");
    if (!h->d_ring) {
        return fail(AWPU_ERR_STATE, "no block ingested yet");
    }
    AWPU_HIP_TRY(hipSetDevice(h->cfg.device));
    if (const int rc = enter_stream(h, h->stream); rc != AWPU_OK) return rc;
    AWPU_HIP_TRY(hipMemcpy2DAsync(frames, AWPU_HIST * sizeof(float), h->d_ring + h->ring_pos, 2048 * sizeof(float),
                                  AWPU_HIST * sizeof(float), h->cfg.n_streams, hipMemcpyDeviceToHost, h->stream));
    AWPU_HIP_TRY(hipStreamSynchronize(h->stream));
    return AWPU_OK;
}

int awpu_hip_heatmap_u8_device(awpu_hip_t *h, const float *d_power, int32_t n, int32_t batch, float *d_peak,
                               int32_t peak_given, uint8_t *d_pix, void *stream) {
    h = first_device(h);
    AWPU_CTX(h);
    if (!h || !d_power || !d_peak || !d_pix || n < 1 || batch < 1 || batch > 65535) return invalid("bad argument");
    AWPU_HIP_TRY(hipSetDevice(h->cfg.device));
    hipStream_t s = stream_of(h, stream);  // (no enter_stream: nothing of the handle's is used)
    AWPU_HIP_TRY(awpu::launch_heatmap(d_power, n, batch, d_peak, peak_given != 0, d_pix, s));
    return AWPU_OK;
}

int awpu_hip_upscale_u8_device(awpu_hip_t *h, const uint8_t *d_pix, int32_t rows, int32_t cols, int32_t batch,
                               const uint8_t *d_colormap, uint8_t *d_out, int32_t out_rows, int32_t out_cols,
                               void *stream) {
    h = first_device(h);
    AWPU_CTX(h);
    if (!h || !d_pix || !d_out || rows < 1 || cols < 1 || batch < 1 || batch > 65535) return invalid("bad argument");
    if (out_rows < rows || out_cols < cols || out_rows > 65535) return invalid("upscale only: out >= in, out_rows <= 65535");
    AWPU_HIP_TRY(hipSetDevice(h->cfg.device));
    hipStream_t s = stream_of(h, stream);
    if (int rc = enter_stream(h, s)) return rc;  // (ensure_taps' wait for `s` is then a wait for every earlier reader of the taps)
    if (int rc = ensure_taps(h, rows, cols, out_rows, out_cols, s)) return rc;
    AWPU_HIP_TRY(awpu::launch_upscale(d_pix, rows, cols, batch, h->d_taps, d_colormap, d_out, out_rows, out_cols, s));
    return AWPU_OK;
}

int awpu_hip_resize_linear_u8(const uint8_t *pix, int32_t rows, int32_t cols, uint8_t *out, int32_t out_rows,
                              int32_t out_cols) {
    if (!pix || !out || rows < 1 || cols < 1) return invalid("bad argument");
    if (out_rows < rows || out_cols < cols) return invalid("upscale only: out >= in");
    std::vector<awpu::ResizeTap> taps((size_t) out_cols + out_rows);
    awpu::resize_taps(cols, out_cols, true, taps.data());
    awpu::resize_taps(rows, out_rows, false, taps.data() + out_cols);
    std::vector<int> sums((size_t) 2 * out_cols);  // the two source rows of the current output row, widened
    int have0 = -1, have1 = -1;
    for (int dy = 0; dy < out_rows; dy++) {
        const awpu::ResizeTap ty = taps[(size_t) out_cols + dy];
        const int r0 = std::min(std::max(ty.src, 0), rows - 1), r1 = std::min(std::max(ty.src + 1, 0), rows - 1);
        const int want[2] = {r0, r1};
        int *have[2] = {&have0, &have1};
        for (int k = 0; k < 2; k++) {
            if (*have[k] == want[k]) continue;
            const uint8_t *row = pix + (size_t) want[k] * cols;
            int *line = sums.data() + (size_t) k * out_cols;
            for (int dx = 0; dx < out_cols; dx++) {
                const awpu::ResizeTap tx = taps[dx];
                line[dx] = row[tx.src] * tx.w0 + row[std::min(tx.src + 1, cols - 1)] * tx.w1;
            }
            *have[k] = want[k];
        }
        for (int dx = 0; dx < out_cols; dx++)
            out[(size_t) dy * out_cols + dx] = awpu::resize_combine(sums[dx], sums[(size_t) out_cols + dx], ty.w0, ty.w1);
    }
    return AWPU_OK;
}

namespace {

// the packed layout of a single-device handle that is ready for `batch` frames (packed_shape: awpu_sweep.cpp)
int packed_plan(awpu_hip *h, int batch, awpu::FastPlan *plan) {
    if (!h) return invalid("null handle");
    if (is_group(h)) return fail(AWPU_ERR_STATE, "packed frames: a device group exchanges its frames itself");
    if (!h->band.empty()) return fail(AWPU_ERR_STATE, "packed frames are raw samples: a handle with a band neither packs nor sweeps them");
    const int rc = check_ready(h, batch);
    return rc != AWPU_OK ? rc : packed_shape(h, batch, plan);
}

}  // namespace

int awpu_hip_packed_bytes(awpu_hip_t *h, int32_t batch, uint64_t *bytes) {
    AWPU_CTX(h);
    if (!bytes) return invalid("null argument");
    awpu::FastPlan plan;
    const int rc = packed_plan(h, batch, &plan);
    if (rc != AWPU_OK) return rc;
    *bytes = (uint64_t) packed_floats_of(h, plan, batch) * sizeof(float);
    return AWPU_OK;
}

int awpu_hip_pack_frames(awpu_hip_t *h, const float *d_frames, int32_t batch, float *d_packed, void *stream) {
    AWPU_CTX(h);
    if (!d_frames || !d_packed) return invalid("null argument");
    awpu::FastPlan plan;
    const int rc = packed_plan(h, batch, &plan);
    if (rc != AWPU_OK) return rc;
    // No enter_stream: the pass reads the caller's frames and the mic list and writes the caller's buffer -- nothing of the handle's that
    // a call changes --, and the root of a multi-GPU job runs it on a side stream BESIDE the sweep in progress on the same handle
    hipStream_t s = stream_of(h, stream);
    // (Measured: a throttled variant of this pass -- few persistent workgroups, non-temporal accesses -- meant to be gentler
    // on the sweep it runs beside, slowed that sweep MORE the longer it lasted: 256 / 512 / 1024 workgroups cost the ingest
    // rank 0.90 / 0.55 / 0.35 ms per 1024-frame step against 0.23 ms for this full-speed pass.  Short and fast wins.)
    return pack_for_sweep(h, plan, d_frames, batch, d_packed, s);
}

int awpu_hip_process_packed(awpu_hip_t *h, const float *d_packed, int32_t batch, float *d_power, void *stream) {
    AWPU_CTX(h);
    if (!d_packed || !d_power) return invalid("null argument");
    awpu::FastPlan plan;
    int rc = packed_plan(h, batch, &plan);
    if (rc != AWPU_OK) return rc;
    hipStream_t s = stream_of(h, stream);
    if (rc = enter_stream(h, s); rc != AWPU_OK) return rc;
    // the shape awpu_hip_process_device takes for this batch, as long as that is a frame-pair shape (sweep_packed)
    // (the buffer is the caller's: awpu_hip_packed_bytes(batch) of it are taken to be there, and the sweep reads no further)
    return sweep_packed(h, plan, d_packed, packed_floats_of(h, plan, batch), batch, d_power, s);
}

int awpu_hip_synchronize(awpu_hip_t *h) {
    AWPU_CTX(h);
    if (!h) return invalid("null handle");
    if (is_group(h)) return group_synchronize(h);
    AWPU_HIP_TRY(hipSetDevice(h->cfg.device));
    // (the last call's stream, where that is the caller's: every earlier one is behind it, and the handle's own -- enter_stream)
    if (h->last_stream != h->stream) AWPU_HIP_TRY(hipStreamSynchronize(h->last_stream));
    h->last_stream = h->stream;
    AWPU_HIP_TRY(hipStreamSynchronize(h->stream));
    return AWPU_OK;
}

int awpu_hip_group_peer_status(awpu_hip_t *h, int32_t *status, int32_t n) {
    AWPU_CTX(h);
    if (!h || !status || n < 1) return invalid("null argument");
    if (is_group(h)) return group_peer_status(h, status, n);
    status[0] = AWPU_PEER_SAME_DEVICE;
    return 1;
}

}  // extern "C"

namespace {

// awpu_hip_build_delay_table_device (distance = +INFINITY) and awpu_hip_build_focus_table_device: the per-pixel rotations on the
// host, the P x n part on `device`
int build_table_on_device(int32_t device, const float *xyz, int32_t n, int32_t rows, int32_t columns, float fov_deg, double distance,
                          int32_t row_begin, int32_t row_count, int32_t *off, float *frac) {
    if (!xyz || !off || !frac || n <= 0 || rows <= 0 || columns <= 0) return invalid("null or non-positive argument");
    if (row_begin < 0 || row_count < 0 || row_begin + row_count > rows) return invalid("rows outside the grid");
    if (row_count == 0) return AWPU_OK;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev)
        return fail(AWPU_ERR_NO_DEVICE, "no such HIP device (the host builder awpu_hip_build_delay_table needs none)");
    hipDeviceProp_t prop;
    AWPU_HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(AWPU_ERR_NO_DEVICE, "device is not gfx950 (MI355X); kernels are built for gfx950 only");
    AWPU_HIP_TRY(hipSetDevice(device));
    const size_t P = (size_t) row_count * columns;
    std::vector<float> rot(P * 12);
    awpu::pixel_rotations(rows, columns, fov_deg, row_begin, row_count, rot.data());
    DeviceBuffer<float> d_xyz, d_rot, d_frac;
    DeviceBuffer<int32_t> d_off;
    int rc = d_xyz.ensure((size_t) 3 * n);
    if (rc == AWPU_OK) rc = d_rot.ensure(rot.size());
    if (rc == AWPU_OK) rc = d_off.ensure(P * n);
    if (rc == AWPU_OK) rc = d_frac.ensure(P * n);
    if (rc != AWPU_OK) return rc;
    AWPU_HIP_TRY(hipMemcpy(d_xyz, xyz, (size_t) 3 * n * sizeof(float), hipMemcpyHostToDevice));
    AWPU_HIP_TRY(hipMemcpy(d_rot, rot.data(), rot.size() * sizeof(float), hipMemcpyHostToDevice));
    // one launch per 32 768 pixels (the grid's x dimension is not the limit; this bounds a launch's run time)
    for (size_t p0 = 0; p0 < P; p0 += 32768) {
        const int np = (int) std::min<size_t>(32768, P - p0);
        if (awpu::focus_is_plane_wave(distance))
            AWPU_HIP_TRY(awpu::launch_delay_table(d_xyz, n, d_rot + p0 * 12, np, awpu::samples_per_metre(), d_off + p0 * n, d_frac + p0 * n,
                                                  nullptr));
        else
            AWPU_HIP_TRY(awpu::launch_focus_table(d_xyz, n, d_rot + p0 * 12, np, distance, d_off + p0 * n, d_frac + p0 * n, nullptr));
    }
    AWPU_HIP_TRY(hipMemcpy(off, d_off, P * n * sizeof(int32_t), hipMemcpyDeviceToHost));
    AWPU_HIP_TRY(hipMemcpy(frac, d_frac, P * n * sizeof(float), hipMemcpyDeviceToHost));
    return AWPU_OK;
}

}  // namespace

extern "C" {

int awpu_hip_build_delay_table_device(int32_t device, const float *xyz, int32_t n, int32_t rows, int32_t columns, float fov_deg,
                                      int32_t row_begin, int32_t row_count, int32_t *off, float *frac) {
    return build_table_on_device(device, xyz, n, rows, columns, fov_deg, (double) INFINITY, row_begin, row_count, off, frac);
}

int awpu_hip_build_focus_table_device(int32_t device, const float *xyz, int32_t n, int32_t rows, int32_t columns, float fov_deg,
                                      double distance, int32_t row_begin, int32_t row_count, int32_t *off, float *frac) {
    if (!awpu::focus_distance_ok(distance)) return invalid("distance must be > 0 (+INFINITY: a plane wave)");
    return build_table_on_device(device, xyz, n, rows, columns, fov_deg, distance, row_begin, row_count, off, frac);
}

int awpu_hip_get_stats(awpu_hip_t *h, awpu_hip_stats *stats) {
    AWPU_CTX(h);
    if (!h || !stats) return invalid("null argument");
    if (is_group(h)) return group_stats(h, stats);
    *stats = h->stats;
    return AWPU_OK;
}

const char *awpu_hip_strerror(int status) {
    switch (status) {
        case AWPU_OK: return "ok";
        case AWPU_ERR_INVALID: return "invalid argument or configuration";
        case AWPU_ERR_NO_DEVICE: return "no gfx950 HIP device (no CPU fallback exists)";
        case AWPU_ERR_HIP: return "HIP runtime error";
        case AWPU_ERR_STATE: return "delay table / active mics not set";
        case AWPU_ERR_RANGE: return "delay table reads outside the frame history";
        case AWPU_ERR_NOMEM: return "out of memory";
        default: return "unknown status";
    }
}

const char *awpu_hip_last_error(void) { return g_last_error.c_str(); }

const char *awpu_hip_last_error_of(awpu_hip_t *h) { return h ? h->last_error.c_str() : ""; }

int awpu_hip_abi_version(void) { return AWPU_HIP_ABI_VERSION; }

}  // extern "C"

#ifdef AWPU_TIMING_BUILD
// marker of a build whose AWPU_FAST_DEBUG timing switches are live (wrong results on request): never shipped,
// tests/test_abi.py::test_shipping_build_has_no_wrong_result_switches looks for it
extern "C" int awpu_hip_timing_build(void) { return 1; }
#endif
