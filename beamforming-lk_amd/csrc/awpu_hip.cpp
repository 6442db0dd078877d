// awpu_hip.cpp -- the C ABI of libawpu_hip.so (include/awpu_hip.h) and its call paths: handle lifetime, setters, frame upload,
// the single-call paths, the ring, display, tracking, device groups and the packed-frame entry points.  The tables, the kernel
// launchers and the dispatch rule are the sweep layer (awpu_sweep.cpp); the runs of blocks are awpu_runs.cpp.  No CPU fallback:
// every compute entry point ends in a gfx950 kernel launch or an error status.
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

#include "das_kernels.h"
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
        else if (shape == "exact_verify") exact_pairs = 0;
        else if (shape == "exact_pair") exact_pairs = 2;  // the two-pixel reference-order block even where quads would run
        else if (shape == "exact_quad") exact_pairs = 3;  // round 4's quad kernel on raw sample pairs (cur - next per pixel)
        else if (shape == "exact_nd1") exact_pairs = 4;   // the {next, d} kernel with one quad per wave
        else if (shape == "exact_nd2") exact_pairs = 5;   // ... with two
        else if (shape == "exact_ndp") exact_pairs = 6;   // single frames: one pixel per wave (das_exact_ndp_kernel) wherever its rows can be chunked
        else std::fprintf(stderr, "libawpu_hip: AWPU_SHAPE=%s is not a shape of this build; ignored\n", v);
    }
#ifdef AWPU_TUNING_BUILD
    if (const char *v = std::getenv("AWPU_LISTEN_STREAM")) listen_stream = std::atoi(v);
    if (const char *v = std::getenv("AWPU_FAST_QUADS")) quads = std::atoi(v);
    if (const char *v = std::getenv("AWPU_FAST_PAIRGROUP")) pair_group = std::atoi(v);
    if (const char *v = std::getenv("AWPU_QUAD_VARIANT")) quad_variant = std::atoi(v);
    if (const char *v = std::getenv("AWPU_FAST_HALVES")) halves = std::atoi(v);
    if (const char *v = std::getenv("AWPU_EXACT_PAIRS")) exact_pairs = std::atoi(v);
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
// whoever frees or reallocates one of those retires the graphs first.  The next live calls run step by step and
// capture again once the buffers have settled.
void awpu::host::retire_live_graphs(awpu_hip *h) {
    for (auto &g : h->live_graphs) (void) hipGraphExecDestroy(g.exec);
    h->live_graphs.clear();
    h->live_warm = 0;
}

namespace {

void release_device(awpu_hip *h) {
    retire_live_graphs(h);
    free_tables(h);
    dev_free(h->d_nd_items);
    h->nd_items_cap = 0;
    h->nd_items_key = -1;
    dev_free(h->d_nd_queue);
    dev_free(h->d_done_counter);
    if (h->h_done_flag) (void) hipHostFree(h->h_done_flag);
    h->h_done_flag = nullptr;
    h->done_total = 0;
    dev_free(h->d_index);
    dev_free(h->d_gain);
    dev_free(h->d_calib);
    dev_free(h->d_beam_lut);
    dev_free(h->d_beam_out);
    dev_free(h->d_xyz);
    dev_free(h->d_track_index);
    h->track_index_cap = 0;
    h->track_index.clear();
    dev_free(h->d_track);
    h->track_cap = 0;
    dev_free(h->d_fir);
    dev_free(h->d_ring);
    dev_free(h->d_pack);
    dev_free(h->d_taps);
    dev_free(h->d_display);
    h->display_cap = 0;
    dev_free(h->d_datagrams);
    dev_free(h->d_row_off_ring);
    dev_free(h->d_row_off);
    dev_free(h->d_row_off_compact);
    dev_free(h->d_frames);
    dev_free(h->d_power);
    dev_free(h->d_diag);
    h->diag_cap = 0;
    dev_free(h->d_fan[0]);
    dev_free(h->d_fan[1]);
    h->fan_cap = 0;
    for (BufferPair *pair : {&h->blk_hist, &h->blk_in, &h->blk_out, &h->listen_out, &h->watch}) pair->release();
    dev_free(h->d_blk_frames);
    h->blk_frames_cap = 0;
    dev_free(h->d_listeners);
    h->listeners_cap = 0;
    for (int b = 0; b < 2; b++) {
        if (b == 0) {
            if (h->h_live_in) (void) hipHostFree(h->h_live_in);
            if (h->h_live_out) (void) hipHostFree(h->h_live_out);
            h->h_live_in = h->h_live_out = nullptr;
            h->live_in_cap = h->live_out_cap = 0;
        }
        if (h->h_stage[b]) (void) hipHostFree(h->h_stage[b]);
        if (h->h_tile[b]) (void) hipHostFree(h->h_tile[b]);
        h->h_stage[b] = h->h_tile[b] = nullptr;
    }
    h->stage_cap = h->tile_cap = 0;
    h->beam_cap = h->beam_lut_cap = h->pack_cap = h->frames_cap = h->power_cap = 0;
}

enum PeerPath { kPeerSame = 0, kPeerDirect = 1, kPeerStaged = 2 };

}  // namespace

namespace awpu::host {

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
    return AWPU_OK;
}

int ensure_power(awpu_hip *h, size_t need_power) {
    if (h->power_cap < need_power) {
        retire_live_graphs(h);  // (they write through the old pointer)
        dev_free(h->d_power);
        h->power_cap = 0;
        AWPU_HIP_TRY(hipMalloc(&h->d_power, need_power * sizeof(float)));
        h->power_cap = need_power;
    }
    return AWPU_OK;
}

}  // namespace awpu::host

namespace {

// ------------------------------------------------------------------------------------------------
// Device group (cfg.n_devices > 1): one handle, one part (an ordinary single-device engine) per GPU,
// each owning a contiguous slab of the handle's pixels.  Everything below runs in the caller's thread; the parts'
// streams run concurrently.  No collective library: host frames are uploaded by every device itself, device
// frames fan out from devices[0] by one peer copy per destination (a different xGMI link each).
// ------------------------------------------------------------------------------------------------
int create_group(awpu_hip_t **out, const awpu_hip_cfg &c) {
    if (c.n_devices > AWPU_MAX_DEVICES) return invalid("n_devices above AWPU_MAX_DEVICES");
    const int G = c.n_devices;
    // slabs: whole grid rows when the row length is known and the handle's range is whole rows, else pixels
    const bool by_rows = c.grid_columns > 0 && c.pixel_count % c.grid_columns == 0 && c.pixel_begin % c.grid_columns == 0;
    int unit = by_rows ? c.grid_columns : 1;
    // groups of four rows where that divides (the quad shapes sweep four rows at a time: slabs that start on a
    // multiple of four rows sweep the same quads as one device would, and give the same bits)
    if (by_rows && c.pixel_count % (4 * unit) == 0 && c.pixel_count / (4 * unit) >= G) unit *= 4;
    const int units = c.pixel_count / unit;
    if (units < G) return invalid("fewer grid rows (or pixels) than devices");
    awpu_hip *g = new (std::nothrow) awpu_hip();
    if (!g) return AWPU_ERR_NOMEM;
    g->cfg = c;
    g->cfg.device = c.devices[0];
    // Row groups of four dealt round-robin (device k owns groups k, k + G, ...) where every device gets at least two of them:
    // the sweep's cost per row grows from the centre of the sine-space grid outwards (fewer shared integer delays), and a
    // group's call takes as long as its slowest device; contiguous slabs otherwise.  Either way a quad is four adjacent grid rows.
    const bool interleave = by_rows && unit == 4 * c.grid_columns && units >= 2 * G;
    int begin = 0;
    for (int k = 0; k < G; k++) {
        awpu_hip_cfg pc = c;
        pc.n_devices = 1;
        pc.device = c.devices[k];
        const int n = units / G + (k < units % G ? 1 : 0);  // the first units % G devices take one more
        std::vector<std::pair<int, int>> ranges;
        if (interleave) {
            for (int u = k; u < units; u += G) ranges.emplace_back(u * unit, unit);
        } else {
            ranges.emplace_back(begin * unit, n * unit);
        }
        pc.pixel_begin = c.pixel_begin + (interleave ? 0 : begin * unit);  // (a part's pixels are what `ranges` says; this only has to be a row start)
        pc.pixel_count = n * unit;
        begin += n;
        awpu_hip *part = nullptr;
        int rc = awpu_hip_create(&part, &pc);
        if (rc == AWPU_OK) part->ranges = ranges;
        if (rc == AWPU_OK) {  // what the fan-out needs on top of an ordinary engine
            hipError_t e = hipStreamCreateWithFlags(&part->copy_stream, hipStreamNonBlocking);
            for (int b = 0; b < 2 && e == hipSuccess; b++) {
                e = hipEventCreateWithFlags(&part->ev_copied[b], hipEventDisableTiming);
                if (e == hipSuccess) e = hipEventCreateWithFlags(&part->ev_swept[b], hipEventDisableTiming);
                if (e == hipSuccess) e = hipEventCreateWithFlags(&part->ev_staged_read[b], hipEventDisableTiming);
            }
            if (e == hipSuccess) e = hipEventCreateWithFlags(&part->ev_done, hipEventDisableTiming);
            if (e != hipSuccess) rc = hip_fail(e, "group stream/event creation");
            g->parts.push_back(part);
        }
        if (rc != AWPU_OK) {
            const std::string why = g_last_error;
            awpu_hip_destroy(g);
            note_error(why);
            return rc;
        }
    }
    // Direct copies between devices[0] and the others need peer access both ways.  Asked for and CHECKED: a pair
    // without it (another PCIe root, IOMMU settings, a container that hides the links) takes the explicit staged path
    // through pinned host memory -- slower, correct, and said so in awpu_hip_last_error_of / awpu_hip_group_peer_status.
    std::string staged_note;
    for (int k = 0; k < G; k++) {
        awpu_hip *part = g->parts[k];
        if (c.devices[k] == c.devices[0]) {
            part->peer = env().group_copy >= 2 ? kPeerStaged : kPeerSame;
            continue;
        }
        int can_out = 0, can_in = 0;
        hipError_t e_out = hipDeviceCanAccessPeer(&can_out, c.devices[0], c.devices[k]);
        hipError_t e_in = hipDeviceCanAccessPeer(&can_in, c.devices[k], c.devices[0]);
        if (e_out == hipSuccess && e_in == hipSuccess && can_out && can_in) {
            e_out = hipSetDevice(c.devices[0]);
            if (e_out == hipSuccess) e_out = hipDeviceEnablePeerAccess(c.devices[k], 0);
            e_in = hipSetDevice(c.devices[k]);
            if (e_in == hipSuccess) e_in = hipDeviceEnablePeerAccess(c.devices[0], 0);
        }
        const auto enabled = [](hipError_t e) { return e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled; };
        part->peer = can_out && can_in && enabled(e_out) && enabled(e_in) && env().group_copy < 2 ? kPeerDirect : kPeerStaged;
        if (part->peer == kPeerStaged) {
            staged_note += "device " + std::to_string(c.devices[0]) + " <-> " + std::to_string(c.devices[k]) + ": " +
                           (!(can_out && can_in) ? std::string("hipDeviceCanAccessPeer says no")
                                                 : std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(enabled(e_out) ? e_in : e_out)) + "; ";
        }
    }
    (void) hipGetLastError();
    if (!staged_note.empty())
        g->last_error = "device group without peer access (" + staged_note + "): frames and tiles are staged through pinned host memory";
    AWPU_HIP_TRY(hipSetDevice(c.devices[0]));
    hipError_t e = hipEventCreateWithFlags(&g->ev_fan, hipEventDisableTiming);
    for (int b = 0; b < 2 && e == hipSuccess; b++) e = hipEventCreateWithFlags(&g->ev_staged[b], hipEventDisableTiming);
    // a staged part's ev_tile_free[] is recorded on the CALLER's stream (devices[0]) and only waited for on the part's own:
    // an event must be recorded on a stream of the device it was created on, so these belong to devices[0], not the part's
    for (awpu_hip *part : g->parts)
        for (int b = 0; b < 2 && e == hipSuccess; b++) e = hipEventCreateWithFlags(&part->ev_tile_free[b], hipEventDisableTiming);
    if (e != hipSuccess) {
        awpu_hip_destroy(g);
        return hip_fail(e, "group event creation");
    }
    *out = g;
    return AWPU_OK;
}

// a part ran into an error: the group reports it as its own
int part_failed(awpu_hip *g, awpu_hip *part, int rc) {
    g->last_error = part->last_error.empty() ? g_last_error : part->last_error;
    g_last_error = g->last_error;
    return rc;
}

template <class F>
int for_each_part(awpu_hip *g, F f) {
    for (awpu_hip *part : g->parts) {
        const int rc = f(part);
        if (rc != AWPU_OK) return part_failed(g, part, rc);
    }
    return AWPU_OK;
}

// switches a handle's event bracket off for one asynchronous call and back on whichever way the call ends
struct TimingOff {
    awpu_hip *h;
    bool keep;
    explicit TimingOff(awpu_hip *h_) : h(h_), keep(h_->timing) { h->timing = false; }
    ~TimingOff() { h->timing = keep; }
};

}  // namespace

// frames per sweep launch of a host batch: large batches go up in pieces of whole frame pairs, so that piece k+1 crosses PCIe
// while piece k is swept (enqueue_host_process; a run of blocks sweeps its chunks the same way)
int awpu::host::host_piece(int batch) {
    const int n_pieces = batch >= 128 ? 4 : (batch >= 64 ? 2 : 1);
    return ((batch + n_pieces - 1) / n_pieces + 1) & ~1;
}

namespace {

// upload of host frames + the sweep into h->d_power, all on h->stream, nothing waited for
int enqueue_host_process(awpu_hip *h, const float *frames, int batch) {
    int rc = check_ready(h, batch);
    if (rc != AWPU_OK) return rc;
    const bool compact = h->compact_hist > 0;
    const int dev_hist = compact ? h->compact_hist : h->cfg.hist;
    const size_t need_frames = (size_t) h->cfg.n_streams * dev_hist * batch;
    if (h->frames_cap < need_frames) {
        dev_free(h->d_frames);
        h->frames_cap = 0;
        AWPU_HIP_TRY(hipMalloc(&h->d_frames, need_frames * sizeof(float)));
        h->frames_cap = need_frames;
    }
    rc = ensure_power(h, (size_t) h->cfg.pixel_count * batch);
    if (rc != AWPU_OK) return rc;
    // Large batches go up in pieces on a second stream, so that piece k+1 crosses PCIe while piece k is swept (the
    // pieces are whole frame pairs: the same arithmetic as one launch).  last_kernel_ms then spans all the sweeps.
    const int piece = host_piece(batch);
    const int n_pieces = (batch + piece - 1) / piece;
    if (n_pieces > 1) {
        if (!h->copy_stream) AWPU_HIP_TRY(hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
        for (hipEvent_t *ev : {&h->ev_copied[0], &h->ev_copied[1]})
            if (!*ev) AWPU_HIP_TRY(hipEventCreateWithFlags(ev, hipEventDisableTiming));
    }
    const bool keep_timing = h->timing;
    int turn = 0;
    for (int b0 = 0; b0 < batch; b0 += piece, turn++) {
        const int nb = std::min(piece, batch - b0);
        hipStream_t up = n_pieces > 1 ? h->copy_stream : h->stream;
        float *dst = h->d_frames + (size_t) b0 * h->cfg.n_streams * dev_hist;
        const float *src = frames + (size_t) b0 * h->cfg.n_streams * h->cfg.hist;
        if (compact) {  // rows of compact_hist floats cut out of rows of hist floats: a third of the PCIe bytes
            AWPU_HIP_TRY(hipMemcpy2DAsync(dst, (size_t) dev_hist * sizeof(float), src + h->wstart, (size_t) h->cfg.hist * sizeof(float),
                                          (size_t) dev_hist * sizeof(float), (size_t) nb * h->cfg.n_streams, hipMemcpyHostToDevice, up));
        } else {
            AWPU_HIP_TRY(hipMemcpyAsync(dst, src, (size_t) nb * h->cfg.n_streams * dev_hist * sizeof(float), hipMemcpyHostToDevice, up));
        }
        if (n_pieces > 1) {
            AWPU_HIP_TRY(hipEventRecord(h->ev_copied[turn & 1], up));
            AWPU_HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_copied[turn & 1], 0));
            if (keep_timing && b0 == 0) AWPU_HIP_TRY(hipEventRecord(h->ev_begin, h->stream));
            h->timing = false;
        }
        rc = launch(h, dst, nb, h->d_power + (size_t) b0 * h->cfg.pixel_count, h->stream, compact ? kCompact : kFull);
        h->timing = keep_timing;
        if (rc != AWPU_OK) return rc;
    }
    if (n_pieces > 1 && keep_timing) AWPU_HIP_TRY(hipEventRecord(h->ev_end, h->stream));
    return AWPU_OK;
}

// h->d_power [batch][pixel_count] -> host image `power` [batch][pitch] (pitch = this handle's pixels, or the whole group's: a
// part's pixel ranges then land where they belong in the wider image), on h->stream
int enqueue_power_to_host(awpu_hip *h, int batch, float *power, size_t pitch) {
    const size_t row = (size_t) h->cfg.pixel_count * sizeof(float);
    if (h->ranges.empty()) {
        if (pitch == (size_t) h->cfg.pixel_count) {
            AWPU_HIP_TRY(hipMemcpyAsync(power, h->d_power, row * batch, hipMemcpyDeviceToHost, h->stream));
        } else {
            AWPU_HIP_TRY(hipMemcpy2DAsync(power, pitch * sizeof(float), h->d_power, row, row, (size_t) batch, hipMemcpyDeviceToHost, h->stream));
        }
        return AWPU_OK;
    }
    size_t done = 0;  // pixels of the part's own rows already sent
    for (const auto &r : h->ranges) {
        AWPU_HIP_TRY(hipMemcpy2DAsync(power + r.first, pitch * sizeof(float), h->d_power + done, row, (size_t) r.second * sizeof(float),
                                      (size_t) batch, hipMemcpyDeviceToHost, h->stream));
        done += (size_t) r.second;
    }
    return AWPU_OK;
}

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
    if (rc != AWPU_OK) return rc;
    const bool compact = h->compact_hist > 0;
    const int dev_hist = compact ? h->compact_hist : h->cfg.hist;
    const size_t need_frames = (size_t) h->cfg.n_streams * dev_hist;
    if (h->frames_cap < need_frames) {
        dev_free(h->d_frames);
        h->frames_cap = 0;
        AWPU_HIP_TRY(hipMalloc(&h->d_frames, need_frames * sizeof(float)));
        h->frames_cap = need_frames;
    }
    rc = ensure_power(h, (size_t) h->cfg.pixel_count);
    if (rc != AWPU_OK) return rc;
    if (h->live_in_cap < need_frames) {
        if (h->h_live_in) (void) hipHostFree(h->h_live_in);
        h->h_live_in = nullptr;
        h->live_in_cap = 0;
        AWPU_HIP_TRY(hipHostMalloc(&h->h_live_in, need_frames * sizeof(float), hipHostMallocDefault));
        h->live_in_cap = need_frames;
    }
    if (h->live_out_cap < (size_t) h->cfg.pixel_count) {
        if (h->h_live_out) (void) hipHostFree(h->h_live_out);
        h->h_live_out = nullptr;
        h->live_out_cap = 0;
        AWPU_HIP_TRY(hipHostMalloc(&h->h_live_out, (size_t) h->cfg.pixel_count * sizeof(float), hipHostMallocDefault));
        h->live_out_cap = (size_t) h->cfg.pixel_count;
    }
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
        const bool keep = h->timing;
        h->timing = keep && timed;
        h->done_arm = !h->timing;  // (a timed call waits for the stream: its end event)
        rc = launch(h, h->d_frames, 1, h->h_live_out, h->stream, compact ? kCompact : kFull);
        h->done_arm = false;
        if (rc == AWPU_OK) {
#ifdef AWPU_TUNING_BUILD
            if (live_timing) lap(2, t);
#endif
            bool seen = false;
            if (h->done_used) {
                // the sweep's last workgroup stores the call's number behind its powers (das_fast.hip: store_tile_and_signal): ~7 us
                // sooner than the stream's completion signal.  Should it not arrive within 20 ms (it arrives within the sweep's ~25 us),
                // the stream's own completion decides
                const auto spin_from = std::chrono::steady_clock::now();
                for (unsigned spins = 0;; spins++) {
                    if (__atomic_load_n(h->h_done_flag, __ATOMIC_ACQUIRE) == h->done_seq) {
                        seen = true;
                        break;
                    }
                    __builtin_ia32_pause();
                    if ((spins & 0xfff) == 0xfff && std::chrono::steady_clock::now() - spin_from > std::chrono::milliseconds(20)) break;
                }
            }
            if (!seen) rc = wait_and_time(h);
        }
        h->timing = keep;
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

int awpu::host::wait_and_time(awpu_hip *h) {
    AWPU_HIP_TRY(hipSetDevice(h->cfg.device));
    AWPU_HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->timing) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, h->ev_begin, h->ev_end) == hipSuccess) {
            h->stats.last_kernel_ms = ms;
            h->stats.total_kernel_ms += ms;
        }
    }
    return AWPU_OK;
}

namespace {

int group_process(awpu_hip *g, const float *frames, int batch, float *power) {
    const size_t pitch = (size_t) g->cfg.pixel_count;
    int rc = for_each_part(g, [&](awpu_hip *part) {
        AWPU_CTX(part);
        const int r = enqueue_host_process(part, frames, batch);
        return r != AWPU_OK ? r : enqueue_power_to_host(part, batch, power, pitch);
    });
    if (rc != AWPU_OK) return rc;
    return for_each_part(g, [&](awpu_hip *part) { return wait_and_time(part); });
}

// Every part of a group stages the same window -- the union of what the parts' own rows touch -- so that ONE packed buffer
// serves them all (the layout's row length and first sample follow the window).  Results do not depend on the window.
int group_union_window(awpu_hip *g, int batch) {
    if (g->union_window_done) return AWPU_OK;
    int lo = g->cfg.hist, hi = 0;
    for (awpu_hip *part : g->parts) {
        lo = std::min(lo, part->wstart);
        hi = std::max(hi, part->wstart + part->window);
    }
    for (awpu_hip *part : g->parts) {
        if (part->wstart == lo && part->wstart + part->window == hi) continue;
        AWPU_CTX(part);
        part->cfg.window_begin = lo;
        part->cfg.window_end = hi;
        part->prepared = false;
        const int rc = check_ready(part, batch);
        if (rc != AWPU_OK) return part_failed(g, part, rc);
    }
    g->union_window_done = true;
    return AWPU_OK;
}

// a part's tile [batch][its pixels, back to back] -> the group's image [batch][pitch floats]: one 2-D copy per pixel range
int tile_to_image(awpu_hip *part, const float *tile, float *image, size_t pitch_floats, int batch, hipMemcpyKind kind, hipStream_t s) {
    const size_t row = (size_t) part->cfg.pixel_count * sizeof(float);
    size_t done = 0;
    for (const auto &r : part->ranges) {
        AWPU_HIP_TRY(hipMemcpy2DAsync(image + r.first, pitch_floats * sizeof(float), tile + done, row, (size_t) r.second * sizeof(float),
                                      (size_t) batch, kind, s));
        done += (size_t) r.second;
    }
    return AWPU_OK;
}

// Frames and power in the memory of devices[0], on the caller's stream there.  What travels to the other devices:
//   * batches that the parts sweep with a frame-pair shape (takes_packed_pairs): devices[0] runs the sweep's pack pass ONCE
//     (two frames interleaved, filtered: the packed frame pairs of awpu_hip_pack_frames, the exchange format of the
//     one-process-per-GPU path too) and every other device gets that buffer by ONE linear peer copy on its copy stream and
//     sweeps it as it arrives -- no window cut on devices[0], no pack pass anywhere else;
//   * everything else (single frames, FIR8, exact math, gains): the window of every stream that the tables touch, by one 2-D
//     peer copy per device, and every device runs its whole sweep.
// The parts' pixel ranges are swept concurrently; the tiles return by peer copies on the caller's stream, which thereby waits
// for all of it.  Parts without peer access to devices[0] (kPeerStaged) get the same bytes through pinned host memory: ONE
// copy down on the caller's stream for all of them, one copy up per part on its copy stream; their tiles return the same
// way.  Two buffers everywhere, so that call k+1's copies run beside call k's sweeps.
int group_process_device(awpu_hip *g, const float *d_frames, int batch, float *d_power, hipStream_t stream) {
    const int dev0 = g->cfg.devices[0];
    AWPU_HIP_TRY(hipSetDevice(dev0));
    hipStream_t s = stream ? stream : g->parts[0]->stream;
    int rc = for_each_part(g, [&](awpu_hip *part) {
        AWPU_CTX(part);
        return check_ready(part, batch);  // (tables packed: every part's window is known)
    });
    if (rc != AWPU_OK) return rc;
    rc = group_union_window(g, batch);
    if (rc != AWPU_OK) return rc;
    g->stats.group_exchange = AWPU_EXCHANGE_WINDOWS;
    auto in_place = [&](const awpu_hip *part) { return part->cfg.device == dev0 && !env().group_copy; };

    // ---- packed frame pairs, where every part sweeps them
    awpu::FastPlan pplan{};
    bool packed = true;
    for (awpu_hip *part : g->parts) {
        awpu::FastPlan one{};
        packed = packed && takes_packed_pairs(part, batch, &one);
        if (packed && pplan.wr && (one.wr != pplan.wr || one.usable_pad != pplan.usable_pad)) packed = false;
        pplan = one;
    }
    const size_t packed_floats = packed ? packed_floats_of(g->parts[0], pplan, batch) : 0;
    int pb = 0;  // which of the group's two packed buffers this call fills
    AWPU_HIP_TRY(hipSetDevice(dev0));
    if (packed) {
        g->stats.group_exchange = AWPU_EXCHANGE_PACKED_PAIRS;
        const size_t cap = packed_floats_of(g->parts[0], pplan, g->cfg.max_batch);
        if (g->fan_cap < cap) {  // (nobody may still be reading the old buffers)
            for (awpu_hip *part : g->parts) {
                AWPU_HIP_TRY(hipSetDevice(part->cfg.device));
                AWPU_HIP_TRY(hipStreamSynchronize(part->copy_stream));
                AWPU_HIP_TRY(hipStreamSynchronize(part->stream));
            }
            AWPU_HIP_TRY(hipSetDevice(dev0));
            AWPU_HIP_TRY(hipStreamSynchronize(s));
            dev_free(g->d_fan[0]);
            dev_free(g->d_fan[1]);
            g->fan_cap = 0;
            AWPU_HIP_TRY(hipMalloc(&g->d_fan[0], cap * sizeof(float)));
            AWPU_HIP_TRY(hipMalloc(&g->d_fan[1], cap * sizeof(float)));
            g->fan_cap = cap;
            g->fan_used[0] = g->fan_used[1] = false;
        }
        pb = (int) (g->fan_turn++ & 1);
        if (g->fan_used[pb])  // buffer pb was read two calls ago: by the peers' copies and by the in-place parts' sweeps
            for (awpu_hip *part : g->parts) AWPU_HIP_TRY(hipStreamWaitEvent(s, in_place(part) ? part->ev_swept[pb] : part->ev_copied[pb], 0));
        awpu_hip *p0 = g->parts[0];
        if (const int prc = pack_for_sweep(p0, pplan, d_frames, batch, g->d_fan[pb], s); prc != AWPU_OK) return prc;
        g->fan_used[pb] = true;
    }
    AWPU_HIP_TRY(hipEventRecord(g->ev_fan, s));  // the frames (or their packed pairs) are in place once the caller's stream gets here

    // ---- staged parts: what they need goes down to pinned memory once -- the packed buffer, or the union of their windows
    int gb = 0;
    bool any_staged = false;
    for (awpu_hip *part : g->parts) any_staged |= part->peer == kPeerStaged && !in_place(part);
    if (any_staged) {
        int lo = 0, w = 0;
        size_t need = 0;
        if (packed) {
            need = packed_floats_of(g->parts[0], pplan, g->cfg.max_batch);
            lo = -1;  // (marks the packed payload: a change of payload re-sizes the staging like a change of window)
            w = (int) pplan.wr;
        } else {
            lo = g->cfg.hist;
            int hi = 0;
            for (awpu_hip *part : g->parts) {
                if (part->peer != kPeerStaged) continue;
                const bool compact = part->compact_hist > 0;
                lo = std::min(lo, compact ? part->wstart : 0);
                hi = std::max(hi, compact ? part->wstart + part->compact_hist : part->cfg.hist);
            }
            w = hi - lo;
            need = (size_t) g->cfg.n_streams * w * g->cfg.max_batch;
        }
        // (round-4 advisor) Only a buffer that is too SMALL is replaced, behind a synchronize of everybody who may still read it.  A
        // change of payload -- packed pairs one call, raw windows the next: batches alternating with single frames -- keeps the
        // buffers and their turn: every reuse of h_stage[gb] already waits for the uploads that read it two calls ago
        // (ev_staged_read below), whatever they carried.
        if (g->stage_cap < need) {
            for (awpu_hip *part : g->parts) {  // nobody may still be reading the old staging buffers
                AWPU_HIP_TRY(hipSetDevice(part->cfg.device));
                AWPU_HIP_TRY(hipStreamSynchronize(part->copy_stream));
            }
            AWPU_HIP_TRY(hipSetDevice(dev0));
            AWPU_HIP_TRY(hipStreamSynchronize(s));
            for (int b = 0; b < 2; b++) {
                if (g->h_stage[b]) (void) hipHostFree(g->h_stage[b]);
                g->h_stage[b] = nullptr;
            }
            g->stage_cap = 0;
            for (int b = 0; b < 2; b++) AWPU_HIP_TRY(hipHostMalloc(&g->h_stage[b], need * sizeof(float), hipHostMallocPortable));
            g->stage_cap = need;
            g->stage_turn = 0;
            for (awpu_hip *part : g->parts) part->stage_used[0] = part->stage_used[1] = false;
        }
        g->stage_lo = lo;  // what THIS call's payload is (read by the uploads enqueued below, in this call)
        g->stage_w = w;
        gb = g->stage_turn++ & 1;
        for (awpu_hip *part : g->parts)  // h_stage[gb] was read by the staged parts' uploads two calls ago
            if (part->peer == kPeerStaged && !in_place(part) && part->stage_used[gb]) AWPU_HIP_TRY(hipStreamWaitEvent(s, part->ev_staged_read[gb], 0));
        if (packed) {
            AWPU_HIP_TRY(hipMemcpyAsync(g->h_stage[gb], g->d_fan[pb], packed_floats * sizeof(float), hipMemcpyDeviceToHost, s));
        } else {
            AWPU_HIP_TRY(hipMemcpy2DAsync(g->h_stage[gb], (size_t) w * sizeof(float), d_frames + lo, (size_t) g->cfg.hist * sizeof(float),
                                          (size_t) w * sizeof(float), (size_t) batch * g->cfg.n_streams, hipMemcpyDeviceToHost, s));
        }
        AWPU_HIP_TRY(hipEventRecord(g->ev_staged[gb], s));
    }

    rc = for_each_part(g, [&](awpu_hip *part) {
        AWPU_CTX(part);
        AWPU_HIP_TRY(hipSetDevice(part->cfg.device));
        int r = ensure_power(part, (size_t) part->cfg.pixel_count * batch);
        if (r != AWPU_OK) return r;
        TimingOff untimed(part);  // asynchronous path: the caller times its own stream
        const bool staged = part->peer == kPeerStaged && !in_place(part);
        if (in_place(part)) {  // same GPU: sweep the caller's frames (or the group's packed buffer) in place
            AWPU_HIP_TRY(hipStreamWaitEvent(part->stream, g->ev_fan, 0));
            if (packed) {
                r = sweep_packed(part, pplan, g->d_fan[pb], g->fan_cap, batch, part->d_power, part->stream);
                if (r == AWPU_OK) AWPU_HIP_TRY(hipEventRecord(part->ev_swept[pb], part->stream));
            } else {
                r = launch(part, d_frames, batch, part->d_power, part->stream, kFull);
            }
        } else {
            const bool compact = part->compact_hist > 0;
            const int dev_hist = compact ? part->compact_hist : part->cfg.hist;
            const size_t need_window = (size_t) part->cfg.n_streams * dev_hist * part->cfg.max_batch;
            const size_t need_packed = packed ? packed_floats_of(part, pplan, part->cfg.max_batch) : 0;
            const size_t need = std::max(need_window, need_packed);
            if (part->fan_cap < need) {
                AWPU_HIP_TRY(hipStreamSynchronize(part->stream));
                AWPU_HIP_TRY(hipStreamSynchronize(part->copy_stream));
                dev_free(part->d_fan[0]);
                dev_free(part->d_fan[1]);
                part->fan_cap = 0;
                AWPU_HIP_TRY(hipMalloc(&part->d_fan[0], need * sizeof(float)));
                AWPU_HIP_TRY(hipMalloc(&part->d_fan[1], need * sizeof(float)));
                part->fan_cap = need;
                part->fan_used[0] = part->fan_used[1] = false;
            }
            // the part's own receive buffer follows the buffer it reads from: the group's packed buffer (pb) or, for a staged
            // part, the staging buffer (gb); a window copy out of the caller's frames takes its own turns
            const int b = staged ? gb : (packed ? pb : (int) (part->fan_turn++ & 1));
            if (part->fan_used[b]) AWPU_HIP_TRY(hipStreamWaitEvent(part->copy_stream, part->ev_swept[b], 0));  // buffer b is free again
            const size_t row = (size_t) dev_hist * sizeof(float);
            if (staged) {
                AWPU_HIP_TRY(hipStreamWaitEvent(part->copy_stream, g->ev_staged[gb], 0));
                if (packed) {
                    AWPU_HIP_TRY(hipMemcpyAsync(part->d_fan[b], g->h_stage[gb], packed_floats * sizeof(float), hipMemcpyHostToDevice, part->copy_stream));
                } else {
                    AWPU_HIP_TRY(hipMemcpy2DAsync(part->d_fan[b], row, g->h_stage[gb] + ((compact ? part->wstart : 0) - g->stage_lo),
                                                  (size_t) g->stage_w * sizeof(float), row, (size_t) batch * part->cfg.n_streams,
                                                  hipMemcpyHostToDevice, part->copy_stream));
                }
                AWPU_HIP_TRY(hipEventRecord(part->ev_staged_read[gb], part->copy_stream));
                part->stage_used[gb] = true;
            } else {
                AWPU_HIP_TRY(hipStreamWaitEvent(part->copy_stream, g->ev_fan, 0));
                if (packed) {  // ONE linear copy: the packed pairs of the whole batch
                    AWPU_HIP_TRY(hipMemcpyAsync(part->d_fan[b], g->d_fan[pb], packed_floats * sizeof(float), hipMemcpyDeviceToDevice, part->copy_stream));
                } else {
                    AWPU_HIP_TRY(hipMemcpy2DAsync(part->d_fan[b], row, d_frames + (compact ? part->wstart : 0),
                                                  (size_t) part->cfg.hist * sizeof(float), row, (size_t) batch * part->cfg.n_streams,
                                                  hipMemcpyDeviceToDevice, part->copy_stream));
                }
            }
            part->fan_used[b] = true;
            AWPU_HIP_TRY(hipEventRecord(part->ev_copied[b], part->copy_stream));
            AWPU_HIP_TRY(hipStreamWaitEvent(part->stream, part->ev_copied[b], 0));
            r = packed ? sweep_packed(part, pplan, part->d_fan[b], part->fan_cap, batch, part->d_power, part->stream)
                       : launch(part, part->d_fan[b], batch, part->d_power, part->stream, compact ? kCompact : kFull);
            if (r == AWPU_OK) AWPU_HIP_TRY(hipEventRecord(part->ev_swept[b], part->stream));
            if (r == AWPU_OK && staged) {  // the tile's way back starts on the part's own stream: device -> pinned
                const size_t tile = (size_t) part->cfg.pixel_count * part->cfg.max_batch;
                if (part->tile_cap < tile) {
                    AWPU_HIP_TRY(hipStreamSynchronize(part->stream));
                    for (int k = 0; k < 2; k++) {
                        if (part->h_tile[k]) (void) hipHostFree(part->h_tile[k]);
                        part->h_tile[k] = nullptr;
                    }
                    part->tile_cap = 0;
                    for (int k = 0; k < 2; k++) AWPU_HIP_TRY(hipHostMalloc(&part->h_tile[k], tile * sizeof(float), hipHostMallocPortable));
                    part->tile_cap = tile;
                    part->tile_used[0] = part->tile_used[1] = false;
                }
                if (part->tile_used[gb]) AWPU_HIP_TRY(hipStreamWaitEvent(part->stream, part->ev_tile_free[gb], 0));
                AWPU_HIP_TRY(hipMemcpyAsync(part->h_tile[gb], part->d_power, (size_t) part->cfg.pixel_count * batch * sizeof(float),
                                            hipMemcpyDeviceToHost, part->stream));
                part->tile_used[gb] = true;
            }
        }
        if (r == AWPU_OK) AWPU_HIP_TRY(hipEventRecord(part->ev_done, part->stream));
        return r;
    });
    if (rc != AWPU_OK) return rc;
    AWPU_HIP_TRY(hipSetDevice(dev0));
    const size_t pitch = (size_t) g->cfg.pixel_count;
    for (awpu_hip *part : g->parts) {  // tiles back into the caller's [batch][pixel_count] image, range by range
        AWPU_HIP_TRY(hipStreamWaitEvent(s, part->ev_done, 0));
        const bool staged = part->peer == kPeerStaged && !in_place(part);
        if (staged) {
            rc = tile_to_image(part, part->h_tile[gb], d_power, pitch, batch, hipMemcpyHostToDevice, s);
            if (rc != AWPU_OK) return rc;
            AWPU_HIP_TRY(hipEventRecord(part->ev_tile_free[gb], s));
        } else {
            rc = tile_to_image(part, part->d_power, d_power, pitch, batch, hipMemcpyDeviceToDevice, s);
            if (rc != AWPU_OK) return rc;
        }
    }
    return AWPU_OK;
}

int group_stats(awpu_hip *g, awpu_hip_stats *out) {
    awpu_hip_stats st = g->parts[0]->stats;
    st.group_exchange = g->stats.group_exchange;
    st.group_ranges = (int32_t) g->parts[0]->ranges.size();
    for (size_t k = 1; k < g->parts.size(); k++) {
        const awpu_hip_stats &p = g->parts[k]->stats;
        st.launches += p.launches;
        st.last_kernel_ms = std::max(st.last_kernel_ms, p.last_kernel_ms);   // the slabs run side by side
        st.total_kernel_ms = std::max(st.total_kernel_ms, p.total_kernel_ms);
        st.alg_bytes_frame += p.alg_bytes_frame;
        st.alg_flops_frame += p.alg_flops_frame;
        st.tau_max = std::max(st.tau_max, p.tau_max);
        st.window = std::max(st.window, p.window);
    }
    *out = st;
    return AWPU_OK;
}

}  // namespace

// what the runs of blocks (awpu_runs.cpp) share with the calls below
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
    if (h->track_index_cap < (size_t) U) {
        dev_free(h->d_track_index);
        h->track_index_cap = 0;
        AWPU_HIP_TRY(hipMalloc(&h->d_track_index, (size_t) U * sizeof(int32_t)));
        h->track_index_cap = U;
    }
    h->track_index.clear();
    AWPU_HIP_TRY(hipMemcpy(h->d_track_index, h->index.data(), (size_t) U * sizeof(int32_t), hipMemcpyHostToDevice));
    h->track_index = h->index;
    return AWPU_OK;
}

// the ingest ring and its one-block staging, allocated at first use: the ring starts zeroed (on h->stream)
int ensure_ring(awpu_hip *h) {
    if (h->d_ring) return AWPU_OK;
    const size_t ring_bytes = (size_t) h->cfg.n_streams * 2048 * sizeof(float);
    AWPU_HIP_TRY(hipMalloc(&h->d_ring, ring_bytes));
    AWPU_HIP_TRY(hipMemsetAsync(h->d_ring, 0, ring_bytes, h->stream));
    AWPU_HIP_TRY(hipMalloc(&h->d_datagrams, (size_t) awpu::kSamples * AWPU_DATAGRAM_BYTES));
    h->ring_pos = 0;
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
        dev_free(h->d_taps);
        AWPU_HIP_TRY(hipMalloc(&h->d_taps, taps.size() * sizeof(awpu::ResizeTap)));
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
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&h->ev_begin);
    if (e == hipSuccess) e = hipEventCreate(&h->ev_end);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_fan, hipEventDisableTiming);
    if (e != hipSuccess) {
        awpu_hip_destroy(h);
        return hip_fail(e, "stream/event creation");
    }
    *out = h;
    return AWPU_OK;
}

int awpu_hip_destroy(awpu_hip_t *h) {
    if (!h) return AWPU_OK;
    for (awpu_hip *part : h->parts) awpu_hip_destroy(part);
    h->parts.clear();
    (void) hipSetDevice(h->cfg.device);
    if (h->stream) (void) hipStreamSynchronize(h->stream);
    if (h->copy_stream) (void) hipStreamSynchronize(h->copy_stream);
    if (h->listen_stream) (void) hipStreamSynchronize(h->listen_stream);
    release_device(h);
    for (hipEvent_t ev : {h->ev_begin, h->ev_end, h->ev_fan, h->ev_copied[0], h->ev_copied[1], h->ev_swept[0], h->ev_swept[1], h->ev_done,
                          h->ev_staged[0], h->ev_staged[1], h->ev_tile_free[0], h->ev_tile_free[1], h->ev_staged_read[0], h->ev_staged_read[1],
                          h->ev_blk_in[0], h->ev_blk_in[1], h->ev_blk_hist[0], h->ev_blk_hist[1], h->ev_blk_cut[0], h->ev_blk_cut[1],
                          h->ev_blk_swept[0], h->ev_blk_swept[1], h->ev_blk_out[0], h->ev_blk_out[1], h->ev_blk_ring,
                          h->ev_listened[0], h->ev_listened[1], h->ev_listen_out[0], h->ev_listen_out[1]})
        if (ev) (void) hipEventDestroy(ev);
    if (h->stream) (void) hipStreamDestroy(h->stream);
    if (h->copy_stream) (void) hipStreamDestroy(h->copy_stream);
    if (h->listen_stream) (void) hipStreamDestroy(h->listen_stream);
    delete h;
    return AWPU_OK;
}

int awpu_hip_set_delay_table(awpu_hip_t *h, const int32_t *off, const float *frac) {
    AWPU_CTX(h);
    if (!h || !off || !frac) return invalid("null argument");
    if (!h->parts.empty()) {  // every device gets the rows of its pixel ranges, back to back
        h->union_window_done = false;
        return for_each_part(h, [&](awpu_hip *part) {
            part->cfg.window_begin = h->cfg.window_begin;  // (the union window of the OLD table is void: back to the caller's, if any)
            part->cfg.window_end = h->cfg.window_end;
            const size_t stride = (size_t) h->cfg.lut_stride;
            if (part->ranges.size() == 1) {
                const size_t first = (size_t) part->ranges[0].first * stride;
                return awpu_hip_set_delay_table(part, off + first, frac + first);
            }
            std::vector<int32_t> o((size_t) part->cfg.pixel_count * stride);
            std::vector<float> f(o.size());
            size_t done = 0;
            for (const auto &r : part->ranges) {
                std::memcpy(&o[done * stride], off + (size_t) r.first * stride, (size_t) r.second * stride * sizeof(int32_t));
                std::memcpy(&f[done * stride], frac + (size_t) r.first * stride, (size_t) r.second * stride * sizeof(float));
                done += (size_t) r.second;
            }
            return awpu_hip_set_delay_table(part, o.data(), f.data());
        });
    }
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
    if (!h->parts.empty()) {
        h->union_window_done = false;
        return for_each_part(h, [&](awpu_hip *part) {
            part->cfg.window_begin = h->cfg.window_begin;  // (as in awpu_hip_set_delay_table: the union is taken anew)
            part->cfg.window_end = h->cfg.window_end;
            return awpu_hip_set_active_mics(part, index, usable);
        });
    }
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
    if (!h->parts.empty()) return for_each_part(h, [&](awpu_hip *part) { return awpu_hip_set_mic_gains(part, gains); });
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

// aw_processing_unit.cpp:145-200 on the 64 mean squares of one array
int usable_from_power(const float *power, float reference_power_level, int32_t *index, float *correction,
                      float *median_out) {
    float sorted[AWPU_ELEMENTS];
    std::copy(power, power + AWPU_ELEMENTS, sorted);
    std::sort(sorted, sorted + AWPU_ELEMENTS);
    // the reference averages elements 32 and 33 of the sorted list (.cpp:150), in double, then rounds
    const float median = (float) ((sorted[AWPU_ELEMENTS / 2] + sorted[AWPU_ELEMENTS / 2 + 1]) / 2.0);
    int count = 0;
    for (int s = 0; s < AWPU_ELEMENTS; s++) {
        const bool far_off = std::fabs(power[s] - median) > 1e-4;  // float promoted against a double bound
        const bool dead = power[s] < median * 1e-3;
        if (far_off || dead) continue;
        index[count] = s;
        correction[count] = reference_power_level / power[s];
        count++;
    }
    if (median_out) *median_out = median;
    return count;
}

int calibrate_rows(awpu_hip *h, const float *d_rows, int pitch, int hist, float reference_power_level, int32_t *index,
                   float *correction, float *median, int32_t *usable, hipStream_t s) {
    if (!h->d_calib) AWPU_HIP_TRY(hipMalloc(&h->d_calib, AWPU_ELEMENTS * sizeof(float)));
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
    if (h && !h->parts.empty()) h = h->parts[0];  // not pixel-sharded: a device group answers with its first device
    AWPU_CTX(h);
    if (!h || !d_frame || !index || !correction || !usable) return invalid("null argument");
    if (array < 0 || (array + 1) * AWPU_ELEMENTS > h->cfg.n_streams) return invalid("array outside the streams");
    if (h->cfg.hist > 16384) return invalid("history too long for the calibration kernel");
    AWPU_HIP_TRY(hipSetDevice(h->cfg.device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
    return calibrate_rows(h, d_frame + (size_t) array * AWPU_ELEMENTS * h->cfg.hist, h->cfg.hist, h->cfg.hist,
                          reference_power_level, index, correction, median, usable, s);
}

int awpu_hip_calibrate_host(awpu_hip_t *h, const float *frame, int32_t array, float reference_power_level,
                             int32_t *index, float *correction, float *median, int32_t *usable) {
    const bool busy = h && h->in_flight;  // (the staging buffer below is the one an asynchronous call uploads into)
    if (h && !h->parts.empty()) h = h->parts[0];  // not pixel-sharded: a device group answers with its first device
    AWPU_CTX(h);
    if (!h || !frame || !index || !correction || !usable) return invalid("null argument");
    if (array < 0 || (array + 1) * AWPU_ELEMENTS > h->cfg.n_streams) return invalid("array outside the streams");
    if (h->cfg.hist > 16384) return invalid("history too long for the calibration kernel");
    if (busy) return fail(AWPU_ERR_STATE, "an awpu_hip_process_async call is in flight on this handle: awpu_hip_wait first");
    AWPU_HIP_TRY(hipSetDevice(h->cfg.device));
    // only the array's 64 streams travel; they share the frame staging buffer of awpu_hip_process
    const size_t need = (size_t) AWPU_ELEMENTS * h->cfg.hist;
    if (h->frames_cap < need) {
        dev_free(h->d_frames);
        h->frames_cap = 0;
        AWPU_HIP_TRY(hipMalloc(&h->d_frames, need * sizeof(float)));
        h->frames_cap = need;
    }
    AWPU_HIP_TRY(hipMemcpyAsync(h->d_frames, frame + (size_t) array * AWPU_ELEMENTS * h->cfg.hist, need * sizeof(float),
                                hipMemcpyHostToDevice, h->stream));
    return calibrate_rows(h, h->d_frames, h->cfg.hist, h->cfg.hist, reference_power_level, index, correction, median,
                          usable, h->stream);
}

int awpu_hip_calibrate_ring(awpu_hip_t *h, int32_t array, float reference_power_level, int32_t *index,
                            float *correction, float *median, int32_t *usable) {
    if (h && !h->parts.empty()) h = h->parts[0];  // not pixel-sharded: a device group answers with its first device
    AWPU_CTX(h);
    if (!h || !index || !correction || !usable) return invalid("null argument");
    if (array < 0 || (array + 1) * AWPU_ELEMENTS > h->cfg.n_streams) return invalid("array outside the streams");
    if (!h->d_ring) {
        return fail(AWPU_ERR_STATE, "no block ingested yet");
    }
    AWPU_HIP_TRY(hipSetDevice(h->cfg.device));
    return calibrate_rows(h, h->d_ring + (size_t) array * AWPU_ELEMENTS * 2048 + h->ring_pos, 2048, AWPU_HIST,
                          reference_power_level, index, correction, median, usable, h->stream);
}

int awpu_hip_beams(awpu_hip_t *h, const float *d_frame, const int32_t *off, const float *frac, int32_t n_dir,
                   float *power, float *beams) {
    if (h && !h->parts.empty()) h = h->parts[0];  // not pixel-sharded: a device group answers with its first device
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
    if (h->beam_lut_cap < entries.size()) {
        dev_free(h->d_beam_lut);
        h->beam_lut_cap = 0;
        AWPU_HIP_TRY(hipMalloc(&h->d_beam_lut, entries.size() * sizeof(awpu::LutEntry)));
        h->beam_lut_cap = entries.size();
    }
    if (h->beam_cap < (size_t) n_dir) {
        dev_free(h->d_beam_out);
        h->beam_cap = 0;
        AWPU_HIP_TRY(hipMalloc(&h->d_beam_out, (size_t) n_dir * (1 + awpu::kSamples) * sizeof(float)));
        h->beam_cap = n_dir;
    }
    float *d_power = h->d_beam_out, *d_beams = h->d_beam_out + h->beam_cap;
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
    if (h && !h->parts.empty()) h = h->parts[0];  // not pixel-sharded: a device group answers with its first device
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
        dev_free(h->d_xyz);
        h->antenna.clear();
        AWPU_HIP_TRY(hipMalloc(&h->d_xyz, (size_t) 3 * n * sizeof(float)));
    }
    AWPU_HIP_TRY(hipMemcpy(h->d_xyz, xyz, (size_t) 3 * n * sizeof(float), hipMemcpyHostToDevice));
    h->antenna.assign(xyz, xyz + (size_t) 3 * n);
    return AWPU_OK;
}

namespace {

int ensure_track_buffer(awpu_hip *h, size_t bytes) {
    if (h->track_cap >= bytes) return AWPU_OK;
    dev_free(h->d_track);
    h->track_cap = 0;
    AWPU_HIP_TRY(hipMalloc(&h->d_track, bytes));
    h->track_cap = bytes;
    return AWPU_OK;
}

}  // namespace

int awpu_hip_steer_table_device(awpu_hip_t *h, const double *theta, const double *phi, int32_t n_dir, int32_t *off,
                                float *frac) {
    if (h && !h->parts.empty()) h = h->parts[0];  // not pixel-sharded: a device group answers with its first device
    AWPU_CTX(h);
    if (!h || !theta || !phi || !off || !frac) return invalid("null argument");
    if (n_dir < 1 || n_dir > 65535) return invalid("n_dir outside [1, 65535]");
    if (h->antenna.empty()) return fail(AWPU_ERR_STATE, "antenna not set (awpu_hip_set_antenna)");
    const int n = (int) (h->antenna.size() / 3);
    AWPU_HIP_TRY(hipSetDevice(h->cfg.device));
    const size_t angles = align16((size_t) n_dir * sizeof(double)), table = (size_t) n_dir * n;
    if (int rc = ensure_track_buffer(h, 2 * angles + table * (sizeof(int32_t) + sizeof(float)))) return rc;
    double *d_theta = (double *) h->d_track, *d_phi = (double *) (h->d_track + angles);
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
    if (h && !h->parts.empty()) h = h->parts[0];  // not pixel-sharded: a device group answers with its first device
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
    const int U = h->usable();
    if (int rc = ensure_track_index(h)) return rc;
    const size_t particles = (size_t) n * sizeof(awpu_particle_t), head = align16(particles + sizeof(double));
    if (int rc = ensure_track_buffer(h, head + (beams ? (size_t) n * awpu::kSamples * sizeof(float) : 0))) return rc;
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
    if (!h->parts.empty()) return for_each_part(h, [&](awpu_hip *part) { return awpu_hip_set_fir_table(part, coeffs); });
    AWPU_HIP_TRY(hipSetDevice(h->cfg.device));
    // (on the device: the caller's 101 rows followed by zero rows up to kFir8CoeffRows -- the plane kernel's padding
    // entries name row 101, and its entry requests run a few items past a row's end, where any 7-bit row may stand)
    if (!h->d_fir) AWPU_HIP_TRY(hipMalloc(&h->d_fir, awpu::kFir8CoeffRows * 8 * sizeof(float)));
    AWPU_HIP_TRY(hipStreamSynchronize(h->stream));  // (a sweep still reading the old coefficients)
    AWPU_HIP_TRY(hipMemset(h->d_fir, 0, awpu::kFir8CoeffRows * 8 * sizeof(float)));
    AWPU_HIP_TRY(hipMemcpy(h->d_fir, coeffs, 101 * 8 * sizeof(float), hipMemcpyHostToDevice));
    h->fir.assign(coeffs, coeffs + 101 * 8);
    h->have_fir = true;  // (the plane table names coefficient rows, it does not carry them: nothing to rebuild)
    return AWPU_OK;
}

int awpu_hip_process(awpu_hip_t *h, const float *frames, int32_t batch, float *power) {
    AWPU_CTX(h);
    if (!h) return invalid("null handle");
    if (!frames || !power) return invalid("null argument");
    if (h->in_flight) return fail(AWPU_ERR_STATE, "an awpu_hip_process_async call is in flight on this handle: awpu_hip_wait first");
    if (!h->parts.empty()) return group_process(h, frames, batch, power);
    if (batch == 1 && h->ranges.empty()) return live_host_call(h, frames, power);
    int rc = enqueue_host_process(h, frames, batch);
    if (rc != AWPU_OK) return rc;
    rc = enqueue_power_to_host(h, batch, power, (size_t) h->cfg.pixel_count);
    if (rc != AWPU_OK) return rc;
    return wait_and_time(h);
}

int awpu_hip_process_async(awpu_hip_t *h, const float *frames, int32_t batch, float *power) {
    AWPU_CTX(h);
    if (!h) return invalid("null handle");
    if (!frames || !power) return invalid("null argument");
    if (h->in_flight) return fail(AWPU_ERR_STATE, "a call is in flight already: awpu_hip_wait first");
    int rc;
    if (!h->parts.empty()) {
        const size_t pitch = (size_t) h->cfg.pixel_count;
        rc = for_each_part(h, [&](awpu_hip *part) {
            AWPU_CTX(part);
            const int r = enqueue_host_process(part, frames, batch);
            return r != AWPU_OK ? r : enqueue_power_to_host(part, batch, power, pitch);
        });
        if (rc != AWPU_OK) {  // parts before the failing one hold copies from `frames` and into `power` in flight, and
            const std::string why = h->last_error;  // the caller is about to hear "failed": finish them before it does
            for (awpu_hip *part : h->parts)
                if (hipSetDevice(part->cfg.device) == hipSuccess) {
                    if (part->copy_stream) (void) hipStreamSynchronize(part->copy_stream);
                    (void) hipStreamSynchronize(part->stream);
                }
            (void) hipGetLastError();
            note_error(why);
        }
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
    if (!h->parts.empty()) return for_each_part(h, [&](awpu_hip *part) { return wait_and_time(part); });
    return wait_and_time(h);
}

int awpu_hip_process_device(awpu_hip_t *h, const float *d_frames, int32_t batch, float *d_power,
                            void *stream) {
    AWPU_CTX(h);
    if (!h) return invalid("null handle");
    if (!d_frames || !d_power) return invalid("null argument");
    if (!h->parts.empty()) return group_process_device(h, d_frames, batch, d_power, static_cast<hipStream_t>(stream));
    const int rc = check_ready(h, batch);
    if (rc != AWPU_OK) return rc;
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
    TimingOff untimed(h);  // asynchronous path: the caller times its own stream
    return launch(h, d_frames, batch, d_power, s);
}

int awpu_hip_process_device_sums(awpu_hip_t *h, const float *d_frames, int32_t batch, float *d_power, float *d_sums, void *stream) {
    AWPU_CTX(h);
    if (!h) return invalid("null handle");
    if (!d_frames || !d_power || !d_sums) return invalid("null argument");
    if (!h->parts.empty()) return invalid("the pre-epilogue sums are exported by single-device handles only");
    const int rc = check_ready(h, batch);
    if (rc != AWPU_OK) return rc;
    if (!h->exact_pairs_ok) return fail(AWPU_ERR_STATE, "the pre-epilogue sums need AWPU_MATH_F32_EXACT with AWPU_INTERP_LERP");
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
    TimingOff untimed(h);
    h->sums_out = d_sums;
    const int lrc = launch(h, d_frames, batch, d_power, s);
    h->sums_out = nullptr;
    return lrc;
}

namespace {

// H2D of one block of raw datagrams + the unpack launch, enqueued on the handle's stream (no wait)
int enqueue_ingest(awpu_hip *h, const void *datagrams, int32_t stride_bytes) {
    if (!h || !datagrams) return invalid("null argument");
    if (h->cfg.hist != AWPU_HIST || h->cfg.n_streams > 256) return invalid("ingest needs hist 1024 and <= 256 streams");
    if (stride_bytes < AWPU_DATAGRAM_BYTES) return invalid("datagram stride below 1032 bytes");
    AWPU_HIP_TRY(hipSetDevice(h->cfg.device));
    const int rc = ensure_ring(h);
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

}  // namespace

int awpu_hip_ingest_block(awpu_hip_t *h, const void *datagrams, int32_t stride_bytes) {
    AWPU_CTX(h);
    if (h && !h->parts.empty()) {  // every device keeps the whole ring (264 KB per block each, over its own PCIe link)
        int rc = for_each_part(h, [&](awpu_hip *part) {
            AWPU_CTX(part);
            return enqueue_ingest(part, datagrams, stride_bytes);
        });
        if (rc != AWPU_OK) return rc;
        return for_each_part(h, [&](awpu_hip *part) {
            AWPU_HIP_TRY(hipSetDevice(part->cfg.device));
            AWPU_HIP_TRY(hipStreamSynchronize(part->stream));
            return (int) AWPU_OK;
        });
    }
    const int rc = enqueue_ingest(h, datagrams, stride_bytes);
    if (rc != AWPU_OK) return rc;
    // the staging buffer is reused by the next call: finish the copy before returning
    AWPU_HIP_TRY(hipStreamSynchronize(h->stream));
    return AWPU_OK;
}

namespace {

// the steps of one live block on h->stream, without the final wait
int enqueue_live_block(awpu_hip *h, const void *datagrams, int32_t stride_bytes, float *power, int32_t rows, int32_t cols,
                       uint8_t *image, int32_t out_rows, int32_t out_cols, const uint8_t *d_colormap, uint8_t *big_image) {
    const int n = h->cfg.n_pixels;
    int rc = enqueue_ingest(h, datagrams, stride_bytes);
    if (rc != AWPU_OK) return rc;
    rc = ensure_power(h, (size_t) n);
    if (rc != AWPU_OK) return rc;
    rc = launch(h, h->d_ring + h->ring_pos, 1, h->d_power, h->stream, kRing);
    if (rc != AWPU_OK) return rc;
    if (power) AWPU_HIP_TRY(hipMemcpyAsync(power, h->d_power, (size_t) n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (image || big_image) {
        const size_t channels = d_colormap ? 3 : 1;
        const size_t need = sizeof(float) + (size_t) n + (big_image ? (size_t) out_rows * out_cols * channels : 0);
        if (h->display_cap < need) {
            retire_live_graphs(h);
            dev_free(h->d_display);
            h->display_cap = 0;
            AWPU_HIP_TRY(hipMalloc(&h->d_display, need));
            h->display_cap = need;
        }
        float *d_peak = reinterpret_cast<float *>(h->d_display);
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
    if (h && !h->parts.empty()) return invalid("the display step needs the whole grid on one device");
    if (h && h->in_flight) return fail(AWPU_ERR_STATE, "an awpu_hip_process_async call is in flight on this handle: awpu_hip_wait first");
    int rc = check_ready(h, 1);
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
            const bool keep_timing = h->timing;
            const int keep_pos = h->ring_pos;
            const auto keep_stats = h->stats;
            h->timing = false;  // (event records inside a graph would not bracket anything)
            hipGraph_t graph = nullptr;
            hipError_t e = hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal);
            if (e == hipSuccess) {
                rc = enqueue_live_block(h, datagrams, stride_bytes, power, rows, cols, image, out_rows, out_cols, d_colormap, big_image);
                e = hipStreamEndCapture(h->stream, &graph);  // (also on failure: it takes the stream out of capture mode)
            } else {
                rc = AWPU_ERR_HIP;
            }
            h->timing = keep_timing;
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
    rc = enqueue_live_block(h, datagrams, stride_bytes, power, rows, cols, image, out_rows, out_cols, d_colormap, big_image);
    if (rc != AWPU_OK) return rc;
    AWPU_HIP_TRY(hipStreamSynchronize(h->stream));
    h->live_warm++;
    return AWPU_OK;
}

int awpu_hip_process_ring(awpu_hip_t *h, float *power) {
    AWPU_CTX(h);
    if (!h) return invalid("null handle");
    if (!power) return invalid("null argument");
    if (!h->parts.empty()) {  // every device sweeps its slab of its own ring's snapshot
        int grc = for_each_part(h, [&](awpu_hip *part) {
            AWPU_CTX(part);
            int r = check_ready(part, 1);
            if (r != AWPU_OK) return r;
            if (!part->d_ring) return fail(AWPU_ERR_STATE, "no block ingested yet");
            r = ensure_power(part, (size_t) part->cfg.pixel_count);
            if (r == AWPU_OK) r = launch(part, part->d_ring + part->ring_pos, 1, part->d_power, part->stream, kRing);
            return r != AWPU_OK ? r : enqueue_power_to_host(part, 1, power, (size_t) h->cfg.pixel_count);
        });
        if (grc != AWPU_OK) return grc;
        return for_each_part(h, [&](awpu_hip *part) { return wait_and_time(part); });
    }
    int rc = check_ready(h, 1);
    if (rc != AWPU_OK) return rc;
    if (!h->d_ring) {
        return fail(AWPU_ERR_STATE, "no block ingested yet");
    }
    const size_t need_power = (size_t) h->cfg.pixel_count;
    rc = ensure_power(h, need_power);
    if (rc != AWPU_OK) return rc;
    rc = launch(h, h->d_ring + h->ring_pos, 1, h->d_power, h->stream, kRing);
    if (rc != AWPU_OK) return rc;
    AWPU_HIP_TRY(hipMemcpyAsync(power, h->d_power, need_power * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    AWPU_HIP_TRY(hipStreamSynchronize(h->stream));
    return AWPU_OK;
}

int awpu_hip_ring_snapshot(awpu_hip_t *h, float *frames) {
    if (h && !h->parts.empty()) h = h->parts[0];  // not pixel-sharded: a device group answers with its first device
    AWPU_CTX(h);
    if (!h || !frames) return invalid("null argument");
    if (!h->d_ring) {
        return fail(AWPU_ERR_STATE, "no block ingested yet");
    }
    AWPU_HIP_TRY(hipSetDevice(h->cfg.device));
    AWPU_HIP_TRY(hipMemcpy2DAsync(frames, AWPU_HIST * sizeof(float), h->d_ring + h->ring_pos, 2048 * sizeof(float),
                                  AWPU_HIST * sizeof(float), h->cfg.n_streams, hipMemcpyDeviceToHost, h->stream));
    AWPU_HIP_TRY(hipStreamSynchronize(h->stream));
    return AWPU_OK;
}

int awpu_hip_heatmap_u8_device(awpu_hip_t *h, const float *d_power, int32_t n, int32_t batch, float *d_peak,
                               int32_t peak_given, uint8_t *d_pix, void *stream) {
    if (h && !h->parts.empty()) h = h->parts[0];  // not pixel-sharded: a device group answers with its first device
    AWPU_CTX(h);
    if (!h || !d_power || !d_peak || !d_pix || n < 1 || batch < 1 || batch > 65535) return invalid("bad argument");
    AWPU_HIP_TRY(hipSetDevice(h->cfg.device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
    AWPU_HIP_TRY(awpu::launch_heatmap(d_power, n, batch, d_peak, peak_given != 0, d_pix, s));
    return AWPU_OK;
}

int awpu_hip_upscale_u8_device(awpu_hip_t *h, const uint8_t *d_pix, int32_t rows, int32_t cols, int32_t batch,
                               const uint8_t *d_colormap, uint8_t *d_out, int32_t out_rows, int32_t out_cols,
                               void *stream) {
    if (h && !h->parts.empty()) h = h->parts[0];  // not pixel-sharded: a device group answers with its first device
    AWPU_CTX(h);
    if (!h || !d_pix || !d_out || rows < 1 || cols < 1 || batch < 1 || batch > 65535) return invalid("bad argument");
    if (out_rows < rows || out_cols < cols || out_rows > 65535) return invalid("upscale only: out >= in, out_rows <= 65535");
    AWPU_HIP_TRY(hipSetDevice(h->cfg.device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
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
    if (!h->parts.empty()) return fail(AWPU_ERR_STATE, "packed frames: a device group exchanges its frames itself");
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
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
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
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
    TimingOff untimed(h);  // asynchronous path: the caller times its own stream
    // the shape awpu_hip_process_device takes for this batch, as long as that is a frame-pair shape (sweep_packed)
    // (the buffer is the caller's: awpu_hip_packed_bytes(batch) of it are taken to be there, and the sweep reads no further)
    return sweep_packed(h, plan, d_packed, packed_floats_of(h, plan, batch), batch, d_power, s);
}

int awpu_hip_synchronize(awpu_hip_t *h) {
    AWPU_CTX(h);
    if (!h) return invalid("null handle");
    if (!h->parts.empty())
        return for_each_part(h, [&](awpu_hip *part) {
            AWPU_HIP_TRY(hipSetDevice(part->cfg.device));
            AWPU_HIP_TRY(hipStreamSynchronize(part->copy_stream));
            AWPU_HIP_TRY(hipStreamSynchronize(part->stream));
            return (int) AWPU_OK;
        });
    AWPU_HIP_TRY(hipSetDevice(h->cfg.device));
    AWPU_HIP_TRY(hipStreamSynchronize(h->stream));
    return AWPU_OK;
}

int awpu_hip_group_peer_status(awpu_hip_t *h, int32_t *status, int32_t n) {
    AWPU_CTX(h);
    if (!h || !status || n < 1) return invalid("null argument");
    const int have = h->parts.empty() ? 1 : (int) h->parts.size();
    if (n < have) return invalid("status array shorter than the device group");
    if (h->parts.empty()) {
        status[0] = AWPU_PEER_SAME_DEVICE;
    } else {
        for (int k = 0; k < have; k++)
            status[k] = h->parts[k]->peer == kPeerSame     ? AWPU_PEER_SAME_DEVICE
                        : h->parts[k]->peer == kPeerDirect ? AWPU_PEER_DIRECT
                                                           : AWPU_PEER_HOST_STAGED;
    }
    return have;
}

int awpu_hip_build_delay_table_device(int32_t device, const float *xyz, int32_t n, int32_t rows, int32_t columns, float fov_deg,
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
    float *d_xyz = nullptr, *d_rot = nullptr, *d_frac = nullptr;
    int32_t *d_off = nullptr;
    auto body = [&]() -> int {
        AWPU_HIP_TRY(hipMalloc(&d_xyz, (size_t) 3 * n * sizeof(float)));
        AWPU_HIP_TRY(hipMalloc(&d_rot, rot.size() * sizeof(float)));
        AWPU_HIP_TRY(hipMalloc(&d_off, P * n * sizeof(int32_t)));
        AWPU_HIP_TRY(hipMalloc(&d_frac, P * n * sizeof(float)));
        AWPU_HIP_TRY(hipMemcpy(d_xyz, xyz, (size_t) 3 * n * sizeof(float), hipMemcpyHostToDevice));
        AWPU_HIP_TRY(hipMemcpy(d_rot, rot.data(), rot.size() * sizeof(float), hipMemcpyHostToDevice));
        // one launch per 32 768 pixels (the grid's x dimension is not the limit; this bounds a launch's run time)
        for (size_t p0 = 0; p0 < P; p0 += 32768) {
            const int np = (int) std::min<size_t>(32768, P - p0);
            AWPU_HIP_TRY(awpu::launch_delay_table(d_xyz, n, d_rot + p0 * 12, np, awpu::samples_per_metre(), d_off + p0 * n, d_frac + p0 * n,
                                                  nullptr));
        }
        AWPU_HIP_TRY(hipMemcpy(off, d_off, P * n * sizeof(int32_t), hipMemcpyDeviceToHost));
        AWPU_HIP_TRY(hipMemcpy(frac, d_frac, P * n * sizeof(float), hipMemcpyDeviceToHost));
        return AWPU_OK;
    };
    const int rc = body();
    dev_free(d_xyz);
    dev_free(d_rot);
    dev_free(d_off);
    dev_free(d_frac);
    return rc;
}

int awpu_hip_get_stats(awpu_hip_t *h, awpu_hip_stats *stats) {
    AWPU_CTX(h);
    if (!h || !stats) return invalid("null argument");
    if (!h->parts.empty()) return group_stats(h, stats);
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
