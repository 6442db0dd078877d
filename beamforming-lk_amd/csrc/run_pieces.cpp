// run_pieces.cpp -- the piece pipeline (run_pieces.h): a run of consecutive blocks of a recording, whatever is made of it, is
// cut into pieces that are staged, uploaded, swept and brought back beside one another.  The handle and what is called here out
// of awpu_hip.cpp and awpu_sweep.cpp: awpu_handle.h.
#include "run_pieces.h"

#include <cstring>

#include "block_kernels.h"

namespace awpu::host {

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

}  // namespace awpu::host
