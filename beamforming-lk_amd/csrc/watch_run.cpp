// watch_run.cpp -- the bodies of watch_run.h: the display step, the watch run's consumer and the checks of a watch call and a find
// request that read no handle.
#include "watch_run.h"

#include "find_kernels.h"
#include "find_rule.h"

namespace awpu::host {

Display::Display(awpu_hip *h_, const WatchRun &wr_, bool host_)
    : h(h_), wr(wr_), w(wr_.w), fr(wr_.find), lr(wr_.find ? wr_.find->locate : nullptr), host(host_), want_small(wr_.image || wr_.big),
      P((size_t) h_->cfg.pixel_count), big_bytes((size_t) wr_.w.out_rows * wr_.w.out_cols * (wr_.w.d_colormap ? 3 : 1)) {}

int Display::check() const {
    if (h->cfg.pixel_count != h->cfg.n_pixels) return invalid("the display step needs the whole grid on this handle");
    if ((long long) w.rows * w.cols != h->cfg.n_pixels) return invalid("rows x cols must be the grid");
    return lr ? check_antenna(h) : (int) AWPU_OK;
}

int Display::ensure(int piece_max, hipStream_t sw) {
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

int Display::range(int b, int j0, int nf, const awpu_source_t *d_sources, const float *hist, int hist_pitch, long long frame_step, hipStream_t s) {
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

int Display::show(int b, int j0, int nf, const float *d_rows, hipStream_t s, const float *hist, int hist_pitch, long long frame_step) {
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

int Display::fetch(int b, int nf, hipStream_t s) {
    if (nf == 0) return AWPU_OK;
    if (fr)
        AWPU_HIP_TRY(hipMemcpyAsync(h->find_out.h[b], h->find_out.d[b], lr ? rpower_off + rpower_bytes(nf) : sources_off + source_bytes(nf),
                                    hipMemcpyDeviceToHost, s));
    uint8_t *to = h->watch.h[b], *from = h->watch.d[b];
    if (wr.image) AWPU_HIP_TRY(hipMemcpyAsync(to + small_off, from + small_off, (size_t) nf * P, hipMemcpyDeviceToHost, s));
    if (wr.big) AWPU_HIP_TRY(hipMemcpyAsync(to + big_off, from + big_off, (size_t) nf * big_bytes, hipMemcpyDeviceToHost, s));
    return AWPU_OK;
}

int Display::deliver(int b, int j0, int nf) {
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

// ... of a watch piece (watch_kernels.h)
static void stage_watch(awpu_hip *h, const BlockRun &src, int b0, int every, int q, int slots, int b) {
    const int m = std::min(every, 4);
    stage_slots(h, src, [=](int slot) { return awpu::watch_slot_block(slot, b0, every, m); }, q, slots, b);
}

int ring_tail(awpu_hip *h, const BlockRun &src, int n_blocks, hipStream_t s) {
    const int S = h->cfg.n_streams, b0 = n_blocks - 1, q = std::max(0, std::min(3 - b0, 4));
    const float *snapshot = h->d_ring + h->ring_pos;
    if (!src.device) {
        stage_watch(h, src, b0, 1, q, 4, 0);
        const size_t block_bytes = (size_t) awpu::kSamples * (src.wire ? (size_t) AWPU_DATAGRAM_BYTES : (size_t) S * sizeof(float));
        AWPU_HIP_TRY(hipMemcpyAsync(h->blk_in.d[0], h->blk_in.h[0], block_bytes * (4 - q), hipMemcpyHostToDevice, s));
    }
    const int rc = gathered_history(h, src, 0, q, 4, AWPU_HIST, s, [&](const float *from, long long from_pitch, int n) {
        return awpu::launch_watch_gather(from, from_pitch, snapshot, b0, 1, S, hist_of(h, 0), AWPU_HIST, 0, n, s);
    });
    if (rc != AWPU_OK) return rc;
    const int pos = (int) ((h->ring_pos + (long long) awpu::kSamples * n_blocks) % AWPU_HIST);
    AWPU_HIP_TRY(awpu::launch_ring_write(hist_of(h, 0), AWPU_HIST, 0, S, h->d_ring, pos, s));
    h->ring_pos = pos;
    return AWPU_OK;
}

WatchPieces::WatchPieces(awpu_hip *h_, const BlockRun &src_, int n_blocks_, const WatchRun &wr_)
    : h(h_), src(src_), wr(wr_), w(wr_.w), host(!src_.device), S(h_->cfg.n_streams), m(std::min(wr_.w.every, 4)), P((size_t) h_->cfg.pixel_count),
      display(h_, wr_, !src_.device) {
    n_items = wr.n_frames;
    n_blocks = n_blocks_;
    power = wr.power;
    // the last block of the call shown: the ring's new snapshot is the tail of the last piece's history
    tail = n_items == 0 || w.first + (n_items - 1) * w.every != n_blocks - 1;
}

WatchPieces::Span WatchPieces::span(const Piece &p) const {
    const int b0 = p.tail ? n_blocks - 1 : w.first + p.first * w.every, every = p.tail ? 1 : w.every;
    return {b0, every, awpu::watch_slots(every, p.tail ? 1 : p.n), std::max(0, std::min(3 - b0, 4))};
}

int WatchPieces::ensure(int piece_max, int lo_, int width_, hipStream_t sw) {
    lo = lo_, width = width_;
    const int slots_max = awpu::watch_slots(w.every, piece_max);
    pitch = awpu::kSamples * slots_max;
    snapshot = h->d_ring + h->ring_pos;
    int rc = ensure_run_buffers(h, src, piece_max, width, true, slots_max - 3, slots_max, bands.planes());
    if (rc == AWPU_OK && !host && !wr.power) rc = ensure_power(h, (size_t) piece_max * P * bands.planes());
    return rc != AWPU_OK ? rc : display.ensure(piece_max, sw);
}

int WatchPieces::staged_blocks(const Piece &p) {
    const Span g = span(p);
    stage_watch(h, src, g.b0, g.every, g.q, g.slots, p.b);
    return g.slots - g.q;
}

int WatchPieces::history(const Piece &p, hipStream_t s) {
    const Span g = span(p);
    return gathered_history(h, src, p.b, g.q, g.slots, pitch, s, [&](const float *from, long long from_pitch, int n) {
        return awpu::launch_watch_gather(from, from_pitch, snapshot, g.b0, g.every, S, hist_of(h, p.b), pitch, 0, n, s);
    });
}

int WatchPieces::cut(const Piece &p, hipStream_t s) {
    if (bands.n) return band_cut(h, bands, hist_of(h, p.b), awpu::kSamples * m, pitch, h->wstart, p.n, h->d_blk_frames, (long long) S * width * p.n, h->compact_hist > 0 ? kCompact : kFull, s);
    AWPU_HIP_TRY(awpu::launch_watch_cut(hist_of(h, p.b), pitch, S, p.n, awpu::kSamples * m, lo, width, h->d_blk_frames, s));
    return AWPU_OK;
}

int check_find_request(const awpu_watch_t *w, const awpu_find_t *f, const awpu_source_t *sources, const int32_t *count) {
    if (!sources != !count) return invalid("sources and count come together");
    if (!f != !sources) return invalid("a find request exactly when sources and count are asked for");
    if (!f) return AWPU_OK;
    if (const char *why = awpu::find_refusal(f)) return invalid(why);
    if (f->rows != w->rows || f->cols != w->cols) return invalid("the find grid must be the watch grid");
    return AWPU_OK;
}

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

}  // namespace awpu::host
