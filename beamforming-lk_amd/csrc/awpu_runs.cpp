// awpu_runs.cpp -- runs of consecutive blocks of a recording through the pipeline of pieces (run_pieces.h): a heatmap of every
// block (include/awpu_hip_blocks.h), the beam audio of every block (awpu_hip_listen.h), display images of every Nth block
// (awpu_hip_watch.h), the sources in every Nth block (awpu_hip_find.h) and their distances (awpu_hip_focus.h).  The watch run's
// consumer and display step: watch_run.h; spectral, exposed, coherence and peel runs: awpu_spectral.cpp, awpu_expose.cpp,
// awpu_cohere.cpp, awpu_peel.cpp.
#include "watch_run.h"

#include "awpu_hip_blocks.h"
#include "awpu_hip_listen.h"
#include "find_kernels.h"
#include "find_rule.h"

using namespace awpu::host;

namespace {

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

// the checks of a watch call that read no handle (check_watch); then the run
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

}  // namespace

extern "C" {

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

}  // extern "C"
