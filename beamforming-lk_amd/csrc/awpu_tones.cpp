// awpu_tones.cpp -- the handle forms of the tone sweep (include/awpu_hip_tones.h): awpu_hip_tones, _device and _device_bins.  The
// rule is tones_rule.h's, the kernel tones_kernels.hip's, the launcher awpu_sweep.cpp's (launch_tones); the band in front of it is
// band_sweep's pre-pass (awpu_hip.cpp).  And the tone runs of blocks, watch runs (watch_run.h) swept by that sweep.
#include "watch_run.h"

#include "awpu_hip_tones.h"
#include "tones_rule.h"

using namespace awpu::host;

namespace {

// the refusals of the three forms that come before the handle is made ready
int check_tones(awpu_hip *h, const void *frames, const awpu_tones_t *t, bool any_output) {
    if (!h) return invalid("null handle");
    if (!frames) return invalid("null argument");
    if (const char *why = awpu::tones_refusal(t)) return invalid(why);
    if (!any_output) return invalid("no output asked for");
    if (is_group(h)) return fail(AWPU_ERR_STATE, "a device group takes no tone sweep");
    if (h->in_flight) return fail(AWPU_ERR_STATE, "an awpu_hip_process_async call is in flight on this handle: awpu_hip_wait first");
    if (h->cfg.interp != AWPU_INTERP_LERP) return fail(AWPU_ERR_STATE, "the tone sweep interpolates linearly: AWPU_INTERP_FIR8 is not taken");
    return AWPU_OK;
}

// behind check_ready: the steps that may block, before the call enqueues anything
int ensure_tones(awpu_hip *h) {
    const int rc = ensure_cohere_table(h);
    return rc != AWPU_OK ? rc : ensure_tones_tables(h);
}

int tones_device(awpu_hip *h, const float *d_frames, int batch, const awpu_tones_t *t, const TonesOut &out, void *stream) {
    AWPU_CTX(h);
    if (int rc = check_tones(h, d_frames, t, out.tone || out.pitch || out.bins || out.spectrum)) return rc;
    int rc = check_ready(h, batch);
    hipStream_t s = stream_of(h, stream);
    if (rc == AWPU_OK) rc = ensure_tones(h);
    if (rc == AWPU_OK) rc = enter_stream(h, s);
    if (rc != AWPU_OK) return rc;
    const OwnSweep sweep = [&](const float *frames, bool timed) { return launch_tones(h, frames, batch, *t, out, s, kFull, timed); };
    return band_sweep(h, own_band(h), d_frames, (long long) h->cfg.n_streams * h->cfg.hist, h->cfg.hist, h->wstart, batch, nullptr, 0, s, kFull, {}, &sweep);
}

// ---- tone runs (awpu_hip_tones.h; kernel in tones_kernels.hip) --------------------------------------------------------------------
// A watch run whose pieces are swept by the tone sweep (launch_tones) in place of launch(): the row a frame shows -- and everything
// behind it -- is one group's plane or the pitch row.  A group's plane does not depend on the other groups, so the sweep is asked
// for that group alone; the pitch ranges over all of them.  Pieces, histories, the band's pre-pass in the cut, the ring: the watch
// run's.
struct TonesPieces final : WatchPieces {
    awpu_tones_t t;
    const bool pitch;
    TonesPieces(awpu_hip *h_, const BlockRun &src_, int n_blocks_, const WatchRun &wr_, const awpu_tones_t &t_, int show)
        : WatchPieces(h_, src_, n_blocks_, wr_), t(t_), pitch(show == AWPU_TONES_SHOW_PITCH) {
        if (!pitch) t.n_groups = 1, t.edge[0] = t_.edge[show], t.edge[1] = t_.edge[show + 1];
    }
    int check() override {
        if (h->cfg.interp != AWPU_INTERP_LERP) return fail(AWPU_ERR_STATE, "the tone sweep interpolates linearly: AWPU_INTERP_FIR8 is not taken");
        return WatchPieces::check();
    }
    int ensure(int piece_max, int lo_, int width_, hipStream_t sw) override {  // (the handle is ready; none of the run's work is enqueued yet)
        const int rc = ensure_tones(h);
        return rc != AWPU_OK ? rc : WatchPieces::ensure(piece_max, lo_, width_, sw);
    }
    int sweep_frames(awpu_hip *, const Piece &p, const float *d_frames, float *d_pow, hipStream_t s, int layout) override {
        TonesOut out;
        (pitch ? out.pitch_row : out.tone) = d_pow;
        return launch_tones(h, d_frames, p.n, t, out, s, layout);
    }
};

// the checks of a tone run that read no handle; then the run
int tones_run(awpu_hip *h, const BlockRun &src, int n_blocks, const awpu_watch_t *w, const awpu_tones_t *t, int32_t show, const awpu_find_t *f,
              uint8_t *image, uint8_t *big, float *power, awpu_source_t *sources, int32_t *count, hipStream_t user) {
    ShownRun sr;
    if (const int rc = sr.open(w, n_blocks, [&] { return awpu::tones_refusal(t, show); }, f, image, big, power, sources, count)) return rc;
    AWPU_CTX(h);
    TonesPieces c(h, src, n_blocks, sr.wr, *t, show);
    return run_pieces(h, src, user, c);
}

}  // namespace

extern "C" {

int awpu_hip_tones(awpu_hip_t *h, const float *frames, int32_t batch, const awpu_tones_t *t, float *tone, int32_t *pitch) {
    AWPU_CTX(h);
    if (int rc = check_tones(h, frames, t, tone || pitch)) return rc;
    int rc = check_ready(h, batch);
    if (rc == AWPU_OK) rc = ensure_tones(h);
    if (rc == AWPU_OK) rc = enter_stream(h, h->stream);
    if (rc != AWPU_OK) return rc;
    // what awpu_hip_cohere uploads of a batch, in one copy on the handle's stream in front of the sweep
    const BandSet bands = own_band(h);
    const bool compact = h->compact_hist > 0;
    const int pre = compact ? std::max(bands.max_taps() - 1, 0) : 0;
    const int S = h->cfg.n_streams, dev_hist = (compact ? h->compact_hist : h->cfg.hist) + pre;
    const size_t plane = (size_t) h->cfg.pixel_count * batch;
    const size_t tone_floats = tone ? plane * (size_t) t->n_groups : 0;
    rc = h->d_frames.ensure((size_t) S * dev_hist * batch);
    if (rc == AWPU_OK) rc = h->d_tones_out.ensure(tone_floats + (pitch ? plane : 0));
    if (rc != AWPU_OK) return rc;
    if (compact) {
        AWPU_HIP_TRY(hipMemcpy2DAsync(h->d_frames, (size_t) dev_hist * sizeof(float), frames + h->wstart - pre, (size_t) h->cfg.hist * sizeof(float),
                                      (size_t) dev_hist * sizeof(float), (size_t) batch * S, hipMemcpyHostToDevice, h->stream));
    } else {
        AWPU_HIP_TRY(hipMemcpyAsync(h->d_frames, frames, (size_t) batch * S * dev_hist * sizeof(float), hipMemcpyHostToDevice, h->stream));
    }
    TonesOut out;
    if (tone) out.tone = h->d_tones_out.get();
    if (pitch) out.pitch = reinterpret_cast<int32_t *>(h->d_tones_out.get() + tone_floats);
    const int layout = compact ? kCompact : kFull;
    const OwnSweep sweep = [&](const float *swept, bool timed) { return launch_tones(h, swept, batch, *t, out, h->stream, layout, timed); };
    rc = band_sweep(h, bands, h->d_frames, (long long) S * dev_hist, dev_hist, compact ? pre : h->wstart, batch, nullptr, 0, h->stream, layout, kTimed,
                    &sweep);
    if (rc != AWPU_OK) return rc;
    if (tone) AWPU_HIP_TRY(hipMemcpyAsync(tone, out.tone, tone_floats * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (pitch) AWPU_HIP_TRY(hipMemcpyAsync(pitch, out.pitch, plane * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    return wait_and_time(h, true);
}

int awpu_hip_tones_device(awpu_hip_t *h, const float *d_frames, int32_t batch, const awpu_tones_t *t, float *d_tone, int32_t *d_pitch,
                          void *stream) {
    TonesOut out;
    out.tone = d_tone, out.pitch = d_pitch;
    return tones_device(h, d_frames, batch, t, out, stream);
}

int awpu_hip_tones_device_bins(awpu_hip_t *h, const float *d_frames, int32_t batch, const awpu_tones_t *t, float *d_tone, int32_t *d_pitch,
                               float *d_bins, float *d_spectrum, void *stream) {
    TonesOut out;
    out.tone = d_tone, out.pitch = d_pitch, out.bins = d_bins, out.spectrum = d_spectrum;
    return tones_device(h, d_frames, batch, t, out, stream);
}

int awpu_hip_tones_blocks(awpu_hip_t *h, const void *datagrams, int32_t stride_bytes, int32_t n_blocks, const awpu_watch_t *w,
                          const awpu_tones_t *t, int32_t show, const awpu_find_t *f, uint8_t *image, uint8_t *big_image, float *power,
                          awpu_source_t *sources, int32_t *count) {
    BlockRun src;
    if (int rc = wire_source(h, datagrams, stride_bytes, n_blocks, &src)) return rc;
    return tones_run(h, src, n_blocks, w, t, show, f, image, big_image, power, sources, count, nullptr);
}

int awpu_hip_tones_samples(awpu_hip_t *h, const float *samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                           const awpu_tones_t *t, int32_t show, const awpu_find_t *f, uint8_t *image, uint8_t *big_image, float *power,
                           awpu_source_t *sources, int32_t *count) {
    BlockRun src;
    if (int rc = sample_source(h, samples, pitch, n_blocks, false, &src)) return rc;
    return tones_run(h, src, n_blocks, w, t, show, f, image, big_image, power, sources, count, nullptr);
}

int awpu_hip_tones_samples_device(awpu_hip_t *h, const float *d_samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                                  const awpu_tones_t *t, int32_t show, const awpu_find_t *f, uint8_t *d_image, uint8_t *d_big_image,
                                  float *d_power, awpu_source_t *d_sources, int32_t *d_count, void *stream) {
    BlockRun src;
    if (int rc = sample_source(h, d_samples, pitch, n_blocks, true, &src)) return rc;
    return tones_run(h, src, n_blocks, w, t, show, f, d_image, d_big_image, d_power, d_sources, d_count, static_cast<hipStream_t>(stream));
}

}  // extern "C"
