// awpu_cohere.cpp -- the handle forms of the coherence sweep (include/awpu_hip_cohere.h): awpu_hip_cohere, _device and
// _device_sums.  The rule is cohere_rule.h's, the kernel cohere_kernels.hip's, the launcher awpu_sweep.cpp's (launch_cohere); the
// band in front of it is band_sweep's pre-pass (awpu_hip.cpp).  And the coherence runs of blocks, watch runs (watch_run.h) swept
// by that sweep.
#include "watch_run.h"

#include "awpu_hip_cohere.h"
#include "cohere_rule.h"

using namespace awpu::host;

namespace {

// the refusals of the three forms that come before the handle is made ready
int check_cohere(awpu_hip *h, const void *frames, bool any_output) {
    if (!h) return invalid("null handle");
    if (!frames) return invalid("null argument");
    if (!any_output) return invalid("no output asked for");
    if (is_group(h)) return fail(AWPU_ERR_STATE, "a device group takes no coherence sweep");
    if (h->in_flight) return fail(AWPU_ERR_STATE, "an awpu_hip_process_async call is in flight on this handle: awpu_hip_wait first");
    if (h->cfg.interp != AWPU_INTERP_LERP) return fail(AWPU_ERR_STATE, "the coherence sweep interpolates linearly: AWPU_INTERP_FIR8 is not taken");
    return AWPU_OK;
}

int cohere_device(awpu_hip *h, const float *d_frames, int batch, const CohereOut &out, void *stream) {
    AWPU_CTX(h);
    if (int rc = check_cohere(h, d_frames, out.power || out.coherence || out.weighted || out.sums || out.energy)) return rc;
    int rc = check_ready(h, batch);
    hipStream_t s = stream_of(h, stream);
    if (rc == AWPU_OK) rc = ensure_cohere_table(h);
    if (rc == AWPU_OK) rc = enter_stream(h, s);
    if (rc != AWPU_OK) return rc;
    const OwnSweep sweep = [&](const float *frames, bool timed) { return launch_cohere(h, frames, batch, out, s, kFull, timed); };
    return band_sweep(h, own_band(h), d_frames, (long long) h->cfg.n_streams * h->cfg.hist, h->cfg.hist, h->wstart, batch, nullptr, 0, s, kFull, {}, &sweep);
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
    ShownRun sr;
    if (const int rc = sr.open(w, n_blocks, [&] { return awpu::cohere_refusal(co); }, f, image, big, power, sources, count)) return rc;
    AWPU_CTX(h);
    CoherePieces c(h, src, n_blocks, sr.wr, co->show);
    return run_pieces(h, src, user, c);
}

}  // namespace

extern "C" {

int awpu_hip_cohere(awpu_hip_t *h, const float *frames, int32_t batch, float *power, float *coherence, float *weighted) {
    AWPU_CTX(h);
    if (int rc = check_cohere(h, frames, power || coherence || weighted)) return rc;
    int rc = check_ready(h, batch);
    if (rc == AWPU_OK) rc = ensure_cohere_table(h);
    if (rc == AWPU_OK) rc = enter_stream(h, h->stream);
    if (rc != AWPU_OK) return rc;
    // what awpu_hip_process uploads of a batch -- the window alone where it can be cut out, with the band's history in front of
    // it --, here in one copy on the handle's stream in front of the sweep (not in pieces on a copy stream beside it)
    const BandSet bands = own_band(h);
    const bool compact = h->compact_hist > 0;
    const int pre = compact ? std::max(bands.max_taps() - 1, 0) : 0;
    const int S = h->cfg.n_streams, dev_hist = (compact ? h->compact_hist : h->cfg.hist) + pre;
    const size_t plane = (size_t) h->cfg.pixel_count * batch;
    float *const host_out[3] = {power, coherence, weighted};
    float *d_out[3] = {nullptr, nullptr, nullptr};
    size_t planes = 0;  // one plane of d_cohere_out per map asked for
    for (float *o : host_out) planes += o != nullptr;
    rc = h->d_frames.ensure((size_t) S * dev_hist * batch);
    if (rc == AWPU_OK) rc = h->d_cohere_out.ensure(planes * plane);
    if (rc != AWPU_OK) return rc;
    if (compact) {
        AWPU_HIP_TRY(hipMemcpy2DAsync(h->d_frames, (size_t) dev_hist * sizeof(float), frames + h->wstart - pre, (size_t) h->cfg.hist * sizeof(float),
                                      (size_t) dev_hist * sizeof(float), (size_t) batch * S, hipMemcpyHostToDevice, h->stream));
    } else {
        AWPU_HIP_TRY(hipMemcpyAsync(h->d_frames, frames, (size_t) batch * S * dev_hist * sizeof(float), hipMemcpyHostToDevice, h->stream));
    }
    for (size_t k = 0, at = 0; k < 3; k++)
        if (host_out[k]) d_out[k] = h->d_cohere_out + plane * at++;
    CohereOut out;
    out.power = d_out[0], out.coherence = d_out[1], out.weighted = d_out[2];
    const int layout = compact ? kCompact : kFull;
    const OwnSweep sweep = [&](const float *swept, bool timed) { return launch_cohere(h, swept, batch, out, h->stream, layout, timed); };
    rc = band_sweep(h, bands, h->d_frames, (long long) S * dev_hist, dev_hist, compact ? pre : h->wstart, batch, nullptr, 0, h->stream, layout, kTimed,
                    &sweep);
    if (rc != AWPU_OK) return rc;
    for (int k = 0; k < 3; k++)
        if (host_out[k]) AWPU_HIP_TRY(hipMemcpyAsync(host_out[k], d_out[k], plane * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    return wait_and_time(h, true);
}

int awpu_hip_cohere_device(awpu_hip_t *h, const float *d_frames, int32_t batch, float *d_power, float *d_coherence, float *d_weighted,
                           void *stream) {
    CohereOut out;
    out.power = d_power, out.coherence = d_coherence, out.weighted = d_weighted;
    return cohere_device(h, d_frames, batch, out, stream);
}

int awpu_hip_cohere_device_sums(awpu_hip_t *h, const float *d_frames, int32_t batch, float *d_power, float *d_coherence, float *d_weighted,
                                float *d_sums, float *d_energy, void *stream) {
    CohereOut out;
    out.power = d_power, out.coherence = d_coherence, out.weighted = d_weighted, out.sums = d_sums, out.energy = d_energy;
    return cohere_device(h, d_frames, batch, out, stream);
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
