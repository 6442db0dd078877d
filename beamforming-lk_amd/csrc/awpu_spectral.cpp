// awpu_spectral.cpp -- the handle forms of include/awpu_hip_spectral.h: awpu_hip_process_bands and _device, and the spectral runs
// of blocks.  The rule is spectral_rule.h's, the kernels spectral_kernels.hip's; the bands' pre-pass and the sweeps behind it are
// band_cut and band_sweep (awpu_hip.cpp), the run the watch run's (watch_run.h); awpu_hip_spectral_compose is spectral_host.cpp's.
#include "watch_run.h"

#include "awpu_hip_spectral.h"
#include "spectral_kernels.h"
#include "spectral_rule.h"

using namespace awpu::host;

namespace {

// The refusals of a spectral call (awpu_hip_spectral.h) that read the handle, in the header's order, and its bands as a set.  (The
// missing table and the history rule come from check_ready and the caller: they need the prepared handle.)
int check_spectral(awpu_hip *h, const awpu_spectral_t *sp, BandSet *bands) {
    if (!h) return invalid("null handle");
    if (const char *why = awpu::spectral_refusal(sp)) return invalid(why);
    if (is_group(h)) return fail(AWPU_ERR_STATE, "a device group takes no bands");
    if (h->in_flight) return fail(AWPU_ERR_STATE, "an awpu_hip_process_async call is in flight on this handle: awpu_hip_wait first");
    if (!h->band.empty()) return fail(AWPU_ERR_STATE, "the handle has a band of its own: clear it (awpu_hip_set_band) before a spectral call");
    bands->n = sp->n_bands;
    for (int b = 0; b < sp->n_bands; b++) bands->taps[b] = sp->taps[b], bands->coef[b] = sp->coef[b];
    return AWPU_OK;
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

}  // namespace

extern "C" {

int awpu_hip_process_bands(awpu_hip_t *h, const float *frames, int32_t batch, const awpu_spectral_t *sp, float *power) {
    AWPU_CTX(h);
    if (!h) return invalid("null handle");
    if (!frames || !power) return invalid("null argument");
    BandSet bands;
    int rc = check_spectral(h, sp, &bands);
    if (rc != AWPU_OK) return rc;
    rc = enqueue_host_process(h, frames, batch, &bands);
    if (rc != AWPU_OK) return rc;
    rc = enqueue_power_to_host(h, batch * bands.n, power, (size_t) h->cfg.pixel_count);
    if (rc != AWPU_OK) return rc;
    return wait_and_time(h, true);
}

int awpu_hip_process_bands_device(awpu_hip_t *h, const float *d_frames, int32_t batch, const awpu_spectral_t *sp, float *d_power, void *stream) {
    AWPU_CTX(h);
    if (!h) return invalid("null handle");
    if (!d_frames || !d_power) return invalid("null argument");
    BandSet bands;
    int rc = check_spectral(h, sp, &bands);
    if (rc != AWPU_OK) return rc;
    rc = check_ready(h, batch);
    if (rc != AWPU_OK) return rc;
    if (bands.max_taps() - 1 > h->wstart) return fail(AWPU_ERR_RANGE, kBandHistory);
    hipStream_t s = stream_of(h, stream);
    if (rc = enter_stream(h, s); rc != AWPU_OK) return rc;
    return band_sweep(h, bands, d_frames, (long long) h->cfg.n_streams * h->cfg.hist, h->cfg.hist, h->wstart, batch, d_power,
                      (long long) batch * h->cfg.pixel_count, s, kFull);
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

}  // extern "C"
