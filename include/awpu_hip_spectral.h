/*
 * awpu_hip_spectral.h -- spectral heatmaps: up to four FIR bands swept from one pass over the samples, and the colour-by-frequency
 * picture of an acoustic camera -- low band red, middle green, high blue -- composed on the device.  A drone's whine and a
 * ventilator's rumble separate by colour even where their lobes overlap.
 *
 * The reference wanted three bands side by side and built none: math_toolbox/filter_produce.m designs fir1(..., 'bandpass')
 * filters for 1950-3541, 3541-6375 and 6375-9000 Hz, and src/dsp/particle.h:17 carries USE_BANDPASS.
 *
 * Without this header a caller gets the picture by running a recording once per band (awpu_hip_set_band, then a watch run), which
 * uploads, unpacks, ingests and stages the same samples once per band.  Here the samples travel once: one pre-pass writes every
 * band's filtered window from one read of the history, every band is swept by the very launch the band-by-band call makes, and
 * one display step turns up to three of the power planes into an interleaved three-byte image and names the band that dominates
 * every pixel.
 *
 * DEFINED BY COMPOSITION with calls that exist, bit for bit:
 *   - powers:  band b's powers are what the call of the same form returns on the same handle with awpu_hip_set_band(coef[b],
 *     taps[b]) in force (awpu_hip_band.h), in every math mode and interpolation.  Per-mic gains stay behind the filter.
 *   - images:  awpu_hip_spectral_compose below -- pure host C -- of a frame's band powers; the large image is
 *     awpu_hip_resize_linear_u8 of every byte plane of the compact one, interleaved again, mirrored left-right on request.
 *
 * Conventions are those of awpu_hip.h (status codes, host pointers owned by the caller, one thread per handle).
 */
#ifndef AWPU_HIP_SPECTRAL_H
#define AWPU_HIP_SPECTRAL_H

#include "awpu_hip_watch.h"
#include "awpu_hip_band.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AWPU_SPECTRAL_MAX_BANDS 4      /* 4 x 128 coefficients = 2 KB: they still travel as kernel arguments (4 KB limit) */
#define AWPU_SPECTRAL_SCALE_COMMON 0   /* one maximum per frame over the shown bands: colours compare bands */
#define AWPU_SPECTRAL_SCALE_PER_BAND 1 /* each shown band scaled by its own maximum, as awpu_hip_heatmap_u8 does */

typedef struct awpu_spectral {
    int32_t n_bands;                               /* 1 .. AWPU_SPECTRAL_MAX_BANDS */
    int32_t taps[AWPU_SPECTRAL_MAX_BANDS];         /* each in [1, AWPU_BAND_MAX_TAPS]; the bands may differ */
    const float *coef[AWPU_SPECTRAL_MAX_BANDS];    /* host, [taps[b]], finite; copied by the call */
    int32_t channel[3];                            /* the band shown in byte 0, 1, 2 of a pixel, or -1: that byte is 0 */
    int32_t scale;                                 /* AWPU_SPECTRAL_SCALE_* */
} awpu_spectral_t;

/* THE DISPLAY RULE, pure host code, no handle: one frame.  Band b's n pixels are at power + b * band_pitch.
 * image [n][3] bytes, dominant [n] bytes; either may be NULL, not both.
 *   SCALE_PER_BAND: byte c of pixel i = awpu_hip_heatmap_u8(power of band channel[c], n)[i].
 *   SCALE_COMMON:   max_v = awpu_hip_heatmap_u8's running maximum from 0 (a NaN never replaces it) over all pixels of the bands
 *                   named in channel[]; every level is that function's expression -- float division, double multiply by 255,
 *                   clip, truncate; a NaN level is 0 -- with this max_v.  That is: the bytes awpu_hip_heatmap_u8 gives for the
 *                   shown planes laid end to end.  An all-zero frame gives an all-zero image.
 *   channel[c] == -1: byte c is 0.
 *   dominant[i] = the band b in [0, n_bands) -- all of them, shown or not -- that beats the others at pixel i in
 *                   awpu_hip_find.h's order: the greater bits(power) as an unsigned 32-bit number wins, equal bits go to the
 *                   lower b.  Outside finite non-negative powers the rule applies as written.
 * AWPU_ERR_INVALID with nothing written: null power or channel, both outputs null, n < 1, n_bands outside [1, 4], a channel
 * outside [-1, n_bands), an unknown scale. */
int awpu_hip_spectral_compose(const float *power, int64_t band_pitch, int32_t n_bands, int32_t n, const int32_t *channel, int32_t scale,
                              uint8_t *image, uint8_t *dominant);

/* frames [batch][n_streams][hist] (host) -> power [n_bands][batch][pixel_count] (host): power[b] is, bit for bit, what
 * awpu_hip_process returns for the same batch on the same handle with band b set.  One upload, one pre-pass per upload piece,
 * one sweep per band.  batch <= cfg.max_batch (not batch * n_bands).  channel and scale are checked and not used.  Synchronous.
 * awpu_hip_get_stats counts frames and launches as the band-by-band calls do in sum; last_kernel_ms spans the pre-pass and
 * every band's sweep.
 *
 * Refusals of every call below, before anything is enqueued, handle and ring untouched:
 *   AWPU_ERR_INVALID  a bad `sp` (null, n_bands, taps, a null or non-finite coefficient, channel, scale) or bad arguments of the
 *                     call (for the runs: the watch run's checks);
 *   AWPU_ERR_STATE    a device-group handle; an awpu_hip_process_async call in flight; a handle with a band of its own set (the
 *                     two would compose ambiguously: clear it first); then: no delay table, mic list or (FIR8) FIR table;
 *   AWPU_ERR_RANGE    max_b taps[b] - 1 exceeds the table's smallest `off` (the band's history rule, awpu_hip_band.h). */
int awpu_hip_process_bands(awpu_hip_t *h, const float *frames, int32_t batch, const awpu_spectral_t *sp, float *power);

/* The same on device buffers, enqueued on `stream` (a hipStream_t, NULL = the handle's own; awpu_hip.h, "Streams"); asynchronous: power[b] is what
 * awpu_hip_process_device writes with band b set. */
int awpu_hip_process_bands_device(awpu_hip_t *h, const float *d_frames, int32_t batch, const awpu_spectral_t *sp, float *d_power,
                                  void *stream);

/* RUNS: the arguments of awpu_hip_watch_blocks / _samples / _samples_device, then the bands and the outputs.  With n_frames as
 * awpu_hip_watch_count gives it, each output may be NULL, at least one is not:
 *   image      [n_frames][rows * cols][3]: row j = awpu_hip_spectral_compose of frame j's band powers
 *   big_image  [n_frames][out_rows][out_cols][3]: every byte plane is awpu_hip_resize_linear_u8 of the same plane of `image`
 *              row j, interleaved again, then mirrored left-right when w->flip
 *   dominant   [n_frames][rows * cols]: row j = awpu_hip_spectral_compose's `dominant` of frame j's band powers
 *   power      [n_bands][n_frames][pixel_count]: power[b] = the `power` of the watch call of the same form on a handle whose
 *              band is band b, bit for bit
 * w->d_colormap must be NULL (AWPU_ERR_INVALID).  The ring -- it keeps raw samples --, next_first, a recording split over calls,
 * mixing with the other runs, n_frames == 0 and the memory statement are the watch run's; the per-piece windows, powers and
 * images are held once per band, and nothing grows with n_blocks.  In the device form the powers stay on the device:
 * awpu_hip_find_peaks_device on d_power + b * n_frames * pixel_count finds the sources of band b. */
int awpu_hip_spectral_blocks(awpu_hip_t *h, const void *datagrams, int32_t stride_bytes, int32_t n_blocks, const awpu_watch_t *w,
                             const awpu_spectral_t *sp, uint8_t *image, uint8_t *big_image, uint8_t *dominant, float *power);

int awpu_hip_spectral_samples(awpu_hip_t *h, const float *samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                              const awpu_spectral_t *sp, uint8_t *image, uint8_t *big_image, uint8_t *dominant, float *power);

int awpu_hip_spectral_samples_device(awpu_hip_t *h, const float *d_samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                                     const awpu_spectral_t *sp, uint8_t *d_image, uint8_t *d_big_image, uint8_t *d_dominant,
                                     float *d_power, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AWPU_HIP_SPECTRAL_H */
