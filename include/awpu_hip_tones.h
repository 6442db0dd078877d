/*
 * awpu_hip_tones.h -- tone maps: the spectrum of every pixel's beam from one sweep.  Heatmaps say where the sound comes from, the
 * bands (awpu_hip_band.h, awpu_hip_spectral.h) where it comes from inside a band fixed before the run -- at most four FIR bands a
 * pass, each a sweep of its own.  None of them says which frequency a pixel emits, where the 3 kHz is, or what the spectrum of
 * the source found here looks like.  The sweep already holds the answer: behind the mic loop it owns out[0..255] of its pixel, the
 * delayed and summed beam, and one 256-point transform of those values gives 129 bins, 190.7 Hz wide at the reference's sample
 * rate, from DC to 24.4 kHz -- at a fixed cost per pixel that does not grow with the mic count.  The reference has nothing like
 * this; nothing of it is replaced.
 *
 * This is a sweep of its own (the shape of awpu_hip_cohere.h's).  Its planes are power-like -- with the rectangular window the
 * bins of a pixel add up to the power awpu_hip_process returns for it (Parseval) -- so they go wherever a power row goes:
 * awpu_hip_heatmap_u8, the upscale, awpu_hip_find_peaks, and the runs below.
 *
 * THE RULE.  Plain C with one arithmetic: it does not depend on cfg.math.  Two tables come from the host functions below and every
 * implementation, host or device, reads them; nothing evaluates a cosine on the device:
 *
 *     w[i]  = 1.0f (AWPU_TONES_RECT)  or  (float) (0.5 - 0.5 cos(2 pi i / 256)) (AWPU_TONES_HANN), i = 0..255, evaluated in double
 *     t[k]  = {(float) cos(2 pi k / 256), (float) (-sin(2 pi k / 256))},                           k = 0..127, evaluated in double
 *
 * For one frame, a table off / frac with lut_stride, the active list index[usable] and optional gain[usable], for pixel p:
 *
 *   1. out[0..255]: awpu_hip_cohere_host's `sums` exactly (one lerp per sample and mic in the list's order: the reference's bits,
 *      awpu_hip_process_device_sums' in AWPU_MATH_F32_EXACT; gains apply as there).
 *   2. MA[i] = out[i]*0.5f - 0.25f*(out[i+1] + out[i-1]),  y[i] = MA[i] * w[i]  for i = 1..254;  y[0] = y[255] = 0.
 *   3. A 256-point complex FFT of z[i] = (y[i], 0), radix 2, decimation in time: the input in bit-reversed order, then stages
 *      h = 1, 2, 4, .., 128.  The butterfly on a = z[base+j], b = z[base+j+h] (base a multiple of 2h, j = 0..h-1) takes
 *      tw = t[j * (128/h)]:
 *          tr = b.re*tw.re - b.im*tw.im;   ti = b.re*tw.im + b.im*tw.re;      (every product rounded, then one - or +: no fma)
 *          z[base+j] = a + (tr, ti);       z[base+j+h] = a - (tr, ti)
 *      The full multiply is done at j = 0 too: nothing is special-cased.  The rule fixes the arithmetic, not the storage: any
 *      layout or fusion of stages that performs these butterflies gives the same bits.
 *   4. s = re*re + im*im (two rounded products, one add);  bins[k] = (c_k * s) / (wss * (float) (256 * usable)),  k = 0..128,
 *      c_0 = c_128 = 1.0f and every other c_k = 2.0f;  wss = 256.0f (RECT) or 96.0f (HANN): the sum of w squared, exact for the
 *      periodic Hann window.
 *   5. tone[g] = the sum of bins[k] over group g, k ascending, starting from +0.0f.
 *   6. pitch[p] = the bin in [edge[0], edge[n_groups]) whose bins[k] wins in awpu_hip_find.h's order: the greater bits as an
 *      unsigned 32-bit number win, equal bits go to the lower k.
 *
 * Non-finite input takes the rule as written.  The stencil removes a DC bias before the transform sees it.
 *   The device forms perform steps 1 to 4 and 6 with these operations on these operands: bins, spectrum and pitch equal the
 * rule's bit for bit, and so do groups of one bin -- wherever the values are finite or infinite.  Where a NaN arises the host and
 * the device agree on WHERE (the same entries of bins, spectrum and tone are NaN), not on its sign and payload (a host's default
 * NaN may be negative, the device's is positive), and the pitch, which compares bits, may differ at a pixel whose range holds a NaN.
 *   A wider group is added in a fixed order of the device's own (lane partials, then a wave reduction): within 2e-5 (relative) of
 * the rule's, the worst case for two orders of a sum of at most 129 non-negative terms, 2 * 128 * 2^-24.
 *
 * Out of scope here: all groups' planes from a run (a run shows one plane or the pitch), and per-source spectra inside a run --
 * callers take awpu_hip_tones_device_bins at the source's pixel.
 *
 * Conventions are those of awpu_hip.h (status codes, host pointers owned by the caller, one thread per handle).
 */
#ifndef AWPU_HIP_TONES_H
#define AWPU_HIP_TONES_H

#include "awpu_hip_find.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AWPU_TONES_BINS 129
#define AWPU_TONES_RECT 0
#define AWPU_TONES_HANN 1
#define AWPU_TONES_SHOW_PITCH (-1)

/* Which bins make which plane: 528 bytes.  window is AWPU_TONES_RECT or AWPU_TONES_HANN; n_groups lies in [1, 129];
 * edge[0 .. n_groups] is strictly ascending inside [0, 129].  Group g holds bins edge[g] .. edge[g+1] - 1; bins outside
 * [edge[0], edge[n_groups]) are in no group.  Anything else: AWPU_ERR_INVALID with nothing written. */
typedef struct awpu_tones {
    int32_t window;
    int32_t n_groups;
    int32_t edge[AWPU_TONES_BINS + 1];
} awpu_tones_t;

/* The two tables of the rule.  A window outside {RECT, HANN} or a null pointer: AWPU_ERR_INVALID. */
int awpu_hip_tones_window(int32_t window, float w[256]);
int awpu_hip_tones_twiddles(float t[128][2]);

/* Fill t->n_groups and t->edge[] (t->window is left alone): bin k belongs to [lo_hz, hi_hz) when its centre
 * k * sample_rate / 256 does; the bins in range are dealt into n_groups runs as equal as possible, wider ones first.  Fewer bins in
 * range than groups, n_groups outside [1, 129], a rate that is not positive or a null t: AWPU_ERR_INVALID, *t untouched. */
int awpu_hip_tones_linear(float lo_hz, float hi_hz, int32_t n_groups, float sample_rate, awpu_tones_t *t);

/* The rule as executable C: pure host code, no handle.  Inputs as awpu_hip_cohere_host takes them.  Each output may be NULL, at
 * least one is not: tone [batch][n_groups][n_pixels] (plane-major: a plane is a power row), pitch [batch][n_pixels], bins
 * [batch][n_pixels][129], spectrum [batch][n_pixels][129][2] (re, im of z[0..128]).  Refusals are awpu_hip_cohere_host's, plus a
 * bad t or no output: AWPU_ERR_INVALID.  Nothing is written on refusal. */
int awpu_hip_tones_host(const float *frames, int32_t batch, int32_t n_streams, int32_t hist, const int32_t *off, const float *frac,
                        int32_t lut_stride, int32_t n_pixels, const int32_t *index, int32_t usable, const float *gain,
                        const awpu_tones_t *t, float *tone, int32_t *pitch, float *bins, float *spectrum);

/* The sweep on a handle.  The forms need the delay table and the active mics; the handle's gains apply; a slab handle
 * (pixel_count < n_pixels) sweeps its own pixels: planes of pixel_count floats.  AWPU_INTERP_FIR8 and a device group:
 * AWPU_ERR_STATE; so is a call while an awpu_hip_process_async call is in flight.  With a band set on the handle (awpu_hip_band.h)
 * the input passes the band first: the result is the band-less call's on awpu_hip_band_filter'ed input, bit for bit.  An
 * AWPU_MATH_F32_FAST handle builds its table as the coherence sweep does (awpu_hip_cohere.h): a blocking copy in the first call,
 * made before the call enqueues anything.  The first call on a handle uploads the two tables of the rule in the same way.
 *
 * awpu_hip_tones: host frames [batch][n_streams][hist]; host tone [batch][n_groups][pixel_count] and pitch [batch][pixel_count],
 * each or NULL, not both; synchronous.  It uploads what awpu_hip_cohere uploads of a frame. */
int awpu_hip_tones(awpu_hip_t *h, const float *frames, int32_t batch, const awpu_tones_t *t, float *tone, int32_t *pitch);

/* ... on device buffers, enqueued on `stream` (a hipStream_t, NULL = the handle's own); asynchronous.  *t is read before the
 * call returns (it travels as a kernel argument). */
int awpu_hip_tones_device(awpu_hip_t *h, const float *d_frames, int32_t batch, const awpu_tones_t *t, float *d_tone, int32_t *d_pitch,
                          void *stream);

/* ... and with every pixel's bins [batch][pixel_count][129] and spectrum [batch][pixel_count][129][2] exported, each or NULL
 * (verification).  Here the maps may both be NULL when an export is asked for. */
int awpu_hip_tones_device_bins(awpu_hip_t *h, const float *d_frames, int32_t batch, const awpu_tones_t *t, float *d_tone, int32_t *d_pitch,
                               float *d_bins, float *d_spectrum, void *stream);

/* Tones in a run of blocks.  The three calls take the arguments of awpu_hip_cohere_blocks / _samples / _samples_device with
 * (t, show) in place of co.
 *
 * The result is defined by composition.  Row j of `power` is, for the snapshot of shown block b_j = w->first + j * w->every, plane
 * `show` of awpu_hip_tones' tone (show in [0, t->n_groups)) or (float) pitch (show == AWPU_TONES_SHOW_PITCH: a row whose heatmap
 * is brighter where the pitch is higher); `image`, `big_image`, `sources` and `count` are awpu_hip_heatmap_u8, the upscale /
 * colour / flip chain of awpu_hip_watch.h and awpu_hip_find_peaks of that row, bit for bit.  Everything else is the watch run's;
 * AWPU_INTERP_FIR8 is refused with AWPU_ERR_STATE, a bad t or show with AWPU_ERR_INVALID before the handle is touched. */
int awpu_hip_tones_blocks(awpu_hip_t *h, const void *datagrams, int32_t stride_bytes, int32_t n_blocks, const awpu_watch_t *w,
                          const awpu_tones_t *t, int32_t show, const awpu_find_t *f, uint8_t *image, uint8_t *big_image, float *power,
                          awpu_source_t *sources, int32_t *count);

int awpu_hip_tones_samples(awpu_hip_t *h, const float *samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                           const awpu_tones_t *t, int32_t show, const awpu_find_t *f, uint8_t *image, uint8_t *big_image, float *power,
                           awpu_source_t *sources, int32_t *count);

int awpu_hip_tones_samples_device(awpu_hip_t *h, const float *d_samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                                  const awpu_tones_t *t, int32_t show, const awpu_find_t *f, uint8_t *d_image, uint8_t *d_big_image,
                                  float *d_power, awpu_source_t *d_sources, int32_t *d_count, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AWPU_HIP_TONES_H */
