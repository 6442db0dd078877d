/*
 * awpu_hip_cohere.h -- coherence heatmaps: a sweep that weighs every pixel of a delay-and-sum map by its coherence factor, the
 * energy of the summed beam over the summed energy of the aligned channels.  A plain power map of one 8 x 8 array shows the side
 * lobes of a source 10-25 dB under its peak, and awpu_hip_find.h reports them as sources; the coherence factor is 1 where the
 * mics agree and 1 / usable on incoherent noise, so the weighted map keeps the source and drops its side lobes.  The bands
 * (awpu_hip_band.h) narrow what is shown, exposure (awpu_hip_expose.h) averages it and focus (awpu_hip_focus.h) sharpens the main
 * lobe; none of them removes side lobes.  The reference has nothing like this; nothing of it is replaced.
 *
 * This is a sweep of its own, not a pass behind one: the denominator needs every delayed mic signal of every pixel before they
 * are added.  Its rows are power-like, so they go wherever a power row goes: awpu_hip_heatmap_u8, the upscale,
 * awpu_hip_find_peaks, and the runs below.
 *
 * THE RULE.  Plain C with one arithmetic: it does not depend on cfg.math.  For one frame X [n_streams][hist], a table off / frac
 * with lut_stride, the active list index[usable] and optional gain[usable] (x = X * g, one fp32 multiply per sample, as the
 * sweeps stage it), for pixel p:
 *
 *     out[0..255] = 0;  e[1..254] = 0
 *     for s = 0 .. usable-1, id = index[s], x = X[id] + off[p*lut_stride+id], f = frac[p*lut_stride+id]:
 *         for i = 0..255:  t[i] = fmaf(f, x[i] - x[i+1], x[i+1]);       // delay(): src/dsp/delay.cpp:19-25
 *         for i = 0..255:  out[i] = out[i] + t[i];                      // the reference's bits, as in AWPU_MATH_F32_EXACT
 *         for i = 1..254:  ma = t[i]*0.5f - 0.25f*(t[i+1] + t[i-1]);    // the stencil of src/dsp/mimo.cpp:132-135, on ONE mic
 *                          e[i] = fmaf(ma, ma, e[i]);
 *     MA[i] = out[i]*0.5f - 0.25f*(out[i+1] + out[i-1]);   num = sum_{i=1..254} MA[i]*MA[i]     (i ascending)
 *     den = sum_{i=1..254} e[i]                                                                  (i ascending)
 *     power[p]     = num / (float) (256 * usable)          // the power of awpu_hip_process in AWPU_MATH_F32_EXACT, bit for bit
 *     c            = den > 0 ? num / ((float) usable * den) : 0;   if (c > 1) c = 1;
 *     coherence[p] = c;   weighted[p] = power[p] * c;      // one fp32 multiply
 *
 * Nothing is contracted except the two fmaf that are written out.  The stencil is taken on the delayed signal, so the rule reads
 * exactly X[off .. off + 256], the reach of delay(): no new range requirement.  The stencil is linear, so MA(out) is the sum of
 * the mics' MA(t) in real arithmetic and Cauchy-Schwarz gives c <= 1; the clamp covers rounding only (with one active mic num
 * and den are the same 254 numbers).  A DC bias cancels in the numerator and in the denominator alike.  Non-finite input takes
 * the rule as written: a NaN den gives 0, a NaN num over a positive den gives NaN.
 *   The device forms evaluate out[] and e[] with these operations on these operands -- their exports equal the rule's bit for
 * bit -- and add the two 254-term sums in a fixed order of their own (a wave reduction): power, coherence and weighted are then
 * within 1e-5, 2e-5 and 3e-5 (relative) of the rule's.
 *
 * Conventions are those of awpu_hip.h (status codes, host pointers owned by the caller, one thread per handle).
 */
#ifndef AWPU_HIP_COHERE_H
#define AWPU_HIP_COHERE_H

#include "awpu_hip_find.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AWPU_COHERE_WEIGHTED 0
#define AWPU_COHERE_FACTOR 1

/* What a coherence run shows: 4 bytes.  AWPU_COHERE_WEIGHTED: the weighted rows; AWPU_COHERE_FACTOR: the coherence rows.
 * Anything else: AWPU_ERR_INVALID with nothing written. */
typedef struct awpu_cohere {
    int32_t show;
} awpu_cohere_t;

/* The rule as executable C: pure host code, no handle.  frames [batch][n_streams][hist]; off / frac [n_pixels][lut_stride];
 * index [usable] stream ids; gain [usable] in the active list's order, or NULL.  Each output may be NULL: power, coherence,
 * weighted [batch][n_pixels]; sums and energy [batch][n_pixels][256] hold out[] and e[], e[0] and e[255] written as 0.  An entry
 * that reads outside the history: AWPU_ERR_RANGE; a fraction outside [0, 1], a stream id outside the frame, a null input or a
 * size below 1: AWPU_ERR_INVALID.  Nothing is written on refusal. */
int awpu_hip_cohere_host(const float *frames, int32_t batch, int32_t n_streams, int32_t hist, const int32_t *off, const float *frac,
                         int32_t lut_stride, int32_t n_pixels, const int32_t *index, int32_t usable, const float *gain, float *power,
                         float *coherence, float *weighted, float *sums, float *energy);

/* The sweep on a handle.  The three forms need the delay table and the active mics; at least one output is non-NULL; the
 * handle's gains apply; a slab handle (pixel_count < n_pixels) sweeps its own pixels: rows of pixel_count floats.
 * AWPU_INTERP_FIR8 and a device group: AWPU_ERR_STATE.  With a band set on the handle (awpu_hip_band.h) the input passes the band
 * first: the result is the band-less call's on awpu_hip_band_filter'ed input, bit for bit.
 *
 *   On an AWPU_MATH_F32_FAST handle, whose own sweeps keep no table of this sweep's kind, the first coherence call after the handle's
 * tables were built or rebuilt (a new delay table, mic list or gains) builds one: a blocking copy, made before the call enqueues
 * anything.  Make that first call outside a stream capture.
 *
 * awpu_hip_cohere: host frames [batch][n_streams][hist] and host outputs [batch][pixel_count]; synchronous.  It uploads what
 * awpu_hip_process uploads of a frame (the window the table reads, where it can be cut out), in one copy in front of the sweep. */
int awpu_hip_cohere(awpu_hip_t *h, const float *frames, int32_t batch, float *power, float *coherence, float *weighted);

/* ... on device buffers, enqueued on `stream` (a hipStream_t, NULL = the handle's own; awpu_hip.h, "Streams"); asynchronous. */
int awpu_hip_cohere_device(awpu_hip_t *h, const float *d_frames, int32_t batch, float *d_power, float *d_coherence, float *d_weighted,
                           void *stream);

/* ... and with out[] and e[] of every pixel exported: d_sums, d_energy [batch][pixel_count][256], each or NULL (verification, like
 * awpu_hip_process_device_sums).  Here the three maps may all be NULL when an export is asked for. */
int awpu_hip_cohere_device_sums(awpu_hip_t *h, const float *d_frames, int32_t batch, float *d_power, float *d_coherence, float *d_weighted,
                                float *d_sums, float *d_energy, void *stream);

/* Coherence in a run of blocks.  The three calls take the arguments of awpu_hip_watch_blocks / _samples / _samples_device plus
 * (co, f) in front of the outputs and (sources, count) behind them; f, sources and count are all NULL or none of them is.
 *
 * The result is defined by composition.  Row j of `power` is the weighted (co->show == AWPU_COHERE_WEIGHTED) or the coherence
 * (AWPU_COHERE_FACTOR) row awpu_hip_cohere gives for the snapshot of shown block b_j = w->first + j * w->every; `image`,
 * `big_image`, `sources` and `count` are awpu_hip_heatmap_u8, the upscale / colour / flip chain of awpu_hip_watch.h and
 * awpu_hip_find_peaks of that row, bit for bit.  The ring, the stats, the refusals, next_first (awpu_hip_watch_count) and mixing
 * with the other run calls are the watch run's; AWPU_INTERP_FIR8 is refused with AWPU_ERR_STATE, a show outside {0, 1} with
 * AWPU_ERR_INVALID before the handle is touched.  Pieces are those of every run: nothing grows with n_blocks. */
int awpu_hip_cohere_blocks(awpu_hip_t *h, const void *datagrams, int32_t stride_bytes, int32_t n_blocks, const awpu_watch_t *w,
                           const awpu_cohere_t *co, const awpu_find_t *f, uint8_t *image, uint8_t *big_image, float *power,
                           awpu_source_t *sources, int32_t *count);

int awpu_hip_cohere_samples(awpu_hip_t *h, const float *samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                            const awpu_cohere_t *co, const awpu_find_t *f, uint8_t *image, uint8_t *big_image, float *power,
                            awpu_source_t *sources, int32_t *count);

int awpu_hip_cohere_samples_device(awpu_hip_t *h, const float *d_samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                                   const awpu_cohere_t *co, const awpu_find_t *f, uint8_t *d_image, uint8_t *d_big_image, float *d_power,
                                   awpu_source_t *d_sources, int32_t *d_count, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AWPU_HIP_COHERE_H */
