/*
 * awpu_hip_peel.h -- peeling sources: time-domain CLEAN.  Every map of this library is a "dirty" map: each source appears with
 * the array's beam pattern around it.  awpu_hip_cohere.h takes the side lobes of ONE dominant source out of the picture; a weak
 * source that lies under a strong source's side lobes stays hidden (the channels are a mixture there, the coherence factor is
 * low), and awpu_hip_find_peaks lists the strong source's side lobes ahead of it.  Peeling shows it: sweep, take the strongest
 * pixel, form that direction's beam over the whole touched window, subtract the beam -- delayed back -- from every active mic,
 * sweep the residual again.  No model of the point-spread function is needed, because every mic's samples are at hand.  The
 * reference has nothing like this (AWProcessingUnit::targets() is empty for MIMO); nothing of it is replaced.
 *
 * THE RULE.  Plain C with one arithmetic: it does not depend on cfg.math.  The table off / frac with lut_stride, the active list
 * index[usable] (no stream twice) and optional gain[usable] are those of awpu_hip_cohere.h.
 *
 *   Reach.  E = max off - min off over all pixels of the table and the active mics; the beam is formed for i in [lo, hi],
 * lo = -E - 1, hi = 256 + E: with it every sample that ANY pixel of the table reads lies inside the subtracted range of its mic.
 * The step reads X[id][off + lo .. off + hi + 1]; where that leaves [0, hist) for any active entry of the table: AWPU_ERR_RANGE,
 * nothing enqueued or written.
 *
 *   Step.  One frame X [n_streams][hist], updated in place, a pixel p and a loop gain y.  o = off[p*lut_stride+id],
 * f = frac[p*lut_stride+id]:
 *
 *     for i = lo .. hi:        out = 0
 *                              for s = 0 .. usable-1 (list order), x = X[id] * g[s] (one fp32 multiply, as the sweeps stage it):
 *                                  out = out + fmaf(f, x[o+i] - x[o+i+1], x[o+i+1])
 *                              b[i] = out * norm                      // norm = 1.0f / (float) usable, formed once on the host
 *     for s, for i = lo .. hi-1:   c = fmaf(f, b[i+1] - b[i], b[i])   // the beam at i + f: where mic sample o+i+1 sits
 *                              X[id][o+i+1] = fmaf(-u[s], c, X[id][o+i+1])
 *
 * u[s] is formed once on the host in fp32: y without gains, y / g[s] with gains, 0 where g[s] == 0; the device takes u[] as data
 * and divides nothing.  For i in 0..255 `out` is the direction's pre-epilogue sum of awpu_hip_process_device_sums, bit for bit.
 * Nothing is contracted but the fmaf written out.  The whole beam is formed before anything is subtracted.  Mics outside the
 * active list, and a frame whose p is -1, are untouched.
 *
 *   Loop.  steps in [1, 32], gain in (0, 1], stop_ratio in [0, 1).  P_k = the power row of the current residual.  For
 * k = 0 .. steps-1, per frame:
 *     pick: among pixels with a finite power > 0 the greatest by awpu_hip_find.h's order (power bits, then the lower index);
 *           none: the frame is done
 *     k = 0: first = P_0[pick]
 *     P_k[pick] < (stop_ratio == 0 ? 0 : stop_ratio * first): the frame is done
 *     step[k] = {pixel = pick, before = P_k[pick]}; the step
 * and step[k].removed = d > 0 ? d : 0 with d = before - P_{k+1}[pixel], one fp32 subtract; a final sweep P_steps closes the last
 * step.  A done frame is no longer modified; unused steps are {-1, 0, 0}.  Per frame: residual = the last row; clean[p] = the
 * `removed` of the steps at p, added in step order (steps may come back to a pixel: one step leaves about -16 dB of a source, the
 * linear interpolation applied twice); map = clean + residual, one add.  Non-finite samples take the rule as written: a NaN frame
 * has no finite pick, is done at once and never reaches another frame of the batch.
 *   The host rule sweeps with the power of awpu_hip_cohere.h's rule (AWPU_MATH_F32_EXACT's, bit for bit); a handle with its own
 * sweep in its math mode.  On an AWPU_MATH_F32_EXACT handle picks and residual frames are the host rule's wherever the top two
 * powers of a row differ by more than the sweeps' 1e-5; the rows are within 1e-5 (relative) of it.
 *
 * Conventions are those of awpu_hip.h (status codes, host pointers owned by the caller, one thread per handle).
 */
#ifndef AWPU_HIP_PEEL_H
#define AWPU_HIP_PEEL_H

#include "awpu_hip_cohere.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AWPU_PEEL_MAX_STEPS 32
#define AWPU_PEEL_MAX_MICS 256 /* active mics a handle's step takes: u[] travels to the kernel with its arguments */
#define AWPU_PEEL_MAP 0      /* what a peel run shows: clean + residual, */
#define AWPU_PEEL_CLEAN 1    /* the removed powers at their pixels, */
#define AWPU_PEEL_RESIDUAL 2 /* the last sweep */

/* The loop's parameters: 12 bytes.  Outside their ranges: AWPU_ERR_INVALID with nothing written, before a handle is touched. */
typedef struct awpu_peel {
    int32_t steps;    /* [1, AWPU_PEEL_MAX_STEPS] */
    float gain;       /* (0, 1] */
    float stop_ratio; /* [0, 1) */
} awpu_peel_t;

/* One step of one frame: 12 bytes.  Unused: {-1, 0, 0}. */
typedef struct awpu_peel_step {
    int32_t pixel;
    float before;
    float removed;
} awpu_peel_step_t;

/* The beam's length hi - lo + 1 = 258 + 2 E of a table (pure host); < 0: a status (the refusals of awpu_hip_cohere_host). */
int32_t awpu_hip_peel_beam_length(int32_t n_streams, int32_t hist, const int32_t *off, const float *frac, int32_t lut_stride,
                                  int32_t n_pixels, const int32_t *index, int32_t usable);

/* The step as executable C: pure host code, no handle.  frames [batch][n_streams][hist] are updated in place; pixel [batch],
 * each in [0, n_pixels) or -1; beams [batch][258 + 2 E] or NULL (a row of a frame without a pixel is zeroed).  Refusals as in
 * awpu_hip_cohere_host, plus: the range rule above (AWPU_ERR_RANGE); a stream twice in the list, a pixel or gain outside its
 * range (AWPU_ERR_INVALID).  Nothing is written on refusal. */
int awpu_hip_peel_step_host(float *frames, int32_t batch, int32_t n_streams, int32_t hist, const int32_t *off, const float *frac,
                            int32_t lut_stride, int32_t n_pixels, const int32_t *index, int32_t usable, const float *gain,
                            const int32_t *pixel, float loop_gain, float *beams);

/* The loop as executable C: pure host code, no handle; `frames` is not written.  Each output may be NULL: steps [batch][pe->steps];
 * clean, residual, map [batch][n_pixels]; residual_frames [batch][n_streams][hist].  Refusals as above. */
int awpu_hip_peel_host(const float *frames, int32_t batch, int32_t n_streams, int32_t hist, const int32_t *off, const float *frac,
                       int32_t lut_stride, int32_t n_pixels, const int32_t *index, int32_t usable, const float *gain,
                       const awpu_peel_t *pe, awpu_peel_step_t *steps, float *clean, float *residual, float *map,
                       float *residual_frames);

/* The handle forms need the delay table and the active mics; the handle's gains apply.  AWPU_ERR_STATE: AWPU_INTERP_FIR8; a
 * device group; a slab handle (pixel_count < n_pixels: the pick needs the whole map); a stream twice in the active list, or more
 * than AWPU_PEEL_MAX_MICS of them; a handle with a band set (awpu_hip_band.h) -- the band's pre-pass writes only the window, and
 * the step reads E + 1 samples either side of it: peeling a band-limited map is out of scope here.
 *   The step reads the pixel's row of the table the coherence sweep uses.  On an AWPU_MATH_F32_FAST handle, whose own sweeps keep
 * no table of that kind, the first peel or coherence call after the handle's tables were built or rebuilt builds one: a blocking
 * copy, made before the call enqueues anything.  The loop forms keep buffers of the handle's -- the residual frames where the
 * caller gives none, the loop's power row, its bookkeeping, a host form's results --, allocated at their first call and again
 * at a call with a larger batch: allocation waits for the device, and it too happens before the call enqueues anything.  Make
 * the first call of a batch size outside a stream capture; every later one enqueues and returns.
 *
 * One step: d_frames [batch][n_streams][hist] updated in place; d_pixel [batch] device memory, each in [0, n_pixels) or -1 (what
 * else it holds is not checked: the kernel skips a frame whose pixel is outside the table); d_beams [batch][258 + 2 E] or NULL.
 * Enqueued on `stream` (a hipStream_t, NULL = the handle's own; awpu_hip.h, "Streams"); asynchronous. */
int awpu_hip_peel_step_device(awpu_hip_t *h, float *d_frames, int32_t batch, const int32_t *d_pixel, float loop_gain, float *d_beams,
                              void *stream);

/* The loop.  The result is defined by composition: it equals, bit for bit, what a caller gets by driving awpu_hip_process_device
 * on the same batch, the pick and awpu_hip_peel_step_device by hand -- the sweeps are the handle's own, in its math mode.
 *
 * awpu_hip_peel: host frames [batch][n_streams][hist] (whole frames travel: the step reads outside the sweep's window) and host
 * outputs as in awpu_hip_peel_host, each or NULL; synchronous. */
int awpu_hip_peel(awpu_hip_t *h, const float *frames, int32_t batch, const awpu_peel_t *pe, awpu_peel_step_t *steps, float *clean,
                  float *residual, float *map, float *residual_frames);

/* ... on device buffers, enqueued on `stream`; asynchronous, and nothing inside the loop waits for the device: the picks, the
 * stop tests and the steps' records stay on the device.  d_frames is not written; the residual is kept in a buffer of the
 * handle's, or in d_residual_frames [batch][n_streams][hist] where that is given (it must not overlap d_frames) -- awpu_hip_beams
 * on it is a weak source's audio with the strong one removed. */
int awpu_hip_peel_device(awpu_hip_t *h, const float *d_frames, int32_t batch, const awpu_peel_t *pe, awpu_peel_step_t *d_steps,
                         float *d_clean, float *d_residual, float *d_map, float *d_residual_frames, void *stream);

/* Peeling in a run of blocks.  The three calls take the arguments of awpu_hip_watch_blocks / _samples / _samples_device plus
 * (pe, show, f) in front of the outputs and (steps, sources, count) behind them; f, sources and count are all NULL or none of
 * them is; steps [n_frames][pe->steps] or NULL.
 *
 * The result is defined by composition.  Row j of `power` is the map (show == AWPU_PEEL_MAP), the clean (AWPU_PEEL_CLEAN) or the
 * residual (AWPU_PEEL_RESIDUAL) row, and row j of `steps` the steps, that awpu_hip_peel gives for the snapshot of shown block
 * b_j = w->first + j * w->every; `image`, `big_image`, `sources` and `count` are awpu_hip_heatmap_u8, the upscale / colour / flip
 * chain of awpu_hip_watch.h and awpu_hip_find_peaks of that row, bit for bit.  The ring, the refusals, next_first
 * (awpu_hip_watch_count) and mixing with the other run calls are the watch run's; the stats count every sweep of the loop
 * (pe->steps + 1 launches a piece).  The handle forms' AWPU_ERR_STATE and AWPU_ERR_RANGE refusals apply; pe or show outside their
 * ranges: AWPU_ERR_INVALID before the handle is touched.  A piece's snapshots are cut whole, not as the window the table touches
 * (the step reads outside it).  Pieces are those of every run: nothing grows with n_blocks. */
int awpu_hip_peel_blocks(awpu_hip_t *h, const void *datagrams, int32_t stride_bytes, int32_t n_blocks, const awpu_watch_t *w,
                         const awpu_peel_t *pe, int32_t show, const awpu_find_t *f, uint8_t *image, uint8_t *big_image, float *power,
                         awpu_peel_step_t *steps, awpu_source_t *sources, int32_t *count);

int awpu_hip_peel_samples(awpu_hip_t *h, const float *samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                          const awpu_peel_t *pe, int32_t show, const awpu_find_t *f, uint8_t *image, uint8_t *big_image, float *power,
                          awpu_peel_step_t *steps, awpu_source_t *sources, int32_t *count);

int awpu_hip_peel_samples_device(awpu_hip_t *h, const float *d_samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                                 const awpu_peel_t *pe, int32_t show, const awpu_find_t *f, uint8_t *d_image, uint8_t *d_big_image,
                                 float *d_power, awpu_peel_step_t *d_steps, awpu_source_t *d_sources, int32_t *d_count, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AWPU_HIP_PEEL_H */
