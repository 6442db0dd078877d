/*
 * awpu_hip_csm.h -- cross-spectral maps: conventional, diagonal-removed and Capon beamforming on the cross-spectral matrix (CSM) of
 * a recording.  Every other map of the library comes from the time-domain delay-and-sum sweep, and none of them narrows the main
 * lobe below what delay-and-sum gives: at 3 kHz the wavelength is 11 cm and the 8 x 8 array is 14 cm across, so two sources of one
 * bin that are closer than a beam width are one blob in the power map, the tone map, the coherence map and the peel run.  The
 * usual answer in array acoustics is the quadratic form P(p, k) = s^H C_k s on the matrix C_k of the microphones' cross spectra:
 * with C as it is, the conventional map; without C's diagonal, a map free of uncorrelated microphone self-noise (wind, preamp),
 * which no sweep here can remove; with a loaded inverse of C in the same form, Capon's minimum-variance map 1 / (s^H C^-1 s), which
 * resolves two incoherent sources that delay-and-sum merges.  The reference has nothing like this; nothing of it is replaced.
 *
 * THE RULE.  Plain fp32 with one arithmetic: it does not depend on cfg.math.  Every step is written with explicit fmaf and no
 * contraction.  The only tables are awpu_hip_tones_window's w[256] and awpu_hip_tones_twiddles' t[128] (awpu_hip_tones.h); t_j
 * below is e^{-j 2 pi j / 256}: t[j] for j < 128 and the negation of t[j - 128] (both parts) for j >= 128.  Nothing evaluates a
 * cosine on the device.
 *
 *   1. Spectra.  A block is 256 consecutive samples x[0..255] of one mic; no history and no ring are involved.  For the mic at
 *      position a of the active list and bin k = c->bin[..]:
 *          v = x[i] * w[i]                 (with gains: (x[i] * g) * w[i], two rounded products, staged as the sweeps stage them)
 *          j = (k * i) & 255;   re = fmaf(v, t_j.re, re);   im = fmaf(v, t_j.im, im);      i ascending, from re = im = +0
 *   2. Accumulate.  C[k][a][b], a and b positions of the active list, is an unnormalised sum over blocks in block order.  For
 *      b < a, with Xa and Xb the block's spectra, in this order:
 *          re = fmaf(Xa.re, Xb.re, re);   re = fmaf(Xa.im, Xb.im, re);   im = fmaf(Xa.im, Xb.re, im);   im = fmaf(-Xa.re, Xb.im, im)
 *      (Xa conj(Xb)).  The diagonal accumulates re the same way (b = a) and its im is written as +0.  C[k][b][a] is written as the
 *      exact conjugate (re, -im) of C[k][a][b]; only the diagonal and the entries b < a are ever read.  The call adds into the
 *      caller's matrix and into the caller's block count: a recording split over several calls gives the bits of one call.
 *   3. Steering.  For pixel p, mic id m = index[a] and bin k, from the table's off and frac:
 *          n = 256 - off;  f = frac;  g = (float) k * f;  gi = (int) g;  gf = g - (float) gi;  j = (k * n + gi) & 255  (unsigned)
 *          th = gf * 0.024543693f          ((float) (2 pi / 256): the small angle left over, at most 0.0246 rad)
 *          t2 = th * th
 *          cr = fmaf(t2, 1/24, -0.5f);    cr = fmaf(cr, t2, 1.0f)                                      (cos th, degree 4)
 *          sn = fmaf(t2, 1/120, -1/6);    sn = fmaf(sn, t2, 1.0f);    sn = sn * th                     (sin th, degree 5)
 *          s.re = t_j.re * cr + t_j.im * sn;      s.im = t_j.im * cr - t_j.re * sn           (every product rounded, then one + or -)
 *      with 1/24, 1/120 and 1/6 the nearest floats.  s = e^{-j 2 pi k tau / 256} with tau = n + f.  The constant one-sample shift
 *      of delay() is a phase common to all mics, and the rule drops it.
 *   4. The quadratic form of a Hermitian matrix H (C, or the G of step 6), per pixel and bin:
 *          y_a = sum over b < a, b ascending, of H[a][b] conj(s_b), from +0:
 *              y.re = fmaf(H.re, s_b.re, y.re);  y.re = fmaf(H.im, s_b.im, y.re);  y.im = fmaf(H.im, s_b.re, y.im);  y.im = fmaf(-H.re, s_b.im, y.im)
 *          d = sum over a ascending of H[a][a].re, plain additions from +0
 *          x = sum over a ascending of Re(s_a y_a), from +0:   x = fmaf(s_a.re, y_a.re, x);   x = fmaf(-s_a.im, y_a.im, x)
 *          q = d + (x + x);     AWPU_CSM_DIAGONAL_REMOVED:  q = x + x
 *   5. The maps.  c_0 = c_128 = 1.0f, every other c_k = 2.0f; wss = 256.0f (RECT) or 96.0f (HANN), as in the tones rule:
 *          conventional        map = (c_k * q) / (wss * 256.0f * ((float) (usable * usable) * (float) n_blocks))
 *          diagonal-removed    the same with usable * (usable - 1); a result below zero becomes +0; usable == 1 is refused
 *          Capon               map = q > 0 ? c_k / ((wss * 256.0f) * q) : +0,   with H = G
 *      With the rectangular window a unit-amplitude sine at a bin centre that arrives from p gives 0.5 in the first two maps and
 *      0.5 (1 + loading / usable) in Capon's.
 *   6. G = awpu_hip_csm_invert_host(C): per bin, in double, A = C / n_blocks + loading * (trace(C / n_blocks) / usable) * I, a
 *      Cholesky factorisation and the inverse from it, rounded to float; Hermitian exactly by mirroring the entries b < a, with an
 *      exactly real diagonal.  Host only: usable^3 work per bin.  Its bits are whatever the compiler makes of std::complex<double>.
 *  6a. The same mathematics with a written arithmetic, on the host and on the device (awpu_hip_csm_invert.h declares the calls;
 *      csrc/csm_invert_rule.h is the rule as code).  Doubles throughout; fma is the fused double operation, `/` and sqrt are the
 *      IEEE double operations, nothing else is fused.  Per bin, with n = (double) n_blocks and U = usable:
 *        Load.    For b < a:  A[a][b] = ((double) C.re / n, (double) C.im / n);   A[a][a] = (double) C[a][a].re / n.
 *                 trace = the sum of A[a][a], a ascending, plain additions from 0;   load = (double) loading * (trace / (double) U);
 *                 A[a][a] = A[a][a] + load.  Of C only the diagonal's real parts and the entries b < a are read.
 *        Factor   (A = L L^H).  For the entry (a, b), b <= a, from (sr, si) = A[a][b]; for j < b ascending, l = L[a][j], m = L[b][j]:
 *                     sr = fma(-l.re, m.re, sr);  sr = fma(-l.im, m.im, sr);  si = fma(-l.im, m.re, si);  si = fma(l.re, m.im, si)
 *                 b < a:   L[a][b] = (sr / L[b][b], si / L[b][b]).
 *                 b == a:  si is not formed.  If !(sr > 0) or sr is not finite the bin is UNSOLVED; otherwise L[a][a] = sqrt(sr).
 *        Invert the factor (M = L^-1, lower).  For the entry (a, col), a >= col, from (a == col ? 1 : 0, 0); for j = col .. a-1
 *                 ascending, l = L[a][j], m = M[j][col]:
 *                     sr = fma(-l.re, m.re, sr);  sr = fma(l.im, m.im, sr);  si = fma(-l.re, m.im, si);  si = fma(-l.im, m.re, si)
 *                 M[a][col] = (sr / L[a][a], si / L[a][a]).
 *        G = M^H M.  For b <= a, from 0; for j = a .. U-1 ascending, u = M[j][a], v = M[j][b]:
 *                     sr = fma(u.re, v.re, sr);  sr = fma(u.im, v.im, sr);  si = fma(u.re, v.im, si);  si = fma(-u.im, v.re, si)
 *                 A sum that is not finite (either part, on the diagonal too) makes the bin unsolved.
 *                 G[a][b] = ((float) sr, b < a ? (float) si : +0), mirrored as the exact conjugate.
 *        An unsolved bin: every entry of its G is +0, both parts -- Capon's step 5 then gives a +0 plane --, and its `solved`
 *                 word is 0; every other bin's is 1.
 *      Each entry's sum is serial in ascending j; the device spreads ENTRIES (and bins) over its threads, as a right-looking
 *      factorisation does whose trailing updates each take step j, so the bits do not depend on the launch shape: the device's
 *      G and solved words equal the host's bit for bit.
 *   7. CLEAN-SC: the conventional map deconvolved per bin -- map, take the strongest pixel, subtract the part of C that is
 *      coherent with its beam, map again.  awpu_hip_csm_clean.h states the step's arithmetic and declares its calls;
 *      csrc/csm_clean_rule.h is the rule as code.
 *   8. The eigendecomposition C = V L V^H and the two subspace maps built on it, MUSIC and functional beamforming
 *      (awpu_hip_csm_eig.h declares the calls; csrc/csm_eig_rule.h is the rule as code).  Doubles in 8a, floats in 8b and 8c;
 *      fma / fmaf are the fused operations, `/` and sqrt the IEEE operations, nothing else is fused.
 *  8a. Parallel-order cyclic Jacobi, per bin, with n = (double) n_blocks and U = usable:
 *        Load.    As step 6a reads C: for b < a, A[a][b] = ((double) C.re / n, (double) C.im / n) and A[b][a] its exact conjugate;
 *                 A[a][a] = ((double) C[a][a].re / n, 0);  V = I.  trace = the sum of A[a][a].re, a ascending, plain additions
 *                 from 0.  The bin is UNSOLVED (with sweeps 0) if a read entry is not finite or trace is not finite or not > 0.
 *                 thr = (trace / (double) U) * 2^-52.
 *        Order.   M = U + (U & 1): the index U of an odd U is a dummy that sits out.  A sweep is M - 1 rounds; round r pairs
 *                 (M-1, r) and ((r + i) mod (M-1), (r - i) mod (M-1)) for i = 1 .. M/2 - 1, each taken as p < q; a pair with the
 *                 dummy is dropped.  The pairs of a round are disjoint.
 *        A pair's parameters, from the matrix as the round finds it: beta = A[q][p], app = A[p][p].re, aqq = A[q][q].re;
 *                 g = sqrt(fma(beta.re, beta.re, beta.im * beta.im));  the pair rotates iff g > thr;
 *                 phi = (beta.re / g, beta.im / g);  theta = (aqq - app) / (g + g);  r = sqrt(fma(theta, theta, 1));
 *                 t = 1 / (|theta| + r), negated when theta < 0;  c = 1 / sqrt(fma(t, t, 1));  s = t * c.
 *        Phase 1, columns.  For X in {A, V}, every row i and every rotating pair, x = X[i][p], y = X[i][q], w = y phi:
 *                     w.re = fma(y.re, phi.re, -(y.im * phi.im));   w.im = fma(y.re, phi.im, y.im * phi.re)
 *                     X[i][p] = (fma(c, x.re, -(s * w.re)), fma(c, x.im, -(s * w.im)))
 *                     X[i][q] = (fma(s, x.re, c * w.re), fma(s, x.im, c * w.im))
 *        Phase 2, rows of A, behind phase 1 of the whole round.  For every column j other than p and q, x = A[p][j],
 *                 y = A[q][j], w = y conj(phi):
 *                     w.re = fma(y.re, phi.re, y.im * phi.im);      w.im = fma(y.im, phi.re, -(y.re * phi.im))
 *                 and the same two combinations.  The pair's own four entries are written in closed form:
 *                     A[p][p] = (fma(-t, g, app), 0);   A[q][q] = (fma(t, g, aqq), 0);   A[p][q] = A[q][p] = (0, 0).
 *                 Every entry is written by at most one rotation a phase: the launch shape cannot change a bit.
 *        Stop.    After the first sweep in which no pair rotated; `sweeps` counts the sweeps run, that one included.  A bin that
 *                 still rotates in its 32nd sweep is unsolved.
 *        Sort and round.  Eigenvalue j (A[j][j].re) has rank = the number of i with l_i > l_j, or l_i == l_j and i < j;
 *                 values[k][rank] = (float) l_j;  vectors[k][rank][a] = ((float) V[a][j].re, (float) V[a][j].im): an eigenvector
 *                 is one contiguous row.  A bin with an eigenvalue that does not fit a float -- (float) l_j is not finite: a NaN,
 *                 an infinity, or a finite double that rounds past FLT_MAX -- is unsolved.  An unsolved bin: every value and
 *                 every vector word +0, `solved` 0, `sweeps` as run; every other bin's `solved` is 1 and its values are finite.
 *  8b. The weighed matrix H [n_bins][usable][usable][2] from the float values and vectors and an awpu_csm_eig_t:
 *          AWPU_CSM_EIG_MUSIC        w_r = r < n_sources ? 0 : 1                  (the projector on the noise subspace)
 *          AWPU_CSM_EIG_FUNCTIONAL   w_r = l_r > 0 ? (float) ((double) l_r, square-rooted `root` times in double) : +0
 *      -- nu = 2^root keeps the root and the power in written arithmetic; pow is not the same on host and device.  For b <= a, r
 *      ascending, from +0, with u = vectors[r][a] and v = vectors[r][b] (w u conj(v)):
 *          t = w_r * u.re;  re = fmaf(t, v.re, re);  t2 = w_r * u.im;  re = fmaf(t2, v.im, re);  im = fmaf(t2, v.re, im);  im = fmaf(-t, v.im, im)
 *      The diagonal's im is written as +0, the mirror as the exact conjugate.
 *  8c. The map.  q is steps 3 and 4 on H (kind AWPU_CSM_CONVENTIONAL); Uf = (float) usable; wss and c_k as in step 5:
 *          MUSIC        floor = Uf * 2^-24;   map = Uf / (q > floor ? q : floor)     (a perfect match, a NaN or a negative q: 2^24)
 *          functional   y = (q > 0 ? q : +0) / Uf;  y squared `root` times;  map = (c_k * y) / ((wss * 256.0f) * Uf)
 *      A single source that arrives from the pixel shows the conventional map's level in the functional map (0.5 for a unit sine
 *      at a bin centre).  An unsolved bin is a +0 plane in both kinds.
 *
 * The device forms perform these operations on these operands: spectra, C, q and the maps equal the host functions' bit for bit
 * wherever the values are finite or infinite; where a NaN arises host and device agree on WHERE, not on its sign and payload.
 *
 * The planes are power rows: awpu_hip_heatmap_u8, the upscale and awpu_hip_find_peaks take them as they are.  Runs with images, a map
 * per shown block of a recording: awpu_hip_csm_watch.h.
 *
 * Conventions are those of awpu_hip.h (status codes, host pointers owned by the caller, one thread per handle).
 */
#ifndef AWPU_HIP_CSM_H
#define AWPU_HIP_CSM_H

#include "awpu_hip_tones.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AWPU_CSM_MAX_BINS 8
#define AWPU_CSM_CONVENTIONAL 0
#define AWPU_CSM_DIAGONAL_REMOVED 1
#define AWPU_CSM_CAPON 2

/* What to map: 48 bytes.  window is AWPU_TONES_RECT or AWPU_TONES_HANN; n_bins lies in [1, 8]; bin[0 .. n_bins) is strictly
 * ascending inside [0, 128]; kind is one of the three above; loading is finite and >= 0 and is read by awpu_hip_csm_invert_host
 * alone.  Anything else: AWPU_ERR_INVALID with nothing written. */
typedef struct awpu_csm {
    int32_t window;
    int32_t n_bins;
    int32_t bin[AWPU_CSM_MAX_BINS];
    int32_t kind;
    float loading;
} awpu_csm_t;

/* The rule as executable C: pure host code, no handle.  samples [n_streams][pitch] as awpu_hip_process_samples takes them, block b
 * of stream m at samples[m * pitch + 256 * b]; index [usable] stream ids, gain [usable] in the list's order or NULL; off / frac
 * [n_pixels][lut_stride] by stream id.  Refusals follow awpu_hip_cohere_host: a null input or output, a bad c, counts below 1, a
 * pitch below 256 * n_blocks, an index outside the streams (or the table's row), a frac outside [0, 1] or an off below 0 give
 * AWPU_ERR_INVALID.  Nothing is written on refusal.
 *
 * Step 1: spectra [n_blocks][n_bins][usable][2]. */
int awpu_hip_csm_spectra_host(const float *samples, int64_t pitch, int32_t n_streams, int32_t n_blocks, const int32_t *index, int32_t usable,
                              const float *gain, const awpu_csm_t *c, float *spectra);

/* Steps 1 and 2: adds the blocks into matrix [n_bins][usable][usable][2] and n_blocks into *block_count (both the caller's: zero
 * them before the first call).  A *block_count below 0, or one that would pass 2^31 - 1: AWPU_ERR_INVALID. */
int awpu_hip_csm_accumulate_host(const float *samples, int64_t pitch, int32_t n_streams, int32_t n_blocks, const int32_t *index, int32_t usable,
                                 const float *gain, const awpu_csm_t *c, float *matrix, int32_t *block_count);

/* Step 3: steer [n_pixels][n_bins][usable][2]. */
int awpu_hip_csm_steer_host(const int32_t *off, const float *frac, int32_t lut_stride, int32_t n_pixels, const int32_t *index, int32_t usable,
                            const awpu_csm_t *c, float *steer);

/* Steps 3 to 5 on matrix [n_bins][usable][usable][2] -- C with its block count, or for AWPU_CSM_CAPON the G of step 6 (the count
 * is then not read, but must still be >= 1): map [n_bins][n_pixels] and q [n_bins][n_pixels], each or NULL, not both.
 * AWPU_CSM_DIAGONAL_REMOVED with usable == 1: AWPU_ERR_INVALID. */
int awpu_hip_csm_map_host(const float *matrix, int32_t block_count, const int32_t *off, const float *frac, int32_t lut_stride, int32_t n_pixels,
                          const int32_t *index, int32_t usable, const awpu_csm_t *c, float *map, float *q);

/* Step 6: inverse [n_bins][usable][usable][2] of matrix with its block count (>= 1).  Of matrix the diagonal's real parts and the
 * entries b < a are read.  A bin whose loaded matrix is not positive definite (or not finite): AWPU_ERR_RANGE, nothing written. */
int awpu_hip_csm_invert_host(const float *matrix, int32_t block_count, int32_t usable, const awpu_csm_t *c, float *inverse);

/* The handle forms use the handle's delay table, active list and gains; a slab handle (pixel_count < n_pixels) maps its own
 * pixels: planes of pixel_count floats.  An AWPU_MATH_F32_FAST handle builds its off / frac table as the coherence sweep does
 * (awpu_hip_cohere.h): a blocking copy in the first call, made before the call enqueues anything; the first call on a handle uploads
 * the two tables of the rule in the same way.  AWPU_INTERP_FIR8, a band set on the handle (awpu_hip_band.h), a device group and a
 * call while an awpu_hip_process_async call is in flight: AWPU_ERR_STATE.  These calls leave awpu_hip_stats' kernel_variant alone.
 *
 * awpu_hip_csm_samples: steps 1 and 2 of host samples [n_streams][pitch] into the host matrix and *block_count, as
 * awpu_hip_csm_accumulate_host adds them; spectra [n_blocks][n_bins][usable][2] or NULL.  Synchronous. */
int awpu_hip_csm_samples(awpu_hip_t *h, const float *samples, int64_t pitch, int32_t n_blocks, const awpu_csm_t *c, float *matrix,
                         int32_t *block_count, float *spectra);

/* ... on device buffers (d_samples, d_matrix, d_spectra; block_count stays a host pointer and is updated before the call
 * returns), enqueued on `stream` (a hipStream_t, NULL = the handle's own); asynchronous. */
int awpu_hip_csm_samples_device(awpu_hip_t *h, const float *d_samples, int64_t pitch, int32_t n_blocks, const awpu_csm_t *c, float *d_matrix,
                                int32_t *block_count, float *d_spectra, void *stream);

/* Steps 3 to 5 of a host matrix [n_bins][usable][usable][2] with its block count, as awpu_hip_csm_map_host takes them: host map
 * [n_bins][pixel_count] and q [n_bins][pixel_count], each or NULL, not both.  Synchronous.  More active mics than the kernel can
 * keep steering vectors for in one compute unit's LDS (2048): AWPU_ERR_RANGE. */
int awpu_hip_csm_map(awpu_hip_t *h, const float *matrix, int32_t block_count, const awpu_csm_t *c, float *map, float *q);

/* ... on device buffers, enqueued on `stream`; asynchronous.  *c is read before the call returns. */
int awpu_hip_csm_map_device(awpu_hip_t *h, const float *d_matrix, int32_t block_count, const awpu_csm_t *c, float *d_map, float *d_q,
                            void *stream);

#ifdef __cplusplus
}
#endif

#include "awpu_hip_csm_invert.h" /* step 6a's calls */
#include "awpu_hip_csm_watch.h"  /* runs: a map per shown block */
#include "awpu_hip_csm_clean.h"  /* step 7: CLEAN-SC, its rule and its calls */
#include "awpu_hip_csm_eig.h"    /* step 8: the eigendecomposition and the subspace maps */

#endif /* AWPU_HIP_CSM_H */
