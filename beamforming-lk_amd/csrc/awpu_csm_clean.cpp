// awpu_csm_clean.cpp -- the handle forms of CLEAN-SC (include/awpu_hip_csm_clean.h): awpu_hip_csm_clean_step_device,
// awpu_hip_csm_clean and awpu_hip_csm_clean_device.  The rule is csm_clean_rule.h's, the kernels csm_clean_kernels.hip's; the
// loop's dirty maps are awpu_hip_csm_map_device's own launch (csm_calls.h), so their bits.  Nothing in the loop waits for the
// device: picks, stop tests, `first`, the done flags and the records stay there (CsmCleanState).  The calls count no sweep launch
// and leave stats.kernel_variant alone.
#include "awpu_hip_csm.h"

#include <cstring>

#include "csm_calls.h"
#include "csm_clean_kernels.h"
#include "csm_clean_rule.h"

using namespace awpu::host;

namespace {

// the refusals that come before the handle is made ready
int check_clean(awpu_hip *h, const awpu_csm_t *c, const void *matrix) {
    if (int rc = csm_clean_check(h, c)) return rc;
    if (!matrix) return invalid("null argument");
    return AWPU_OK;
}

}  // namespace

namespace awpu::host {

int csm_clean_check(awpu_hip *h, const awpu_csm_t *c) {
    if (!h) return invalid("null handle");
    if (const char *why = awpu::csm_clean_kind_refusal(c)) return invalid(why);
    if (int rc = csm_check(h, c)) return rc;
    if (h->cfg.pixel_count < h->cfg.n_pixels) return fail(AWPU_ERR_STATE, "a slab handle takes no CLEAN-SC: the pick needs the whole map");
    return AWPU_OK;
}

int csm_clean_ready(awpu_hip *h, const awpu_csm_t &c, bool own_matrix) {
    int rc = check_ready(h, 1);
    if (rc == AWPU_OK) rc = csm_ready_map(h, &c);  // (more than 2048 active mics: AWPU_ERR_RANGE)
    if (rc == AWPU_OK) rc = h->d_csm_clean_rows.ensure(csm_spectra_floats(h, c) + csm_plane_floats(h, c));
    if (rc == AWPU_OK) rc = h->d_csm_clean_state.ensure((size_t) AWPU_CSM_MAX_BINS * sizeof(awpu::CsmCleanState));
    if (rc == AWPU_OK && own_matrix) rc = h->d_csm_clean_matrix.ensure(csm_matrix_floats(h, c));
    return rc;
}

}  // namespace awpu::host

namespace {

// the component kernel's arguments on the working matrix D, behind csm_clean_ready
int clean_args(awpu_hip *h, const awpu_csm_t &c, float gain, const float *D, awpu::CsmCleanArgs *a) {
    if (!csm_lut(h) || !h->d_tones_tables || !h->d_csm_clean_rows.holds(csm_spectra_floats(h, c) + csm_plane_floats(h, c)) || !h->d_csm_clean_state)
        return fail(AWPU_ERR_STATE, "csm_clean_ready comes first");
    *a = awpu::CsmCleanArgs{};
    a->matrix = D;
    a->lut = csm_lut(h);
    a->twiddles = csm_twiddles(h);
    a->v = h->d_csm_clean_rows.get();
    a->state = reinterpret_cast<awpu::CsmCleanState *>(h->d_csm_clean_state.get());
    a->usable = h->usable(), a->n_pixels = h->cfg.pixel_count, a->wstart = h->wstart, a->n_bins = c.n_bins;
    a->gain = gain;
    for (int i = 0; i < c.n_bins; i++) a->bin[i] = c.bin[i];
    return AWPU_OK;
}

// the loop on D, which holds the loaded matrix and is left holding the residual's; all on s, behind csm_clean_ready: nothing here
// allocates or waits.  Two launches between two maps.
int enqueue_loop(awpu_hip *h, float *D, int block_count, const awpu_csm_t &c, const awpu_csm_clean_t &cl, const CsmCleanOut &out, hipStream_t s) {
    awpu::CsmCleanArgs a;
    if (int rc = clean_args(h, c, cl.gain, D, &a)) return rc;
    float *plane = h->d_csm_clean_rows.get() + csm_spectra_floats(h, c);
    for (int i = 0; i < cl.steps; i++) {
        if (int rc = csm_enqueue_map(h, D, block_count, c, plane, nullptr, s)) return rc;  // P_i
        AWPU_HIP_TRY(awpu::launch_csm_clean_iteration(a, plane, i, cl.stop_ratio, s));
        AWPU_HIP_TRY(awpu::launch_csm_clean_update(D, a.v, a.state, a.usable, a.n_bins, s));
    }
    if (int rc = csm_enqueue_map(h, D, block_count, c, plane, nullptr, s)) return rc;  // the residual closes the loop
    AWPU_HIP_TRY(awpu::launch_csm_clean_finish(plane, a.state, cl.steps, a.n_pixels, a.n_bins, out.steps, out.clean, out.residual, out.map, s));
    return AWPU_OK;
}

bool overlap(const float *a, const float *b, size_t floats) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b), n = floats * sizeof(float);
    return x < y + n && y < x + n;
}

}  // namespace

namespace awpu::host {
int csm_clean_enqueue(awpu_hip *h, const float *d_matrix, float *D, int block_count, const awpu_csm_t &c, const awpu_csm_clean_t &cl,
                      const CsmCleanOut &out, hipStream_t s) {
    AWPU_HIP_TRY(awpu::launch_csm_clean_load(d_matrix, D, h->usable(), c.n_bins, s));
    return enqueue_loop(h, D, block_count, c, cl, out, s);
}
}  // namespace awpu::host

extern "C" {

int awpu_hip_csm_clean_step_device(awpu_hip_t *h, float *d_matrix, const int32_t *d_pixel, const awpu_csm_t *c, float gain, float *d_component,
                                   float *d_qs, void *stream) {
    if (const char *why = awpu::csm_clean_gain_refusal(gain)) return invalid(why);  // (before the handle is touched)
    AWPU_CTX(h);
    if (int rc = check_clean(h, c, d_matrix)) return rc;
    if (!d_pixel) return invalid("null argument");
    int rc = csm_clean_ready(h, *c, false);
    hipStream_t s = stream_of(h, stream);
    awpu::CsmCleanArgs a;
    if (rc == AWPU_OK) rc = clean_args(h, *c, gain, d_matrix, &a);
    if (rc == AWPU_OK) rc = enter_stream(h, s);
    if (rc != AWPU_OK) return rc;
    AWPU_HIP_TRY(awpu::launch_csm_clean_load(d_matrix, d_matrix, a.usable, a.n_bins, s));  // (the caller's upper triangle is never read)
    AWPU_HIP_TRY(awpu::launch_csm_clean_component(a, d_pixel, d_component, d_qs, s));
    AWPU_HIP_TRY(awpu::launch_csm_clean_update(d_matrix, a.v, a.state, a.usable, a.n_bins, s));
    return AWPU_OK;
}

int awpu_hip_csm_clean_device(awpu_hip_t *h, const float *d_matrix, int32_t block_count, const awpu_csm_t *c, const awpu_csm_clean_t *cl,
                              awpu_csm_clean_step_t *d_steps, float *d_clean, float *d_residual, float *d_map, float *d_residual_matrix,
                              void *stream) {
    if (const char *why = awpu::csm_clean_refusal(cl)) return invalid(why);  // (before the handle is touched)
    AWPU_CTX(h);
    if (int rc = check_clean(h, c, d_matrix)) return rc;
    if (!d_steps && !d_clean && !d_residual && !d_map && !d_residual_matrix) return invalid("no output asked for");
    if (block_count < 1) return invalid("the block count is at least 1");
    int rc = csm_clean_ready(h, *c, d_residual_matrix == nullptr);
    if (rc == AWPU_OK && d_residual_matrix && overlap(d_matrix, d_residual_matrix, csm_matrix_floats(h, *c)))
        rc = invalid("d_residual_matrix overlaps d_matrix");
    hipStream_t s = stream_of(h, stream);
    if (rc == AWPU_OK) rc = enter_stream(h, s);
    if (rc != AWPU_OK) return rc;
    float *D = d_residual_matrix ? d_residual_matrix : h->d_csm_clean_matrix.get();
    CsmCleanOut out;
    out.steps = d_steps, out.clean = d_clean, out.residual = d_residual, out.map = d_map;
    return csm_clean_enqueue(h, d_matrix, D, block_count, *c, *cl, out, s);
}

int awpu_hip_csm_clean(awpu_hip_t *h, const float *matrix, int32_t block_count, const awpu_csm_t *c, const awpu_csm_clean_t *cl,
                       awpu_csm_clean_step_t *steps, float *clean, float *residual, float *map, float *residual_matrix) {
    if (const char *why = awpu::csm_clean_refusal(cl)) return invalid(why);  // (before the handle is touched)
    AWPU_CTX(h);
    if (int rc = check_clean(h, c, matrix)) return rc;
    if (!steps && !clean && !residual && !map && !residual_matrix) return invalid("no output asked for");
    if (block_count < 1) return invalid("the block count is at least 1");
    int rc = csm_clean_ready(h, *c, false);
    // the matrix goes up; D, the three planes and the steps come back through a buffer of the library's
    const size_t M = rc == AWPU_OK ? csm_matrix_floats(h, *c) : 0, plane = rc == AWPU_OK ? csm_plane_floats(h, *c) : 0;
    const size_t step_bytes = (size_t) c->n_bins * cl->steps * sizeof(awpu_csm_clean_step_t), back_bytes = (M + 3 * plane) * sizeof(float) + step_bytes;
    if (rc == AWPU_OK) rc = h->d_csm_clean_io.ensure(M * sizeof(float) + back_bytes);
    if (rc == AWPU_OK) rc = enter_stream(h, h->stream);
    if (rc != AWPU_OK) return rc;
    hipStream_t s = h->stream;
    float *d_in = reinterpret_cast<float *>(h->d_csm_clean_io.get()), *D = d_in + M, *d_planes = D + M;
    CsmCleanOut out;
    out.steps = reinterpret_cast<awpu_csm_clean_step_t *>(d_planes + 3 * plane);
    out.clean = d_planes, out.residual = d_planes + plane, out.map = d_planes + 2 * plane;
    AWPU_HIP_TRY(hipMemcpyAsync(d_in, matrix, M * sizeof(float), hipMemcpyHostToDevice, s));
    if (rc = csm_clean_enqueue(h, d_in, D, block_count, *c, *cl, out, s); rc != AWPU_OK) return rc;
    // a call that fails on the device leaves the caller's outputs alone
    std::vector<unsigned char> back(back_bytes);
    AWPU_HIP_TRY(hipMemcpyAsync(back.data(), D, back_bytes, hipMemcpyDeviceToHost, s));
    rc = wait_and_time(h, false);
    if (rc != AWPU_OK) return rc;
    const float *b = reinterpret_cast<const float *>(back.data());
    if (residual_matrix) std::memcpy(residual_matrix, b, M * sizeof(float));
    float *const host_out[3] = {clean, residual, map};
    for (int k = 0; k < 3; k++)
        if (host_out[k]) std::memcpy(host_out[k], b + M + (size_t) k * plane, plane * sizeof(float));
    if (steps) std::memcpy(steps, b + M + 3 * plane, step_bytes);
    return AWPU_OK;
}

}  // extern "C"
