// awpu_peel.cpp -- the handle forms of peeling (include/awpu_hip_peel.h): awpu_hip_peel_step_device, awpu_hip_peel and
// awpu_hip_peel_device.  The rule is peel_rule.h's, the kernels peel_kernels.hip's; the loop's sweeps are the handle's own
// launch() (awpu_sweep.cpp), the step's table the coherence sweep's (ensure_cohere_table).  Nothing in the loop waits for the
// device: picks, stop tests and records stay there (PeelState).
#include "awpu_handle.h"

#include "awpu_hip_peel.h"
#include "peel_kernels.h"
#include "peel_rule.h"

using namespace awpu::host;

namespace awpu::host {

// the refusals of a handle that come before it is made ready (awpu_hip_peel.h)
int peel_handle_refusal(awpu_hip *h) {
    if (is_group(h)) return fail(AWPU_ERR_STATE, "a device group takes no peel");
    if (h->in_flight) return fail(AWPU_ERR_STATE, "an awpu_hip_process_async call is in flight on this handle: awpu_hip_wait first");
    if (h->cfg.interp != AWPU_INTERP_LERP) return fail(AWPU_ERR_STATE, "the peel interpolates linearly: AWPU_INTERP_FIR8 is not taken");
    if (h->cfg.pixel_count < h->cfg.n_pixels) return fail(AWPU_ERR_STATE, "a slab handle takes no peel: the pick needs the whole map");
    if (!h->band.empty()) return fail(AWPU_ERR_STATE, "a handle with a band takes no peel: the step reads outside the window the band's pre-pass writes");
    return AWPU_OK;
}

}  // namespace awpu::host

namespace {

int check_peel(awpu_hip *h, const void *frames) {
    if (!h) return invalid("null handle");
    if (!frames) return invalid("null argument");
    return peel_handle_refusal(h);
}

// the step's arguments (all but frames, beams and u[]) of a handle that check_ready has made ready: the table's reach, the range
// rule, the table of an AWPU_MATH_F32_FAST handle.  May block (ensure_cohere_table): before the call enqueues anything
int peel_args(awpu_hip *h, int batch, awpu::PeelArgs *a) {
    const int U = h->usable();
    if (U > AWPU_PEEL_MAX_MICS) return fail(AWPU_ERR_STATE, "more than AWPU_PEEL_MAX_MICS active mics");
    if (h->peel_gen != h->table_gen) {
        if (awpu::peel_listed_twice(h->index.data(), U)) return fail(AWPU_ERR_STATE, "the active list names a stream twice: the peel subtracts from each stream once");
        const awpu::PeelReach r = awpu::peel_reach(h->off.data(), h->cfg.lut_stride, h->cfg.pixel_count, h->index.data(), U);
        h->peel_min_off = r.min_off, h->peel_max_off = r.max_off;
        h->peel_gen = h->table_gen;
    }
    awpu::PeelReach reach{h->peel_min_off, h->peel_max_off, 0, 0};
    const int E = reach.max_off - reach.min_off;
    reach.lo = -E - 1, reach.len = awpu::kPeelSamples + 2 * E + 2;
    if (!awpu::peel_in_range(reach, h->cfg.hist)) return fail(AWPU_ERR_RANGE, "the peel reads E + 1 samples either side of the delay window: outside the frame history");
    if (const int rc = ensure_cohere_table(h); rc != AWPU_OK) return rc;
    *a = awpu::PeelArgs{};
    a->lut = h->d_lut ? h->d_lut.get() : h->d_cohere_lut.get();
    a->index = h->d_index;
    a->gain = h->d_gain;
    a->n_streams = h->cfg.n_streams, a->hist = h->cfg.hist, a->usable = U, a->n_pixels = h->cfg.pixel_count;
    a->wstart = h->wstart, a->lo = reach.lo, a->len = reach.len, a->batch = batch;
    a->norm = 1.0f / (float) U;
    return AWPU_OK;
}

int ready_peel(awpu_hip *h, int batch, awpu::PeelArgs *a) {
    const int rc = check_ready(h, batch);
    return rc != AWPU_OK ? rc : peel_args(h, batch, a);
}

void set_u(const awpu_hip *h, float loop_gain, awpu::PeelArgs *a) {
    std::vector<float> g;  // the gains in the active list's order, as d_gain holds them
    for (int s = 0; s < a->usable && !h->gain.empty(); s++) g.push_back(h->gain[h->index[s]]);
    for (int s = 0; s < a->usable; s++) a->u[s] = awpu::peel_u(loop_gain, g.empty() ? nullptr : g.data(), s);
}

}  // namespace

namespace awpu::host {

// Everything of a loop that may block -- the checks of peel_args, the table, the loop's own buffers for `batch` frames --, on a
// handle that check_ready has made ready and before the call enqueues anything
int peel_prepare(awpu_hip *h, int batch) {
    awpu::PeelArgs a;
    int rc = peel_args(h, batch, &a);
    if (rc == AWPU_OK) rc = h->d_peel_power.ensure((size_t) batch * a.n_pixels);
    if (rc == AWPU_OK) rc = h->d_peel_state.ensure((size_t) batch * sizeof(awpu::PeelState));
    return rc;
}

// the loop on `work` [batch][n_streams][hist], which holds the frames and is left holding the residual; all on s, behind
// peel_prepare for at least this batch: nothing here allocates or waits
int peel_enqueue(awpu_hip *h, float *work, int batch, const awpu_peel_t &pe, const PeelOut &out, hipStream_t s) {
    awpu::PeelArgs a;
    int rc = peel_args(h, batch, &a);
    if (rc != AWPU_OK) return rc;
    if (!h->d_peel_power.holds((size_t) batch * a.n_pixels) || !h->d_peel_state.holds((size_t) batch * sizeof(awpu::PeelState)))
        return fail(AWPU_ERR_STATE, "peel_prepare comes first");
    awpu::PeelState *state = reinterpret_cast<awpu::PeelState *>(h->d_peel_state.get());
    a.frames = work, a.beams = nullptr;
    set_u(h, pe.gain, &a);
    for (int k = 0; k < pe.steps; k++) {
        if (rc = launch(h, work, batch, h->d_peel_power, s, kFull); rc != AWPU_OK) return rc;  // P_k
        AWPU_HIP_TRY(awpu::launch_peel_iteration(a, h->d_peel_power, state, k, pe.stop_ratio, s));
    }
    if (rc = launch(h, work, batch, h->d_peel_power, s, kFull); rc != AWPU_OK) return rc;  // P_steps closes the last step
    AWPU_HIP_TRY(awpu::launch_peel_finish(h->d_peel_power, state, pe.steps, a.n_pixels, batch, out.steps, out.clean, out.residual, out.map, s));
    return AWPU_OK;
}

}  // namespace awpu::host

extern "C" {

int awpu_hip_peel_step_device(awpu_hip_t *h, float *d_frames, int32_t batch, const int32_t *d_pixel, float loop_gain, float *d_beams,
                              void *stream) {
    if (const char *why = awpu::peel_gain_refusal(loop_gain)) return invalid(why);  // (before the handle is touched)
    AWPU_CTX(h);
    if (int rc = check_peel(h, d_frames)) return rc;
    if (!d_pixel) return invalid("null argument");
    awpu::PeelArgs a;
    int rc = ready_peel(h, batch, &a);
    hipStream_t s = stream_of(h, stream);
    if (rc == AWPU_OK) rc = enter_stream(h, s);
    if (rc != AWPU_OK) return rc;
    a.frames = d_frames, a.beams = d_beams;
    set_u(h, loop_gain, &a);
    AWPU_HIP_TRY(awpu::launch_peel_step(a, d_pixel, s));
    return AWPU_OK;
}

int awpu_hip_peel_device(awpu_hip_t *h, const float *d_frames, int32_t batch, const awpu_peel_t *pe, awpu_peel_step_t *d_steps,
                         float *d_clean, float *d_residual, float *d_map, float *d_residual_frames, void *stream) {
    if (const char *why = awpu::peel_refusal(pe)) return invalid(why);  // (before the handle is touched)
    AWPU_CTX(h);
    if (int rc = check_peel(h, d_frames)) return rc;
    awpu::PeelArgs a;
    int rc = ready_peel(h, batch, &a);
    hipStream_t s = stream_of(h, stream);
    const size_t floats = (size_t) batch * h->cfg.n_streams * h->cfg.hist;
    if (rc == AWPU_OK) rc = peel_prepare(h, batch);
    if (rc == AWPU_OK && !d_residual_frames) rc = h->d_peel_frames.ensure(floats);
    if (rc == AWPU_OK) rc = enter_stream(h, s);
    if (rc != AWPU_OK) return rc;
    float *work = d_residual_frames ? d_residual_frames : h->d_peel_frames.get();
    AWPU_HIP_TRY(hipMemcpyAsync(work, d_frames, floats * sizeof(float), hipMemcpyDeviceToDevice, s));
    PeelOut out;
    out.steps = d_steps, out.clean = d_clean, out.residual = d_residual, out.map = d_map;
    return peel_enqueue(h, work, batch, *pe, out, s);
}

int awpu_hip_peel(awpu_hip_t *h, const float *frames, int32_t batch, const awpu_peel_t *pe, awpu_peel_step_t *steps, float *clean,
                  float *residual, float *map, float *residual_frames) {
    if (const char *why = awpu::peel_refusal(pe)) return invalid(why);  // (before the handle is touched)
    AWPU_CTX(h);
    if (int rc = check_peel(h, frames)) return rc;
    awpu::PeelArgs a;
    int rc = ready_peel(h, batch, &a);
    const size_t floats = (size_t) batch * h->cfg.n_streams * h->cfg.hist, plane = (size_t) batch * h->cfg.pixel_count;
    const size_t step_bytes = align16((size_t) batch * pe->steps * sizeof(awpu_peel_step_t));
    if (rc == AWPU_OK) rc = peel_prepare(h, batch);
    if (rc == AWPU_OK) rc = h->d_peel_frames.ensure(floats);
    if (rc == AWPU_OK) rc = h->d_peel_out.ensure(step_bytes + 3 * plane * sizeof(float));
    if (rc == AWPU_OK) rc = enter_stream(h, h->stream);
    if (rc != AWPU_OK) return rc;
    hipStream_t s = h->stream;
    AWPU_HIP_TRY(hipMemcpyAsync(h->d_peel_frames, frames, floats * sizeof(float), hipMemcpyHostToDevice, s));
    float *const d_maps = reinterpret_cast<float *>(h->d_peel_out.get() + step_bytes);
    PeelOut out;
    out.steps = reinterpret_cast<awpu_peel_step_t *>(h->d_peel_out.get());
    out.clean = d_maps, out.residual = d_maps + plane, out.map = d_maps + 2 * plane;
    if (rc = peel_enqueue(h, h->d_peel_frames, batch, *pe, out, s); rc != AWPU_OK) return rc;
    if (steps) AWPU_HIP_TRY(hipMemcpyAsync(steps, out.steps, (size_t) batch * pe->steps * sizeof(awpu_peel_step_t), hipMemcpyDeviceToHost, s));
    float *const host_out[3] = {clean, residual, map};
    for (int k = 0; k < 3; k++)
        if (host_out[k]) AWPU_HIP_TRY(hipMemcpyAsync(host_out[k], d_maps + (size_t) k * plane, plane * sizeof(float), hipMemcpyDeviceToHost, s));
    if (residual_frames) AWPU_HIP_TRY(hipMemcpyAsync(residual_frames, h->d_peel_frames, floats * sizeof(float), hipMemcpyDeviceToHost, s));
    AWPU_HIP_TRY(hipStreamSynchronize(s));
    return AWPU_OK;
}

}  // extern "C"
