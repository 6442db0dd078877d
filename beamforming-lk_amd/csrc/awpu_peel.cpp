// awpu_peel.cpp -- the handle forms of peeling (include/awpu_hip_peel.h): awpu_hip_peel_step_device, awpu_hip_peel and
// awpu_hip_peel_device.  The rule is peel_rule.h's, the kernels peel_kernels.hip's; the loop's sweeps are the handle's own
// launch() (awpu_sweep.cpp), the step's table the coherence sweep's (ensure_cohere_table).  Nothing in the loop waits for the
// device: picks, stop tests and records stay there (PeelState).  And the peel runs of blocks, watch runs (watch_run.h) whose
// pieces go through the same loop.
#include "watch_run.h"

#include "awpu_hip_peel.h"
#include "peel_kernels.h"
#include "peel_rule.h"

using namespace awpu::host;

namespace {

struct PeelOut {  // what a loop writes, device memory, each or null: steps [batch][pe.steps]; clean, residual, map [batch][pixel_count]
    awpu_peel_step_t *steps = nullptr;
    float *clean = nullptr, *residual = nullptr, *map = nullptr;
};

// the refusals of a handle that come before it is made ready (awpu_hip_peel.h)
int peel_handle_refusal(awpu_hip *h) {
    if (is_group(h)) return fail(AWPU_ERR_STATE, "a device group takes no peel");
    if (h->in_flight) return fail(AWPU_ERR_STATE, "an awpu_hip_process_async call is in flight on this handle: awpu_hip_wait first");
    if (h->cfg.interp != AWPU_INTERP_LERP) return fail(AWPU_ERR_STATE, "the peel interpolates linearly: AWPU_INTERP_FIR8 is not taken");
    if (h->cfg.pixel_count < h->cfg.n_pixels) return fail(AWPU_ERR_STATE, "a slab handle takes no peel: the pick needs the whole map");
    if (!h->band.empty()) return fail(AWPU_ERR_STATE, "a handle with a band takes no peel: the step reads outside the window the band's pre-pass writes");
    return AWPU_OK;
}

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

// ---- peel runs (awpu_hip_peel.h) ----------------------------------------------------------------------------------------------------
// A watch run whose pieces are peeled (peel_enqueue) in place of swept: a piece's snapshots are cut whole -- the step reads E + 1
// samples either side of the window -- into d_blk_frames, which the loop then turns into the residual, and the row a frame shows
// -- and everything behind it -- is its map, clean or residual row.  The steps go to the caller's array (device form) or come back
// with the piece's images through peel_steps (host forms).  Pieces, histories, the ring: the watch run's.
struct PeelPieces final : WatchPieces {
    const awpu_peel_t pe;
    const int show_row;
    awpu_peel_step_t *const steps;  // [n_frames][pe.steps], host or device memory as the run's other outputs, or null
    PeelPieces(awpu_hip *h_, const BlockRun &src_, int n_blocks_, const WatchRun &wr_, const awpu_peel_t &pe_, int show_, awpu_peel_step_t *steps_)
        : WatchPieces(h_, src_, n_blocks_, wr_), pe(pe_), show_row(show_), steps(steps_) {
        whole_frames = true;
    }
    size_t step_bytes(int n) const { return (size_t) n * pe.steps * sizeof(awpu_peel_step_t); }
    int check() override {
        const int rc = peel_handle_refusal(h);
        return rc != AWPU_OK ? rc : WatchPieces::check();
    }
    int ensure(int piece_max, int lo_, int width_, hipStream_t sw) override {  // (the handle is ready; none of the run's work is enqueued yet)
        int rc = peel_prepare(h, piece_max);
        if (rc == AWPU_OK && host && steps) rc = h->peel_steps.ensure(step_bytes(piece_max), true);
        return rc != AWPU_OK ? rc : WatchPieces::ensure(piece_max, lo_, width_, sw);
    }
    int sweep_frames(awpu_hip *, const Piece &p, const float *d_frames, float *d_pow, hipStream_t s, int layout) override {
        if (layout != kFull) return fail(AWPU_ERR_STATE, "a peel run cuts its snapshots whole");
        PeelOut out;
        (show_row == AWPU_PEEL_CLEAN ? out.clean : show_row == AWPU_PEEL_RESIDUAL ? out.residual : out.map) = d_pow;
        if (steps) out.steps = host ? reinterpret_cast<awpu_peel_step_t *>(h->peel_steps.d[p.b].get()) : steps + (size_t) p.first * pe.steps;
        return peel_enqueue(h, const_cast<float *>(d_frames), p.n, pe, out, s);  // (d_blk_frames: the run's own scratch, cut anew for every piece)
    }
    int fetch_shown(const Piece &p, hipStream_t s) override {
        if (steps) AWPU_HIP_TRY(hipMemcpyAsync(h->peel_steps.h[p.b], h->peel_steps.d[p.b], step_bytes(p.n), hipMemcpyDeviceToHost, s));
        return WatchPieces::fetch_shown(p, s);
    }
    int deliver_shown(const Piece &p) override {
        if (steps) std::memcpy(steps + (size_t) p.first * pe.steps, h->peel_steps.h[p.b], step_bytes(p.n));
        return WatchPieces::deliver_shown(p);
    }
};

// the checks of a peel run that read no handle; then the run
int peel_run(awpu_hip *h, const BlockRun &src, int n_blocks, const awpu_watch_t *w, const awpu_peel_t *pe, int32_t show, const awpu_find_t *f,
             uint8_t *image, uint8_t *big, float *power, awpu_peel_step_t *steps, awpu_source_t *sources, int32_t *count, hipStream_t user) {
    ShownRun sr;
    const bool shows = show == AWPU_PEEL_MAP || show == AWPU_PEEL_CLEAN || show == AWPU_PEEL_RESIDUAL;
    const auto refusal = [&] { const char *why = awpu::peel_refusal(pe); return why || shows ? why : "show is AWPU_PEEL_MAP, AWPU_PEEL_CLEAN or AWPU_PEEL_RESIDUAL"; };
    if (const int rc = sr.open(w, n_blocks, refusal, f, image, big, power, sources, count, steps != nullptr)) return rc;
    AWPU_CTX(h);
    PeelPieces c(h, src, n_blocks, sr.wr, *pe, show, steps);
    return run_pieces(h, src, user, c);
}

}  // namespace

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

int awpu_hip_peel_blocks(awpu_hip_t *h, const void *datagrams, int32_t stride_bytes, int32_t n_blocks, const awpu_watch_t *w,
                         const awpu_peel_t *pe, int32_t show, const awpu_find_t *f, uint8_t *image, uint8_t *big_image, float *power,
                         awpu_peel_step_t *steps, awpu_source_t *sources, int32_t *count) {
    BlockRun src;
    if (int rc = wire_source(h, datagrams, stride_bytes, n_blocks, &src)) return rc;
    return peel_run(h, src, n_blocks, w, pe, show, f, image, big_image, power, steps, sources, count, nullptr);
}

int awpu_hip_peel_samples(awpu_hip_t *h, const float *samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                          const awpu_peel_t *pe, int32_t show, const awpu_find_t *f, uint8_t *image, uint8_t *big_image, float *power,
                          awpu_peel_step_t *steps, awpu_source_t *sources, int32_t *count) {
    BlockRun src;
    if (int rc = sample_source(h, samples, pitch, n_blocks, false, &src)) return rc;
    return peel_run(h, src, n_blocks, w, pe, show, f, image, big_image, power, steps, sources, count, nullptr);
}

int awpu_hip_peel_samples_device(awpu_hip_t *h, const float *d_samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                                 const awpu_peel_t *pe, int32_t show, const awpu_find_t *f, uint8_t *d_image, uint8_t *d_big_image,
                                 float *d_power, awpu_peel_step_t *d_steps, awpu_source_t *d_sources, int32_t *d_count, void *stream) {
    BlockRun src;
    if (int rc = sample_source(h, d_samples, pitch, n_blocks, true, &src)) return rc;
    return peel_run(h, src, n_blocks, w, pe, show, f, d_image, d_big_image, d_power, d_steps, d_sources, d_count, static_cast<hipStream_t>(stream));
}

}  // extern "C"
