// awpu_csm_run.cpp -- the cross-spectral runs (include/awpu_hip_csm_watch.h): awpu_hip_csm_watch_blocks, _samples and
// _samples_device, and the CLEAN-SC runs awpu_hip_csm_clean_blocks, _samples and _samples_device (awpu_hip_csm_clean.h), the same
// run with one more way to turn a frame's matrix into planes.  Their pieces read spectra, not snapshots, so the loop is their own
// beside run_pieces.cpp's; its arithmetic is csm_run_plan.h's, every launch csm_calls.h's.
#include "watch_run.h"

#include "awpu_hip_csm.h"

#include "csm_calls.h"
#include "csm_clean_rule.h"
#include "csm_kernels.h"
#include "csm_run_plan.h"

using namespace awpu::host;

namespace {

static_assert(awpu::kCsmRunDatagramBytes == AWPU_DATAGRAM_BYTES && awpu::kSamples == awpu::kCsmSamples, "csm_run_plan.h's constants");
static_assert(sizeof(awpu_csm_clean_step_t) == awpu::kCsmRunStepFloats * sizeof(float), "a piece's steps lie in the float buffer");
static_assert(sizeof(int32_t) == sizeof(float), "the solved words lie in the float buffer");

const char *csm_watch_refusal(const awpu_csm_t *c, int32_t length, int32_t show, const float *carry, const int32_t *carried) {
    if (const char *why = awpu::csm_refusal(c)) return why;
    if (length < 1 || length > AWPU_CSM_MAX_LENGTH) return "length lies in [1, 1024]";
    if (show != AWPU_CSM_SHOW_SUM && (show < 0 || show >= c->n_bins)) return "show is a bin index of the request or AWPU_CSM_SHOW_SUM";
    if (!carried || (length > 1 && !carry)) return "null argument";
    if (*carried < 0 || *carried > length - 1) return "carried lies in [0, length - 1]";
    return nullptr;
}

struct CsmWatchOut {
    float *carry;
    int32_t *carried;
    float *planes;
    int32_t *solved;
};

// How a frame's matrix becomes its planes: the map; the loaded inverse, then the map (a run asks for kMap and gets kCapon by the
// request's kind); CLEAN-SC in place of the map -- the frame's planes are then the chosen rows of the loop on its matrix, the one
// awpu_hip_csm_clean_device runs (csm_calls.h), so its bits.
enum class Planes { kMap, kCapon, kClean };

struct CsmCleanRun {               // of a kClean run
    const awpu_csm_clean_t *cl;
    int32_t what;                  // AWPU_CSM_CLEAN_MAP, _CLEAN or _RESIDUAL
    awpu_csm_clean_step_t *steps;  // [n_frames][n_bins][cl->steps], host or device memory as the run's other outputs, or null
};

const char *csm_clean_run_refusal(const awpu_csm_t *c, const CsmCleanRun &cr) {
    if (const char *why = awpu::csm_clean_refusal(cr.cl)) return why;
    if (cr.what != AWPU_CSM_CLEAN_MAP && cr.what != AWPU_CSM_CLEAN_CLEAN && cr.what != AWPU_CSM_CLEAN_RESIDUAL)
        return "what is AWPU_CSM_CLEAN_MAP, AWPU_CSM_CLEAN_CLEAN or AWPU_CSM_CLEAN_RESIDUAL";
    return awpu::csm_clean_kind_refusal(c);
}

// A run walks the call's blocks in chunks of at most kRunChunk NEW blocks.  The spectra store holds length - 1 blocks in front of
// the chunk's -- at the start the carry, later the tail of the chunk before --, so every window that ends in the chunk is a run of
// consecutive slots.  A chunk: its samples onto the device (host forms; the wire's datagrams unpacked as every run unpacks them),
// step 1 for its blocks, then frame by frame on the one stream: the matrix zeroed, step 2 over the window (the kernel of
// awpu_hip_csm_samples_device, so its bits), the planes, the shown row; then the display step for the chunk's frames (at most
// max_batch: the chunk ends behind the last of them), and the store's tail moved to the front by way of the carry.  The host
// forms bring a chunk's results back before the next one; the device form never waits.  At the end the last four blocks go into
// the ring as a watch run's tail piece puts them there.
struct Run {
    awpu_hip *const h;
    const BlockRun &src;
    const awpu_watch_t &w;
    const awpu_csm_t &c;
    const Planes how;
    const CsmCleanRun cr;
    const CsmWatchOut o;
    float *const power;
    Display &display;
    const int n_blocks, n_frames, piece, keep, carried_in, show;
    const hipStream_t s;
    const awpu::CsmRunLayout L;
    const bool host = !src.device;
    const int S = h->cfg.n_streams, K = c.n_bins, chunk = awpu::csm_run_chunk_blocks(n_blocks);
    const size_t P = (size_t) h->cfg.pixel_count, per_block = csm_spectra_floats(h, c), frame_steps = how == Planes::kClean ? (size_t) K * cr.cl->steps : 0;
    float *const base = h->d_csm_run.get(), *const spec = base + L.spectra.off, *const d_carry = host ? base + L.carry.off : o.carry;

    // where frame k of the piece behind j shown frames puts an output asked for: the piece's scratch (host forms) or the caller's array
    template <class T>
    T *out_of(T *callers, const awpu::CsmRunRegion &r, int j, int k, size_t per_frame) const {
        if (!callers) return nullptr;
        return host ? reinterpret_cast<T *>(base + r.off) + (size_t) k * per_frame : callers + (size_t) (j + k) * per_frame;
    }

    // a -> b: what b's stream gets from here on comes behind what a's holds
    int order(hipStream_t a, hipStream_t b) const {
        AWPU_HIP_TRY(hipEventRecord(h->ev_blk_ring, a));
        AWPU_HIP_TRY(hipStreamWaitEvent(b, h->ev_blk_ring, 0));
        return AWPU_OK;
    }

    // blocks [c0, c0 + n_new) as samples on the device: where they start, and their pitch
    struct Samples {
        const float *d_x;
        long long pitch;
    };
    int chunk_samples(int c0, int n_new, Samples *x) const {
        float *d_stage = base + L.stage.off;
        if (src.wire) {
            unsigned char *d_wire = reinterpret_cast<unsigned char *>(base + L.wire.off);
            AWPU_HIP_TRY(hipMemcpy2DAsync(d_wire, AWPU_DATAGRAM_BYTES, src.wire + (size_t) c0 * awpu::kSamples * src.stride, (size_t) src.stride,
                                          AWPU_DATAGRAM_BYTES, (size_t) awpu::kSamples * n_new, hipMemcpyHostToDevice, s));
            AWPU_HIP_TRY(awpu::launch_unpack_blocks(d_wire, n_new, S, d_stage, awpu::kSamples * chunk, 0, s));
            *x = {d_stage, (long long) awpu::kSamples * chunk};
            return AWPU_OK;
        }
        *x = {src.samples + (size_t) awpu::kSamples * c0, src.pitch};
        if (!host) return AWPU_OK;
        const size_t row = (size_t) awpu::kSamples * n_new * sizeof(float);
        AWPU_HIP_TRY(hipMemcpy2DAsync(d_stage, row, x->d_x, (size_t) src.pitch * sizeof(float), row, (size_t) S, hipMemcpyHostToDevice, s));
        *x = {d_stage, (long long) awpu::kSamples * n_new};
        return AWPU_OK;
    }

    // the planes of frame k behind j out of its matrix d_C over n blocks; d_G is the inverse's place, or the loop's working matrix
    int planes_of(const float *d_C, float *d_G, int n, int j, int k, float *planes_k) const {
        int32_t *solved_k = out_of(o.solved, L.solved, j, k, (size_t) K);
        switch (how) {
        case Planes::kClean: {
            CsmCleanOut out;
            (cr.what == AWPU_CSM_CLEAN_CLEAN ? out.clean : cr.what == AWPU_CSM_CLEAN_RESIDUAL ? out.residual : out.map) = planes_k;
            out.steps = out_of(cr.steps, L.steps, j, k, frame_steps);
            return csm_clean_enqueue(h, d_C, d_G, n, c, *cr.cl, out, s);
        }
        case Planes::kCapon:
            if (const int rc = csm_enqueue_invert(h, d_C, n, c, d_G, solved_k, s)) return rc;
            return csm_enqueue_map(h, d_G, n, c, planes_k, nullptr, s);
        case Planes::kMap:
            if (solved_k) AWPU_HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(solved_k), 1, (size_t) K, s));
            return csm_enqueue_map(h, d_C, n, c, planes_k, nullptr, s);
        }
        return AWPU_ERR_INVALID;
    }

    // the chunk's nf frames behind j: each one's matrix over its window, its planes, its shown row
    int frames(int c0, int j, int nf, float *rows) const {
        float *d_C = base + L.matrix.off, *d_G = base + L.second.off;
        for (int k = 0; k < nf; k++) {
            const awpu::CsmRunWindow win = awpu::csm_run_window(w.first + (j + k) * w.every, keep, carried_in, c0);
            float *planes_k = o.planes ? out_of(o.planes, L.planes, j, k, K * P) : base + L.planes.off;
            AWPU_HIP_TRY(hipMemsetAsync(d_C, 0, csm_matrix_floats(h, c) * sizeof(float), s));
            awpu::CsmAccumulateArgs ac{};
            ac.spectra = spec + (size_t) win.slot * per_block, ac.matrix = d_C;
            ac.usable = h->usable(), ac.n_blocks = win.n, ac.n_bins = K;
            AWPU_HIP_TRY(awpu::launch_csm_accumulate(ac, s));
            if (const int rc = planes_of(d_C, d_G, win.n, j, k, planes_k)) return rc;
            AWPU_HIP_TRY(awpu::launch_csm_show(planes_k, K, (int) P, show, rows + (size_t) k * P, s));
        }
        return AWPU_OK;
    }

    // host forms: the piece's results to the caller, before the next chunk overwrites the scratch
    int bring_back(int j, int nf) const {
        const auto back = [&](auto *callers, const awpu::CsmRunRegion &r, size_t per_frame) {
            return !callers ? hipSuccess : hipMemcpyAsync(callers + (size_t) j * per_frame, base + r.off, (size_t) nf * per_frame * sizeof(*callers), hipMemcpyDeviceToHost, s);
        };
        AWPU_HIP_TRY(back(power, L.rows, P));
        AWPU_HIP_TRY(back(o.planes, L.planes, K * P));
        AWPU_HIP_TRY(back(o.solved, L.solved, (size_t) K));
        AWPU_HIP_TRY(back(cr.steps, L.steps, frame_steps));
        if (const int rc = display.fetch(0, nf, s)) return rc;
        AWPU_HIP_TRY(hipStreamSynchronize(s));
        return display.deliver(0, j, nf);
    }

    // the store's last length - 1 blocks to its front, by way of the carry (the two ranges may overlap)
    int shift_store(int n_new) const {
        const size_t bytes = (size_t) keep * per_block * sizeof(float);
        AWPU_HIP_TRY(hipMemcpyAsync(d_carry, spec + (size_t) n_new * per_block, bytes, hipMemcpyDeviceToDevice, s));
        AWPU_HIP_TRY(hipMemcpyAsync(spec, d_carry, bytes, hipMemcpyDeviceToDevice, s));
        return AWPU_OK;
    }

    int chunks() const {
        for (int c0 = 0, j = 0; c0 < n_blocks;) {
            const awpu::CsmRunChunk ch = awpu::csm_run_chunk(n_blocks, w.first, w.every, n_frames, piece, c0, j);
            const int n_new = ch.c1 - c0;
            Samples x;
            if (const int rc = chunk_samples(c0, n_new, &x)) return rc;
            // step 1 of the new blocks, behind the length - 1 before them
            if (const int rc = csm_enqueue_spectra(h, x.d_x, x.pitch, n_new, c, spec + (size_t) keep * per_block, s)) return rc;
            float *rows = host || !power ? base + L.rows.off : power + (size_t) j * P;
            if (const int rc = frames(c0, j, ch.nf, rows)) return rc;
            if (const int rc = display.show(0, j, ch.nf, rows, s)) return rc;
            if (host && ch.nf > 0)
                if (const int rc = bring_back(j, ch.nf)) return rc;
            if (keep > 0)
                if (const int rc = shift_store(n_new)) return rc;
            j += ch.nf, c0 = ch.c1;
        }
        return AWPU_OK;
    }

    int body() const {
        if (s != h->stream)  // behind what is queued on the handle's stream: the ring's zeroing, a device-form run not over
            if (const int rc = order(h->stream, s)) return rc;
        if (keep > 0)
            AWPU_HIP_TRY(hipMemcpyAsync(spec, o.carry, (size_t) keep * per_block * sizeof(float), host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
        if (const int rc = chunks()) return rc;
        if (const int rc = ring_tail(h, src, n_blocks, s)) return rc;
        if (!host) return s != h->stream ? order(s, h->stream) : (int) AWPU_OK;  // later calls on the ring (the handle's stream) come after this one
        std::vector<float> back((size_t) keep * per_block);
        if (keep > 0) AWPU_HIP_TRY(hipMemcpyAsync(back.data(), d_carry, back.size() * sizeof(float), hipMemcpyDeviceToHost, s));
        if (const int rc = wait_and_time(h, false)) return rc;
        std::copy(back.begin(), back.end(), o.carry);
        return AWPU_OK;
    }
};

// open and refuse, make ready, lay out the scratch, run; `how` is kMap (the request's kind decides between it and kCapon) or kClean
int csm_watch_run(awpu_hip *h, const BlockRun &src, int n_blocks, const awpu_watch_t *w, const awpu_csm_t *c, int32_t length, int32_t show,
                  const awpu_find_t *f, uint8_t *image, uint8_t *big, float *power, awpu_source_t *sources, int32_t *count, const CsmWatchOut &o,
                  hipStream_t user, Planes how, const CsmCleanRun &cr) {
    const bool clean = how == Planes::kClean;
    ShownRun sr;
    const auto refusal = [&] {
        const char *why = csm_watch_refusal(c, length, show, o.carry, o.carried);
        return why || !clean ? why : csm_clean_run_refusal(c, cr);
    };
    if (const int rc = sr.open(w, n_blocks, refusal, f, image, big, power, sources, count, o.planes || o.solved || cr.steps)) return rc;
    AWPU_CTX(h);
    if (int rc = clean ? csm_clean_check(h, c) : csm_check(h, c)) return rc;
    if (h->cfg.hist != AWPU_HIST) return invalid("runs of blocks need hist 1024");
    if (src.wire && h->cfg.n_streams > 256) return invalid("the wire carries at most 256 streams");
    if (!clean && c->kind == AWPU_CSM_CAPON) how = Planes::kCapon;
    const bool host = !src.device;
    Display display(h, sr.wr, host);
    if (int rc = display.check()) return rc;
    int rc = check_ready(h, 1);
    if (rc == AWPU_OK) rc = csm_ready_map(h, c);
    if (rc == AWPU_OK && how == Planes::kCapon) rc = csm_ready_invert(h, c);
    if (rc == AWPU_OK && clean) rc = csm_clean_ready(h, *c, false);  // (the working matrix is the run's: the inverse's place)
    if (rc != AWPU_OK) return rc;

    const int piece = awpu::csm_run_piece(sr.wr.n_frames, h->cfg.max_batch), keep = length - 1;
    const awpu::CsmRunLayout L = awpu::csm_run_layout({host, src.wire != nullptr, h->cfg.n_streams, h->usable(), c->n_bins, h->cfg.pixel_count, keep,
                                                       awpu::csm_run_chunk_blocks(n_blocks), piece, o.planes != nullptr, o.solved != nullptr,
                                                       cr.steps != nullptr, power != nullptr, clean ? cr.cl->steps : 0});
    rc = h->d_csm_run.ensure(L.total);
    hipStream_t s = host ? (hipStream_t) h->stream : (user ? user : (hipStream_t) h->stream);
    if (rc == AWPU_OK) rc = enter_stream(h, s);
    if (rc == AWPU_OK) rc = ensure_ring(h);
    if (rc == AWPU_OK) rc = ensure_run_buffers(h, src, 1, AWPU_HIST, false, 1, 4, 1);  // (the ring's tail: a history of four blocks)
    if (rc == AWPU_OK) rc = display.ensure(piece, s);
    if (rc != AWPU_OK) return rc;
    const Run run{h, src, *w, *c, how, cr, o, power, display, n_blocks, sr.wr.n_frames, piece, keep, *o.carried, show, s, L};
    rc = run.body();
    if (rc != AWPU_OK) {
        if (host) (void) hipStreamSynchronize(s);  // nothing of the call may still read the caller's buffers
        return rc;
    }
    *o.carried = awpu::csm_run_carried(run.carried_in, n_blocks, keep);
    return AWPU_OK;
}

}  // namespace

extern "C" {

int awpu_hip_csm_watch_blocks(awpu_hip_t *h, const void *datagrams, int32_t stride_bytes, int32_t n_blocks, const awpu_watch_t *w,
                              const awpu_csm_t *c, int32_t length, int32_t show, const awpu_find_t *f, float *carry, int32_t *carried,
                              uint8_t *image, uint8_t *big_image, float *power, awpu_source_t *sources, int32_t *count, float *planes,
                              int32_t *solved) {
    BlockRun src;
    if (int rc = wire_source(h, datagrams, stride_bytes, n_blocks, &src)) return rc;
    return csm_watch_run(h, src, n_blocks, w, c, length, show, f, image, big_image, power, sources, count, {carry, carried, planes, solved}, nullptr, Planes::kMap, {});
}

int awpu_hip_csm_watch_samples(awpu_hip_t *h, const float *samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                               const awpu_csm_t *c, int32_t length, int32_t show, const awpu_find_t *f, float *carry, int32_t *carried,
                               uint8_t *image, uint8_t *big_image, float *power, awpu_source_t *sources, int32_t *count, float *planes,
                               int32_t *solved) {
    BlockRun src;
    if (int rc = sample_source(h, samples, pitch, n_blocks, false, &src)) return rc;
    return csm_watch_run(h, src, n_blocks, w, c, length, show, f, image, big_image, power, sources, count, {carry, carried, planes, solved}, nullptr, Planes::kMap, {});
}

int awpu_hip_csm_watch_samples_device(awpu_hip_t *h, const float *d_samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                                      const awpu_csm_t *c, int32_t length, int32_t show, const awpu_find_t *f, float *d_carry,
                                      int32_t *carried, uint8_t *d_image, uint8_t *d_big_image, float *d_power, awpu_source_t *d_sources,
                                      int32_t *d_count, float *d_planes, int32_t *d_solved, void *stream) {
    BlockRun src;
    if (int rc = sample_source(h, d_samples, pitch, n_blocks, true, &src)) return rc;
    return csm_watch_run(h, src, n_blocks, w, c, length, show, f, d_image, d_big_image, d_power, d_sources, d_count,
                         {d_carry, carried, d_planes, d_solved}, static_cast<hipStream_t>(stream), Planes::kMap, {});
}

// CLEAN-SC runs (awpu_hip_csm_clean.h): the watch run with the loop in place of the map

int awpu_hip_csm_clean_blocks(awpu_hip_t *h, const void *datagrams, int32_t stride_bytes, int32_t n_blocks, const awpu_watch_t *w,
                              const awpu_csm_t *c, int32_t length, int32_t show, const awpu_find_t *f, float *carry, int32_t *carried,
                              const awpu_csm_clean_t *cl, int32_t what, uint8_t *image, uint8_t *big_image, float *power, awpu_source_t *sources,
                              int32_t *count, float *planes, awpu_csm_clean_step_t *steps) {
    BlockRun src;
    if (int rc = wire_source(h, datagrams, stride_bytes, n_blocks, &src)) return rc;
    return csm_watch_run(h, src, n_blocks, w, c, length, show, f, image, big_image, power, sources, count, {carry, carried, planes, nullptr}, nullptr,
                         Planes::kClean, {cl, what, steps});
}

int awpu_hip_csm_clean_samples(awpu_hip_t *h, const float *samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                               const awpu_csm_t *c, int32_t length, int32_t show, const awpu_find_t *f, float *carry, int32_t *carried,
                               const awpu_csm_clean_t *cl, int32_t what, uint8_t *image, uint8_t *big_image, float *power, awpu_source_t *sources,
                               int32_t *count, float *planes, awpu_csm_clean_step_t *steps) {
    BlockRun src;
    if (int rc = sample_source(h, samples, pitch, n_blocks, false, &src)) return rc;
    return csm_watch_run(h, src, n_blocks, w, c, length, show, f, image, big_image, power, sources, count, {carry, carried, planes, nullptr}, nullptr,
                         Planes::kClean, {cl, what, steps});
}

int awpu_hip_csm_clean_samples_device(awpu_hip_t *h, const float *d_samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                                      const awpu_csm_t *c, int32_t length, int32_t show, const awpu_find_t *f, float *d_carry,
                                      int32_t *carried, const awpu_csm_clean_t *cl, int32_t what, uint8_t *d_image, uint8_t *d_big_image,
                                      float *d_power, awpu_source_t *d_sources, int32_t *d_count, float *d_planes,
                                      awpu_csm_clean_step_t *d_steps, void *stream) {
    BlockRun src;
    if (int rc = sample_source(h, d_samples, pitch, n_blocks, true, &src)) return rc;
    return csm_watch_run(h, src, n_blocks, w, c, length, show, f, d_image, d_big_image, d_power, d_sources, d_count,
                         {d_carry, carried, d_planes, nullptr}, static_cast<hipStream_t>(stream), Planes::kClean, {cl, what, d_steps});
}

}  // extern "C"
