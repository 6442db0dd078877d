// awpu_csm.cpp -- the handle forms of the cross-spectral maps (include/awpu_hip_csm.h): awpu_hip_csm_samples, _samples_device,
// _map and _map_device, step 6a's awpu_hip_csm_invert and _invert_device, and the runs awpu_hip_csm_watch_blocks, _samples and
// _samples_device (a loop of their own beside run_pieces.cpp's: their pieces read spectra, not snapshots) with the CLEAN-SC runs
// awpu_hip_csm_clean_blocks, _samples and _samples_device, the same loop with one more way to turn a frame's matrix into planes.
// The rule is csm_rule.h's and csm_invert_rule.h's, the kernels and their launchers csm_kernels.hip's and csm_invert_kernels.hip's;
// CLEAN-SC's loop is awpu_csm_clean.cpp's (csm_calls.h).  The calls read the handle's active list, gains and delay table (the coherence sweep's LutEntry table: ensure_cohere_table) and the tone sweep's two tables
// (ensure_tones_tables); they count no sweep launch and leave stats.kernel_variant alone.
#include "watch_run.h"

#include "awpu_hip_csm.h"

#include <cstring>

#include "csm_calls.h"
#include "csm_clean_rule.h"
#include "csm_invert_kernels.h"
#include "csm_kernels.h"
#include "csm_rule.h"

using namespace awpu::host;

namespace {

constexpr int kBlocksPerLaunch = 1024;  // a recording is accumulated in pieces of so many blocks: what the spectra scratch holds

// the refusals that come before the handle is made ready
int check_csm(awpu_hip *h, const awpu_csm_t *c) {
    if (!h) return invalid("null handle");
    if (const char *why = awpu::csm_refusal(c)) return invalid(why);
    if (is_group(h)) return fail(AWPU_ERR_STATE, "a device group takes no cross-spectral call");
    if (h->in_flight) return fail(AWPU_ERR_STATE, "an awpu_hip_process_async call is in flight on this handle: awpu_hip_wait first");
    if (h->cfg.interp != AWPU_INTERP_LERP) return fail(AWPU_ERR_STATE, "the cross-spectral maps steer by the linear table: AWPU_INTERP_FIR8 is not taken");
    if (!h->band.empty()) return fail(AWPU_ERR_STATE, "a band is set on the handle: the cross-spectral maps choose their bins themselves");
    return AWPU_OK;
}

int check_samples(awpu_hip *h, const float *samples, int64_t pitch, int32_t n_blocks, const awpu_csm_t *c, const float *matrix,
                  const int32_t *block_count) {
    if (int rc = check_csm(h, c)) return rc;
    if (!samples || !matrix || !block_count) return invalid("null argument");
    if (n_blocks < 1 || pitch < (int64_t) awpu::kCsmSamples * n_blocks) return invalid("n_blocks >= 1 and pitch >= 256 * n_blocks");
    if (*block_count < 0 || *block_count > INT32_MAX - n_blocks) return invalid("the block count lies in [0, 2^31 - 1 - n_blocks]");
    return AWPU_OK;
}

int check_map(awpu_hip *h, const float *matrix, int32_t block_count, const awpu_csm_t *c, const float *map, const float *q) {
    if (int rc = check_csm(h, c)) return rc;
    if (!matrix) return invalid("null argument");
    if (!map && !q) return invalid("no output asked for");
    if (block_count < 1) return invalid("the block count is at least 1");
    return AWPU_OK;
}

// behind check_ready: the map's refusals that read the active list, then the steps that may block, before anything is enqueued
int ready_map(awpu_hip *h, const awpu_csm_t *c) {
    if (c->kind == AWPU_CSM_DIAGONAL_REMOVED && h->usable() == 1) return invalid("diagonal removal needs two active mics");
    if (awpu::csm_map_pixels_per_wave(h->usable()) == 0) return fail(AWPU_ERR_RANGE, "more than 2048 active mics: their steering vectors do not fit the LDS");
    const int rc = ensure_cohere_table(h);
    return rc != AWPU_OK ? rc : ensure_tones_tables(h);
}

// steps 1 and 2 on device buffers, enqueued on s; the scratch is there (or the caller keeps the spectra)
int enqueue_samples(awpu_hip *h, const float *d_samples, int64_t pitch, int n_blocks, const awpu_csm_t &c, float *d_matrix, float *d_spectra,
                    hipStream_t s) {
    const int U = h->usable();
    const size_t per_block = (size_t) c.n_bins * U * 2;
    for (int first = 0; first < n_blocks; first += kBlocksPerLaunch) {
        const int n = std::min(kBlocksPerLaunch, n_blocks - first);
        float *spectra = d_spectra ? d_spectra + (size_t) first * per_block : h->d_csm_spectra.get();
        awpu::CsmSpectraArgs sp{};
        sp.samples = d_samples + (size_t) first * awpu::kCsmSamples;
        sp.pitch = pitch;
        sp.index = h->d_index;
        sp.gain = h->d_gain;
        sp.window = h->d_tones_tables.get() + (c.window == AWPU_TONES_HANN ? awpu::kCsmSamples : 0);
        sp.twiddles = h->d_tones_tables.get() + 2 * awpu::kCsmSamples;
        sp.spectra = spectra;
        sp.usable = U, sp.n_blocks = n, sp.n_bins = c.n_bins;
        for (int i = 0; i < c.n_bins; i++) sp.bin[i] = c.bin[i];
        AWPU_HIP_TRY(awpu::launch_csm_spectra(sp, s));
        awpu::CsmAccumulateArgs ac{};
        ac.spectra = spectra, ac.matrix = d_matrix;
        ac.usable = U, ac.n_blocks = n, ac.n_bins = c.n_bins;
        AWPU_HIP_TRY(awpu::launch_csm_accumulate(ac, s));
    }
    return AWPU_OK;
}

int ready_samples(awpu_hip *h, int n_blocks, const awpu_csm_t &c, bool own_spectra) {
    if (const int rc = ensure_tones_tables(h); rc != AWPU_OK) return rc;
    if (own_spectra) return AWPU_OK;
    return h->d_csm_spectra.ensure((size_t) std::min(n_blocks, kBlocksPerLaunch) * c.n_bins * h->usable() * 2);
}

// steps 3 to 5 on device buffers, enqueued on s
int enqueue_map(awpu_hip *h, const float *d_matrix, int block_count, const awpu_csm_t &c, float *d_map, float *d_q, hipStream_t s) {
    const awpu::LutEntry *lut = h->d_lut ? h->d_lut.get() : h->d_cohere_lut.get();
    if (!lut || !h->d_tones_tables) return fail(AWPU_ERR_STATE, "the cross-spectral map has no tables: ensure_cohere_table and ensure_tones_tables come first");
    awpu::CsmMapArgs a{};
    a.matrix = d_matrix;
    a.lut = lut;
    a.twiddles = h->d_tones_tables.get() + 2 * awpu::kCsmSamples;
    a.map = d_map, a.q = d_q;
    a.usable = h->usable(), a.pixel_count = h->cfg.pixel_count, a.wstart = h->wstart, a.n_bins = c.n_bins, a.kind = c.kind;
    a.scale = c.kind == AWPU_CSM_CAPON ? awpu::csm_wss(c.window) * 256.0f : awpu::csm_scale(c, h->usable(), block_count);
    for (int i = 0; i < c.n_bins; i++) a.bin[i] = c.bin[i];
    AWPU_HIP_TRY(awpu::launch_csm_map(a, s));
    return AWPU_OK;
}

int check_invert(awpu_hip *h, const float *matrix, int32_t block_count, const awpu_csm_t *c, const float *inverse) {
    if (int rc = check_csm(h, c)) return rc;
    if (!matrix || !inverse) return invalid("null argument");
    if (block_count < 1) return invalid("the block count is at least 1");
    return AWPU_OK;
}

// behind check_ready: the inverse's refusal that reads the active list, then its scratch, before anything is enqueued
int ready_invert(awpu_hip *h, const awpu_csm_t *c) {
    if (h->usable() > awpu::kCsmInvertMaxUsable) return fail(AWPU_ERR_RANGE, "more than 512 active mics: the loaded inverse takes no more");
    return h->d_csm_invert.ensure(awpu::csm_invert_scratch_doubles(h->usable(), c->n_bins));
}

// step 6a on device buffers, enqueued on s
int enqueue_invert(awpu_hip *h, const float *d_matrix, int block_count, const awpu_csm_t &c, float *d_inverse, int32_t *d_solved, hipStream_t s) {
    awpu::CsmInvertArgs a{};
    a.matrix = d_matrix, a.inverse = d_inverse, a.solved = d_solved;
    a.scratch = h->d_csm_invert.get();
    a.usable = h->usable(), a.n_bins = c.n_bins, a.block_count = block_count, a.loading = c.loading;
    AWPU_HIP_TRY(awpu::launch_csm_invert(a, s));
    return AWPU_OK;
}

// ---- runs (awpu_hip_csm_watch.h) ------------------------------------------------------------------------------------------------
// A run walks the call's blocks in chunks of at most kRunChunk NEW blocks.  The spectra store holds length - 1 blocks in front of
// the chunk's -- at the start the carry, later the tail of the chunk before --, so every window that ends in the chunk is a run of
// consecutive slots.  A chunk: its samples onto the device (host forms; the wire's datagrams unpacked as every run unpacks them),
// step 1 for its blocks, then frame by frame on the one stream: the matrix zeroed, step 2 over the window (the kernel of
// awpu_hip_csm_samples_device, so its bits), step 6a for Capon, steps 3 to 5, the shown row; then the display step for the
// chunk's frames (at most max_batch: the chunk ends behind the last of them), and the store's tail moved to the front by way of
// the carry.  The host forms bring a chunk's results back before the next one; the device form never waits.  At the end the last
// four blocks go into the ring as a watch run's tail piece puts them there.
constexpr int kRunChunk = 256;

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

// One more way to turn a frame's matrix into planes: CLEAN-SC in place of the map (the runs of awpu_hip_csm_clean.h).  The frame's
// planes are then the chosen rows of the loop on its matrix -- the one awpu_hip_csm_clean_device runs (csm_calls.h), so its bits.
struct CsmCleanRun {
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

int csm_watch_run(awpu_hip *h, const BlockRun &src, int n_blocks, const awpu_watch_t *w, const awpu_csm_t *c, int32_t length, int32_t show,
                  const awpu_find_t *f, uint8_t *image, uint8_t *big, float *power, awpu_source_t *sources, int32_t *count, const CsmWatchOut &o,
                  hipStream_t user, const CsmCleanRun *cr = nullptr) {
    ShownRun sr;
    const auto refusal = [&] {
        const char *why = csm_watch_refusal(c, length, show, o.carry, o.carried);
        return why || !cr ? why : csm_clean_run_refusal(c, *cr);
    };
    if (const int rc = sr.open(w, n_blocks, refusal, f, image, big, power, sources, count, o.planes || o.solved || (cr && cr->steps))) return rc;
    AWPU_CTX(h);
    if (int rc = cr ? csm_clean_check(h, c) : check_csm(h, c)) return rc;
    if (h->cfg.hist != AWPU_HIST) return invalid("runs of blocks need hist 1024");
    if (src.wire && h->cfg.n_streams > 256) return invalid("the wire carries at most 256 streams");
    const bool host = !src.device, capon = c->kind == AWPU_CSM_CAPON;
    Display display(h, sr.wr, host);
    if (int rc = display.check()) return rc;
    int rc = check_ready(h, 1);
    if (rc == AWPU_OK) rc = ready_map(h, c);
    if (rc == AWPU_OK && capon) rc = ready_invert(h, c);
    if (rc == AWPU_OK && cr) rc = csm_clean_ready(h, *c, false);  // (the working matrix is the run's: the inverse's place)
    if (rc != AWPU_OK) return rc;

    const int S = h->cfg.n_streams, U = h->usable(), K = c->n_bins, n_frames = sr.wr.n_frames;
    const size_t P = (size_t) h->cfg.pixel_count, per_block = (size_t) K * U * 2, matrix_floats = (size_t) K * U * U * 2;
    const int chunk = std::min(kRunChunk, n_blocks), piece = std::max(1, std::min(n_frames, h->cfg.max_batch));
    const int keep = length - 1, carried_in = *o.carried;
    // the run's scratch, carved out of one buffer (every part a multiple of 4 floats long)
    const auto part = [](size_t floats) { return (floats + 3) / 4 * 4; };
    const size_t spec_floats = part((size_t) (keep + chunk) * per_block), carry_floats = host ? part((size_t) keep * per_block) : 0;
    const size_t rows_floats = host || !power ? part((size_t) piece * P) : 0;
    const size_t planes_floats = host ? (o.planes ? part((size_t) piece * K * P) : part((size_t) K * P)) : (o.planes ? 0 : part((size_t) K * P));
    const size_t solved_floats = host && o.solved ? part((size_t) piece * K) : 0;
    static_assert(sizeof(awpu_csm_clean_step_t) == 3 * sizeof(float), "a piece's steps lie in the float buffer");
    const size_t frame_steps = cr ? (size_t) K * cr->cl->steps : 0;  // records of a frame
    const size_t steps_floats = host && cr && cr->steps ? part((size_t) piece * frame_steps * 3) : 0;
    const size_t stage_floats = host ? part((size_t) S * awpu::kSamples * chunk) : 0;
    const size_t wire_floats = src.wire ? part((size_t) awpu::kSamples * chunk * AWPU_DATAGRAM_BYTES / sizeof(float) + 1) : 0;
    rc = h->d_csm_run.ensure(spec_floats + carry_floats + 2 * part(matrix_floats) + rows_floats + planes_floats + solved_floats + steps_floats + stage_floats + wire_floats);
    hipStream_t s = host ? (hipStream_t) h->stream : (user ? user : (hipStream_t) h->stream);
    if (rc == AWPU_OK) rc = enter_stream(h, s);
    if (rc == AWPU_OK) rc = ensure_ring(h);
    if (rc == AWPU_OK) rc = ensure_run_buffers(h, src, 1, AWPU_HIST, false, 1, 4, 1);  // (the ring's tail: a history of four blocks)
    if (rc == AWPU_OK) rc = display.ensure(piece, s);
    if (rc != AWPU_OK) return rc;
    float *spec = h->d_csm_run.get(), *d_carry = host ? spec + spec_floats : o.carry;
    float *d_C = spec + spec_floats + carry_floats, *d_G = d_C + part(matrix_floats), *d_rows = d_G + part(matrix_floats);
    float *d_planes = d_rows + rows_floats;
    int32_t *d_solved = reinterpret_cast<int32_t *>(d_planes + planes_floats);
    awpu_csm_clean_step_t *d_steps = reinterpret_cast<awpu_csm_clean_step_t *>(d_planes + planes_floats + solved_floats);
    float *d_stage = d_planes + planes_floats + solved_floats + steps_floats;
    unsigned char *d_wire = reinterpret_cast<unsigned char *>(d_stage + stage_floats);

    const auto body = [&]() -> int {
        if (s != h->stream) {  // behind what is queued on the handle's stream: the ring's zeroing, a device-form run not over
            AWPU_HIP_TRY(hipEventRecord(h->ev_blk_ring, h->stream));
            AWPU_HIP_TRY(hipStreamWaitEvent(s, h->ev_blk_ring, 0));
        }
        if (keep > 0)
            AWPU_HIP_TRY(hipMemcpyAsync(spec, o.carry, (size_t) keep * per_block * sizeof(float), host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
        int j = 0;
        for (int c0 = 0; c0 < n_blocks;) {
            int c1 = std::min(c0 + chunk, n_blocks), nf = 0;
            const auto shown = [&](int k) { return w->first + (j + k) * w->every; };
            while (j + nf < n_frames && nf < piece && shown(nf) < c1) nf++;
            if (j + nf < n_frames && shown(nf) < c1) c1 = shown(nf - 1) + 1;  // the piece is full: the chunk ends behind its last frame
            const int n_new = c1 - c0;
            // the chunk's samples
            const float *d_x = src.samples + (size_t) awpu::kSamples * c0;
            long long x_pitch = src.pitch;
            if (src.wire) {
                AWPU_HIP_TRY(hipMemcpy2DAsync(d_wire, AWPU_DATAGRAM_BYTES, src.wire + (size_t) c0 * awpu::kSamples * src.stride, (size_t) src.stride,
                                              AWPU_DATAGRAM_BYTES, (size_t) awpu::kSamples * n_new, hipMemcpyHostToDevice, s));
                AWPU_HIP_TRY(awpu::launch_unpack_blocks(d_wire, n_new, S, d_stage, awpu::kSamples * chunk, 0, s));
                d_x = d_stage, x_pitch = (long long) awpu::kSamples * chunk;
            } else if (host) {
                const size_t row = (size_t) awpu::kSamples * n_new * sizeof(float);
                AWPU_HIP_TRY(hipMemcpy2DAsync(d_stage, row, d_x, (size_t) src.pitch * sizeof(float), row, (size_t) S, hipMemcpyHostToDevice, s));
                d_x = d_stage, x_pitch = (long long) awpu::kSamples * n_new;
            }
            // step 1 of the new blocks, behind the length - 1 before them
            awpu::CsmSpectraArgs sp{};
            sp.samples = d_x, sp.pitch = x_pitch;
            sp.index = h->d_index, sp.gain = h->d_gain;
            sp.window = h->d_tones_tables.get() + (c->window == AWPU_TONES_HANN ? awpu::kCsmSamples : 0);
            sp.twiddles = h->d_tones_tables.get() + 2 * awpu::kCsmSamples;
            sp.spectra = spec + (size_t) keep * per_block;
            sp.usable = U, sp.n_blocks = n_new, sp.n_bins = K;
            for (int i = 0; i < K; i++) sp.bin[i] = c->bin[i];
            AWPU_HIP_TRY(awpu::launch_csm_spectra(sp, s));
            // the chunk's frames
            float *rows = host || !power ? d_rows : power + (size_t) j * P;
            for (int k = 0; k < nf; k++) {
                const int t = shown(k), lo = std::max(t - keep, -carried_in), n = t - lo + 1;
                float *planes_k = host ? (o.planes ? d_planes + (size_t) k * K * P : d_planes) : (o.planes ? o.planes + (size_t) (j + k) * K * P : d_planes);
                int32_t *solved_k = !o.solved ? nullptr : (host ? d_solved + (size_t) k * K : o.solved + (size_t) (j + k) * K);
                AWPU_HIP_TRY(hipMemsetAsync(d_C, 0, matrix_floats * sizeof(float), s));
                awpu::CsmAccumulateArgs ac{};
                ac.spectra = spec + (size_t) (keep + lo - c0) * per_block, ac.matrix = d_C;
                ac.usable = U, ac.n_blocks = n, ac.n_bins = K;
                AWPU_HIP_TRY(awpu::launch_csm_accumulate(ac, s));
                if (cr) {  // the loop on the frame's matrix, its working D where the inverse would lie; the chosen rows are the frame's planes
                    CsmCleanOut out;
                    (cr->what == AWPU_CSM_CLEAN_CLEAN ? out.clean : cr->what == AWPU_CSM_CLEAN_RESIDUAL ? out.residual : out.map) = planes_k;
                    if (cr->steps) out.steps = host ? d_steps + (size_t) k * frame_steps : cr->steps + (size_t) (j + k) * frame_steps;
                    if (const int brc = csm_clean_enqueue(h, d_C, d_G, n, *c, *cr->cl, out, s)) return brc;
                    AWPU_HIP_TRY(awpu::launch_csm_show(planes_k, K, (int) P, show, rows + (size_t) k * P, s));
                    continue;
                }
                if (capon) {
                    if (const int brc = enqueue_invert(h, d_C, n, *c, d_G, solved_k, s)) return brc;
                } else if (solved_k) {
                    AWPU_HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(solved_k), 1, (size_t) K, s));
                }
                if (const int brc = enqueue_map(h, capon ? d_G : d_C, n, *c, planes_k, nullptr, s)) return brc;
                AWPU_HIP_TRY(awpu::launch_csm_show(planes_k, K, (int) P, show, rows + (size_t) k * P, s));
            }
            if (const int brc = display.show(0, j, nf, rows, s)) return brc;
            if (host && nf > 0) {
                if (power) AWPU_HIP_TRY(hipMemcpyAsync(power + (size_t) j * P, d_rows, (size_t) nf * P * sizeof(float), hipMemcpyDeviceToHost, s));
                if (o.planes) AWPU_HIP_TRY(hipMemcpyAsync(o.planes + (size_t) j * K * P, d_planes, (size_t) nf * K * P * sizeof(float), hipMemcpyDeviceToHost, s));
                if (o.solved) AWPU_HIP_TRY(hipMemcpyAsync(o.solved + (size_t) j * K, d_solved, (size_t) nf * K * sizeof(int32_t), hipMemcpyDeviceToHost, s));
                if (cr && cr->steps)
                    AWPU_HIP_TRY(hipMemcpyAsync(cr->steps + (size_t) j * frame_steps, d_steps, (size_t) nf * frame_steps * sizeof(awpu_csm_clean_step_t),
                                                hipMemcpyDeviceToHost, s));
                if (const int brc = display.fetch(0, nf, s)) return brc;
                AWPU_HIP_TRY(hipStreamSynchronize(s));
                if (const int brc = display.deliver(0, j, nf)) return brc;
            }
            // the store's last length - 1 blocks to its front, by way of the carry (the two ranges may overlap)
            if (keep > 0) {
                const size_t bytes = (size_t) keep * per_block * sizeof(float);
                AWPU_HIP_TRY(hipMemcpyAsync(d_carry, spec + (size_t) n_new * per_block, bytes, hipMemcpyDeviceToDevice, s));
                AWPU_HIP_TRY(hipMemcpyAsync(spec, d_carry, bytes, hipMemcpyDeviceToDevice, s));
            }
            j += nf, c0 = c1;
        }
        // the ring: the call's last four blocks, as a watch run's tail piece leaves them
        const int b0 = n_blocks - 1, q = std::max(0, std::min(3 - b0, 4));
        const float *snapshot = h->d_ring + h->ring_pos;
        if (host) {
            stage_slots(h, src, [=](int slot) { return awpu::watch_slot_block(slot, b0, 1, 1); }, q, 4, 0);
            const size_t block_bytes = (size_t) awpu::kSamples * (src.wire ? (size_t) AWPU_DATAGRAM_BYTES : (size_t) S * sizeof(float));
            AWPU_HIP_TRY(hipMemcpyAsync(h->blk_in.d[0], h->blk_in.h[0], block_bytes * (4 - q), hipMemcpyHostToDevice, s));
        }
        const int grc = gathered_history(h, src, 0, q, 4, AWPU_HIST, s, [&](const float *from, long long from_pitch, int n) {
            return awpu::launch_watch_gather(from, from_pitch, snapshot, b0, 1, S, hist_of(h, 0), AWPU_HIST, 0, n, s);
        });
        if (grc != AWPU_OK) return grc;
        const int pos = (int) ((h->ring_pos + (long long) awpu::kSamples * n_blocks) % AWPU_HIST);
        AWPU_HIP_TRY(awpu::launch_ring_write(hist_of(h, 0), AWPU_HIST, 0, S, h->d_ring, pos, s));
        h->ring_pos = pos;
        if (!host) {
            if (s != h->stream) {  // later calls on the ring (the handle's stream) come after this one
                AWPU_HIP_TRY(hipEventRecord(h->ev_blk_ring, s));
                AWPU_HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_blk_ring, 0));
            }
            return AWPU_OK;
        }
        std::vector<float> back((size_t) keep * per_block);
        if (keep > 0) AWPU_HIP_TRY(hipMemcpyAsync(back.data(), d_carry, back.size() * sizeof(float), hipMemcpyDeviceToHost, s));
        if (const int wrc = wait_and_time(h, false)) return wrc;
        std::copy(back.begin(), back.end(), o.carry);
        return AWPU_OK;
    };
    rc = body();
    if (rc != AWPU_OK) {
        if (host) (void) hipStreamSynchronize(s);  // nothing of the call may still read the caller's buffers
        return rc;
    }
    *o.carried = (int32_t) std::min<long long>((long long) carried_in + n_blocks, keep);
    return AWPU_OK;
}

}  // namespace

// what the other cross-spectral files call (csm_calls.h)
namespace awpu::host {
int csm_check(awpu_hip *h, const awpu_csm_t *c) { return check_csm(h, c); }
int csm_ready_map(awpu_hip *h, const awpu_csm_t *c) { return ready_map(h, c); }
int csm_enqueue_map(awpu_hip *h, const float *d_matrix, int block_count, const awpu_csm_t &c, float *d_map, float *d_q, hipStream_t s) {
    return enqueue_map(h, d_matrix, block_count, c, d_map, d_q, s);
}
}  // namespace awpu::host

extern "C" {

int awpu_hip_csm_samples_device(awpu_hip_t *h, const float *d_samples, int64_t pitch, int32_t n_blocks, const awpu_csm_t *c, float *d_matrix,
                                int32_t *block_count, float *d_spectra, void *stream) {
    AWPU_CTX(h);
    if (int rc = check_samples(h, d_samples, pitch, n_blocks, c, d_matrix, block_count)) return rc;
    int rc = check_ready(h, 1);
    hipStream_t s = stream_of(h, stream);
    if (rc == AWPU_OK) rc = ready_samples(h, n_blocks, *c, d_spectra != nullptr);
    if (rc == AWPU_OK) rc = enter_stream(h, s);
    if (rc == AWPU_OK) rc = enqueue_samples(h, d_samples, pitch, n_blocks, *c, d_matrix, d_spectra, s);
    if (rc != AWPU_OK) return rc;
    *block_count += n_blocks;
    return AWPU_OK;
}

int awpu_hip_csm_samples(awpu_hip_t *h, const float *samples, int64_t pitch, int32_t n_blocks, const awpu_csm_t *c, float *matrix,
                         int32_t *block_count, float *spectra) {
    AWPU_CTX(h);
    if (int rc = check_samples(h, samples, pitch, n_blocks, c, matrix, block_count)) return rc;
    int rc = check_ready(h, 1);
    if (rc == AWPU_OK) rc = ready_samples(h, n_blocks, *c, spectra != nullptr);
    if (rc != AWPU_OK) return rc;
    // the blocks alone go up, [n_streams][256 * n_blocks], then the caller's matrix; the spectra, where asked for, lie behind them
    const int S = h->cfg.n_streams, U = h->usable();
    const size_t row = (size_t) awpu::kCsmSamples * n_blocks;
    const size_t sample_floats = (size_t) S * row, matrix_floats = (size_t) c->n_bins * U * U * 2;
    const size_t spectra_floats = spectra ? (size_t) n_blocks * c->n_bins * U * 2 : 0;
    rc = h->d_csm_io.ensure(sample_floats + matrix_floats + spectra_floats);
    if (rc == AWPU_OK) rc = enter_stream(h, h->stream);
    if (rc != AWPU_OK) return rc;
    float *d_samples = h->d_csm_io.get(), *d_matrix = d_samples + sample_floats, *d_spectra = spectra ? d_matrix + matrix_floats : nullptr;
    AWPU_HIP_TRY(hipMemcpy2DAsync(d_samples, row * sizeof(float), samples, (size_t) pitch * sizeof(float), row * sizeof(float), (size_t) S,
                                  hipMemcpyHostToDevice, h->stream));
    AWPU_HIP_TRY(hipMemcpyAsync(d_matrix, matrix, matrix_floats * sizeof(float), hipMemcpyHostToDevice, h->stream));
    rc = enqueue_samples(h, d_samples, (int64_t) row, n_blocks, *c, d_matrix, d_spectra, h->stream);
    if (rc != AWPU_OK) return rc;
    // the results cross a buffer of the library's first: a call that fails on the device leaves the caller's matrix alone
    std::vector<float> back(matrix_floats + spectra_floats);
    AWPU_HIP_TRY(hipMemcpyAsync(back.data(), d_matrix, back.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    rc = wait_and_time(h, false);
    if (rc != AWPU_OK) return rc;
    std::copy(back.begin(), back.begin() + matrix_floats, matrix);
    if (spectra) std::copy(back.begin() + matrix_floats, back.end(), spectra);
    *block_count += n_blocks;
    return AWPU_OK;
}

int awpu_hip_csm_map_device(awpu_hip_t *h, const float *d_matrix, int32_t block_count, const awpu_csm_t *c, float *d_map, float *d_q,
                            void *stream) {
    AWPU_CTX(h);
    if (int rc = check_map(h, d_matrix, block_count, c, d_map, d_q)) return rc;
    int rc = check_ready(h, 1);
    hipStream_t s = stream_of(h, stream);
    if (rc == AWPU_OK) rc = ready_map(h, c);
    if (rc == AWPU_OK) rc = enter_stream(h, s);
    if (rc != AWPU_OK) return rc;
    return enqueue_map(h, d_matrix, block_count, *c, d_map, d_q, s);
}

int awpu_hip_csm_map(awpu_hip_t *h, const float *matrix, int32_t block_count, const awpu_csm_t *c, float *map, float *q) {
    AWPU_CTX(h);
    if (int rc = check_map(h, matrix, block_count, c, map, q)) return rc;
    int rc = check_ready(h, 1);
    if (rc == AWPU_OK) rc = ready_map(h, c);
    if (rc != AWPU_OK) return rc;
    const int U = h->usable();
    const size_t matrix_floats = (size_t) c->n_bins * U * U * 2, plane = (size_t) c->n_bins * h->cfg.pixel_count;
    rc = h->d_csm_io.ensure(matrix_floats + 2 * plane);
    if (rc == AWPU_OK) rc = enter_stream(h, h->stream);
    if (rc != AWPU_OK) return rc;
    float *d_matrix = h->d_csm_io.get(), *d_map = d_matrix + matrix_floats, *d_q = d_map + plane;
    AWPU_HIP_TRY(hipMemcpyAsync(d_matrix, matrix, matrix_floats * sizeof(float), hipMemcpyHostToDevice, h->stream));
    rc = enqueue_map(h, d_matrix, block_count, *c, map ? d_map : nullptr, q ? d_q : nullptr, h->stream);
    if (rc != AWPU_OK) return rc;
    // the planes cross a buffer of the library's first, as awpu_hip_csm_samples' results do: a call that fails on the device leaves
    // the caller's map and q alone
    std::vector<float> back(2 * plane);
    AWPU_HIP_TRY(hipMemcpyAsync(back.data(), d_map, back.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    rc = wait_and_time(h, false);
    if (rc != AWPU_OK) return rc;
    if (map) std::copy(back.begin(), back.begin() + plane, map);
    if (q) std::copy(back.begin() + plane, back.end(), q);
    return AWPU_OK;
}

int awpu_hip_csm_invert_device(awpu_hip_t *h, const float *d_matrix, int32_t block_count, const awpu_csm_t *c, float *d_inverse,
                               int32_t *d_solved, void *stream) {
    AWPU_CTX(h);
    if (int rc = check_invert(h, d_matrix, block_count, c, d_inverse)) return rc;
    int rc = check_ready(h, 1);
    hipStream_t s = stream_of(h, stream);
    if (rc == AWPU_OK) rc = ready_invert(h, c);
    if (rc == AWPU_OK) rc = enter_stream(h, s);
    if (rc != AWPU_OK) return rc;
    return enqueue_invert(h, d_matrix, block_count, *c, d_inverse, d_solved, s);
}

int awpu_hip_csm_invert(awpu_hip_t *h, const float *matrix, int32_t block_count, const awpu_csm_t *c, float *inverse) {
    AWPU_CTX(h);
    if (int rc = check_invert(h, matrix, block_count, c, inverse)) return rc;
    int rc = check_ready(h, 1);
    if (rc == AWPU_OK) rc = ready_invert(h, c);
    if (rc != AWPU_OK) return rc;
    // the matrix goes up; the inverse and the bins' solved words (one float's room each) come back through a buffer of the library's
    const int U = h->usable();
    const size_t matrix_floats = (size_t) c->n_bins * U * U * 2;
    static_assert(sizeof(int32_t) == sizeof(float), "the solved words lie in the float buffer");
    rc = h->d_csm_io.ensure(2 * matrix_floats + (size_t) c->n_bins);
    if (rc == AWPU_OK) rc = enter_stream(h, h->stream);
    if (rc != AWPU_OK) return rc;
    float *d_matrix = h->d_csm_io.get(), *d_inverse = d_matrix + matrix_floats;
    int32_t *d_solved = reinterpret_cast<int32_t *>(d_inverse + matrix_floats);
    AWPU_HIP_TRY(hipMemcpyAsync(d_matrix, matrix, matrix_floats * sizeof(float), hipMemcpyHostToDevice, h->stream));
    rc = enqueue_invert(h, d_matrix, block_count, *c, d_inverse, d_solved, h->stream);
    if (rc != AWPU_OK) return rc;
    std::vector<float> back(matrix_floats + (size_t) c->n_bins);
    AWPU_HIP_TRY(hipMemcpyAsync(back.data(), d_inverse, back.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    rc = wait_and_time(h, false);
    if (rc != AWPU_OK) return rc;
    for (int kb = 0; kb < c->n_bins; kb++) {
        int32_t word;
        std::memcpy(&word, &back[matrix_floats + (size_t) kb], sizeof word);
        if (!word) return fail(AWPU_ERR_RANGE, "a bin's loaded matrix is not positive definite (or not finite): nothing written");
    }
    std::copy(back.begin(), back.begin() + matrix_floats, inverse);
    return AWPU_OK;
}

int awpu_hip_csm_watch_blocks(awpu_hip_t *h, const void *datagrams, int32_t stride_bytes, int32_t n_blocks, const awpu_watch_t *w,
                              const awpu_csm_t *c, int32_t length, int32_t show, const awpu_find_t *f, float *carry, int32_t *carried,
                              uint8_t *image, uint8_t *big_image, float *power, awpu_source_t *sources, int32_t *count, float *planes,
                              int32_t *solved) {
    BlockRun src;
    if (int rc = wire_source(h, datagrams, stride_bytes, n_blocks, &src)) return rc;
    return csm_watch_run(h, src, n_blocks, w, c, length, show, f, image, big_image, power, sources, count, {carry, carried, planes, solved}, nullptr);
}

int awpu_hip_csm_watch_samples(awpu_hip_t *h, const float *samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                               const awpu_csm_t *c, int32_t length, int32_t show, const awpu_find_t *f, float *carry, int32_t *carried,
                               uint8_t *image, uint8_t *big_image, float *power, awpu_source_t *sources, int32_t *count, float *planes,
                               int32_t *solved) {
    BlockRun src;
    if (int rc = sample_source(h, samples, pitch, n_blocks, false, &src)) return rc;
    return csm_watch_run(h, src, n_blocks, w, c, length, show, f, image, big_image, power, sources, count, {carry, carried, planes, solved}, nullptr);
}

int awpu_hip_csm_watch_samples_device(awpu_hip_t *h, const float *d_samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                                      const awpu_csm_t *c, int32_t length, int32_t show, const awpu_find_t *f, float *d_carry,
                                      int32_t *carried, uint8_t *d_image, uint8_t *d_big_image, float *d_power, awpu_source_t *d_sources,
                                      int32_t *d_count, float *d_planes, int32_t *d_solved, void *stream) {
    BlockRun src;
    if (int rc = sample_source(h, d_samples, pitch, n_blocks, true, &src)) return rc;
    return csm_watch_run(h, src, n_blocks, w, c, length, show, f, d_image, d_big_image, d_power, d_sources, d_count,
                         {d_carry, carried, d_planes, d_solved}, static_cast<hipStream_t>(stream));
}

// CLEAN-SC runs (awpu_hip_csm_clean.h): the watch run with the loop in place of the map

int awpu_hip_csm_clean_blocks(awpu_hip_t *h, const void *datagrams, int32_t stride_bytes, int32_t n_blocks, const awpu_watch_t *w,
                              const awpu_csm_t *c, int32_t length, int32_t show, const awpu_find_t *f, float *carry, int32_t *carried,
                              const awpu_csm_clean_t *cl, int32_t what, uint8_t *image, uint8_t *big_image, float *power, awpu_source_t *sources,
                              int32_t *count, float *planes, awpu_csm_clean_step_t *steps) {
    BlockRun src;
    if (int rc = wire_source(h, datagrams, stride_bytes, n_blocks, &src)) return rc;
    const CsmCleanRun cr{cl, what, steps};
    return csm_watch_run(h, src, n_blocks, w, c, length, show, f, image, big_image, power, sources, count, {carry, carried, planes, nullptr}, nullptr, &cr);
}

int awpu_hip_csm_clean_samples(awpu_hip_t *h, const float *samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                               const awpu_csm_t *c, int32_t length, int32_t show, const awpu_find_t *f, float *carry, int32_t *carried,
                               const awpu_csm_clean_t *cl, int32_t what, uint8_t *image, uint8_t *big_image, float *power, awpu_source_t *sources,
                               int32_t *count, float *planes, awpu_csm_clean_step_t *steps) {
    BlockRun src;
    if (int rc = sample_source(h, samples, pitch, n_blocks, false, &src)) return rc;
    const CsmCleanRun cr{cl, what, steps};
    return csm_watch_run(h, src, n_blocks, w, c, length, show, f, image, big_image, power, sources, count, {carry, carried, planes, nullptr}, nullptr, &cr);
}

int awpu_hip_csm_clean_samples_device(awpu_hip_t *h, const float *d_samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                                      const awpu_csm_t *c, int32_t length, int32_t show, const awpu_find_t *f, float *d_carry,
                                      int32_t *carried, const awpu_csm_clean_t *cl, int32_t what, uint8_t *d_image, uint8_t *d_big_image,
                                      float *d_power, awpu_source_t *d_sources, int32_t *d_count, float *d_planes,
                                      awpu_csm_clean_step_t *d_steps, void *stream) {
    BlockRun src;
    if (int rc = sample_source(h, d_samples, pitch, n_blocks, true, &src)) return rc;
    const CsmCleanRun cr{cl, what, d_steps};
    return csm_watch_run(h, src, n_blocks, w, c, length, show, f, d_image, d_big_image, d_power, d_sources, d_count,
                         {d_carry, carried, d_planes, nullptr}, static_cast<hipStream_t>(stream), &cr);
}

}  // extern "C"
