// awpu_csm.cpp -- the handle forms of the cross-spectral maps (include/awpu_hip_csm.h): awpu_hip_csm_samples, _samples_device,
// _map and _map_device, and step 6a's awpu_hip_csm_invert and _invert_device, with what the other cross-spectral files enqueue
// through csm_calls.h (the runs are awpu_csm_run.cpp's, CLEAN-SC's loop awpu_csm_clean.cpp's).
// The rule is csm_rule.h's and csm_invert_rule.h's, the kernels and their launchers csm_kernels.hip's and csm_invert_kernels.hip's.
// The calls read the handle's active list, gains and delay table (the coherence sweep's LutEntry table: ensure_cohere_table) and the tone sweep's two tables
// (ensure_tones_tables); they count no sweep launch and leave stats.kernel_variant alone.
#include "awpu_hip_csm.h"

#include <cstring>

#include "csm_calls.h"
#include "csm_invert_kernels.h"
#include "csm_kernels.h"
#include "csm_run_plan.h"  // kBlocksPerLaunch

using namespace awpu::host;

namespace awpu::host {

int csm_check(awpu_hip *h, const awpu_csm_t *c) {
    if (!h) return invalid("null handle");
    if (const char *why = awpu::csm_refusal(c)) return invalid(why);
    if (is_group(h)) return fail(AWPU_ERR_STATE, "a device group takes no cross-spectral call");
    if (h->in_flight) return fail(AWPU_ERR_STATE, "an awpu_hip_process_async call is in flight on this handle: awpu_hip_wait first");
    if (h->cfg.interp != AWPU_INTERP_LERP) return fail(AWPU_ERR_STATE, "the cross-spectral maps steer by the linear table: AWPU_INTERP_FIR8 is not taken");
    if (!h->band.empty()) return fail(AWPU_ERR_STATE, "a band is set on the handle: the cross-spectral maps choose their bins themselves");
    return AWPU_OK;
}

int csm_enqueue_spectra(awpu_hip *h, const float *d_samples, long long pitch, int n_blocks, const awpu_csm_t &c, float *d_spectra, hipStream_t s) {
    awpu::CsmSpectraArgs sp{};
    sp.samples = d_samples, sp.pitch = pitch;
    sp.index = h->d_index, sp.gain = h->d_gain;
    sp.window = h->d_tones_tables.get() + (c.window == AWPU_TONES_HANN ? awpu::kCsmSamples : 0);
    sp.twiddles = csm_twiddles(h);
    sp.spectra = d_spectra;
    sp.usable = h->usable(), sp.n_blocks = n_blocks, sp.n_bins = c.n_bins;
    for (int i = 0; i < c.n_bins; i++) sp.bin[i] = c.bin[i];
    AWPU_HIP_TRY(awpu::launch_csm_spectra(sp, s));
    return AWPU_OK;
}

int csm_ready_map(awpu_hip *h, const awpu_csm_t *c) {
    if (c->kind == AWPU_CSM_DIAGONAL_REMOVED && h->usable() == 1) return invalid("diagonal removal needs two active mics");
    if (awpu::csm_map_pixels_per_wave(h->usable()) == 0) return fail(AWPU_ERR_RANGE, "more than 2048 active mics: their steering vectors do not fit the LDS");
    const int rc = ensure_cohere_table(h);
    return rc != AWPU_OK ? rc : ensure_tones_tables(h);
}

int csm_enqueue_map(awpu_hip *h, const float *d_matrix, int block_count, const awpu_csm_t &c, float *d_map, float *d_q, hipStream_t s) {
    if (!csm_lut(h) || !h->d_tones_tables) return fail(AWPU_ERR_STATE, "the cross-spectral map has no tables: ensure_cohere_table and ensure_tones_tables come first");
    awpu::CsmMapArgs a{};
    a.matrix = d_matrix;
    a.lut = csm_lut(h);
    a.twiddles = csm_twiddles(h);
    a.map = d_map, a.q = d_q;
    a.usable = h->usable(), a.pixel_count = h->cfg.pixel_count, a.wstart = h->wstart, a.n_bins = c.n_bins, a.kind = c.kind;
    a.scale = c.kind == AWPU_CSM_CAPON ? awpu::csm_wss(c.window) * 256.0f : awpu::csm_scale(c, h->usable(), block_count);
    for (int i = 0; i < c.n_bins; i++) a.bin[i] = c.bin[i];
    AWPU_HIP_TRY(awpu::launch_csm_map(a, s));
    return AWPU_OK;
}

int csm_ready_invert(awpu_hip *h, const awpu_csm_t *c) {
    if (h->usable() > awpu::kCsmInvertMaxUsable) return fail(AWPU_ERR_RANGE, "more than 512 active mics: the loaded inverse takes no more");
    return h->d_csm_invert.ensure(awpu::csm_invert_scratch_doubles(h->usable(), c->n_bins));
}

int csm_enqueue_invert(awpu_hip *h, const float *d_matrix, int block_count, const awpu_csm_t &c, float *d_inverse, int32_t *d_solved, hipStream_t s) {
    awpu::CsmInvertArgs a{};
    a.matrix = d_matrix, a.inverse = d_inverse, a.solved = d_solved;
    a.scratch = h->d_csm_invert.get();
    a.usable = h->usable(), a.n_bins = c.n_bins, a.block_count = block_count, a.loading = c.loading;
    AWPU_HIP_TRY(awpu::launch_csm_invert(a, s));
    return AWPU_OK;
}

}  // namespace awpu::host

namespace {

int check_samples(awpu_hip *h, const float *samples, int64_t pitch, int32_t n_blocks, const awpu_csm_t *c, const float *matrix,
                  const int32_t *block_count) {
    if (int rc = csm_check(h, c)) return rc;
    if (!samples || !matrix || !block_count) return invalid("null argument");
    if (n_blocks < 1 || pitch < (int64_t) awpu::kCsmSamples * n_blocks) return invalid("n_blocks >= 1 and pitch >= 256 * n_blocks");
    if (*block_count < 0 || *block_count > INT32_MAX - n_blocks) return invalid("the block count lies in [0, 2^31 - 1 - n_blocks]");
    return AWPU_OK;
}

int check_map(awpu_hip *h, const float *matrix, int32_t block_count, const awpu_csm_t *c, const float *map, const float *q) {
    if (int rc = csm_check(h, c)) return rc;
    if (!matrix) return invalid("null argument");
    if (!map && !q) return invalid("no output asked for");
    if (block_count < 1) return invalid("the block count is at least 1");
    return AWPU_OK;
}

int check_invert(awpu_hip *h, const float *matrix, int32_t block_count, const awpu_csm_t *c, const float *inverse) {
    if (int rc = csm_check(h, c)) return rc;
    if (!matrix || !inverse) return invalid("null argument");
    if (block_count < 1) return invalid("the block count is at least 1");
    return AWPU_OK;
}

// steps 1 and 2 on device buffers, enqueued on s; the scratch is there (or the caller keeps the spectra)
int enqueue_samples(awpu_hip *h, const float *d_samples, int64_t pitch, int n_blocks, const awpu_csm_t &c, float *d_matrix, float *d_spectra,
                    hipStream_t s) {
    for (int first = 0; first < n_blocks; first += awpu::kBlocksPerLaunch) {
        const int n = std::min(awpu::kBlocksPerLaunch, n_blocks - first);
        float *spectra = d_spectra ? d_spectra + (size_t) first * csm_spectra_floats(h, c) : h->d_csm_spectra.get();
        if (int rc = csm_enqueue_spectra(h, d_samples + (size_t) first * awpu::kCsmSamples, pitch, n, c, spectra, s)) return rc;
        awpu::CsmAccumulateArgs ac{};
        ac.spectra = spectra, ac.matrix = d_matrix;
        ac.usable = h->usable(), ac.n_blocks = n, ac.n_bins = c.n_bins;
        AWPU_HIP_TRY(awpu::launch_csm_accumulate(ac, s));
    }
    return AWPU_OK;
}

int ready_samples(awpu_hip *h, int n_blocks, const awpu_csm_t &c, bool own_spectra) {
    if (const int rc = ensure_tones_tables(h); rc != AWPU_OK) return rc;
    if (own_spectra) return AWPU_OK;
    return h->d_csm_spectra.ensure((size_t) std::min(n_blocks, awpu::kBlocksPerLaunch) * csm_spectra_floats(h, c));
}

}  // namespace

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
    const int S = h->cfg.n_streams;
    const size_t row = (size_t) awpu::kCsmSamples * n_blocks;
    const size_t sample_floats = (size_t) S * row, matrix_floats = csm_matrix_floats(h, *c);
    const size_t spectra_floats = spectra ? (size_t) n_blocks * csm_spectra_floats(h, *c) : 0;
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
    if (rc == AWPU_OK) rc = csm_ready_map(h, c);
    if (rc == AWPU_OK) rc = enter_stream(h, s);
    if (rc != AWPU_OK) return rc;
    return csm_enqueue_map(h, d_matrix, block_count, *c, d_map, d_q, s);
}

int awpu_hip_csm_map(awpu_hip_t *h, const float *matrix, int32_t block_count, const awpu_csm_t *c, float *map, float *q) {
    AWPU_CTX(h);
    if (int rc = check_map(h, matrix, block_count, c, map, q)) return rc;
    int rc = check_ready(h, 1);
    if (rc == AWPU_OK) rc = csm_ready_map(h, c);
    if (rc != AWPU_OK) return rc;
    const size_t matrix_floats = csm_matrix_floats(h, *c), plane = csm_plane_floats(h, *c);
    rc = h->d_csm_io.ensure(matrix_floats + 2 * plane);
    if (rc == AWPU_OK) rc = enter_stream(h, h->stream);
    if (rc != AWPU_OK) return rc;
    float *d_matrix = h->d_csm_io.get(), *d_map = d_matrix + matrix_floats, *d_q = d_map + plane;
    AWPU_HIP_TRY(hipMemcpyAsync(d_matrix, matrix, matrix_floats * sizeof(float), hipMemcpyHostToDevice, h->stream));
    rc = csm_enqueue_map(h, d_matrix, block_count, *c, map ? d_map : nullptr, q ? d_q : nullptr, h->stream);
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
    if (rc == AWPU_OK) rc = csm_ready_invert(h, c);
    if (rc == AWPU_OK) rc = enter_stream(h, s);
    if (rc != AWPU_OK) return rc;
    return csm_enqueue_invert(h, d_matrix, block_count, *c, d_inverse, d_solved, s);
}

int awpu_hip_csm_invert(awpu_hip_t *h, const float *matrix, int32_t block_count, const awpu_csm_t *c, float *inverse) {
    AWPU_CTX(h);
    if (int rc = check_invert(h, matrix, block_count, c, inverse)) return rc;
    int rc = check_ready(h, 1);
    if (rc == AWPU_OK) rc = csm_ready_invert(h, c);
    if (rc != AWPU_OK) return rc;
    // the matrix goes up; the inverse and the bins' solved words (one float's room each) come back through a buffer of the library's
    const size_t matrix_floats = csm_matrix_floats(h, *c);
    static_assert(sizeof(int32_t) == sizeof(float), "the solved words lie in the float buffer");
    rc = h->d_csm_io.ensure(2 * matrix_floats + (size_t) c->n_bins);
    if (rc == AWPU_OK) rc = enter_stream(h, h->stream);
    if (rc != AWPU_OK) return rc;
    float *d_matrix = h->d_csm_io.get(), *d_inverse = d_matrix + matrix_floats;
    int32_t *d_solved = reinterpret_cast<int32_t *>(d_inverse + matrix_floats);
    AWPU_HIP_TRY(hipMemcpyAsync(d_matrix, matrix, matrix_floats * sizeof(float), hipMemcpyHostToDevice, h->stream));
    rc = csm_enqueue_invert(h, d_matrix, block_count, *c, d_inverse, d_solved, h->stream);
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

}  // extern "C"
