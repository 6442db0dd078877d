// awpu_csm_eig.cpp -- the handle forms of step 8 of include/awpu_hip_csm.h (include/awpu_hip_csm_eig.h): awpu_hip_csm_eig and
// _eig_device, the eigendecomposition of a cross-spectral matrix; awpu_hip_csm_eig_weigh_device, the weighed matrix; and
// awpu_hip_csm_eig_map and _eig_map_device, the subspace maps, which enqueue those two, the map's q (csm_calls.h) on the weighed
// matrix and the finish.  The rule is csm_eig_rule.h's, the kernels and their launchers csm_eig_kernels.hip's.  The refusals and
// everything that may block come before a call enqueues anything; the device forms wait for nothing on the host.
#include "awpu_hip_csm.h"

#include <cstring>

#include "csm_calls.h"
#include "csm_eig_kernels.h"

using namespace awpu::host;

namespace {

static_assert(sizeof(int32_t) == sizeof(float), "the solved and sweep words lie in float buffers");

// the refusals that come before the handle is made ready
int check_eig(awpu_hip *h, const awpu_csm_t *c, bool pointers, int32_t block_count) {
    if (int rc = csm_check(h, c)) return rc;
    if (!pointers) return invalid("null argument");
    if (block_count < 1) return invalid("the block count is at least 1");
    return AWPU_OK;
}
int check_conventional(const awpu_csm_t *c) {
    return c->kind == AWPU_CSM_CONVENTIONAL ? (int) AWPU_OK : invalid("the subspace maps take c->kind AWPU_CSM_CONVENTIONAL");
}
// behind check_ready: the refusals that read the active list
int check_mics(awpu_hip *h) {
    return h->usable() > awpu::kCsmEigMaxUsable ? fail(AWPU_ERR_RANGE, "more than 256 active mics: the eigendecomposition takes no more") : (int) AWPU_OK;
}
int check_request(awpu_hip *h, const awpu_csm_eig_t *e) {
    if (const char *why = awpu::csm_eig_refusal(e, h->usable())) return invalid(why);
    return AWPU_OK;
}
int ready_eig(awpu_hip *h, const awpu_csm_t &c) { return h->d_csm_eig.ensure(awpu::csm_eig_scratch_doubles(h->usable(), c.n_bins)); }

int enqueue_eig(awpu_hip *h, const float *d_matrix, int block_count, const awpu_csm_t &c, float *d_values, float *d_vectors, int32_t *d_solved,
                int32_t *d_sweeps, hipStream_t s) {
    awpu::CsmEigArgs a{};
    a.matrix = d_matrix, a.values = d_values, a.vectors = d_vectors, a.solved = d_solved, a.sweeps = d_sweeps;
    a.scratch = h->d_csm_eig.get();
    a.usable = h->usable(), a.n_bins = c.n_bins, a.block_count = block_count;
    AWPU_HIP_TRY(awpu::launch_csm_eig(a, s));
    return AWPU_OK;
}

int enqueue_weigh(awpu_hip *h, const float *d_values, const float *d_vectors, const awpu_csm_t &c, const awpu_csm_eig_t &e, float *d_weighed,
                  hipStream_t s) {
    awpu::CsmEigWeighArgs a{};
    a.values = d_values, a.vectors = d_vectors, a.weighed = d_weighed;
    a.usable = h->usable(), a.n_bins = c.n_bins, a.kind = e.kind, a.n_sources = e.n_sources, a.root = e.root;
    AWPU_HIP_TRY(awpu::launch_csm_eig_weigh(a, s));
    return AWPU_OK;
}

// what a subspace map keeps in the handle's rows: csm_eig_rows below lays it out
struct EigRows {
    float *vectors, *weighed, *q, *values;
    int32_t *solved;
};
size_t eig_rows_floats(const awpu_hip *h, const awpu_csm_t &c) {
    return 2 * csm_matrix_floats(h, c) + csm_plane_floats(h, c) + (size_t) c.n_bins * h->usable() + (size_t) c.n_bins;
}
EigRows eig_rows(awpu_hip *h, const awpu_csm_t &c) {
    EigRows r{};
    r.vectors = h->d_csm_eig_rows.get();
    r.weighed = r.vectors + csm_matrix_floats(h, c);
    r.q = r.weighed + csm_matrix_floats(h, c);
    r.values = r.q + csm_plane_floats(h, c);
    r.solved = reinterpret_cast<int32_t *>(r.values + (size_t) c.n_bins * h->usable());
    return r;
}

// everything of a subspace map that may block, behind check_ready
int ready_eig_map(awpu_hip *h, const awpu_csm_t *c) {
    int rc = csm_ready_map(h, c);
    if (rc == AWPU_OK) rc = ready_eig(h, *c);
    if (rc == AWPU_OK) rc = h->d_csm_eig_rows.ensure(eig_rows_floats(h, *c));
    return rc;
}

// steps 8a to 8c on device buffers, enqueued on s, behind ready_eig_map: nothing here allocates or waits
int enqueue_eig_map(awpu_hip *h, const float *d_matrix, int block_count, const awpu_csm_t &c, const awpu_csm_eig_t &e, float *d_map,
                    float *d_values, int32_t *d_solved, hipStream_t s) {
    const EigRows r = eig_rows(h, c);
    float *values = d_values ? d_values : r.values;
    int32_t *solved = d_solved ? d_solved : r.solved;
    if (int rc = enqueue_eig(h, d_matrix, block_count, c, values, r.vectors, solved, nullptr, s)) return rc;
    if (int rc = enqueue_weigh(h, values, r.vectors, c, e, r.weighed, s)) return rc;
    if (int rc = csm_enqueue_map(h, r.weighed, 1, c, nullptr, r.q, s)) return rc;
    awpu::CsmEigFinishArgs f{};
    f.q = r.q, f.solved = solved, f.map = d_map;
    f.usable = h->usable(), f.pixel_count = h->cfg.pixel_count, f.n_bins = c.n_bins, f.kind = e.kind, f.root = e.root;
    f.scale = awpu::csm_wss(c.window) * 256.0f;
    for (int i = 0; i < c.n_bins; i++) f.bin[i] = c.bin[i];
    AWPU_HIP_TRY(awpu::launch_csm_eig_finish(f, s));
    return AWPU_OK;
}

}  // namespace

extern "C" {

int awpu_hip_csm_eig_device(awpu_hip_t *h, const float *d_matrix, int32_t block_count, const awpu_csm_t *c, float *d_values, float *d_vectors,
                            int32_t *d_solved, int32_t *d_sweeps, void *stream) {
    AWPU_CTX(h);
    if (int rc = check_eig(h, c, d_matrix && d_values && d_vectors, block_count)) return rc;
    int rc = check_ready(h, 1);
    hipStream_t s = stream_of(h, stream);
    if (rc == AWPU_OK) rc = check_mics(h);
    if (rc == AWPU_OK) rc = ready_eig(h, *c);
    if (rc == AWPU_OK) rc = enter_stream(h, s);
    if (rc != AWPU_OK) return rc;
    return enqueue_eig(h, d_matrix, block_count, *c, d_values, d_vectors, d_solved, d_sweeps, s);
}

int awpu_hip_csm_eig(awpu_hip_t *h, const float *matrix, int32_t block_count, const awpu_csm_t *c, float *values, float *vectors,
                     int32_t *solved, int32_t *sweeps) {
    AWPU_CTX(h);
    if (int rc = check_eig(h, c, matrix && values && vectors, block_count)) return rc;
    int rc = check_ready(h, 1);
    if (rc == AWPU_OK) rc = check_mics(h);
    if (rc == AWPU_OK) rc = ready_eig(h, *c);
    if (rc != AWPU_OK) return rc;
    // the matrix goes up; the vectors, the values and the bins' solved and sweep words come back through a buffer of the library's
    const size_t matrix_floats = csm_matrix_floats(h, *c), K = (size_t) c->n_bins, value_floats = K * h->usable();
    rc = h->d_csm_io.ensure(2 * matrix_floats + value_floats + 2 * K);
    if (rc == AWPU_OK) rc = enter_stream(h, h->stream);
    if (rc != AWPU_OK) return rc;
    float *d_matrix = h->d_csm_io.get(), *d_vectors = d_matrix + matrix_floats, *d_values = d_vectors + matrix_floats;
    int32_t *d_solved = reinterpret_cast<int32_t *>(d_values + value_floats), *d_sweeps = d_solved + K;
    AWPU_HIP_TRY(hipMemcpyAsync(d_matrix, matrix, matrix_floats * sizeof(float), hipMemcpyHostToDevice, h->stream));
    rc = enqueue_eig(h, d_matrix, block_count, *c, d_values, d_vectors, d_solved, d_sweeps, h->stream);
    if (rc != AWPU_OK) return rc;
    std::vector<float> back(matrix_floats + value_floats + 2 * K);
    AWPU_HIP_TRY(hipMemcpyAsync(back.data(), d_vectors, back.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    rc = wait_and_time(h, false);
    if (rc != AWPU_OK) return rc;
    std::copy(back.begin(), back.begin() + matrix_floats, vectors);
    std::copy(back.begin() + matrix_floats, back.begin() + matrix_floats + value_floats, values);
    if (solved) std::memcpy(solved, &back[matrix_floats + value_floats], K * sizeof(int32_t));
    if (sweeps) std::memcpy(sweeps, &back[matrix_floats + value_floats + K], K * sizeof(int32_t));
    return AWPU_OK;
}

int awpu_hip_csm_eig_weigh_device(awpu_hip_t *h, const float *d_values, const float *d_vectors, const awpu_csm_t *c, const awpu_csm_eig_t *e,
                                  float *d_weighed, void *stream) {
    AWPU_CTX(h);
    if (int rc = check_eig(h, c, d_values && d_vectors && d_weighed && e, 1)) return rc;
    if (int rc = check_conventional(c)) return rc;
    const awpu_csm_eig_t request = *e;
    int rc = check_ready(h, 1);
    hipStream_t s = stream_of(h, stream);
    if (rc == AWPU_OK) rc = check_mics(h);
    if (rc == AWPU_OK) rc = check_request(h, &request);
    if (rc == AWPU_OK) rc = enter_stream(h, s);
    if (rc != AWPU_OK) return rc;
    return enqueue_weigh(h, d_values, d_vectors, *c, request, d_weighed, s);
}

int awpu_hip_csm_eig_map_device(awpu_hip_t *h, const float *d_matrix, int32_t block_count, const awpu_csm_t *c, const awpu_csm_eig_t *e,
                                float *d_map, float *d_values, int32_t *d_solved, void *stream) {
    AWPU_CTX(h);
    if (int rc = check_eig(h, c, d_matrix && d_map && e, block_count)) return rc;
    if (int rc = check_conventional(c)) return rc;
    const awpu_csm_eig_t request = *e;
    int rc = check_ready(h, 1);
    hipStream_t s = stream_of(h, stream);
    if (rc == AWPU_OK) rc = check_mics(h);
    if (rc == AWPU_OK) rc = check_request(h, &request);
    if (rc == AWPU_OK) rc = ready_eig_map(h, c);
    if (rc == AWPU_OK) rc = enter_stream(h, s);
    if (rc != AWPU_OK) return rc;
    return enqueue_eig_map(h, d_matrix, block_count, *c, request, d_map, d_values, d_solved, s);
}

int awpu_hip_csm_eig_map(awpu_hip_t *h, const float *matrix, int32_t block_count, const awpu_csm_t *c, const awpu_csm_eig_t *e, float *map,
                         float *values, int32_t *solved) {
    AWPU_CTX(h);
    if (int rc = check_eig(h, c, matrix && map && e, block_count)) return rc;
    if (int rc = check_conventional(c)) return rc;
    const awpu_csm_eig_t request = *e;
    int rc = check_ready(h, 1);
    if (rc == AWPU_OK) rc = check_mics(h);
    if (rc == AWPU_OK) rc = check_request(h, &request);
    if (rc == AWPU_OK) rc = ready_eig_map(h, c);
    if (rc != AWPU_OK) return rc;
    // the matrix goes up; the map, the values and the solved words come back through a buffer of the library's
    const size_t matrix_floats = csm_matrix_floats(h, *c), plane = csm_plane_floats(h, *c), K = (size_t) c->n_bins, value_floats = K * h->usable();
    rc = h->d_csm_io.ensure(matrix_floats + plane + value_floats + K);
    if (rc == AWPU_OK) rc = enter_stream(h, h->stream);
    if (rc != AWPU_OK) return rc;
    float *d_matrix = h->d_csm_io.get(), *d_map = d_matrix + matrix_floats, *d_values = d_map + plane;
    int32_t *d_solved = reinterpret_cast<int32_t *>(d_values + value_floats);
    AWPU_HIP_TRY(hipMemcpyAsync(d_matrix, matrix, matrix_floats * sizeof(float), hipMemcpyHostToDevice, h->stream));
    rc = enqueue_eig_map(h, d_matrix, block_count, *c, request, d_map, d_values, d_solved, h->stream);
    if (rc != AWPU_OK) return rc;
    std::vector<float> back(plane + value_floats + K);
    AWPU_HIP_TRY(hipMemcpyAsync(back.data(), d_map, back.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    rc = wait_and_time(h, false);
    if (rc != AWPU_OK) return rc;
    std::copy(back.begin(), back.begin() + plane, map);
    if (values) std::copy(back.begin() + plane, back.begin() + plane + value_floats, values);
    if (solved) std::memcpy(solved, &back[plane + value_floats], K * sizeof(int32_t));
    return AWPU_OK;
}

}  // extern "C"
