// awpu_focus.cpp -- ranging (include/awpu_hip_focus.h): awpu_hip_range, one launch of range_kernel (track_kernels.hip) over every
// (source, candidate distance), and awpu_hip_range_pick, the host definition of which candidate wins.  The focused tables' rule
// is geometry_host.cpp's; locating in runs of blocks is awpu_runs.cpp's.
#include "awpu_handle.h"

#include <cmath>
#include <vector>

#include "focus_rule.h"

using namespace awpu::host;

namespace awpu::host {

// what awpu_hip_range and the locate runs ask of their candidates (reads no handle)
int check_candidates(const double *distance, int32_t n_dist) {
    if (!distance) return invalid("null argument");
    if (n_dist < 1 || n_dist > AWPU_RANGE_MAX_CANDIDATES) return invalid("n_dist outside [1, 64]");
    for (int j = 0; j < n_dist; j++)
        if (!awpu::focus_distance_ok(distance[j])) return invalid("a candidate distance must be > 0 (+INFINITY: a plane wave)");
    return AWPU_OK;
}

}  // namespace awpu::host

extern "C" {

int awpu_hip_range_pick(const float *power, int32_t n_src, const double *distance, int32_t n_dist, awpu_range_t *best) {
    if (!power || !best) return invalid("null argument");
    if (n_src < 1) return invalid("n_src below 1");
    if (const int rc = check_candidates(distance, n_dist)) return rc;
    for (int k = 0; k < n_src; k++) awpu::range_pick_one(power + (size_t) k * n_dist, distance, n_dist, best + k);
    return AWPU_OK;
}

int awpu_hip_range(awpu_hip_t *h, const float *d_frame, const double *theta, const double *phi, int32_t n_src, const double *distance,
                   int32_t n_dist, float *power, awpu_range_t *best) {
    h = first_device(h);
    AWPU_CTX(h);
    if (!h || !theta || !phi || !power) return invalid("null argument");
    if (n_src < 1 || n_src > AWPU_FIND_MAX_SOURCES) return invalid("n_src outside [1, 32]");
    if (const int rc = check_candidates(distance, n_dist)) return rc;
    for (int k = 0; k < n_src; k++)
        if (!std::isfinite(theta[k]) || !std::isfinite(phi[k])) return invalid("direction not finite");
    if (int rc = check_antenna(h)) return rc;
    int pitch = h->cfg.hist;
    const float *frame = d_frame;
    if (!frame) {  // the current snapshot of the ingest ring
        if (!h->d_ring) return fail(AWPU_ERR_STATE, "no block ingested yet");
        frame = h->d_ring + h->ring_pos;
        pitch = 2048;
    } else if (h->cfg.hist < 2 * awpu::kSamples + 1) {
        return fail(AWPU_ERR_RANGE, "history shorter than 513 samples: a focused delay can read outside it");
    }
    AWPU_HIP_TRY(hipSetDevice(h->cfg.device));
    if (int rc = enter_stream(h, h->stream)) return rc;
    if (int rc = ensure_track_index(h)) return rc;
    const size_t angles = align16((size_t) n_src * sizeof(double)), powers = (size_t) n_src * n_dist * sizeof(float);
    if (int rc = h->d_track.ensure(2 * angles + powers)) return rc;
    awpu::RangeArgs a{};
    a.frame = frame;
    a.frame_step = 0;
    a.per_frame = n_src;
    a.pitch = pitch;
    a.xyz = h->d_xyz;
    a.n = (int) (h->antenna.size() / 3);
    a.index = h->d_track_index;
    a.usable = h->usable();
    a.theta = (const double *) h->d_track.get();
    a.phi = (const double *) (h->d_track + angles);
    a.n_src = n_src;
    a.n_dist = n_dist;
    a.power = (float *) (h->d_track + 2 * angles);
    for (int j = 0; j < n_dist; j++) a.distance[j] = distance[j];
    AWPU_HIP_TRY(hipMemcpyAsync(h->d_track, theta, (size_t) n_src * sizeof(double), hipMemcpyHostToDevice, h->stream));
    AWPU_HIP_TRY(hipMemcpyAsync(h->d_track + angles, phi, (size_t) n_src * sizeof(double), hipMemcpyHostToDevice, h->stream));
    AWPU_HIP_TRY(awpu::launch_range(a, h->stream));
    std::vector<float> back((size_t) n_src * n_dist);  // (the caller's row is written only when the call succeeds)
    AWPU_HIP_TRY(hipMemcpyAsync(back.data(), a.power, powers, hipMemcpyDeviceToHost, h->stream));
    AWPU_HIP_TRY(hipStreamSynchronize(h->stream));
    std::copy(back.begin(), back.end(), power);
    if (best) return awpu_hip_range_pick(power, n_src, distance, n_dist, best);
    return AWPU_OK;
}

}  // extern "C"
