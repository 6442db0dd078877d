// track_kernels.hip -- gfx950 particle tracking: steering on the device and the fused monopulse gradient step of the
// reference's --tracking / --miso modes (include/awpu_hip_track.h), and MISO's block-after-block audio over a run of blocks
// (include/awpu_hip_listen.h: listen_blocks_kernel, listen_fixed_kernel).
//
// Replaces (reference tree acoustic-warfare/beamforming-lk):
//   GradientParticle::step        src/dsp/gradient_ascend.cpp:30-81 (quadrant monopulse, RELATIVE 1)
//   Spherical::quadrant, rotateTo src/geometry/geometry.cpp:120-142, :181-216
//   normalizeSpherical            src/dsp/particle.h:24-27, src/geometry/geometry.cpp:7-20
//   Particle::steer / beam / das / step   src/dsp/particle.cpp:22-27, :37-103
//
// The direction arithmetic is the reference's, in fp64; the steering is awpu_hip_steer_table's (geometry_host.cpp):
// angles cast to float, their cosines and sines taken in double and rounded to float, fp32 products without
// contraction, the minimum over every element removed, then the modf split of particle.cpp:39-47.  The beams are
// das_beam_kernel's own body (beam_sums / beam_powers, das_kernels.h).  Contraction into FMAs is off wherever the
// reference (x86, no FMA) rounds a product before the add.
#include "block_kernels.h"
#include "das_kernels.h"

#include "awpu_hip_track.h"
#include "focus_rule.h"

namespace awpu {

namespace {

constexpr float kScale = (float) (48828.0 / 340.0);  // samples per metre, antenna.h:16-17 (= samples_per_metre())
constexpr int kThreads = kSamples;                    // one lane per output sample
constexpr double kPi = 3.14159265358979323846;

// The four floats steer() builds a direction's delays from: Rz((float) phi) = {{cz, -sz, 0}, {sz, cz, 0}, {0, 0, 1}} and row
// z of Ry(-(float) theta) = {-sy, 0, cy} (geometry_host.cpp, rotate_z / rotate_y).
struct Steer {
    float cz, sz, cy, sy;
};

__device__ __forceinline__ Steer steer_of(double theta, double phi) {
    const float fphi = (float) phi;
    const float fy = -(float) theta;
    double sz, cz, sy, cy;
    sincos((double) fphi, &sz, &cz);
    sincos((double) fy, &sy, &cy);
    return Steer{(float) cz, (float) sz, (float) cy, (float) sy};
}

// steering_delays() before the minimum is removed: the z row of Ry * (Rz * p), scaled to samples
__device__ __forceinline__ float raw_delay(const Steer &r, const float *xyz, int n, int i) {
#pragma clang fp contract(off)
    const float p0 = xyz[i], p1 = xyz[n + i], p2 = xyz[2 * n + i];
    const float t0 = r.cz * p0 + -r.sz * p1 + 0.0f * p2;
    const float t1 = r.sz * p0 + r.cz * p1 + 0.0f * p2;
    const float t2 = 0.0f * p0 + 0.0f * p1 + 1.0f * p2;
    const float z = -r.sy * t0 + 0.0f * t1 + r.cy * t2;
    return z * kScale;
}

// particle.cpp:39-47: frac = modf((double) tau), off = N_SAMPLES - whole (exact in float: tau is a float)
__device__ __forceinline__ void split_delay(float tau, int32_t *off, float *frac) {
#pragma clang fp contract(off)
    // whole is in [0, 256] for every table of an antenna awpu_hip_set_antenna accepts; the clamp keeps a NaN delay (a
    // direction made NaN by a zero reference power) from reaching the float-to-int conversion, and every read in bounds
    const float whole = fminf(fmaxf(truncf(tau), 0.0f), (float) kSamples);
    *frac = tau - whole;
    *off = kSamples - (int) whole;
}

// normalizeSpherical: phi wrapped to [0, 2 pi) by fmod, theta clipped to [0, limit]
__device__ __forceinline__ void normalize(double &theta, double &phi, double limit) {
    const double r = fmod(phi, 2.0 * kPi);
    phi = r < 0.0 ? 2.0 * kPi + r : r;
    theta = fmax(0.0, fmin(theta, limit));
}

// Minimum over the workgroup of one value per lane (four waves); `slot` [4] in LDS.  Holds one barrier; the caller
// separates two uses of the same slot by another.
__device__ __forceinline__ float block_min(float v, float *slot) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fminf(v, __shfl_xor(v, d));
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    return fminf(fminf(slot[0], slot[1]), fminf(slot[2], slot[3]));
}

}  // namespace

// ---------------------------------------------------------------------------------------
// awpu_hip_steer_table_device: one workgroup per direction, Particle::steer for all n elements.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void steer_table_kernel(const float *xyz, int n, const double *theta, const double *phi,
                                                               int32_t *off, float *frac) {
    __shared__ float lowest_of_wave[4];
    const int d = blockIdx.x;
    const Steer r = steer_of(theta[d], phi[d]);
    float lowest = __builtin_inff();
    for (int i = threadIdx.x; i < n; i += kThreads) lowest = fminf(lowest, raw_delay(r, xyz, n, i));
    lowest = block_min(lowest, lowest_of_wave);
    for (int i = threadIdx.x; i < n; i += kThreads) {  // (recomputed: the same operations give the same bits)
#pragma clang fp contract(off)
        split_delay(raw_delay(r, xyz, n, i) - lowest, off + (size_t) d * n + i, frac + (size_t) d * n + i);
    }
}

hipError_t launch_steer_table(const float *d_xyz, int n, const double *d_theta, const double *d_phi, int n_dir, int32_t *d_off,
                              float *d_frac, hipStream_t stream) {
    hipLaunchKernelGGL(steer_table_kernel, dim3(n_dir), dim3(kThreads), 0, stream, d_xyz, n, d_theta, d_phi, d_off, d_frac);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// The step and the steered beam of the listen kernels at the end of this file, as functions: gradient_track_kernel's
// operations in its order, so a listener carried over blocks on the device ends with the bits the per-block calls of
// awpu_hip_track give.  (gradient_track_kernel below keeps its own statement of them: written through these functions it
// computes the same but parks a seventh scalar register in lanes, and its register allocation is pinned by the tests.
// A change to either is a change to both.)  One workgroup of 256 lanes per particle, lane = output sample.
// ---------------------------------------------------------------------------------------

// beam_sums (das_kernels.h) with the loads of AHEAD mics issued before the first of their sums: the same operations in the
// same order per beam, so the same bits.  A listener's workgroup is alone with its chain of dependent blocks: what bounds it
// is the latency of the L2 reads, which beam_sums' one-mic-at-a-time loop waits out mic by mic.
template <int NB, int AHEAD>
__device__ __forceinline__ void beam_sums_ahead(const float *frame, const LutEntry *rows, size_t row_stride, int usable, int i,
                                                float (&out)[NB]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int q = 0; q < NB; q++) out[q] = 0.0f;
    int s = 0;
    for (; s + AHEAD <= usable; s += AHEAD) {
        float cur[AHEAD][NB], nxt[AHEAD][NB], frac[AHEAD][NB];
#pragma unroll
        for (int k = 0; k < AHEAD; k++)
#pragma unroll
            for (int q = 0; q < NB; q++) {
                const LutEntry e = rows[q * row_stride + s + k];  // uniform
                const float *x = frame + e.off_rel + i;
                cur[k][q] = x[0];
                nxt[k][q] = x[1];
                frac[k][q] = e.frac;
            }
#pragma unroll
        for (int k = 0; k < AHEAD; k++)
#pragma unroll
            for (int q = 0; q < NB; q++) {
                const float d = cur[k][q] - nxt[k][q];
                const float t = __builtin_fmaf(frac[k][q], d, nxt[k][q]);
                out[q] = out[q] + t;
            }
    }
    for (; s < usable; s++) {
#pragma unroll
        for (int q = 0; q < NB; q++) {
            const LutEntry e = rows[q * row_stride + s];
            const float *x = frame + e.off_rel + i;
            const float cur = x[0], nxt = x[1];
            const float d = cur - nxt;
            const float t = __builtin_fmaf(e.frac, d, nxt);
            out[q] = out[q] + t;
        }
    }
}

// LDS of one workgroup beside the entries (dynamic: [4][usable] for the steps, [usable] for a beam alone)
struct TrackLds {
    float line[4][kSamples];
    float partial[4][kSamples / 64];
    float lowest_of_wave[4][4];
    float ref_sum;
    Steer rot[4];
};

// A particle's direction and the outputs of its last step; kept and updated in lanes 0..3 only (each of them does the same
// fp64 operations, so the four copies hold the same bits; the other lanes' copies stay at the initial values and are never read)
struct TrackWalk {
    double theta, phi;
    double g_theta = 0.0, g_phi = 0.0, radius = 0.0;
    float error = 0.0f;
    float pw[4] = {0.0f, 0.0f, 0.0f, 0.0f};
};

// quadrant(): the offsets Spherical(spread, q).toCartesian() for q = 45, 315, 225, 135 degrees; lane l < 4 holds l's
__device__ __forceinline__ void quadrant_offset(double spread, int lane, double (&v)[3]) {
#pragma clang fp contract(off)
    const int q_own = lane & 3;
    const double q_deg = q_own == 0 ? 45.0 : q_own == 1 ? 315.0 : q_own == 2 ? 225.0 : 135.0;
    const double q_rad = q_deg * (kPi / 180.0);
    double s_sp, c_sp, s_q, c_q;
    sincos(spread, &s_sp, &c_sp);
    sincos(q_rad, &s_q, &c_q);
    v[0] = 1.0 * s_sp * c_q;
    v[1] = 1.0 * s_sp * s_q;
    v[2] = 1.0 * c_sp;
}

// the block's reference power (gradient_ascend.cpp:301-313): stream 0 at off = N_SAMPLES, i.e. its samples
// 256..511, sum_{i=1..254} MA^2 in float, in sample order, then / (N_SAMPLES - 2).  Holds one barrier.
__device__ __forceinline__ double block_reference(const float *frame, TrackLds &L, int i) {
#pragma clang fp contract(off)
    if (i == 0) {
        const float *out = frame + kSamples;
        float acc = 0.0f;
        for (int k = 1; k < kSamples - 1; k++) {
            const float ma = out[k] * 0.5f - 0.25f * (out[k + 1] + out[k - 1]);
            const float sq = ma * ma;  // powf(MA, 2): the exact square, rounded once
            acc = acc + sq;
        }
        L.ref_sum = acc / (float) (kSamples - 2);
    }
    __syncthreads();
    return (double) L.ref_sum;
}

// `steps` times GradientParticle::step; per step:
//   a. lane l < 4 computes neighbour l (Spherical::quadrant + normalizeSpherical) and the four steering floats of it,
//      which the workgroup reads from LDS
//   b. the four neighbours' delays over every element, their minima, and the (off, frac) entries of the active mics
//      into LDS
//   c. four beams in one pass over the mics (beam_sums<4>: each in the reference's order) and their powers
//   d. the quadrant gradient in double (gradient_ascend.cpp:53-78, RELATIVE 1)
//   e. Particle::step and normalizeSpherical
// The frame is read straight from L2: a particle's four beams touch 64 x ~260 floats that every particle shares.
template <class Scene>
__device__ __forceinline__ void gradient_steps(const Scene &sc, const float *frame, double reference, double spread, double rate,
                                               int steps, const double (&v)[3], LutEntry *entries, TrackLds &L, int i, TrackWalk &w) {
#pragma clang fp contract(off)
    const int lane = i & 63;
    const int U = sc.usable;
    for (int step = 0; step < steps; step++) {
        if (i < 4) {
            // a. neighbours (geometry.cpp:181-216): the side effect on the particle's own theta first
            double rot_theta = w.theta;
            if (rot_theta + spread > kPi / 2.0) {
                rot_theta -= spread;
                w.theta -= spread / 2.0;
            }
            double ct, st, cp, sp;
            sincos(rot_theta, &st, &ct);
            sincos(w.phi, &sp, &cp);
            // rotateTo: row vector times Ry * Rz, where (Ry Rz) = {{ct cp, -ct sp, st}, {sp, cp, 0}, {-st cp, st sp, ct}}
            const double r00 = ct * cp, r01 = -(ct * sp), r20 = -st * cp, r21 = st * sp;
            const double x = v[0] * r00 + v[1] * sp + v[2] * r20;
            const double y = v[0] * r01 + v[1] * cp + v[2] * r21;
            const double z = v[0] * st + v[2] * ct;
            double n_theta = acos(z), n_phi = atan2(y, x) - kPi;
            normalize(n_theta, n_phi, sc.theta_limit);
            L.rot[i] = steer_of(n_theta, n_phi);
        }
        __syncthreads();  // (also: the previous step's beams are done with the entries)
        Steer r[4];
#pragma unroll
        for (int q = 0; q < 4; q++) r[q] = L.rot[q];

        // b. delays: minima over every element, then the active mics' entries
        float lo[4] = {__builtin_inff(), __builtin_inff(), __builtin_inff(), __builtin_inff()};
        for (int e = i; e < sc.n; e += kThreads)
#pragma unroll
            for (int q = 0; q < 4; q++) lo[q] = fminf(lo[q], raw_delay(r[q], sc.xyz, sc.n, e));
#pragma unroll
        for (int q = 0; q < 4; q++) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) lo[q] = fminf(lo[q], __shfl_xor(lo[q], d));
            if (lane == 0) L.lowest_of_wave[q][i >> 6] = lo[q];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; q++)
            lo[q] = fminf(fminf(L.lowest_of_wave[q][0], L.lowest_of_wave[q][1]), fminf(L.lowest_of_wave[q][2], L.lowest_of_wave[q][3]));
        for (int s = i; s < U; s += kThreads) {
            const int id = sc.index[s];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                int32_t off;
                float frac;
                split_delay(raw_delay(r[q], sc.xyz, sc.n, id) - lo[q], &off, &frac);
                entries[q * U + s] = LutEntry{id * sc.pitch + off, frac};
            }
        }
        __syncthreads();

        // c. the four beams and their powers
        float out[4];
        beam_sums_ahead<4, 4>(frame, entries, (size_t) U, U, i, out);
        beam_powers<4>(out, i, L.line, L.partial, w.pw);

        if (i < 4) {
            // d. gradient (gradient_ascend.cpp:53-78), in double
            const double q1 = w.pw[0], q2 = w.pw[1], q3 = w.pw[2], q4 = w.pw[3];
            const double sum = q1 + q2 + q3 + q4;
            const double d_phi = (q1 + q4) - (q2 + q3);
            const double d_theta = (q3 + q4) - (q1 + q2);
            w.error = (float) ((fabs(d_phi) + fabs(d_theta)) / sum);
            w.g_theta = d_theta / reference;
            w.g_phi = d_phi / reference;
            w.radius = sum / 4;

            // e. Particle::step (particle.cpp:22-27): phi's step uses the updated theta
            w.theta = w.theta + rate * w.g_theta;
            w.phi = w.phi + (rate * w.g_phi) / sin(1e-9 + w.theta);
            normalize(w.theta, w.phi, sc.theta_limit);
        }
    }
}

// Particle::das at lane 0's (theta, phi) (MISOWorker::update, miso.cpp:40-46): this lane's sample of the beam.  The caller
// has passed a barrier since the entries and L.rot were last read; holds three.
template <class Scene>
__device__ __forceinline__ float steered_beam(const Scene &sc, const float *frame, double theta, double phi, LutEntry *entries,
                                              TrackLds &L, int i) {
#pragma clang fp contract(off)
    const int U = sc.usable;
    if (i == 0) L.rot[0] = steer_of(theta, phi);
    __syncthreads();
    const Steer r = L.rot[0];
    float lo = __builtin_inff();
    for (int e = i; e < sc.n; e += kThreads) lo = fminf(lo, raw_delay(r, sc.xyz, sc.n, e));
    lo = block_min(lo, L.lowest_of_wave[0]);
    for (int s = i; s < U; s += kThreads) {
        const int id = sc.index[s];
        int32_t off;
        float frac;
        split_delay(raw_delay(r, sc.xyz, sc.n, id) - lo, &off, &frac);
        entries[s] = LutEntry{id * sc.pitch + off, frac};
    }
    __syncthreads();
    float out[1];
    beam_sums_ahead<1, 16>(frame, entries, 0, U, i, out);
    return out[0];
}

__device__ __forceinline__ void store_walk(awpu_particle_t *P, const TrackWalk &w) {
    P->theta = w.theta;
    P->phi = w.phi;
    P->error = w.error;
    P->grad_theta = w.g_theta;
    P->grad_phi = w.g_phi;
    P->radius = w.radius;
#pragma unroll
    for (int q = 0; q < 4; q++) P->power[q] = w.pw[q];
}

// ---------------------------------------------------------------------------------------
// gradient_track_kernel: one workgroup of 256 lanes per particle, lane = output sample (as das_beam_kernel).  The
// particle's direction and gradient are kept and updated in lanes 0..3 only (each of them does the same fp64
// operations, so the four copies hold the same bits; the other lanes' copies stay at the initial values and are never
// read); per step:
//   a. lane l < 4 computes neighbour l (Spherical::quadrant + normalizeSpherical) and the four steering floats of it,
//      which the workgroup reads from LDS
//   b. the four neighbours' delays over every element, their minima, and the (off, frac) entries of the active mics
//      into LDS
//   c. four beams in one pass over the mics (beam_sums<4>: each in the reference's order) and their powers
//   d. the quadrant gradient in double (gradient_ascend.cpp:53-78, RELATIVE 1)
//   e. Particle::step and normalizeSpherical
// The frame is read straight from L2: a particle's four beams touch 64 x ~260 floats that every particle shares.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void gradient_track_kernel(TrackArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) LutEntry entries[];  // [4][usable]
    __shared__ float line[4][kSamples];
    __shared__ float partial[4][kSamples / 64];
    __shared__ float lowest_of_wave[4][4];
    __shared__ float ref_sum;
    __shared__ Steer rot[4];
    // What only the end of the kernel needs -- the particle's address and its beam row -- waits in LDS: held in scalar
    // registers over the step loop, where the fp64 libm calls use nearly all of them, these pointers were spilled
    __shared__ awpu_particle_t *particle;
    __shared__ float *beams_out;
    const int i = threadIdx.x;
    const int lane = i & 63;
    awpu_particle_t *P = static_cast<awpu_particle_t *>(a.particles) + blockIdx.x;
    if (i == 0) {
        particle = P;
        beams_out = a.beams ? a.beams + (size_t) blockIdx.x * kSamples : nullptr;
    }

    // the block's reference power (gradient_ascend.cpp:301-313): stream 0 at off = N_SAMPLES, i.e. its samples
    // 256..511, sum_{i=1..254} MA^2 in float, in sample order, then / (N_SAMPLES - 2)
    double reference = a.reference;
    if (!(reference > 0.0)) {
        if (i == 0) {
            const float *out = a.frame + kSamples;
            float acc = 0.0f;
            for (int k = 1; k < kSamples - 1; k++) {
                const float ma = out[k] * 0.5f - 0.25f * (out[k + 1] + out[k - 1]);
                const float sq = ma * ma;  // powf(MA, 2): the exact square, rounded once
                acc = acc + sq;
            }
            ref_sum = acc / (float) (kSamples - 2);
        }
        __syncthreads();
        reference = (double) ref_sum;
    }
    if (blockIdx.x == 0 && i == 0 && a.reference_out) *a.reference_out = reference;

    double theta = P->theta, phi = P->phi;
    const double spread = P->spread, rate = P->rate;
    const int steps = P->steps;
    const int U = a.usable;

    // quadrant(): the offsets Spherical(spread, q).toCartesian() for q = 45, 315, 225, 135 degrees; lane l < 4 holds l's
    const int q_own = lane & 3;
    const double q_deg = q_own == 0 ? 45.0 : q_own == 1 ? 315.0 : q_own == 2 ? 225.0 : 135.0;
    const double q_rad = q_deg * (kPi / 180.0);
    double s_sp, c_sp, s_q, c_q;
    sincos(spread, &s_sp, &c_sp);
    sincos(q_rad, &s_q, &c_q);
    const double v0 = 1.0 * s_sp * c_q, v1 = 1.0 * s_sp * s_q, v2 = 1.0 * c_sp;

    // The direction and the gradient live in lanes 0..3 (the same bits in each); the rest of the workgroup sees only
    // the steering floats and the powers.
    float pw[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    double g_theta = 0.0, g_phi = 0.0, radius = 0.0;
    float error = 0.0f;
    for (int step = 0; step < steps; step++) {
        if (i < 4) {
            // a. neighbours (geometry.cpp:181-216): the side effect on the particle's own theta first
            double rot_theta = theta;
            if (rot_theta + spread > kPi / 2.0) {
                rot_theta -= spread;
                theta -= spread / 2.0;
            }
            double ct, st, cp, sp;
            sincos(rot_theta, &st, &ct);
            sincos(phi, &sp, &cp);
            // rotateTo: row vector times Ry * Rz, where (Ry Rz) = {{ct cp, -ct sp, st}, {sp, cp, 0}, {-st cp, st sp, ct}}
            const double r00 = ct * cp, r01 = -(ct * sp), r20 = -st * cp, r21 = st * sp;
            const double x = v0 * r00 + v1 * sp + v2 * r20;
            const double y = v0 * r01 + v1 * cp + v2 * r21;
            const double z = v0 * st + v2 * ct;
            double n_theta = acos(z), n_phi = atan2(y, x) - kPi;
            normalize(n_theta, n_phi, a.theta_limit);
            rot[i] = steer_of(n_theta, n_phi);
        }
        __syncthreads();  // (also: the previous step's beams are done with the entries)
        Steer r[4];
#pragma unroll
        for (int q = 0; q < 4; q++) r[q] = rot[q];

        // b. delays: minima over every element, then the active mics' entries
        float lo[4] = {__builtin_inff(), __builtin_inff(), __builtin_inff(), __builtin_inff()};
        for (int e = i; e < a.n; e += kThreads)
#pragma unroll
            for (int q = 0; q < 4; q++) lo[q] = fminf(lo[q], raw_delay(r[q], a.xyz, a.n, e));
#pragma unroll
        for (int q = 0; q < 4; q++) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) lo[q] = fminf(lo[q], __shfl_xor(lo[q], d));
            if (lane == 0) lowest_of_wave[q][i >> 6] = lo[q];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; q++)
            lo[q] = fminf(fminf(lowest_of_wave[q][0], lowest_of_wave[q][1]), fminf(lowest_of_wave[q][2], lowest_of_wave[q][3]));
        for (int s = i; s < U; s += kThreads) {
            const int id = a.index[s];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                int32_t off;
                float frac;
                split_delay(raw_delay(r[q], a.xyz, a.n, id) - lo[q], &off, &frac);
                entries[q * U + s] = LutEntry{id * a.pitch + off, frac};
            }
        }
        __syncthreads();

        // c. the four beams and their powers
        float out[4];
        beam_sums<4>(a.frame, entries, (size_t) U, U, i, out);
        beam_powers<4>(out, i, line, partial, pw);

        if (i < 4) {
            // d. gradient (gradient_ascend.cpp:53-78), in double
            const double q1 = pw[0], q2 = pw[1], q3 = pw[2], q4 = pw[3];
            const double sum = q1 + q2 + q3 + q4;
            const double d_phi = (q1 + q4) - (q2 + q3);
            const double d_theta = (q3 + q4) - (q1 + q2);
            error = (float) ((fabs(d_phi) + fabs(d_theta)) / sum);
            g_theta = d_theta / reference;
            g_phi = d_phi / reference;
            radius = sum / 4;

            // e. Particle::step (particle.cpp:22-27): phi's step uses the updated theta
            theta = theta + rate * g_theta;
            phi = phi + (rate * g_phi) / sin(1e-9 + theta);
            normalize(theta, phi, a.theta_limit);
        }
    }

    __syncthreads();
    float *const beams = beams_out;
    if (beams) {  // Particle::das at the final direction (MISOWorker::update, miso.cpp:40-46)
        if (i == 0) rot[0] = steer_of(theta, phi);
        __syncthreads();
        const Steer r = rot[0];
        float lo = __builtin_inff();
        for (int e = i; e < a.n; e += kThreads) lo = fminf(lo, raw_delay(r, a.xyz, a.n, e));
        lo = block_min(lo, lowest_of_wave[0]);
        for (int s = i; s < U; s += kThreads) {
            const int id = a.index[s];
            int32_t off;
            float frac;
            split_delay(raw_delay(r, a.xyz, a.n, id) - lo, &off, &frac);
            entries[s] = LutEntry{id * a.pitch + off, frac};
        }
        __syncthreads();
        float out[1];
        beam_sums<1>(a.frame, entries, 0, U, i, out);
        beams[i] = out[0];
    }

    if (i == 0 && steps > 0) {
        P = particle;
        P->theta = theta;
        P->phi = phi;
        P->error = error;
        P->grad_theta = g_theta;
        P->grad_phi = g_phi;
        P->radius = radius;
#pragma unroll
        for (int q = 0; q < 4; q++) P->power[q] = pw[q];
    }
}

// ---------------------------------------------------------------------------------------
// listen_blocks_kernel / listen_fixed_kernel: MISOWorker::update (src/dsp/miso.cpp:27-55) for every block of a sweep
// piece's history (block_kernels.h: snapshot k starts at history sample 256 * k).  Per block: the reference power from
// the block's own snapshot if asked, the listener's steps, Particle::das at where it then points -- 256 samples of its
// audio row -- and its state into the trail.
//   tracking listeners (steps > 0) are sequential over blocks: one workgroup per listener walks the piece, the direction
//   in registers from block to block and in a.listeners between pieces and calls
//   fixed listeners (steps == 0) are not: one workgroup per (block, listener)
// Each kernel is launched over all listeners and leaves the other kind's at once.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void listen_blocks_kernel(ListenArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) LutEntry entries[];  // [4][usable]
    __shared__ TrackLds L;
    const int i = threadIdx.x;
    awpu_particle_t *const P = static_cast<awpu_particle_t *>(a.listeners) + blockIdx.x;
    const int steps = P->steps;
    if (steps == 0) return;
    TrackWalk w;
    w.theta = P->theta;
    w.phi = P->phi;
    const double spread = P->spread, rate = P->rate;
    double v[3];
    quadrant_offset(spread, i & 63, v);
    for (int k = 0; k < a.n_blocks; k++) {
        const float *frame = a.hist + (size_t) kSamples * k;
        double reference = a.reference;
        if (!(reference > 0.0)) reference = block_reference(frame, L, i);
        gradient_steps(a, frame, reference, spread, rate, steps, v, entries, L, i, w);
        __syncthreads();
        a.audio[(size_t) blockIdx.x * a.audio_pitch + (size_t) kSamples * k + i] = steered_beam(a, frame, w.theta, w.phi, entries, L, i);
        if (i == 0 && a.trail) {
            awpu_particle_t *T = static_cast<awpu_particle_t *>(a.trail) + (size_t) k * a.n_listeners + blockIdx.x;
            T->spread = spread;
            T->rate = rate;
            T->steps = steps;
            store_walk(T, w);
        }
    }
    if (i == 0) store_walk(P, w);
}

__global__ __launch_bounds__(kThreads) void listen_fixed_kernel(ListenArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) LutEntry entries[];  // [usable]
    __shared__ TrackLds L;
    const int i = threadIdx.x, k = blockIdx.x, l = blockIdx.y;
    const awpu_particle_t *const P = static_cast<const awpu_particle_t *>(a.listeners) + l;
    if (P->steps != 0) return;
    const float *frame = a.hist + (size_t) kSamples * k;
    a.audio[(size_t) l * a.audio_pitch + (size_t) kSamples * k + i] = steered_beam(a, frame, P->theta, P->phi, entries, L, i);
    if (a.trail && i < (int) (sizeof(awpu_particle_t) / sizeof(uint32_t)))  // untouched, as awpu_hip_track leaves steps == 0
        reinterpret_cast<uint32_t *>(static_cast<awpu_particle_t *>(a.trail) + (size_t) k * a.n_listeners + l)[i] =
            reinterpret_cast<const uint32_t *>(P)[i];
}

size_t track_lds_bytes(int usable) { return (size_t) 4 * usable * sizeof(LutEntry); }

hipError_t launch_track(const TrackArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(gradient_track_kernel, dim3(a.n_particles), dim3(kThreads), track_lds_bytes(a.usable), stream, a);
    return hipGetLastError();
}

hipError_t launch_listen(const ListenArgs &a, bool tracking, bool fixed, hipStream_t stream) {
    // every window a beam reads ([256 - d, 512 - d] of snapshot k, d in [0, 256]) lies inside the piece's history
    if (a.n_blocks < 1 || a.n_blocks > 65535 || a.n_listeners < 1 || a.n_listeners > 65535 || a.usable < 1 ||
        a.pitch < kBlockPrefix + kSamples * a.n_blocks || a.audio_pitch < (long long) kSamples * a.n_blocks)
        return hipErrorInvalidValue;
    if (tracking)
        hipLaunchKernelGGL(listen_blocks_kernel, dim3(a.n_listeners), dim3(kThreads), track_lds_bytes(a.usable), stream, a);
    if (fixed)
        hipLaunchKernelGGL(listen_fixed_kernel, dim3(a.n_blocks, a.n_listeners), dim3(kThreads), (size_t) a.usable * sizeof(LutEntry),
                           stream, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// range_kernel: awpu_hip_range (include/awpu_hip_focus.h).  One workgroup of 256 lanes, lane = output sample, per (source, four
// consecutive candidate distances); the whole n_src x n_dist sweep is one launch.  Per candidate the delays of every element are
// formed on the device -- the focus rule's doubles (focus_rule.h: the host's expressions, contraction off) and the longest path
// over all elements, or, for a candidate at infinity, steer_table_kernel's plane wave -- and the active mics' entries go to LDS;
// then the four beams in one pass over the mics (beam_sums<4>: each in the reference's order, the four windows of a mic's row
// overlapping in the cache) and their powers (beam_powers), which are das_beam_kernel's operations: the bits awpu_hip_beams
// gives for awpu_hip_focus_steer_table's entries.  Candidates past n_dist repeat the last one and are not written.  The frame
// is read straight from L2, as the trackers read it.  Plain stores, no atomics.
// ---------------------------------------------------------------------------------------
constexpr int kRangeBeams = 4;

__global__ __launch_bounds__(kThreads) void range_kernel(RangeArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) LutEntry entries[];  // [4][usable]
    __shared__ float line[kRangeBeams][kSamples];
    __shared__ float partial[kRangeBeams][kSamples / 64];
    __shared__ float lowest_of_wave[4];
    __shared__ double far_of_wave[4];
    const int i = threadIdx.x, k = blockIdx.y, j0 = blockIdx.x * kRangeBeams;
    const int U = a.usable, n = a.n;
    float *const row = a.power + (size_t) k * a.n_dist;
    double theta, phi;
    if (a.sources) {  // a run's own sources: an unused entry has no direction
        const awpu_source_t *src = static_cast<const awpu_source_t *>(a.sources) + k;
        if (src->pixel < 0) {
            if (i < kRangeBeams && j0 + i < a.n_dist) row[j0 + i] = 0.0f;
            return;
        }
        theta = src->theta, phi = src->phi;
    } else {
        theta = a.theta[k], phi = a.phi[k];
    }
    const float *frame = a.frame + (long long) (k / a.per_frame) * a.frame_step;
    const Steer r = steer_of(theta, phi);
    const float m[12] = {r.cz, -r.sz, 0.0f, r.sz, r.cz, 0.0f, 0.0f, 0.0f, 1.0f, -r.sy, 0.0f, r.cy};  // pixel_rotations' layout
    double w[3];
    focus_direction(m, w);

    for (int q = 0; q < kRangeBeams; q++) {
        const double distance = a.distance[min(j0 + q, a.n_dist - 1)];
        if (focus_is_plane_wave(distance)) {  // steer_table_kernel
            float lo = __builtin_inff();
            for (int e = i; e < n; e += kThreads) lo = fminf(lo, raw_delay(r, a.xyz, n, e));
            lo = block_min(lo, lowest_of_wave);
            for (int s = i; s < U; s += kThreads) {
                const int id = a.index[s];
                int32_t off;
                float frac;
                split_delay(raw_delay(r, a.xyz, n, id) - lo, &off, &frac);
                entries[q * U + s] = LutEntry{id * a.pitch + off, frac};
            }
        } else {
            double F[3];
            focus_point(w, distance, F);
            double far = 0.0;
            for (int e = i; e < n; e += kThreads) far = fmax(far, focus_path(F, a.xyz[e], a.xyz[n + e], a.xyz[2 * n + e]));
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) far = fmax(far, __shfl_xor(far, d));
            if ((i & 63) == 0) far_of_wave[i >> 6] = far;
            __syncthreads();
            far = fmax(fmax(far_of_wave[0], far_of_wave[1]), fmax(far_of_wave[2], far_of_wave[3]));
            for (int s = i; s < U; s += kThreads) {
                const int id = a.index[s];
                int32_t off;
                float frac;
                split_delay(focus_delay(far, focus_path(F, a.xyz[id], a.xyz[n + id], a.xyz[2 * n + id])), &off, &frac);
                entries[q * U + s] = LutEntry{id * a.pitch + off, frac};
            }
        }
        __syncthreads();  // the reduction slots are free for the next candidate; after the last: the entries are there
    }

    float out[kRangeBeams], pw[kRangeBeams];
    beam_sums<kRangeBeams>(frame, entries, (size_t) U, U, i, out);
    beam_powers<kRangeBeams>(out, i, line, partial, pw);
    if (i < kRangeBeams && j0 + i < a.n_dist) row[j0 + i] = i == 0 ? pw[0] : i == 1 ? pw[1] : i == 2 ? pw[2] : pw[3];
}

// awpu_hip_range_pick on the device for a run's ranges: one lane per source, the host definition's own expressions
__global__ void range_pick_kernel(RangeArgs a) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.n_src) return;
    awpu_range_t *out = static_cast<awpu_range_t *>(a.best) + k;
    if (a.sources && static_cast<const awpu_source_t *>(a.sources)[k].pixel < 0) {
        range_unused(out);
        return;
    }
    range_pick_one(a.power + (size_t) k * a.n_dist, a.distance, a.n_dist, out);
}

hipError_t launch_range(const RangeArgs &a, hipStream_t stream) {
    // every window a beam reads ([256 - d, 512 - d] of its snapshot, d in [0, 256]) lies inside the frame: the callers' business
    if (!a.frame || !a.xyz || !a.index || !a.power || (!a.sources && (!a.theta || !a.phi)) || a.n_src < 1 || a.n_src > 65535 || a.n_dist < 1 ||
        a.n_dist > AWPU_RANGE_MAX_CANDIDATES || a.usable < 1 || a.n < 1 || a.per_frame < 1)
        return hipErrorInvalidValue;
    for (int j = 0; j < a.n_dist; j++)
        if (!focus_distance_ok(a.distance[j])) return hipErrorInvalidValue;
    hipLaunchKernelGGL(range_kernel, dim3((a.n_dist + kRangeBeams - 1) / kRangeBeams, a.n_src), dim3(kThreads), track_lds_bytes(a.usable), stream, a);
    if (a.best) hipLaunchKernelGGL(range_pick_kernel, dim3((a.n_src + 63) / 64), dim3(64), 0, stream, a);
    return hipGetLastError();
}

}  // namespace awpu
