/*
 * awpu_hip_listen.h -- listening to a run of consecutive blocks (a recording, a backlog): for every block the delayed-and-summed
 * signal of steered directions that may follow their sources, and on request the heatmaps of the same blocks in the same pass.
 *
 * Replaces (file:line relative to the reference tree) the per-block loop of the reference's --miso mode:
 *   MISOWorker::update / steer         src/dsp/miso.cpp:27-55   (reference power, 3 gradient steps, das of the tracked direction)
 *   GradientParticle::step, Particle::das   src/dsp/gradient_ascend.cpp:30-81, src/dsp/particle.cpp:22-27, :37-103
 *   AudioWrapper                       src/audio/audio_wrapper.cpp:34-36, :76   (the blocks laid end to end at 48 828 Hz)
 * over what awpu_hip_blocks.h replaces (Worker::loop, Streams::write_stream / read_stream, Pipeline::receive_exposure).
 *
 * Definition of the result.  With p = the listeners as passed, for block k = 0 .. n_blocks - 1 of the call:
 *       awpu_hip_ingest_block(h, block k);
 *       awpu_hip_track(h, NULL, p, n, theta_limit, reference, NULL, beams);
 *   audio[l * audio_pitch + 256 * k + i] == beams[l * 256 + i], trail[k * n + l] == p[l] after that call, and `listeners`
 *   on return == p after the last block -- bit for bit.  In words: per block, listener l takes listeners[l].steps gradient
 *   steps on the snapshot after the block was appended (steps == 0: a fixed, steered listener, MISOWorker::steer without
 *   tracking; its state is left as passed), then Particle::das at where it points is its audio for that block.  The window a
 *   beam reads moves by 256 samples per block, so a listener's row is continuous audio: a playable channel.  (A beam reads
 *   samples [256 - d, 512 - d] of the 1024-sample snapshot, d its delay, and the snapshot after block k holds blocks k-3 .. k: row
 *   k is the recording two blocks before block k.  With every delay 0 it is samples 1 .. 256 of block k-2: delay() with fraction
 *   0 returns signal[i + 1], src/dsp/delay.cpp:16-26.  The reference never applies its `norm`: the sum is not divided by the
 *   number of mics.)
 *   `power`, when asked for, is what awpu_hip_process_blocks returns for the same run, bit for bit, in every math mode.
 *
 * The calls append to the handle's ingest ring exactly as the calls of awpu_hip_blocks.h do: a recording may be split over
 * several calls, or mixed with awpu_hip_process_blocks, awpu_hip_ingest_block and the live calls, and neither the audio, the
 * trail nor the ring changes.  The listeners' in/out state is what carries a tracker from one call to the next.  Inside a call
 * the directions stay on the device: every new sample crosses PCIe once, audio and trail come back through pinned memory.
 *
 * A hazard that follows from the definition: the beams and the reference power (reference <= 0: stream 0's samples 256..511 of
 * each block's own snapshot, miso.cpp:31-38) read the OLDEST half of the snapshot.  On a new handle the ring is zeroed, so for
 * the first blocks the reference power is 0, the relative gradient is x / 0, and a tracking listener's direction becomes NaN
 * -- in the per-block loop just the same, whose next awpu_hip_track call then refuses the NaN direction.  A listen call carries
 * the NaN (and NaN audio) to its end, and the next call refuses such a listener.  Listen to the first few blocks with steps = 0
 * (tools/pcap_listen.py --settle), or pass a positive `reference`.
 *
 * Requirements: those of awpu_hip_track -- the antenna set (AWPU_ERR_STATE otherwise), the active mics set and inside the
 * antenna, finite directions, spreads and rates, steps in [0, 4096], n in [1, 65535], theta_limit finite and > 0, reference
 * finite -- and those of the block calls: cfg.hist == AWPU_HIST, n_blocks >= 1, cfg.n_streams <= 256 for the wire form; a
 * device-group handle is refused with AWPU_ERR_STATE.  The delay table (and the FIR table) is needed only when power != NULL:
 * without it no window is cut, nothing is swept and awpu_hip_get_stats counts nothing.  Argument errors are reported before
 * the handle is touched; on any error the ring and `listeners` are left as they were.
 *
 * Conventions are those of awpu_hip.h (status codes, host pointers owned by the caller, one thread per handle).
 */
#ifndef AWPU_HIP_LISTEN_H
#define AWPU_HIP_LISTEN_H

#include "awpu_hip_blocks.h"
#include "awpu_hip_track.h"

#ifdef __cplusplus
extern "C" {
#endif

/* n_blocks x 256 wire datagrams (host, as awpu_hip_process_blocks takes them) ->
 *   listeners  [n], in/out (awpu_hip_track.h); steps = gradient steps PER BLOCK (MISOWorker: 3, rate PARTICLE_RATE / 10)
 *   theta_limit, reference   as in awpu_hip_track; reference <= 0: from each block's own snapshot, which is what MISO does
 *   audio      [n][audio_pitch] floats (host), audio_pitch >= 256 * n_blocks; the first 256 * n_blocks of every row are written
 *   trail      (may be NULL) [n_blocks][n]: every listener after every block -- direction, gradient, error, the four powers
 *   power      (may be NULL) [n_blocks][pixel_count]: the heatmaps of awpu_hip_process_blocks
 * Synchronous. */
int awpu_hip_listen_blocks(awpu_hip_t *h, const void *datagrams, int32_t stride_bytes, int32_t n_blocks, awpu_particle_t *listeners,
                           int32_t n, double theta_limit, double reference, float *audio, int64_t audio_pitch, awpu_particle_t *trail,
                           float *power);

/* The same from unpacked samples [n_streams][pitch] floats (host), as awpu_hip_process_samples takes them.  Any n_streams.
 * Synchronous. */
int awpu_hip_listen_samples(awpu_hip_t *h, const float *samples, int64_t pitch, int32_t n_blocks, awpu_particle_t *listeners, int32_t n,
                            double theta_limit, double reference, float *audio, int64_t audio_pitch, awpu_particle_t *trail,
                            float *power);

/* The same on device buffers: d_samples, d_audio [n][audio_pitch], d_trail (may be NULL) and d_power (may be NULL) in device
 * memory, written on `stream` (a hipStream_t, NULL = the handle's own; awpu_hip.h, "Streams") in the order of awpu_hip_process_samples_device; later
 * calls on the handle's ring are ordered after it.  `listeners` is host memory like everywhere else: it is checked and uploaded
 * before anything is enqueued, and the call returns once the listeners' final state has been read back (80 bytes each), i.e.
 * after the work it enqueued on `stream`; no sample, audio or power crosses PCIe. */
int awpu_hip_listen_samples_device(awpu_hip_t *h, const float *d_samples, int64_t pitch, int32_t n_blocks, awpu_particle_t *listeners,
                                   int32_t n, double theta_limit, double reference, float *d_audio, int64_t audio_pitch,
                                   awpu_particle_t *d_trail, float *d_power, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AWPU_HIP_LISTEN_H */
