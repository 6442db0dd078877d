/*
 * awpu_hip_blocks.h -- one heatmap for every block of a run of consecutive blocks (a recording, a backlog) in batched sweeps.
 *
 * Replaces (file:line relative to the reference tree) the per-block loop of the reference:
 *   Worker::loop                       src/dsp/worker.h:212-224   (one snapshot and one MIMOWorker::update per block)
 *   Streams::write_stream / forward    src/fpga/streams.hpp:103-105, :136-139  (the block appended to every stream)
 *   Streams::read_stream               src/fpga/streams.hpp:113-116  (the snapshot: the last 1024 samples, oldest first)
 *   Pipeline::receive_exposure         src/fpga/pipeline.cpp:260-297 (the wire format: column flip, 2^-23 scale)
 * and what the reference's offline workflow feeds them: recorded FPGA datagrams replayed (udp/README.md).
 *
 * Row k of `power` is the heatmap of the snapshot after block k of the call has been appended: the last 1024 samples of every
 * stream, oldest first -- what awpu_hip_process_ring returns after k + 1 calls of awpu_hip_ingest_block.  The calls append to
 * the handle's ingest ring (awpu_hip.h): the first snapshots of a call see the samples the ring held before it (the ring
 * starts zeroed), and afterwards the ring, awpu_hip_ring_snapshot, awpu_hip_process_ring and awpu_hip_live_block are where
 * n_blocks ingests would have left them.  A recording may therefore be split over several calls, or followed by live calls,
 * and its heatmaps do not change.
 *
 * Every new sample crosses PCIe once; the overlapping snapshots are formed on the device and swept by the batched sweeps of
 * awpu_hip_process, unchanged.  The run is cut into chunks of at most cfg.max_batch blocks, one batch each (the caller sizes
 * the device memory by max_batch, and the sweep takes no more per launch): a handle with max_batch = 1 sweeps one frame per
 * launch, like the live loop.  A chunk of n frames is swept exactly as awpu_hip_process sweeps a batch of n frames, so
 * row k equals, bit for bit, awpu_hip_process of the same snapshots in batches cut the same way, in every math mode and
 * interpolation; in AWPU_MATH_F32_EXACT (the default) it also equals the per-block loop (a frame swept alone gives the bits
 * it gives in a batch).  awpu_hip_get_stats counts the frames and the launches.
 *
 * Requirements: cfg.hist == AWPU_HIST (AWPU_ERR_INVALID otherwise), the delay table and the active-mic list set (and the FIR
 * table for AWPU_INTERP_FIR8: AWPU_ERR_STATE otherwise), n_blocks >= 1.  A device-group handle (cfg.n_devices > 1) is
 * refused with AWPU_ERR_STATE.  Argument errors are reported before the handle is touched; on any error the ring is left
 * as it was.
 *
 * Conventions are those of awpu_hip.h (status codes, host pointers owned by the caller, one thread per handle).
 */
#ifndef AWPU_HIP_BLOCKS_H
#define AWPU_HIP_BLOCKS_H

#include "awpu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* n_blocks x 256 wire datagrams (host memory, stride_bytes >= AWPU_DATAGRAM_BYTES apart, block after block, each block as
 * awpu_hip_ingest_block takes it) -> power [n_blocks][pixel_count] (host).  cfg.n_streams <= 256 (the wire carries 256
 * slots).  Synchronous; the datagrams and the powers cross PCIe through pinned buffers of the handle, the next sweep piece's
 * while one is swept.  A host-form call is ordered after everything already enqueued on the handle's stream. */
int awpu_hip_process_blocks(awpu_hip_t *h, const void *datagrams, int32_t stride_bytes, int32_t n_blocks, float *power);

/* The same from unpacked samples, as Streams::write_stream receives them: samples [n_streams][pitch] floats (host), the
 * first n_blocks * 256 of every row are the new samples, oldest first; pitch >= n_blocks * 256.  Any n_streams (512 mics:
 * two FPGAs).  Synchronous. */
int awpu_hip_process_samples(awpu_hip_t *h, const float *samples, int64_t pitch, int32_t n_blocks, float *power);

/* The same on device buffers: d_samples [n_streams][pitch] floats, d_power [n_blocks][pixel_count], enqueued on `stream`
 * (a hipStream_t, NULL = the handle's own; awpu_hip.h, "Streams"); asynchronous like awpu_hip_process_device.  Later calls on the handle's ring
 * are ordered after it. */
int awpu_hip_process_samples_device(awpu_hip_t *h, const float *d_samples, int64_t pitch, int32_t n_blocks, float *d_power,
                                    void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AWPU_HIP_BLOCKS_H */
