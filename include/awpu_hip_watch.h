/*
 * awpu_hip_watch.h -- watching a run of consecutive blocks (a recording, a backlog): the display images of every Nth block --
 * the compact 8-bit heatmap and, on request, the large image a GUI shows or a video writer records: upscaled, colour-mapped,
 * mirrored -- in batched passes.  Every block is ingested; only the blocks that are shown are swept.
 *
 * Replaces (file:line relative to the reference tree) the per-frame display chain of the reference:
 *   MIMOWorker::populateHeatmap        src/dsp/mimo.cpp:61-95     (per-frame maximum, 8-bit levels)
 *   AWProcessingUnit::draw             src/aw_processing_unit/aw_processing_unit.cpp:245-259   (cv::resize, INTER_LINEAR)
 *   the GUI loop                       src/aw_control_unit/aw_control_unit.cpp:293-378   (cv::applyColorMap, cv::flip(frame, frame, 1),
 *                                      videoWriter.write: the newest heatmap once per GUI frame, not once per block)
 * over what awpu_hip_blocks.h replaces (Worker::loop, Streams::write_stream / read_stream, Pipeline::receive_exposure).
 * Not here: the overlays other workers draw, the circular mask, camera blending, hconcat, MJPG encoding.
 *
 * Definition of the result.  With n_frames and next_first as awpu_hip_watch_count gives them, frame j shows block
 * b_j = first + j * every of the call (j < n_frames, b_j < n_blocks).
 *   - ALL n_blocks blocks are appended to the handle's ingest ring (awpu_hip.h), shown or not.  After the call the ring,
 *     awpu_hip_ring_snapshot, awpu_hip_process_ring and awpu_hip_live_block are where n_blocks calls of awpu_hip_ingest_block
 *     would have left them.  A recording split over several calls (each continuing with the `next_first` of the one before), or
 *     mixed with the calls of awpu_hip_blocks.h, awpu_hip_listen.h and the live calls, gives the same frames.  A call with
 *     n_frames == 0 (first >= n_blocks) is valid: it ingests, and writes nothing.
 *   - Only the shown snapshots -- the last 1024 samples of every stream after block b_j, oldest first -- are swept.  They are
 *     swept in order, in chunks of at most cfg.max_batch, each chunk exactly as awpu_hip_process sweeps a batch of those
 *     snapshots: `power` row j equals that call's bits in every math mode and interpolation, and in AWPU_MATH_F32_EXACT also row
 *     b_j of awpu_hip_process_blocks and of the per-block loop.  awpu_hip_get_stats counts shown frames (and their launches) only.
 *   - `image` row j == awpu_hip_heatmap_u8 of `power` row j (per-frame maximum; the all-zero frame gives an all-zero image).
 *     `big_image` row j == awpu_hip_upscale_u8_device of that image (rows x cols -> out_rows x out_cols) through d_colormap,
 *     then mirrored left-right when `flip` -- bit for bit.  In the exact mode rows j are therefore the `image` / `big_image`
 *     that awpu_hip_live_block returns for block b_j of the per-block loop.
 *
 * Requirements: those of awpu_hip_process_blocks -- cfg.hist == AWPU_HIST (AWPU_ERR_INVALID otherwise), the delay table and the
 * active-mic list set (and the FIR table for AWPU_INTERP_FIR8: AWPU_ERR_STATE otherwise), n_blocks >= 1, cfg.n_streams <= 256
 * for the wire form, a device-group handle refused with AWPU_ERR_STATE -- and those of awpu_hip_live_block: the whole grid on
 * the handle (cfg.pixel_count == cfg.n_pixels) and rows * cols == cfg.n_pixels, AWPU_ERR_INVALID otherwise.  every in
 * [1, 1024], first >= 0, flip 0 or 1, rows and cols >= 1; when big_image is asked for, out_rows >= rows, out_cols >= cols and
 * cols <= AWPU_WATCH_MAX_COLS.  Argument errors are reported before the handle is touched; on any error the ring is left as
 * it was.
 *
 * Memory.  A sweep piece is at most cfg.max_batch frames (awpu_hip_process's own pieces: a quarter of a batch of 128 and
 * more).  The device holds two pieces' worth of: the samples the piece's snapshots read -- 3 + 1 + min(every, 4) * (piece - 1)
 * blocks of every stream: with every = 1 one new block per frame, from every = 4 on four, the whole snapshot, and no more
 * however large `every` is -- their powers, their images; the host forms hold pinned buffers of the same sizes for the way
 * in and the way back.  Skipped blocks that no shown snapshot reads never reach the device, except the last four of a call,
 * which the ring needs.  None of it grows with n_blocks.
 *
 * Conventions are those of awpu_hip.h (status codes, host pointers owned by the caller, one thread per handle).
 */
#ifndef AWPU_HIP_WATCH_H
#define AWPU_HIP_WATCH_H

#include "awpu_hip_blocks.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AWPU_WATCH_MAX_EVERY 1024
#define AWPU_WATCH_MAX_COLS 3584 /* the 18 compact rows a 16-row tile of the large image can read stay in 63 KB of LDS */

/* Which blocks of a call are shown, and how. */
typedef struct awpu_watch {
    int32_t first, every;        /* blocks first, first + every, ... (< n_blocks) of the call are shown */
    int32_t rows, cols;          /* the compact image; rows * cols == cfg.n_pixels */
    int32_t out_rows, out_cols;  /* the large image, each >= rows / cols; used only when a large image is asked for */
    int32_t flip;                /* 0 | 1: cv::flip(frame, frame, 1) of the LARGE image (aw_control_unit.cpp:376-378) */
    const uint8_t *d_colormap;   /* device memory [256][3] as awpu_hip_upscale_u8_device takes it, or NULL = one channel */
} awpu_watch_t;

/* Pure host arithmetic, no handle: how many frames a call of n_blocks blocks shows, and the `first` of the call that continues
 * it.  n_frames = 0 when first >= n_blocks, else (n_blocks - first + every - 1) / every; next_first = first + n_frames * every -
 * n_blocks.  n_blocks >= 1, first >= 0, every >= 1, both outputs non-null: AWPU_ERR_INVALID otherwise. */
int awpu_hip_watch_count(int32_t n_blocks, int32_t first, int32_t every, int32_t *n_frames, int32_t *next_first);

/* n_blocks x 256 wire datagrams (host, as awpu_hip_process_blocks takes them) -> each may be NULL, at least one is not:
 *   image      [n_frames][rows * cols] bytes (host)
 *   big_image  [n_frames][out_rows][out_cols] bytes, x 3 with a colour table (host)
 *   power      [n_frames][pixel_count] floats (host)
 * Synchronous; the datagrams, the images and the powers cross PCIe through pinned buffers of the handle, piece p's way back
 * while piece p + 1 is swept.  Ordered after everything already enqueued on the handle's stream. */
int awpu_hip_watch_blocks(awpu_hip_t *h, const void *datagrams, int32_t stride_bytes, int32_t n_blocks, const awpu_watch_t *w,
                          uint8_t *image, uint8_t *big_image, float *power);

/* The same from unpacked samples [n_streams][pitch] floats (host), as awpu_hip_process_samples takes them: pitch >= 256 *
 * n_blocks, any n_streams.  Synchronous. */
int awpu_hip_watch_samples(awpu_hip_t *h, const float *samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w, uint8_t *image,
                           uint8_t *big_image, float *power);

/* The same on device buffers: d_samples, d_image, d_big_image and d_power in device memory, enqueued on `stream` (a hipStream_t,
 * NULL = the handle's own; awpu_hip.h, "Streams") in the order of awpu_hip_process_samples_device; asynchronous.  Later calls on the handle's ring are
 * ordered after it.  Nothing crosses PCIe. */
int awpu_hip_watch_samples_device(awpu_hip_t *h, const float *d_samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                                  uint8_t *d_image, uint8_t *d_big_image, float *d_power, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AWPU_HIP_WATCH_H */
