#!/usr/bin/env python3
"""How fast a recording is watched (include/awpu_hip_watch.h), default math, one JSON line per measurement:

  --host     per shape (reference: 64 mics, 100 x 100; headline: 256 mics, 128 x 128) and every in {1, 3}, alternating runs,
             medians of --reps: seconds for the whole recording and shown frames per second of
               watch     watch_blocks -> 1024 x 1024 colour frames of every `every`th block (like `live`, into the arrays of the
                         call before: a writer's loop)
               live      what a caller had before: the loop of live_block over ALL blocks with the same large image
               watch_u8  watch_blocks -> the compact image alone
               blocks_u8 what a caller had before: process_blocks + heatmap_u8 of every row on the host (every block)
             and the pinned device -> host and host -> device copy rates of this box, against which the large image's bytes
             per second are put
  --display  the display step alone on device buffers, per frame, HIP events around >= 20 warm launches:
               old       awpu_hip_heatmap_u8_device + awpu_hip_upscale_u8_device (upscale_kernel: a pixel per thread)
               new       watch_samples_device with and without the large image (the difference is watch_upscale_kernel)
             (run it under `rocprofv3 --kernel-trace --stats` for the two kernels' own times)
  --sweeps   launches and frames of awpu_hip_get_stats for every = 3 against every = 1 on the same recording"""
import argparse
import importlib
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))
pkg = importlib.import_module("beamforming-lk_amd")
import torch  # noqa: E402  (after the package: one HIP runtime)
from block_rate import BLOCK_BYTES, SHAPES, engine, wire_of  # noqa: E402
from pcap_video import jet_table  # noqa: E402

SIZE = 1024


def copy_rates():
    """(device -> host, host -> device) bytes per second of 64 MiB pinned copies."""
    host = torch.empty(64 << 20, dtype=torch.uint8).pin_memory()
    dev = torch.empty_like(host, device="cuda")
    out = []
    for dst, src in ((host, dev), (dev, host)):
        dst.copy_(src)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(10):
            dst.copy_(src, non_blocking=True)
        torch.cuda.synchronize()
        out.append(10 * host.numel() / (time.perf_counter() - t))
    return out


def host_part(a):
    d2h, h2d = copy_rates()
    print(json.dumps({"d2h_pinned_GBps": round(d2h / 1e9, 2), "h2d_pinned_GBps": round(h2d / 1e9, 2)}), flush=True)
    table = torch.from_numpy(jet_table()).cuda()
    wire = wire_of(a.blocks)
    for name in a.shapes.split(","):
        arrays, res = SHAPES[name]
        n = 64 * arrays
        with engine(n, res, 32) as watch, engine(n, res, 1) as live, engine(n, res, 128) as blocks:
            out, kept, kept_u8 = None, None, None

            def watch_big(every):
                nonlocal kept
                kept = watch.watch_blocks(wire, res, res, every=every, out_rows=SIZE, out_cols=SIZE, d_colormap_ptr=table.data_ptr(),
                                          want_image=False, out=kept)

            def watch_u8(every):
                nonlocal kept_u8
                kept_u8 = watch.watch_blocks(wire, res, res, every=every, out=kept_u8)

            def live_loop():
                nonlocal out
                for b in range(a.blocks):
                    out = live.live_block(wire[b * BLOCK_BYTES: (b + 1) * BLOCK_BYTES], res, res, SIZE, SIZE, d_colormap_ptr=table.data_ptr(),
                                          want_power=False, out=out)

            def blocks_u8():
                power = blocks.process_blocks(wire)
                return [pkg.heatmap_u8(p) for p in power]

            for every in (1, 3):
                shown = pkg.binding.watch_count(a.blocks, 0, every)[0]
                runs = {
                    "watch": lambda: watch_big(every),
                    "live": live_loop,
                    "watch_u8": lambda: watch_u8(every),
                    "blocks_u8": blocks_u8,
                }
                times = {k: [] for k in runs}
                for rep in range(a.reps + 1):  # (the first round warms every path: buffers, graphs, tables)
                    for k, fn in runs.items():
                        t = time.perf_counter()
                        fn()
                        if rep:
                            times[k].append(time.perf_counter() - t)
                med = {k: statistics.median(v) for k, v in times.items()}
                row = {"shape": name, "mics": n, "grid": f"{res}x{res}", "blocks": a.blocks, "every": every, "shown": shown, "reps": a.reps}
                for k, t in med.items():
                    row[f"{k}_s"] = round(t, 4)
                    row[f"{k}_shown_fps"] = round(shown / t, 1)
                    row[f"{k}_blocks_per_s"] = round(a.blocks / t, 1)
                row["watch_image_GBps"] = round(shown * SIZE * SIZE * 3 / med["watch"] / 1e9, 2)
                row["watch_image_share_of_d2h"] = round(shown * SIZE * SIZE * 3 / med["watch"] / d2h, 3)
                row["watch_vs_live"] = round(med["live"] / med["watch"], 2)
                row["watch_u8_vs_blocks_u8"] = round(med["blocks_u8"] / med["watch_u8"], 2)
                print(json.dumps(row), flush=True)


def display_part(a):
    table = torch.from_numpy(jet_table()).cuda()
    for name in a.shapes.split(","):
        arrays, res = SHAPES[name]
        n, frames = 64 * arrays, 32
        with engine(n, res, 32) as eng:
            samples = (torch.randn(n, 256 * frames, device="cuda") * 1e-3).contiguous()
            power = torch.empty(frames, res * res, device="cuda")
            peak = torch.empty(frames, device="cuda")
            pix = torch.empty(frames, res * res, dtype=torch.uint8, device="cuda")
            big = torch.empty(frames, SIZE, SIZE, 3, dtype=torch.uint8, device="cuda")
            side = torch.cuda.Stream()  # (a stream of its own: 0 would mean the handle's, which torch's events do not see)
            stream = side.cuda_stream

            def watch(with_big):
                eng.watch_samples_device(samples.data_ptr(), 256 * frames, frames, res, res, d_image_ptr=pix.data_ptr(),
                                         d_big_ptr=big.data_ptr() if with_big else 0, d_power_ptr=power.data_ptr(), out_rows=SIZE,
                                         out_cols=SIZE, d_colormap_ptr=table.data_ptr(), stream=stream)

            def old():
                eng.heatmap_device(power.data_ptr(), res * res, frames, peak.data_ptr(), pix.data_ptr(), stream=stream)
                eng.upscale_device(pix.data_ptr(), res, res, frames, big.data_ptr(), SIZE, SIZE, d_colormap_ptr=table.data_ptr(), stream=stream)

            def timed(fn):
                fn()
                torch.cuda.synchronize()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(side)
                for _ in range(a.launches):
                    fn()
                t1.record(side)
                torch.cuda.synchronize()
                return t0.elapsed_time(t1) * 1e3 / (a.launches * frames)  # us per frame

            torch.cuda.synchronize()
            watch(True)
            torch.cuda.synchronize()
            new_bytes = big.cpu()
            big.zero_()
            torch.cuda.synchronize()
            us_old = timed(old)
            assert torch.equal(big.cpu(), new_bytes)  # the same images either way
            us_with, us_without = timed(lambda: watch(True)), timed(lambda: watch(False))
            row = {"shape": name, "grid": f"{res}x{res}", "frames_per_launch": frames, "launches": a.launches,
                   "old_heatmap_plus_upscale_us_per_frame": round(us_old, 2), "watch_with_big_us_per_frame": round(us_with, 2),
                   "watch_without_big_us_per_frame": round(us_without, 2), "new_upscale_us_per_frame": round(us_with - us_without, 2),
                   "new_upscale_TBps": round(SIZE * SIZE * 3 / max(us_with - us_without, 1e-9) / 1e6, 3)}
            print(json.dumps(row), flush=True)


def sweeps_part(a):
    wire = wire_of(96)
    for every in (1, 3):
        with engine(64, 100, 32) as eng:
            eng.watch_blocks(wire, 100, 100, every=every)
            st = eng.stats()
            print(json.dumps({"blocks": 96, "every": every, "frames_swept": st.frames, "launches": st.launches}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--display", action="store_true")
    ap.add_argument("--sweeps", action="store_true")
    ap.add_argument("--blocks", type=int, default=192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--shapes", default="reference,headline")
    a = ap.parse_args()
    if a.host:
        host_part(a)
    if a.display:
        display_part(a)
    if a.sweeps:
        sweeps_part(a)


if __name__ == "__main__":
    main()
