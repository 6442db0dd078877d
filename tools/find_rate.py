#!/usr/bin/env python3
"""What finding sources costs (include/awpu_hip_find.h) at the headline shape (256 mics, 128 x 128, max_batch 128), default math,
one JSON line per measurement:

  --host    blocks per second, every block shown, alternating runs, medians of --reps, of
              find         find_blocks with power = NULL: a few hundred bytes per block come back
              find_power   find_blocks that returns the powers too
              watch_power  watch_blocks that returns the powers only: what a caller had to pull over PCIe to search in numpy
            (and numpy's own search is not in `watch_power`: that figure is the transport alone)
  --kernel  the peak pass alone on a piece of 32 device-resident power rows (max_batch 128 is swept in quarters), HIP events
            around --launches warm launches, per radius: microseconds per piece and per frame"""
import argparse
import importlib
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))
pkg = importlib.import_module("beamforming-lk_amd")
import torch  # noqa: E402  (after the package: one HIP runtime)
from block_rate import SHAPES, engine, wire_of  # noqa: E402

FIND = dict(radius=2, max_sources=4, min_ratio=0.25)


def host_part(a):
    arrays, res = SHAPES[a.shape]
    n = 64 * arrays
    wire = wire_of(a.blocks)
    with engine(n, res, 128) as find, engine(n, res, 128) as watch:
        kept = None

        def watch_power():
            nonlocal kept
            kept = watch.watch_blocks(wire, res, res, want_image=False, want_power=True, out=kept)

        runs = {
            "find": lambda: find.find_blocks(wire, res, res, **FIND),
            "find_power": lambda: find.find_blocks(wire, res, res, want_power=True, **FIND),
            "watch_power": watch_power,
        }
        times = {k: [] for k in runs}
        for rep in range(a.reps + 1):  # (the first round warms every path: buffers, tables)
            for k, fn in runs.items():
                t = time.perf_counter()
                fn()
                if rep:
                    times[k].append(time.perf_counter() - t)
        row = {"shape": a.shape, "mics": n, "grid": f"{res}x{res}", "blocks": a.blocks, "reps": a.reps, **FIND}
        for k, v in times.items():
            row[f"{k}_blocks_per_s"] = round(a.blocks / statistics.median(v), 1)
            row[f"{k}_spread"] = round((max(v) - min(v)) / statistics.median(v), 3)
        row["find_vs_watch_power"] = round(statistics.median(times["watch_power"]) / statistics.median(times["find"]), 3)
        print(json.dumps(row), flush=True)


def kernel_part(a):
    arrays, res = SHAPES[a.shape]
    frames = 32
    with engine(64 * arrays, res, 128) as eng:
        samples = (torch.randn(64 * arrays, 256 * frames, device="cuda") * 1e-3).contiguous()
        power = torch.empty(frames, res * res, device="cuda")
        sources = torch.empty(frames * 32 * 40, dtype=torch.uint8, device="cuda")
        count = torch.empty(frames, dtype=torch.int32, device="cuda")
        side = torch.cuda.Stream()  # (a stream of its own: 0 would mean the handle's, which torch's events do not see)
        torch.cuda.synchronize()
        eng.process_samples_device(samples.data_ptr(), 256 * frames, frames, power.data_ptr(), side.cuda_stream)  # real heatmaps
        torch.cuda.synchronize()
        for radius, max_sources in ((1, 4), (2, 4), (4, 4), (8, 4), (2, 32)):
            def fn():
                eng.find_peaks_device(power.data_ptr(), frames, res, res, sources.data_ptr(), count.data_ptr(), radius=radius,
                                      max_sources=max_sources, min_ratio=0.25, stream=side.cuda_stream)
            fn()
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(side)
            for _ in range(a.launches):
                fn()
            t1.record(side)
            torch.cuda.synchronize()
            us = t0.elapsed_time(t1) * 1e3 / a.launches
            print(json.dumps({"shape": a.shape, "grid": f"{res}x{res}", "frames_per_piece": frames, "radius": radius, "max_sources": max_sources,
                              "launches": a.launches, "find_us_per_piece": round(us, 1), "find_us_per_frame": round(us / frames, 2),
                              "sources_found": int(count.sum().item())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--blocks", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--shape", default="headline")
    a = ap.parse_args()
    if a.host:
        host_part(a)
    if a.kernel:
        kernel_part(a)


if __name__ == "__main__":
    main()
