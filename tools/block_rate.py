#!/usr/bin/env python3
"""Frames per second of a recording's heatmaps, default math, one JSON line per configuration:
  (a) the per-block live loop: ingest_block + process_ring, and live_block (power not read back, no upscaled image)
  (b) process_blocks (include/awpu_hip_blocks.h) with 128 blocks per chunk
  (c) process_device on 128 distinct device-resident frames (bench.py's regime)
at the reference shape (64 mics on one array's wire, 100 x 100) and the headline (256 mics, 128 x 128).  Beside (b): the
bound the wire bytes set (264 KB per block whatever the mic count) at the pinned host -> device copy rate measured here.

  tools/block_rate.py [--blocks 1024] [--only b]     (--only b: just (b), e.g. under rocprofv3 --kernel-trace --stats)"""
import argparse
import importlib
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
pkg = importlib.import_module("beamforming-lk_amd")
import torch  # noqa: E402  (after the package: one HIP runtime)

SHAPES = {"reference": (1, 100), "headline": (4, 128)}  # arrays side by side, grid resolution
BLOCK_BYTES = 256 * 1032


def wire_of(n_blocks, seed=0):
    rng = np.random.default_rng(seed)
    msg = np.zeros(256 * n_blocks, np.dtype([("h", "u1", (8,)), ("stream", "<i4", (256,))]))
    msg["stream"] = rng.integers(-(1 << 21), 1 << 21, (256 * n_blocks, 256), dtype=np.int32)
    return msg.tobytes()


def engine(n, res, max_batch):
    xyz = pkg.create_tiled_antenna(n // 64, 1)
    off, frac = pkg.build_delay_table(xyz, res, res)
    eng = pkg.Engine(n_pixels=res * res, n_streams=n, max_batch=max_batch, grid_columns=res)
    eng.set_delay_table(off, frac)
    eng.set_active_mics(None)
    return eng


def rate(fn, frames, reps):
    fn()  # warm
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    return frames * reps / (time.perf_counter() - t)


def h2d_bytes_per_s():
    src = torch.empty(64 << 20, dtype=torch.uint8).pin_memory()
    dst = torch.empty_like(src, device="cuda")
    dst.copy_(src)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(10):
        dst.copy_(src, non_blocking=True)
    torch.cuda.synchronize()
    return 10 * src.numel() / (time.perf_counter() - t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=1024)
    ap.add_argument("--only", default="abc")
    ap.add_argument("--shapes", default="reference,headline")
    a = ap.parse_args()
    bw = h2d_bytes_per_s() if "b" in a.only else 0.0
    for name in a.shapes.split(","):
        arrays, res = SHAPES[name]
        n = 64 * arrays
        wire = wire_of(a.blocks)
        row = {"shape": name, "mics": n, "grid": f"{res}x{res}", "blocks": a.blocks}
        if "a" in a.only:
            with engine(n, res, 1) as eng:
                nb = min(a.blocks, 256)

                def loop():
                    for b in range(nb):
                        eng.ingest_block(wire[b * BLOCK_BYTES: (b + 1) * BLOCK_BYTES])
                        eng.process_ring()
                row["a_ingest_process_ring_fps"] = round(rate(loop, nb, 2), 1)
                out = None

                def live():
                    nonlocal out
                    for b in range(nb):
                        out = eng.live_block(wire[b * BLOCK_BYTES: (b + 1) * BLOCK_BYTES], res, res, want_power=False, out=out)
                row["a_live_block_fps"] = round(rate(live, nb, 2), 1)
        if "b" in a.only:
            with engine(n, res, 128) as eng:
                row["b_process_blocks_fps"] = round(rate(lambda: eng.process_blocks(wire), a.blocks, 3), 1)
                row["b_wire_bound_fps"] = round(bw / BLOCK_BYTES, 1)
                row["h2d_pinned_GBps"] = round(bw / 1e9, 2)
        if "c" in a.only:
            with engine(n, res, 128) as eng:
                frames = torch.randn(128, n, 1024, device="cuda") * 1e-3
                power = torch.empty(128, res * res, device="cuda")
                s = torch.cuda.current_stream().cuda_stream

                def dev():
                    for _ in range(4):
                        eng.process_device(frames.data_ptr(), 128, power.data_ptr(), s)
                    torch.cuda.synchronize()
                row["c_process_device_fps"] = round(rate(dev, 512, 3), 1)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
