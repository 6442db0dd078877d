#!/usr/bin/env python3
"""What a band costs (include/awpu_hip_band.h) at the headline shape (256 mics, 128 x 128), default math: process_device on 128
device-resident frames, with band_design(6375, 9000, taps) for 63 and for 127 taps and without a band, --steps steps of each,
alternating step by step, in one process; every step timed by HIP events on the stream it runs on.  One JSON line: the median
step of each, and the band-limited steps over the band-less one of the same run.

  tools/band_cost.py --steps 20

The estimate this is held against: the pre-pass reads and writes about 100 MB and takes about 0.7 G fused
multiply-adds at 63 taps, beside a sweep of 553 GF: 1-2 % of a step."""
import argparse
import importlib
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))
pkg = importlib.import_module("beamforming-lk_amd")
import torch  # noqa: E402  (after the package: one HIP runtime)
from block_rate import SHAPES, engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--shape", default="headline")
    a = ap.parse_args()
    arrays, res = SHAPES[a.shape]
    n = 64 * arrays
    frames = (torch.randn(a.batch, n, 1024, device="cuda") * 1e-2 + 0.01).contiguous()
    power = torch.empty(a.batch, res * res, device="cuda")
    side = torch.cuda.Stream()  # (a stream of its own: 0 would mean the handle's, which torch's events do not see)
    cases = {"plain": None, "band63": pkg.binding.band_design(6375, 9000, 63), "band127": pkg.binding.band_design(6375, 9000, 127)}
    engines = {}
    try:
        for name, c in cases.items():
            engines[name] = engine(n, res, a.batch)
            if c is not None:
                engines[name].set_band(c)
        torch.cuda.synchronize()
        times = {name: [] for name in cases}
        for step in range(a.warmup + a.steps):
            for name, eng in engines.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(side)
                eng.process_device(frames.data_ptr(), a.batch, power.data_ptr(), side.cuda_stream)
                t1.record(side)
                torch.cuda.synchronize()
                if step >= a.warmup:
                    times[name].append(t0.elapsed_time(t1))
        st = engines["plain"].stats()
        row = {"shape": a.shape, "mics": n, "grid": f"{res}x{res}", "batch": a.batch, "steps": a.steps, "window": st.window,
               "kernel": pkg.binding.KERNEL_NAMES[st.kernel_variant], "device": torch.cuda.get_device_name(0)}
        for name, v in times.items():
            row[f"{name}_step_ms"] = round(statistics.median(v), 4)
            row[f"{name}_spread"] = round((max(v) - min(v)) / statistics.median(v), 4)
        for name in ("band63", "band127"):
            row[f"{name}_over_plain"] = round(statistics.median(times[name]) / statistics.median(times["plain"]), 4)
        print(json.dumps(row), flush=True)
    finally:
        for eng in engines.values():
            eng.close()


if __name__ == "__main__":
    main()
