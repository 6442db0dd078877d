#!/usr/bin/env python3
"""What the coherence sweep costs (include/awpu_hip_cohere.h): Engine.cohere_device beside Engine.process_device forced to the
verification kernel it is shaped after (AWPU_SHAPE=exact_verify: das_exact_kernel), on the same device-resident frames, at c1
(64 mics, 32 x 32), the reference's default (64 mics, 100 x 100) and the headline shape (256 mics, 128 x 128), for batches of 1
and 32; --steps steps of each, alternating step by step, in one process; every step timed by HIP events on the stream it runs on.
One JSON line per shape and batch: the median step of each, frames per second, and the coherence step over the plain one.

  tools/cohere_rate.py --steps 20

The estimate this is held against: per pixel, mic and sample the coherence sweep issues about 11 vector instructions
and 4 LDS reads where das_exact_kernel issues 3 and 2."""
import argparse
import importlib
import json
import os
import statistics
import sys
from pathlib import Path

os.environ["AWPU_SHAPE"] = "exact_verify"  # read once, when the library loads: process_device below runs das_exact_kernel
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
pkg = importlib.import_module("beamforming-lk_amd")
import torch  # noqa: E402  (after the package: one HIP runtime)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="c1,ref_default,headline")
    ap.add_argument("--batches", default="1,32")
    a = ap.parse_args()
    S = pkg.synthetic
    side = torch.cuda.Stream()  # (a stream of its own: 0 would mean the handle's, which torch's events do not see)
    for shape in a.shapes.split(","):
        spec = S.WORKLOADS[shape]
        xyz = S.geometry(spec)
        off, frac = S.delay_table(spec, xyz)
        for batch in (int(b) for b in a.batches.split(",")):
            frames = (torch.randn(batch, spec.n_mics, 1024, device="cuda") * 1e-2 + 0.01).contiguous()
            power = torch.empty(batch, spec.n_pixels, device="cuda")
            weighted = torch.empty(batch, spec.n_pixels, device="cuda")
            with pkg.Engine(n_pixels=spec.n_pixels, n_streams=spec.n_mics, max_batch=batch, grid_columns=spec.res) as eng:
                eng.set_delay_table(off, frac)
                eng.set_active_mics(None)
                calls = {"plain": lambda: eng.process_device(frames.data_ptr(), batch, power.data_ptr(), side.cuda_stream),
                         "cohere": lambda: eng.cohere_device(frames.data_ptr(), batch, d_weighted_ptr=weighted.data_ptr(), stream=side.cuda_stream)}
                kernels, times = {}, {name: [] for name in calls}
                for step in range(a.warmup + a.steps):
                    for name, call in calls.items():
                        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        t0.record(side)
                        call()
                        t1.record(side)
                        torch.cuda.synchronize()
                        kernels[name] = pkg.binding.KERNEL_NAMES[eng.stats().kernel_variant]
                        if step >= a.warmup:
                            times[name].append(t0.elapsed_time(t1))
                row = {"shape": shape, "mics": spec.n_mics, "grid": f"{spec.res}x{spec.res}", "batch": batch, "steps": a.steps,
                       "window": eng.stats().window, "kernels": kernels, "device": torch.cuda.get_device_name(0)}
                for name, v in times.items():
                    med = statistics.median(v)
                    row[f"{name}_step_ms"] = round(med, 4)
                    row[f"{name}_frames_per_s"] = round(batch / med * 1e3, 1)
                    row[f"{name}_spread"] = round((max(v) - min(v)) / med, 4)
                row["cohere_over_plain"] = round(statistics.median(times["cohere"]) / statistics.median(times["plain"]), 3)
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
