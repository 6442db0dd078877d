#!/usr/bin/env python3
"""What peeling costs (include/awpu_hip_peel.h): Engine.peel_device with 4 steps beside the floor it cannot beat -- the 5 sweeps it
contains, as 5 calls of the same handle's Engine.process_device on the same device-resident frames -- at c1 (64 mics, 32 x 32),
the reference's default (64 mics, 100 x 100) and the headline shape (256 mics, 128 x 128) for batches of 32, and at the
reference's default for one frame; and one call of Engine.peel_step_device, the step kernel alone.  --steps rounds of each,
alternating round by round, in one process; every round timed by HIP events on the stream it runs on.  One JSON line per shape
and batch: the median round of each, and the loop over its floor.

  tools/peel_rate.py --steps 20"""
import argparse
import importlib
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
pkg = importlib.import_module("beamforming-lk_amd")
import torch  # noqa: E402  (after the package: one HIP runtime)

PEEL_STEPS = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="c1:32,ref_default:32,headline:32,ref_default:1", help="shape:batch, comma-separated")
    a = ap.parse_args()
    S = pkg.synthetic
    side = torch.cuda.Stream()  # (a stream of its own: 0 would mean the handle's, which torch's events do not see)
    for case in a.cases.split(","):
        shape, batch = case.split(":")[0], int(case.split(":")[1])
        spec = S.WORKLOADS[shape]
        xyz = S.geometry(spec)
        off, frac = S.delay_table(spec, xyz)
        frames = (torch.randn(batch, spec.n_mics, 1024, device="cuda") * 1e-2).contiguous()
        work = frames.clone()
        power = torch.empty(batch, spec.n_pixels, device="cuda")
        out = torch.empty(batch, spec.n_pixels, device="cuda")
        pixel = torch.full((batch,), spec.n_pixels // 2, dtype=torch.int32, device="cuda")
        with pkg.Engine(n_pixels=spec.n_pixels, n_streams=spec.n_mics, max_batch=batch, grid_columns=spec.res) as eng:
            eng.set_delay_table(off, frac)
            eng.set_active_mics(None)

            def floor():
                for _ in range(PEEL_STEPS + 1):
                    eng.process_device(frames.data_ptr(), batch, power.data_ptr(), side.cuda_stream)

            calls = {"floor": floor,
                     "peel": lambda: eng.peel_device(frames.data_ptr(), batch, PEEL_STEPS, d_map_ptr=out.data_ptr(), stream=side.cuda_stream),
                     "step": lambda: eng.peel_step_device(work.data_ptr(), batch, pixel.data_ptr(), 0.5, stream=side.cuda_stream)}
            times = {name: [] for name in calls}
            for step in range(a.warmup + a.steps):
                for name, call in calls.items():
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record(side)
                    call()
                    t1.record(side)
                    torch.cuda.synchronize()
                    if step >= a.warmup:
                        times[name].append(t0.elapsed_time(t1))
            row = {"shape": shape, "mics": spec.n_mics, "grid": f"{spec.res}x{spec.res}", "batch": batch, "rounds": a.steps, "peel_steps": PEEL_STEPS,
                   "beam_samples": pkg.peel_beam_length(spec.n_mics, 1024, off, frac), "sweep_kernel": pkg.binding.KERNEL_NAMES[eng.stats().kernel_variant],
                   "device": torch.cuda.get_device_name(0)}
            for name, v in times.items():
                med = statistics.median(v)
                row[f"{name}_ms"] = round(med, 4)
                row[f"{name}_spread"] = round((max(v) - min(v)) / med, 4)
            row["peel_over_floor"] = round(statistics.median(times["peel"]) / statistics.median(times["floor"]), 3)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
