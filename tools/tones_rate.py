#!/usr/bin/env python3
"""What the tone sweep costs (include/awpu_hip_tones.h): Engine.tones_device beside Engine.cohere_device and Engine.process_device,
the latter forced to the verification kernel both are shaped after (AWPU_SHAPE=exact_verify: das_exact_kernel), on the same
device-resident frames, at c1 (64 mics, 32 x 32), the reference's default (64 mics, 100 x 100) and the headline shape (256 mics,
128 x 128), for batches of 32; --steps steps of each, alternating step by step, in one process; every step timed by HIP events on
the stream it runs on.  The tone sweep is asked for one group (--tone, Hz) and for the pitch.  One JSON line per shape and batch:
the median step of each, frames per second, and the tone step over the other two.

  tools/tones_rate.py --steps 20

The estimate this is held against ("Tone maps"): per pixel the sweep issues one lerp per mic and sample, as
das_exact_kernel does and where the coherence sweep issues three, plus an epilogue of some 600 vector instructions whatever the
mic count."""
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
    ap.add_argument("--batches", default="32")
    ap.add_argument("--tone", default="8000:10000", help="LO:HI[:hann]: the one group the tone sweep is asked for")
    a = ap.parse_args()
    S = pkg.synthetic
    groups = pkg.binding.tones_from_text(a.tone)
    side = torch.cuda.Stream()  # (a stream of its own: 0 would mean the handle's, which torch's events do not see)
    for shape in a.shapes.split(","):
        spec = S.WORKLOADS[shape]
        xyz = S.geometry(spec)
        off, frac = S.delay_table(spec, xyz)
        for batch in (int(b) for b in a.batches.split(",")):
            frames = (torch.randn(batch, spec.n_mics, 1024, device="cuda") * 1e-2 + 0.01).contiguous()
            power = torch.empty(batch, spec.n_pixels, device="cuda")
            weighted = torch.empty(batch, spec.n_pixels, device="cuda")
            tone = torch.empty(batch, 1, spec.n_pixels, device="cuda")
            pitch = torch.empty(batch, spec.n_pixels, device="cuda", dtype=torch.int32)
            with pkg.Engine(n_pixels=spec.n_pixels, n_streams=spec.n_mics, max_batch=batch, grid_columns=spec.res) as eng:
                eng.set_delay_table(off, frac)
                eng.set_active_mics(None)
                calls = {"plain": lambda: eng.process_device(frames.data_ptr(), batch, power.data_ptr(), side.cuda_stream),
                         "cohere": lambda: eng.cohere_device(frames.data_ptr(), batch, d_weighted_ptr=weighted.data_ptr(), stream=side.cuda_stream),
                         "tones": lambda: eng.tones_device(frames.data_ptr(), batch, groups, d_tone_ptr=tone.data_ptr(), d_pitch_ptr=pitch.data_ptr(),
                                                           stream=side.cuda_stream)}
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
                       "window": eng.stats().window, "kernels": kernels, "tone": a.tone, "device": torch.cuda.get_device_name(0)}
                for name, v in times.items():
                    med = statistics.median(v)
                    row[f"{name}_step_ms"] = round(med, 4)
                    row[f"{name}_frames_per_s"] = round(batch / med * 1e3, 1)
                    row[f"{name}_spread"] = round((max(v) - min(v)) / med, 4)
                row["tones_over_plain"] = round(statistics.median(times["tones"]) / statistics.median(times["plain"]), 3)
                row["tones_over_cohere"] = round(statistics.median(times["tones"]) / statistics.median(times["cohere"]), 3)
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
