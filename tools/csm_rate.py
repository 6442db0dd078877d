#!/usr/bin/env python3
"""What the cross-spectral maps cost (include/awpu_hip_csm.h): Engine.csm_map_device for 1 bin and for 8 bins, and
Engine.csm_samples_device for 8 bins, on device-resident buffers, at c1 (64 mics, 32 x 32), the reference's default (64 mics,
100 x 100) and the headline shape (256 mics, 128 x 128); --repeats launches of each, every launch timed by HIP events on the
stream it runs on.  One JSON line per shape: the median launch of each, maps per second, complex multiply-adds per second of the
quadratic form (pixels x bins x usable (usable - 1) / 2 a map) and accumulated blocks per second.

  tools/csm_rate.py --repeats 20

No figure here is a gate: nobody has measured this workload before."""
import argparse
import importlib
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
pkg = importlib.import_module("beamforming-lk_amd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="c1,ref_default,headline")
    ap.add_argument("--blocks", type=int, default=64, help="blocks per accumulate call")
    a = ap.parse_args()
    import torch  # (after the package: one HIP runtime)

    S = pkg.synthetic
    side = torch.cuda.Stream()  # (a stream of its own: 0 would mean the handle's, which torch's events do not see)
    for shape in a.shapes.split(","):
        spec = S.WORKLOADS[shape]
        xyz = S.geometry(spec)
        off, frac = S.delay_table(spec, xyz)
        U, P = spec.n_mics, spec.n_pixels
        samples = (torch.randn(U, 256 * a.blocks, device="cuda") * 1e-2).contiguous()
        matrix = torch.zeros(8, U, U, 2, device="cuda")
        plane = torch.empty(8, P, device="cuda")
        with pkg.Engine(n_pixels=P, n_streams=U, grid_columns=spec.res) as eng:
            eng.set_delay_table(off, frac)
            eng.set_active_mics(None)
            bins8, bins1 = [8, 16, 24, 32, 40, 48, 56, 64], [16]
            calls = {"accumulate_8": lambda: eng.csm_samples_device(samples.data_ptr(), samples.shape[1], a.blocks, bins8, matrix.data_ptr(),
                                                                    window=1, stream=side.cuda_stream),
                     "map_1": lambda: eng.csm_map_device(matrix.data_ptr(), a.blocks, bins1, 1, d_map_ptr=plane.data_ptr(), stream=side.cuda_stream),
                     "map_8": lambda: eng.csm_map_device(matrix.data_ptr(), a.blocks, bins8, 1, d_map_ptr=plane.data_ptr(), stream=side.cuda_stream)}
            times = {name: [] for name in calls}
            for step in range(a.warmup + a.repeats):
                for name, call in calls.items():
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record(side)
                    call()
                    t1.record(side)
                    torch.cuda.synchronize()
                    if step >= a.warmup:
                        times[name].append(t0.elapsed_time(t1))
            row = {"shape": shape, "mics": U, "grid": f"{spec.res}x{spec.res}", "repeats": a.repeats, "blocks": a.blocks,
                   "device": torch.cuda.get_device_name(0)}
            for name, v in times.items():
                med = statistics.median(v)
                row[f"{name}_ms"] = round(med, 4)
                row[f"{name}_spread"] = round((max(v) - min(v)) / med, 4)
            for n_bins in (1, 8):
                med = statistics.median(times[f"map_{n_bins}"])
                row[f"map_{n_bins}_per_s"] = round(1e3 / med, 1)
                row[f"map_{n_bins}_gcmadd_per_s"] = round(P * n_bins * U * (U - 1) / 2 / med * 1e-6, 2)
            row["blocks_per_s"] = round(a.blocks / statistics.median(times["accumulate_8"]) * 1e3, 1)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
