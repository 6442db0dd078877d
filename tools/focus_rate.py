#!/usr/bin/env python3
"""What focus and range cost (include/awpu_hip_focus.h), measured on the GPU this runs on:

  1. awpu_hip_range against its composition -- the host awpu_hip_focus_steer_table, then awpu_hip_beams for the same directions --
     for 4 sources x 16 candidate distances on the 8 x 8 array and on the 32 x 8 tile.  Both calls are synchronous (they return
     when their stream is idle), so what is timed is the wall clock of the call, the median of --reps calls after a warm-up.
  2. awpu_hip_build_focus_table_device against awpu_hip_build_delay_table_device for the 32 x 8 tile on a 128 x 128 grid, and
     the two host builders beside them.

  tools/focus_rate.py [--reps 200]

Prints one JSON line."""
from __future__ import annotations

import argparse
import importlib
import json
import sys
import time
from pathlib import Path

import numpy as np


def median_ms(fn, reps: int, warm: int = 5) -> float:
    for _ in range(warm):
        fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times) * 1e3)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    pkg = importlib.import_module("beamforming-lk_amd")
    import torch

    S = pkg.synthetic
    out = {"device": torch.cuda.get_device_name(a.device), "reps": a.reps, "range": {}, "table": {}}
    cand = pkg.range_candidates(0.25, np.inf, 16)
    rng = np.random.default_rng(1)
    theta, phi = rng.uniform(0.1, 1.0, 4), rng.uniform(-np.pi, np.pi, 4)
    for name, arrays in (("8x8", (1, 1)), ("32x8", (4, 1))):
        xyz = pkg.create_tiled_antenna(*arrays)
        n = xyz.shape[1]
        d_frame = torch.from_numpy(S.make_point_frames(xyz, 1, 1.0)[0]).cuda(a.device)
        with pkg.Engine(n_pixels=16, n_streams=n, device=a.device) as eng:
            eng.set_antenna(xyz)
            eng.set_active_mics(None)
            ptr = d_frame.data_ptr()

            def composed():
                off, frac = pkg.focus_steer_table(xyz, np.repeat(theta, 16), np.repeat(phi, 16), np.tile(cand, 4))
                return eng.beams(off, frac, d_frame_ptr=ptr, want_beams=False)[0]

            def table_only():
                return pkg.focus_steer_table(xyz, np.repeat(theta, 16), np.repeat(phi, 16), np.tile(cand, 4))

            assert np.array_equal(eng.range(theta, phi, cand, d_frame_ptr=ptr)[0].reshape(-1), composed())
            out["range"][name] = {"range_ms": median_ms(lambda: eng.range(theta, phi, cand, d_frame_ptr=ptr), a.reps),
                                  "composition_ms": median_ms(composed, a.reps), "of_which_host_table_ms": median_ms(table_only, a.reps)}
    xyz = pkg.create_tiled_antenna(4, 1)
    reps = max(3, a.reps // 40)
    out["table"] = {"grid": "128x128", "mics": 256,
                    "focus_device_ms": median_ms(lambda: pkg.build_focus_table_device(xyz, 128, 128, 2.0, device=a.device), reps, 1),
                    "plane_device_ms": median_ms(lambda: pkg.build_delay_table_device(xyz, 128, 128, device=a.device), reps, 1),
                    "focus_host_ms": median_ms(lambda: pkg.build_focus_table(xyz, 128, 128, 2.0), reps, 1),
                    "plane_host_ms": median_ms(lambda: pkg.build_delay_table(xyz, 128, 128), reps, 1)}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
