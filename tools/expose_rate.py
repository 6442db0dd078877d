#!/usr/bin/env python3
"""What exposure costs (include/awpu_hip_expose.h), default math, max_batch 128, one JSON line per shape -- the reference's (64
mics, 100 x 100) and the headline (256 mics, 128 x 128) -- over a recording of --blocks blocks of unpacked samples:

  --host     seconds per recording, interleaved series, medians of --reps, of
               process     process_samples: every block swept, every power row brought back     (the baseline)
               process_b   the same call again, as a series of its own: the spread of two identical series is the margin below
               expose      expose_samples(every = L = --length) asked for the exposed powers: the same blocks swept, one extra pass
                           over them on the device, 1 / L of the rows brought back
               watch       watch_samples(every = --length) asked for powers: what showing every Lth block and skipping the rest costs
             and expose / process, against 1 + max(0.10, that spread).  --baseline DIR takes `process` and `process_b` from another
             build of the package (a checkout of the commit before exposure, built beforehand: DIR/beamforming-lk_amd), loaded
             beside this one in the same process.
  --flicker  what exposure buys, on synthetic.make_frames' plane wave in noise at the c1 shape (64 mics, 32 x 32), frames every
             --length blocks, for L = 1 and L = --length: the relative frame-to-frame standard deviation of the power at the peak
             pixel, and the standard deviation of the strongest source's refined row and column (pixels)."""
import argparse
import importlib
import importlib.util
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))
pkg = importlib.import_module("beamforming-lk_amd")
import torch  # noqa: E402,F401  (after the package: one HIP runtime)
from block_rate import SHAPES  # noqa: E402


def package_at(root):
    """Another build of the package, under a name of its own (its library is loaded from its own directory)."""
    init = Path(root) / "beamforming-lk_amd" / "__init__.py"
    spec = importlib.util.spec_from_file_location("awpu_baseline", init, submodule_search_locations=[str(init.parent)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["awpu_baseline"] = mod
    spec.loader.exec_module(mod)
    return mod


def engine_of(p, n, res, max_batch):
    xyz = p.create_tiled_antenna(n // 64, 1)
    off, frac = p.build_delay_table(xyz, res, res)
    eng = p.Engine(n_pixels=res * res, n_streams=n, max_batch=max_batch, grid_columns=res)
    eng.set_delay_table(off, frac)
    eng.set_active_mics(None)
    return eng


def host_part(a):
    base = package_at(a.baseline) if a.baseline else pkg
    for shape in a.shapes.split(","):
        arrays, res = SHAPES[shape]
        n, L = 64 * arrays, a.length
        rng = np.random.default_rng(0)
        samples = (rng.integers(-(1 << 21), 1 << 21, size=(n, 256 * a.blocks)) / 8388608.0).astype(np.float32)
        with engine_of(base, n, res, 128) as e_base, engine_of(pkg, n, res, 128) as e_new:
            carry = np.zeros(res * res, np.float32)
            runs = {
                "process": lambda: e_base.process_samples(samples),
                "expose": lambda: e_new.expose_samples(samples, res, res, L, carry=carry, want_image=False, want_power=True),
                "process_b": lambda: e_base.process_samples(samples),
                "watch": lambda: e_new.watch_samples(samples, res, res, first=L - 1, every=L, want_image=False, want_power=True),
            }
            times = {k: [] for k in runs}
            for rep in range(a.reps + 1):  # (the first round warms every path: buffers, tables)
                for k, fn in runs.items():
                    t = time.perf_counter()
                    fn()
                    if rep:
                        times[k].append(time.perf_counter() - t)
            med = {k: statistics.median(v) for k, v in times.items()}
            spread = abs(med["process"] - med["process_b"]) / min(med["process"], med["process_b"])
            row = {"shape": shape, "mics": n, "grid": f"{res}x{res}", "blocks": a.blocks, "reps": a.reps, "length": L,
                   "baseline": "another build" if a.baseline else "this build"}
            for k, v in times.items():
                row[f"{k}_s"] = round(med[k], 4)
                row[f"{k}_blocks_per_s"] = round(a.blocks / med[k], 1)
                row[f"{k}_min_max_s"] = [round(min(v), 4), round(max(v), 4)]
            row["baseline_spread"] = round(spread, 4)
            row["expose_vs_process"] = round(med["expose"] / min(med["process"], med["process_b"]), 4)
            row["margin"] = round(max(0.10, spread), 4)
            row["within_margin"] = bool(row["expose_vs_process"] <= 1.0 + row["margin"])
            row["watch_vs_process"] = round(med["watch"] / min(med["process"], med["process_b"]), 4)
            print(json.dumps(row), flush=True)


def flicker_part(a):
    S = pkg.synthetic
    spec = S.WORKLOADS["c1"]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    n_blocks = max(a.length * 40, 240)
    samples = np.ascontiguousarray(S.make_frames(xyz, 1, seed=77, hist=256 * n_blocks)[0])
    for L in (1, a.length):
        with pkg.Engine(n_pixels=spec.res ** 2, n_streams=xyz.shape[1], max_batch=32, grid_columns=spec.res) as eng:
            eng.set_delay_table(off, frac)
            eng.set_active_mics(None)
            got = eng.expose_samples(samples, spec.res, spec.res, L, first=a.length + 3, every=a.length, want_image=False, want_power=True,
                                     find=dict(radius=2, max_sources=1))
        peak = int(np.argmax(got.power.mean(axis=0)))
        at_peak = got.power[:, peak].astype(np.float64)
        found = got.count > 0
        print(json.dumps({"shape": "c1", "blocks": n_blocks, "every": a.length, "length": L, "frames": len(got), "peak_pixel": peak,
                          "peak_power_rel_std": round(float(at_peak.std() / at_peak.mean()), 5),
                          "source_row_std_px": round(float(got.sources["row"][found, 0].std()), 5),
                          "source_col_std_px": round(float(got.sources["col"][found, 0].std()), 5),
                          "frames_with_a_source": int(found.sum())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--flicker", action="store_true")
    ap.add_argument("--blocks", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--length", type=int, default=6)
    ap.add_argument("--shapes", default="reference,headline")
    ap.add_argument("--baseline", default=None, metavar="DIR", help="a checkout of another commit, built: its process_samples is the baseline")
    a = ap.parse_args()
    if a.host:
        host_part(a)
    if a.flicker:
        flicker_part(a)


if __name__ == "__main__":
    main()
