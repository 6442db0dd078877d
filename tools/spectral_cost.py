#!/usr/bin/env python3
"""What three bands at once cost against three bands one after the other (include/awpu_hip_spectral.h) at the headline shape (256
mics, 128 x 128), default math, the reference's three bands (1950-3541, 3541-6375, 6375-9000 Hz) at 63 taps.  One process, the legs
alternating step by step; one JSON line with the medians, the spreads and the two ratios.

  (a) single calls on resident frames: process_bands_device on --batch device-resident frames against the sum of three
      process_device steps, each with one band set (the band is replaced between them); every step timed by HIP events on the
      stream it runs on.
  (b) host run: spectral_samples over a --blocks-block recording with every = 1, powers, images and dominant bands asked for,
      against the sum of three watch_samples runs (powers and images) with one band each; wall time of the synchronous calls.

  tools/spectral_cost.py --steps 20 [--parent-lib tools/ab/parent.so]

The band-by-band legs use only calls the commit before this feature has.  With --parent-lib they run on that library (a build of
the parent commit, tools/build_variant.sh's recipe on its tree) loaded beside this one in the same process -- so their figures are
not taken from the build under test; without it they run on this build, and the line says so.

The expectation this is held against: (a) equal within noise -- the pre-pass is 2-3 % of a step and fusing it saves
two reads of the frames; (b) clearly below the sum -- upload, unpack, history and ring happen once instead of three times."""
import argparse
import ctypes as C
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
from block_rate import SHAPES, engine  # noqa: E402

RANGES = ((1950.0, 3541.0), (3541.0, 6375.0), (6375.0, 9000.0))


def parent_library(path):
    """The parent commit's library beside this build's: every entry point it has, with the binding's signatures."""
    B = pkg.binding
    lib = C.CDLL(str(Path(path).resolve()))
    for table in (B._SIGNATURES, B._TRACK_SIGNATURES, B._BLOCK_SIGNATURES, B._LISTEN_SIGNATURES, B._WATCH_SIGNATURES, B._FIND_SIGNATURES,
                  B._BAND_SIGNATURES, B._FOCUS_SIGNATURES):
        for name, (res, args) in table.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    assert not hasattr(lib, "awpu_hip_process_bands"), "the parent library has the feature: not the parent"
    return lib


def engine_on(lib, *args):
    """block_rate.engine on `lib` (None: this build).  An Engine keeps the library it was created with (Engine._lib, taken from
    binding.load() in its constructor) for every later call, close() included; so binding.loaded_library hands out `lib` for the
    construction alone.  Should Engine stop keeping its library at construction, this is the place that has to change (an explicit
    library parameter on Engine would replace it)."""
    if lib is None:
        return engine(*args)
    with pkg.binding.loaded_library(lib):
        return engine(*args)


def spread(v):
    return round((max(v) - min(v)) / statistics.median(v), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=512)
    ap.add_argument("--taps", type=int, default=63)
    ap.add_argument("--shape", default="headline")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libawpu_hip.so for the band-by-band legs")
    a = ap.parse_args()
    arrays, res = SHAPES[a.shape]
    n = 64 * arrays
    bands = [pkg.binding.band_design(lo, hi, a.taps) for lo, hi in RANGES]
    parent = parent_library(a.parent_lib) if a.parent_lib else None
    frames = (torch.randn(a.batch, n, 1024, device="cuda") * 1e-2 + 0.01).contiguous()
    power = torch.empty(len(bands), a.batch, res * res, device="cuda")
    side = torch.cuda.Stream()  # (a stream of its own: 0 would mean the handle's, which torch's events do not see)
    samples = (np.random.default_rng(0).standard_normal((n, 256 * a.blocks)) * 1e-2 + 0.01).astype(np.float32)
    spec, by_band = engine_on(None, n, res, a.batch), engine_on(parent, n, res, a.batch)
    spec_run, band_run = engine_on(None, n, res, a.batch), engine_on(parent, n, res, a.batch)
    try:
        torch.cuda.synchronize()

        def timed(call):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(side)
            call()
            t1.record(side)
            torch.cuda.synchronize()
            return t0.elapsed_time(t1)

        def walled(call):
            t = time.perf_counter()
            call()
            return (time.perf_counter() - t) * 1e3

        def one_band_step(c, p):
            by_band.set_band(c)
            return timed(lambda: by_band.process_device(frames.data_ptr(), a.batch, p.data_ptr(), side.cuda_stream))

        def one_band_run(c):
            band_run.set_band(c)
            return walled(lambda: band_run.watch_samples(samples, res, res, want_image=True, want_power=True))

        t = {"bands_step": [], "by_band_steps": [], "spectral_run": [], "by_band_runs": []}
        for step in range(a.warmup + a.steps):
            together = timed(lambda: spec.process_bands_device(frames.data_ptr(), a.batch, bands, power.data_ptr(), side.cuda_stream))
            apart = sum(one_band_step(c, power[b]) for b, c in enumerate(bands))
            run = walled(lambda: spec_run.spectral_samples(samples, res, res, bands, want_power=True))
            runs = sum(one_band_run(c) for c in bands)
            if step >= a.warmup:
                for name, v in zip(t, (together, apart, run, runs)):
                    t[name].append(v)
        st = spec.stats()
        row = {"shape": a.shape, "mics": n, "grid": f"{res}x{res}", "batch": a.batch, "blocks": a.blocks, "taps": a.taps, "steps": a.steps,
               "kernel": pkg.binding.KERNEL_NAMES[st.kernel_variant], "device": torch.cuda.get_device_name(0),
               "band_by_band_library": "parent commit" if parent is not None else "this build"}
        for name, v in t.items():
            row[f"{name}_ms"] = round(statistics.median(v), 4)
            row[f"{name}_spread"] = spread(v)
        row["a_bands_over_by_band"] = round(statistics.median(t["bands_step"]) / statistics.median(t["by_band_steps"]), 4)
        row["b_spectral_over_by_band"] = round(statistics.median(t["spectral_run"]) / statistics.median(t["by_band_runs"]), 4)
        print(json.dumps(row), flush=True)
    finally:
        for eng in (spec, by_band, spec_run, band_run):
            eng.close()


if __name__ == "__main__":
    main()
