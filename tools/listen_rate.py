#!/usr/bin/env python3
"""Blocks per second of listening to a recording (include/awpu_hip_listen.h), default math, one JSON line per shape:
  (a) the per-block host loop of the existing API: ingest_block + track(want_beams) -- the baseline
  (b) listen_blocks, audio and trail only, for 1 tracking listener, 8 tracking listeners (3 steps per block each) and 8 fixed ones
  (c) listen_blocks with the heatmaps of the same pass (8 tracking listeners), beside process_blocks alone on the same run
at the reference shape (64 mics on one array's wire, 100 x 100) and the headline (256 mics, 128 x 128), 128 blocks per chunk.
Every configuration is run once to warm up and then `--reps` times, the configurations of a group taking turns in alternating
order; the figure is the median.  Real time is 190.7 blocks/s (48 828 Hz / 256).

  tools/listen_rate.py [--blocks 1024] [--only abc] [--reps 5]
  AWPU_LISTEN_STREAM=0 tools/listen_rate.py --only c     (a -DAWPU_TUNING_BUILD library: the listen kernels queued behind the
                                                          sweeps instead of beside them)
  --only b: e.g. under rocprofv3 --kernel-trace --stats"""
import argparse
import importlib
import json
import math
import os
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
pkg = importlib.import_module("beamforming-lk_amd")

SHAPES = {"reference": (1, 100), "headline": (4, 128)}  # arrays side by side, grid resolution
BLOCK_BYTES = 256 * 1032
LIMIT = math.pi / 2
SETS = {"1_tracking": (1, 3), "8_tracking": (8, 3), "8_fixed": (8, 0)}  # listeners, steps per block


def wire_of(n_blocks, seed=0):
    rng = np.random.default_rng(seed)
    msg = np.zeros(256 * n_blocks, np.dtype([("h", "u1", (8,)), ("stream", "<i4", (256,))]))
    msg["stream"] = rng.integers(-(1 << 21), 1 << 21, (256 * n_blocks, 256), dtype=np.int32)
    return msg.tobytes()


def engine(xyz, res, max_batch, table):
    eng = pkg.Engine(n_pixels=res * res, n_streams=xyz.shape[1], max_batch=max_batch, grid_columns=res)
    eng.set_antenna(xyz)
    eng.set_active_mics(None)
    if table is not None:
        eng.set_delay_table(*table)
    return eng


def listeners(n, steps):
    rng = np.random.default_rng(n)
    return rng.uniform(0.1, 1.0, n), rng.uniform(0.0, 2 * math.pi, n), math.radians(2.0), 5e-5, steps


def medians(runs, reps):
    """runs {name: (fn, blocks per call)} -> {name: blocks/s}: one warm-up each, then `reps` rounds in alternating order."""
    for fn, _ in runs.values():
        fn()
    times = {name: [] for name in runs}
    for r in range(reps):
        for name in (list(runs) if r % 2 == 0 else reversed(list(runs))):
            t = time.perf_counter()
            runs[name][0]()
            times[name].append(time.perf_counter() - t)
    return {name: round(runs[name][1] / float(np.median(times[name])), 1) for name in runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=1024)
    ap.add_argument("--only", default="abc")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="reference,headline")
    a = ap.parse_args()
    for name in a.shapes.split(","):
        arrays, res = SHAPES[name]
        xyz = pkg.create_tiled_antenna(arrays, 1)
        wire = wire_of(a.blocks + 4)
        prime, wire = wire[: 4 * BLOCK_BYTES], wire[4 * BLOCK_BYTES:]
        row = {"shape": name, "mics": xyz.shape[1], "grid": f"{res}x{res}", "blocks": a.blocks,
               "listen_stream": os.environ.get("AWPU_LISTEN_STREAM", "1")}

        def primed(max_batch, table=None):  # (a tracker on a zeroed ring goes NaN: four blocks first)
            eng = engine(xyz, res, max_batch, table)
            for b in range(4):
                eng.ingest_block(prime[b * BLOCK_BYTES: (b + 1) * BLOCK_BYTES])
            return eng

        if "a" in a.only or "b" in a.only:
            with primed(1) as loop_eng, primed(128) as eng:
                nb = min(a.blocks, 256)
                runs = {}
                for label, (n, steps) in SETS.items():
                    who = listeners(n, steps)

                    def loop(who=who):
                        p = who
                        for b in range(nb):
                            loop_eng.ingest_block(wire[b * BLOCK_BYTES: (b + 1) * BLOCK_BYTES])
                            got = loop_eng.track(*p, LIMIT, None, 0, want_beams=True)
                            p = (got.theta, got.phi, got.spread, got.rate, got.steps)

                    if "a" in a.only:
                        runs[f"a_loop_{label}_bps"] = (loop, nb)
                    if "b" in a.only:
                        runs[f"b_listen_{label}_bps"] = (lambda who=who: eng.listen_blocks(wire, *who, LIMIT), a.blocks)
                row.update(medians(runs, a.reps))
        if "c" in a.only:
            table = pkg.build_delay_table(xyz, res, res)
            who = listeners(*SETS["8_tracking"])
            with primed(128, table) as eng, primed(128, table) as sweep:
                row.update(medians({
                    "c_process_blocks_bps": (lambda: sweep.process_blocks(wire), a.blocks),
                    "c_listen_8_tracking_with_power_bps": (lambda: eng.listen_blocks(wire, *who, LIMIT, want_power=True), a.blocks),
                }, a.reps))
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
