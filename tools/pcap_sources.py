#!/usr/bin/env python3
"""The sources in a recorded capture: for a .pcap of FPGA datagrams, the strongest heatmap peaks of every --every'th block, found on
the device while the powers are still there (Engine.find_blocks, include/awpu_hip_find.h), as CSV.  The capture is read by
tools/pcap_heatmaps.py's reader (counter gaps reported, not repaired).

  tools/pcap_sources.py recording.pcap --port 21844 --cols 100 --every 1 --max-sources 4 --min-ratio 0.25 --out sources.csv

--band LO:HI[:TAPS] (Hz; 63 taps unless given) limits the heatmaps to a band, e.g. --band 6375:9000: the sources are those of the band
(Engine.set_band with binding.band_design's coefficients, include/awpu_hip_band.h).

Every block is ingested; every --every'th is swept and searched.  --chunk blocks go to the engine per call, each call continuing
with the `next_first` of the one before, so a long capture streams through bounded memory.

Output: one line per source, strongest first within a block, under the header
    block,rank,pixel,power,row,col,theta,phi
block counts from the first whole block of the capture, rank from 0; power is printed with 9 and the doubles with 17 significant
digits, so that every value parses back to the bits the engine returned; theta and phi are radians and are what
awpu_hip_steering_delays, awpu_hip_steer_table and the listeners of tools/pcap_listen.py take.  A block without a source writes
no line."""
from __future__ import annotations

import argparse
import csv
import importlib
import sys
from pathlib import Path

import numpy as np

HEADER = ["block", "rank", "pixel", "power", "row", "col", "theta", "phi"]


def write_rows(writer, blocks, sources, count) -> int:
    """Lines for the frames of one result: blocks [n_frames] block numbers, sources [n_frames, max_sources] records, count
    [n_frames].  -> lines written."""
    lines = 0
    for block, entries, n in zip(blocks, sources, count):
        for rank in range(int(n)):
            s = entries[rank]
            writer.writerow([int(block), rank, int(s["pixel"]), f"{np.float32(s['power']):.9g}"] +
                            [f"{float(s[name]):.17g}" for name in ("row", "col", "theta", "phi")])
            lines += 1
    return lines


def read_rows(path):
    """-> a structured array with the columns of HEADER (block, rank, pixel int64; power float32; the rest float64)."""
    dtype = np.dtype([("block", "<i8"), ("rank", "<i8"), ("pixel", "<i8"), ("power", "<f4"), ("row", "<f8"), ("col", "<f8"),
                      ("theta", "<f8"), ("phi", "<f8")])
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    if not rows or rows[0] != HEADER:
        raise ValueError(f"{path}: not a sources file (header {rows[:1]})")
    out = np.zeros(len(rows) - 1, dtype)
    for k, row in enumerate(rows[1:]):
        out[k] = (int(row[0]), int(row[1]), int(row[2]), np.float32(row[3]), *(float(v) for v in row[4:]))
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("pcap")
    ap.add_argument("--port", type=int, required=True, help="UDP destination port of the FPGA datagrams")
    ap.add_argument("--arrays", type=int, default=1, help="8x8 arrays side by side (stream id = a*64 + r*8 + c)")
    ap.add_argument("--rows", type=int, default=1, help="rows of arrays")
    ap.add_argument("--cols", type=int, default=100, help="heatmap resolution: cols x cols pixels")
    ap.add_argument("--fov", type=float, default=180.0, help="field of view in degrees")
    ap.add_argument("--every", type=int, default=1, help="search every Nth block")
    ap.add_argument("--radius", type=int, default=2, help="a source beats the (2 * radius + 1)^2 pixels around it")
    ap.add_argument("--max-sources", type=int, default=4, help="sources per block at most")
    ap.add_argument("--min-power", type=float, default=0.0)
    ap.add_argument("--min-ratio", type=float, default=0.25, help="a source has at least this share of its block's maximum")
    ap.add_argument("--chunk", type=int, default=512, help="blocks per engine call")
    ap.add_argument("--max-batch", type=int, default=128, help="frames per sweep launch")
    ap.add_argument("--out", default="sources.csv")
    ap.add_argument("--band", default=None, metavar="LO:HI[:TAPS]", help="limit the heatmaps to LO .. HI Hz (an FIR band of TAPS taps, 63 unless given)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if a.every < 1 or a.chunk < 1:
        ap.error("--every and --chunk are positive")

    sys.path.insert(0, str(Path(__file__).resolve().parent))
    from pcap_heatmaps import blocks_of, read_pcap_payloads

    payloads = read_pcap_payloads(a.pcap, a.port)
    wire, n_blocks, gaps = blocks_of(payloads)
    print(f"{len(payloads)} datagrams to port {a.port}: {n_blocks} blocks, {len(payloads) - 256 * n_blocks} left over")
    for i, missing in gaps:
        print(f"counter gap before datagram {i}: {missing} missing (not repaired)")
    if n_blocks == 0:
        print("no whole block of 256 datagrams")
        return 1

    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    pkg = importlib.import_module("beamforming-lk_amd")
    xyz = pkg.create_tiled_antenna(a.arrays, a.rows)
    off, frac = pkg.build_delay_table(xyz, a.cols, a.cols, a.fov)
    n = xyz.shape[1]
    if n > 256:
        print(f"{n} mics: the wire carries 256 streams per datagram")
        return 1
    searched, lines, first, block_bytes = 0, 0, 0, 256 * 1032
    with open(a.out, "w", newline="") as f, \
            pkg.Engine(n_pixels=a.cols * a.cols, n_streams=n, max_batch=a.max_batch, grid_columns=a.cols, device=a.device) as eng:
        writer = csv.writer(f, lineterminator="\n")
        writer.writerow(HEADER)
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        if a.band:
            eng.set_band(pkg.binding.band_from_text(a.band))
        for b in range(0, n_blocks, a.chunk):
            nb = min(a.chunk, n_blocks - b)
            res = eng.find_blocks(wire[b * block_bytes: (b + nb) * block_bytes], a.cols, a.cols, first=first, every=a.every,
                                  radius=a.radius, max_sources=a.max_sources, min_power=a.min_power, min_ratio=a.min_ratio, fov_deg=a.fov)
            lines += write_rows(writer, b + first + a.every * np.arange(len(res)), res.sources, res.count)
            first = res.next_first
            searched += len(res)
    print(f"{lines} sources in {searched} of {n_blocks} blocks: {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
