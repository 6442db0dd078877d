#!/usr/bin/env python3
"""The sources in a recorded capture: for a .pcap of FPGA datagrams, the strongest heatmap peaks of every --every'th block, found on
the device while the powers are still there (Engine.find_blocks, include/awpu_hip_find.h), as CSV.  The capture is read by
tools/pcap_heatmaps.py's reader (counter gaps reported, not repaired).

  tools/pcap_sources.py recording.pcap --port 21844 --cols 100 --every 1 --max-sources 4 --min-ratio 0.25 --out sources.csv

--band LO:HI[:TAPS] (Hz; 63 taps unless given) limits the heatmaps to a band, e.g. --band 6375:9000: the sources are those of the band
(Engine.set_band with binding.band_design's coefficients, include/awpu_hip_band.h).

--focus METRES focuses the delay table on points METRES away instead of on plane waves (binding.build_focus_table,
include/awpu_hip_focus.h): what a large array needs for anything in a room.  --range LO:HI:N also ranges every source: the beam power
at its direction is swept over N focus distances from LO to HI metres, uniform in 1 / d (HI may be inf), on the block's raw samples
while they are on the device (Engine.locate_blocks), and the distance at which it peaks is written as a last column, `distance`
(metres, 17 significant digits; inf: a plane wave).

--exposure L searches heatmaps integrated over the L blocks that end with every --every'th (1 <= L <= --every): the mean of their
power rows (Engine.expose_blocks, include/awpu_hip_expose.h), which steadies the peaks of a noise-like source; the open window is
carried from one --chunk call to the next, and the first block searched is then block L - 1.  Off unless given; not with --range.

--coherence [weighted|factor] searches the rows of the coherence sweep (Engine.cohere_blocks, include/awpu_hip_cohere.h): the power
weighted by the coherence factor -- a source's side lobes are then no sources --, or with `factor` the coherence factor itself; the
`power` column is that row's value.  Off unless given; not with --exposure or --range.

--peel STEPS[:GAIN] peels every searched block (Engine.peel_blocks, include/awpu_hip_peel.h): STEPS rounds of sweep, take the
strongest pixel, subtract its beam from every mic, with loop gain GAIN (1 unless given).  A block's sources are then its steps
merged per pixel -- the entries of its clean map, strongest first, `power` what the steps removed there, row and col the pixel's
own --, which lists a weak source under a strong one's side lobes and not the side lobes.  Off unless given; not with --band,
--exposure, --coherence or --range.

--tone LO:HI[:hann] searches the rows of the tone sweep (Engine.tones_blocks, include/awpu_hip_tones.h): per pixel, the power of its
beam in the 190.7 Hz transform bins whose centres lie in [LO, HI) Hz (`hann`: behind a Hann window); the `power` column is that
row's value.  Off unless given; --band applies in front; not with --exposure, --coherence, --peel or --range.

--csm LO:HI[:hann] searches the cross-spectral maps (Engine.csm_watch_blocks, include/awpu_hip_csm_watch.h): the map of the
--csm-length blocks (64 unless given) that end with the searched one, summed over the transform bins whose centres lie in [LO, HI)
Hz -- at most 8 of them --, by --csm-kind conventional (the default), diagonal-removed or capon[:LOADING] (Capon's minimum-variance
map, which separates two sources closer than a beam width; loading 1e-2 unless given); the `power` column is that map's value.
Off unless given; not with --band, --exposure, --coherence, --peel, --range or --tone.  With --csm-clean STEPS[:GAIN[:STOP]] every
searched conventional map is deconvolved by CLEAN-SC (Engine.csm_clean_blocks, include/awpu_hip_csm_clean.h), and the sources are
its steps merged per pixel over steps and bins, as with --peel: the `power` column is the power removed there.

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


def write_rows(writer, blocks, sources, count, ranges=None) -> int:
    """Lines for the frames of one result: blocks [n_frames] block numbers, sources [n_frames, max_sources] records, count
    [n_frames]; ranges [n_frames, max_sources] records or None (--range: the `distance` column).  -> lines written."""
    lines = 0
    for j, (block, entries, n) in enumerate(zip(blocks, sources, count)):
        for rank in range(int(n)):
            s = entries[rank]
            writer.writerow([int(block), rank, int(s["pixel"]), f"{np.float32(s['power']):.9g}"] +
                            [f"{float(s[name]):.17g}" for name in ("row", "col", "theta", "phi")] +
                            ([] if ranges is None else [f"{float(ranges[j][rank]['distance']):.17g}"]))
            lines += 1
    return lines


def read_rows(path):
    """-> a structured array with the columns of HEADER (block, rank, pixel int64; power float32; the rest float64), and
    `distance` (float64) where the file has that column."""
    fields = [("block", "<i8"), ("rank", "<i8"), ("pixel", "<i8"), ("power", "<f4"), ("row", "<f8"), ("col", "<f8"),
              ("theta", "<f8"), ("phi", "<f8")]
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    if not rows or rows[0] not in (HEADER, HEADER + ["distance"]):
        raise ValueError(f"{path}: not a sources file (header {rows[:1]})")
    out = np.zeros(len(rows) - 1, np.dtype(fields + ([("distance", "<f8")] if len(rows[0]) > len(HEADER) else [])))
    for k, row in enumerate(rows[1:]):
        out[k] = (int(row[0]), int(row[1]), int(row[2]), np.float32(row[3]), *(float(v) for v in row[4:]))
    return out


def candidates_from_text(pkg, text: str) -> np.ndarray:
    """'LO:HI:N' (metres, HI may be inf; 2 <= N <= 64) -> N candidate distances uniform in 1 / d."""
    parts = text.split(":")
    if len(parts) != 3:
        raise ValueError(f"range '{text}': LO:HI:N, in metres")
    lo, hi, n = float(parts[0]), float(parts[1]), int(parts[2])
    if not (0.0 < lo < hi) or not 2 <= n <= pkg.binding.RANGE_MAX_CANDIDATES:
        raise ValueError(f"range '{text}': 0 < LO < HI and 2 <= N <= {pkg.binding.RANGE_MAX_CANDIDATES}")
    return pkg.range_candidates(lo, hi, n)


def peel_of_text(text: str):
    """"STEPS[:GAIN]" (--peel) -> (steps, gain): steps in [1, 32], gain in (0, 1], 1 unless given."""
    parts = text.split(":")
    if len(parts) not in (1, 2):
        raise ValueError("--peel takes STEPS[:GAIN]")
    steps, gain = int(parts[0]), float(parts[1]) if len(parts) == 2 else 1.0
    if not 1 <= steps <= 32 or not 0.0 < gain <= 1.0:
        raise ValueError("--peel: STEPS in [1, 32], GAIN in (0, 1]")
    return steps, gain


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
    ap.add_argument("--focus", type=float, default=None, metavar="METRES", help="focus the delay table on points METRES away (default: plane waves)")
    ap.add_argument("--range", default=None, metavar="LO:HI:N", dest="range_",
                    help="range every source over N focus distances from LO to HI metres, uniform in 1 / d: the `distance` column")
    ap.add_argument("--exposure", type=int, default=None, metavar="L",
                    help="search heatmaps integrated over the L blocks that end with the searched one, 1 <= L <= --every (include/awpu_hip_expose.h)")
    ap.add_argument("--coherence", nargs="?", const="weighted", default=None, choices=("weighted", "factor"),
                    help="search the coherence-weighted power, or the coherence factor itself (include/awpu_hip_cohere.h)")
    ap.add_argument("--peel", default=None, metavar="STEPS[:GAIN]",
                    help="peel every searched block: its sources are the steps merged per pixel (include/awpu_hip_peel.h)")
    ap.add_argument("--tone", default=None, metavar="LO:HI[:hann]",
                    help="search the power in the transform bins between LO and HI Hz of every pixel's beam (include/awpu_hip_tones.h)")
    ap.add_argument("--csm", default=None, metavar="LO:HI[:hann]",
                    help="search the cross-spectral map of the transform bins between LO and HI Hz, at most 8 (include/awpu_hip_csm_watch.h)")
    ap.add_argument("--csm-kind", default="conventional", metavar="conventional|diagonal-removed|capon[:LOADING]", help="--csm: which map")
    ap.add_argument("--csm-length", type=int, default=64, metavar="L", help="--csm: every searched map's matrix is added up over the L blocks that end with it")
    ap.add_argument("--csm-clean", default=None, metavar="STEPS[:GAIN[:STOP]]",
                    help="--csm: deconvolve every searched map by CLEAN-SC; its sources are the steps merged per pixel (include/awpu_hip_csm_clean.h)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if a.csm and (a.band or a.exposure is not None or a.range_ or a.coherence or a.peel or a.tone):
        ap.error("--csm together with --band, --exposure, --range, --coherence, --peel or --tone: the cross-spectral maps choose their bins themselves")
    if a.csm:
        sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
        binding = importlib.import_module("beamforming-lk_amd").binding
        try:
            csm_bins, csm_window = binding.csm_from_text(a.csm)
            csm_kind, csm_loading = binding.csm_kind_from_text(a.csm_kind)
        except ValueError as e:
            ap.error(str(e))
        if not 1 <= a.csm_length <= binding.CSM_MAX_LENGTH:
            ap.error(f"--csm-length is between 1 and {binding.CSM_MAX_LENGTH}")
        if a.csm_clean:
            try:
                csm_clean = binding.csm_clean_from_text(a.csm_clean)
            except ValueError as e:
                ap.error(str(e))
            if csm_kind != binding.CSM_CONVENTIONAL:
                ap.error("--csm-clean deconvolves the conventional map: not with --csm-kind diagonal-removed or capon")
    elif a.csm_clean:
        ap.error("--csm-clean goes with --csm")
    if a.tone and (a.exposure is not None or a.range_ or a.coherence or a.peel):
        ap.error("--tone together with --exposure, --range, --coherence or --peel: those runs are not swept for tones")
    if a.tone:
        # (the one parser of LO:HI[:hann] is the binding's, and which bins a range takes is the library's to say: both are
        # asked here, before the capture is opened)
        sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
        try:
            tone_groups = importlib.import_module("beamforming-lk_amd").binding.tones_from_text(a.tone)
        except ValueError as e:
            ap.error(str(e))
    if a.peel and (a.exposure is not None or a.range_ or a.coherence or a.band):
        ap.error("--peel together with --exposure, --range, --coherence or --band: those runs are not peeled")
    if a.peel:
        try:
            peel = peel_of_text(a.peel)
        except ValueError as e:
            ap.error(str(e))
    if a.every < 1 or a.chunk < 1:
        ap.error("--every and --chunk are positive")
    if a.coherence and (a.exposure is not None or a.range_):
        ap.error("--coherence together with --exposure or --range: those runs are not swept for coherence")
    if a.exposure is not None and not 1 <= a.exposure <= a.every:
        ap.error("--exposure is between 1 and --every")
    if a.exposure is not None and a.range_:
        ap.error("--exposure together with --range: locate runs are not exposed")

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
    if a.focus is not None:
        off, frac = pkg.build_focus_table(xyz, a.cols, a.cols, a.focus, a.fov)
    else:
        off, frac = pkg.build_delay_table(xyz, a.cols, a.cols, a.fov)
    candidates = candidates_from_text(pkg, a.range_) if a.range_ else None
    n = xyz.shape[1]
    if n > 256:
        print(f"{n} mics: the wire carries 256 streams per datagram")
        return 1
    searched, lines, first, block_bytes = 0, 0, 0 if a.exposure is None else a.exposure - 1, 256 * 1032
    carry, carried = None, 0
    with open(a.out, "w", newline="") as f, \
            pkg.Engine(n_pixels=a.cols * a.cols, n_streams=n, max_batch=a.max_batch, grid_columns=a.cols, device=a.device) as eng:
        writer = csv.writer(f, lineterminator="\n")
        writer.writerow(HEADER + (["distance"] if candidates is not None else []))
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        if candidates is not None:
            eng.set_antenna(xyz)
        if a.band:
            eng.set_band(pkg.binding.band_from_text(a.band))
        for b in range(0, n_blocks, a.chunk):
            nb = min(a.chunk, n_blocks - b)
            find = dict(first=first, every=a.every, radius=a.radius, max_sources=a.max_sources, min_power=a.min_power, min_ratio=a.min_ratio,
                        fov_deg=a.fov)
            chunk = wire[b * block_bytes: (b + nb) * block_bytes]
            if a.exposure is not None:
                what = {k: v for k, v in find.items() if k not in ("first", "every")}
                res = eng.expose_blocks(chunk, a.cols, a.cols, a.exposure, first=first, every=a.every, carry=carry, want_image=False, find=what)
                carry = res.carry
            elif a.peel:
                res = eng.peel_blocks(chunk, a.cols, a.cols, peel[0], peel[1], first=first, every=a.every, want_image=False)
                res.sources, res.count = pkg.binding.peel_source_records(res.steps, a.cols, a.cols, a.max_sources, a.fov)
            elif a.tone:
                what = {k: v for k, v in find.items() if k not in ("first", "every")}
                res = eng.tones_blocks(chunk, a.cols, a.cols, tone_groups, first=first, every=a.every, want_image=False,
                                       find=what)
            elif a.csm and a.csm_clean:
                res = eng.csm_clean_blocks(chunk, a.cols, a.cols, csm_bins, *csm_clean, window=csm_window, length=a.csm_length, first=first,
                                           every=a.every, carry=carry, carried=carried, want_image=False)
                carry, carried = res.carry, res.carried
                res.sources, res.count = pkg.binding.csm_clean_source_records(res.steps, a.cols, a.cols, a.max_sources, a.fov)
            elif a.csm:
                what = {k: v for k, v in find.items() if k not in ("first", "every")}
                res = eng.csm_watch_blocks(chunk, a.cols, a.cols, csm_bins, csm_window, csm_kind, csm_loading, a.csm_length, pkg.binding.CSM_SHOW_SUM,
                                           first=first, every=a.every, carry=carry, carried=carried, want_image=False, find=what)
                carry, carried = res.carry, res.carried
            elif a.coherence:
                what = {k: v for k, v in find.items() if k not in ("first", "every")}
                show = pkg.binding.COHERE_FACTOR if a.coherence == "factor" else pkg.binding.COHERE_WEIGHTED
                res = eng.cohere_blocks(chunk, a.cols, a.cols, first=first, every=a.every, show=show, want_image=False, find=what)
            else:
                res = eng.find_blocks(chunk, a.cols, a.cols, **find) if candidates is None else eng.locate_blocks(chunk, a.cols, a.cols, candidates, **find)
            lines += write_rows(writer, b + first + a.every * np.arange(len(res)), res.sources, res.count, getattr(res, "ranges", None))
            first = res.next_first
            searched += len(res)
    print(f"{lines} sources in {searched} of {n_blocks} blocks: {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
