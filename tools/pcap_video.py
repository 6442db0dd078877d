#!/usr/bin/env python3
"""The video of a recorded capture: what the reference's GUI loop records with key `r` (src/aw_control_unit/aw_control_unit.cpp:
293-378: populateHeatmap, cv::resize, cv::applyColorMap, the optional cv::flip, videoWriter.write) for a .pcap of FPGA datagrams,
in batched passes on the device (Engine.watch_blocks, include/awpu_hip_watch.h).  The capture is read by tools/pcap_heatmaps.py's
reader (counter gaps reported, not repaired).

  tools/pcap_video.py recording.pcap --port 21844 --cols 100 --every 3 --size 1024 --out heatmap

--band LO:HI[:TAPS] (Hz; 63 taps unless given) limits the heatmaps to a band, e.g. --band 6375:9000: the video shows the band
(Engine.set_band with binding.band_design's coefficients, include/awpu_hip_band.h).

--bands LO:HI[:TAPS],LO:HI[:TAPS],LO:HI[:TAPS] (one to three entries, each as --band takes it) writes the colour-by-frequency
video instead: every band is swept from one pass over the capture (Engine.spectral_blocks, include/awpu_hip_spectral.h) and shown
in a colour of its own -- the lowest band red, the next green, the highest blue; the file's pixels are B, G, R, so byte 0 shows
the highest band --, each level scaled by one maximum per frame over the shown bands (--band-scale per-band: by its band's own).
The colour table plays no part.  --bands together with --band is an error.

--focus METRES focuses the delay table on points METRES away instead of on plane waves (binding.build_focus_table,
include/awpu_hip_focus.h): a large array in a room is in its sources' near field, where a plane-wave table blurs them.

--exposure L integrates every frame over the L blocks that end with its shown block (1 <= L <= --every): the mean of their power
rows, or with --peak-hold their per-pixel maximum (Engine.expose_blocks, include/awpu_hip_expose.h); L * 5.2 ms of sound per
frame instead of 5.2, the open window carried from one --chunk call to the next.  The first frame is then block L - 1's.  Off
unless given; not with --bands.

--coherence [weighted|factor] shows every frame through the coherence sweep (Engine.cohere_blocks, include/awpu_hip_cohere.h): its
delay-and-sum power weighted by the coherence factor, which takes the side lobes of a source out of the picture, or with `factor`
the coherence factor itself.  Off unless given; not with --bands or --exposure.

--peel STEPS[:GAIN] shows every frame peeled (Engine.peel_blocks, include/awpu_hip_peel.h): STEPS rounds of sweep, take the
strongest pixel, subtract its beam from every mic, with loop gain GAIN (1 unless given); the frame is the clean map -- the removed
powers at their pixels -- plus the residual, so a source's side lobes go with the source.  Off unless given; not with --band,
--bands, --exposure or --coherence.

--tone LO:HI[:hann] shows every frame through the tone sweep (Engine.tones_blocks, include/awpu_hip_tones.h): per pixel, the power
of its beam in the 190.7 Hz transform bins whose centres lie in [LO, HI) Hz -- no FIR band, any band at the same cost --, with the
rectangular window or, with `hann`, the Hann window.  --pitch LO:HI[:hann] shows instead the strongest bin of that range per pixel,
brighter where the pitch is higher.  Off unless given; --band applies in front; not with --bands, --exposure, --coherence or
--peel, nor with each other.

--csm LO:HI[:hann] shows every frame through the cross-spectral maps (Engine.csm_watch_blocks, include/awpu_hip_csm_watch.h): the
map of the --csm-length blocks (64 unless given) that end with the shown one, summed over the transform bins whose centres lie in
[LO, HI) Hz -- at most 8 of them --, by --csm-kind conventional (the default), diagonal-removed (uncorrelated microphone
self-noise leaves the picture) or capon[:LOADING] (Capon's minimum-variance map, which separates sources closer than a beam width;
loading 1e-2 unless given).  The window's spectra are carried from one --chunk call to the next.  Off unless given; not with
--band, --bands, --exposure, --coherence, --peel, --tone or --pitch.  With --csm-clean STEPS[:GAIN[:STOP]] every frame's conventional
map is deconvolved by CLEAN-SC (Engine.csm_clean_blocks, include/awpu_hip_csm_clean.h): per bin, STEPS rounds of map, take the
strongest pixel, subtract the part of the matrix coherent with its beam, with loop gain GAIN (1 unless given), a bin ending early
below STOP times its first peak; the frame is the clean map plus the residual, summed over the bins.

Every block is ingested; every --every'th is swept and shown.  The default 3 gives 48828 / (256 * 3) = 63.6 frames per second, the
nearest to the 60 the reference opens its writer with.  --chunk blocks go to the engine per call, each call continuing with the
`next_first` of the one before, so a long capture streams through bounded memory.

Output.  The reference writes MJPG; there is no JPEG encoder here, so the frames are written UNCOMPRESSED: AVI 1.0 files with one
BGR24 `DIB ` stream (rows bottom-up, padded to 4 bytes, one `00db` chunk and one idx1 entry per frame, the exact frame rate as the
rational dwRate / dwScale = 48828 / (256 * every), reduced), written with `struct` alone and split into numbered parts
OUT.000.avi, OUT.001.avi, ... each below 1 GiB (AVI 1.0 stops at the RIFF size field).  --raw writes headerless BGR24 frames, rows
top-down, into OUT.bgr instead (e.g. for `ffmpeg -f rawvideo -pix_fmt bgr24 -s 1024x1024 -r 48828/768 -i OUT.bgr`).

Colours.  OpenCV's COLORMAP_JET / COLORMAP_OCEAN tables are not available here and equality with them is NOT claimed.  The tool
builds a jet-like table of its own, piecewise linear in x = level / 255:
    red = clip(1.5 - |4x - 3|),  green = clip(1.5 - |4x - 2|),  blue = clip(1.5 - |4x - 1|),   clip to [0, 1], times 255, rounded
stored [256][3] in B, G, R order.  --gray shows level v as (v, v, v).  A caller with OpenCV passes its own [256][3] table to
Engine.watch_blocks."""
from __future__ import annotations

import argparse
import importlib
import math
import struct
import sys
from pathlib import Path

import numpy as np

SAMPLE_RATE, BLOCK = 48828, 256
PART_LIMIT = (1 << 30) - 1  # bytes per AVI part, headers and index included


def frame_rate(every: int):
    """(dwRate, dwScale): 48828 / (256 * every) frames per second as a reduced fraction."""
    g = math.gcd(SAMPLE_RATE, BLOCK * every)
    return SAMPLE_RATE // g, BLOCK * every // g


def jet_table() -> np.ndarray:
    """The tool's own jet-like colour table [256][3], B G R (formula in the module docstring)."""
    x = np.arange(256, dtype=np.float64) / 255.0
    ramp = lambda centre: np.clip(1.5 - np.abs(4.0 * x - centre), 0.0, 1.0)
    return np.rint(np.stack([ramp(1.0), ramp(2.0), ramp(3.0)], axis=1) * 255.0).astype(np.uint8)


def gray_table() -> np.ndarray:
    return np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)


class AviWriter:
    """Uncompressed BGR24 AVI 1.0 files PREFIX.000.avi, PREFIX.001.avi, ...: a new part begins before one would pass `limit`
    bytes.  write() takes a frame [height][width][3] uint8, B G R, rows top-down."""

    HEADER = 12 + (12 + (8 + 56) + (12 + (8 + 56) + (8 + 40))) + 12  # RIFF, hdrl (avih, strl (strh, strf)), LIST movi

    def __init__(self, prefix, width: int, height: int, every: int, limit: int = PART_LIMIT):
        self.prefix, self.width, self.height, self.limit = str(prefix), width, height, limit
        self.rate, self.scale = frame_rate(every)
        self.row = (3 * width + 3) & ~3
        self.frame_bytes = self.row * height
        if self._size_with(1) > limit:
            raise ValueError(f"one {width} x {height} frame does not fit a part of {limit} bytes")
        self.paths, self.file, self.index = [], None, []

    def _header(self, n_frames: int) -> bytes:
        movi = 4 + n_frames * (8 + self.frame_bytes)
        total = self.HEADER - 8 + n_frames * (8 + self.frame_bytes) + 8 + 16 * n_frames
        avih = struct.pack("<14I", self.scale * 1000000 // self.rate, self.frame_bytes * self.rate // self.scale + 1, 0, 0x10, n_frames, 0, 1,
                           self.frame_bytes, self.width, self.height, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIII4h", b"vids", b"DIB ", 0, 0, 0, 0, self.scale, self.rate, 0, n_frames, self.frame_bytes,
                           0xFFFFFFFF, 0, 0, 0, self.width, self.height)
        strf = struct.pack("<IiiHHIIiiII", 40, self.width, self.height, 1, 24, 0, self.frame_bytes, 0, 0, 0, 0)  # height > 0: bottom-up
        strl = b"LIST" + struct.pack("<I", 4 + 8 + len(strh) + 8 + len(strf)) + b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + \
            b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"LIST" + struct.pack("<I", 4 + 8 + len(avih) + len(strl)) + b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + strl
        out = b"RIFF" + struct.pack("<I", total) + b"AVI " + hdrl + b"LIST" + struct.pack("<I", movi) + b"movi"
        assert len(out) == self.HEADER
        return out

    def _size_with(self, n_frames: int) -> int:
        return self.HEADER + n_frames * (8 + self.frame_bytes) + 8 + 16 * n_frames

    def _finish(self):
        if self.file is None:
            return
        n = len(self.index)
        self.file.write(b"idx1" + struct.pack("<I", 16 * n))
        for k in range(n):
            self.file.write(struct.pack("<4sIII", b"00db", 0x10, 4 + k * (8 + self.frame_bytes), self.frame_bytes))
        self.file.seek(0)
        self.file.write(self._header(n))
        self.file.close()
        self.file, self.index = None, []

    def write(self, frame: np.ndarray) -> None:
        if frame.shape != (self.height, self.width, 3) or frame.dtype != np.uint8:
            raise ValueError(f"a frame is uint8 [{self.height}][{self.width}][3]")
        if self.file is not None and self._size_with(len(self.index) + 1) > self.limit:
            self._finish()
        if self.file is None:
            self.paths.append(f"{self.prefix}.{len(self.paths):03d}.avi")
            self.file = open(self.paths[-1], "wb")
            self.file.write(self._header(0))
        rows = frame[::-1]  # a positive biHeight means the bottom row comes first
        if self.row != 3 * self.width:
            padded = np.zeros((self.height, self.row), np.uint8)
            padded[:, : 3 * self.width] = rows.reshape(self.height, 3 * self.width)
            rows = padded
        self.file.write(b"00db" + struct.pack("<I", self.frame_bytes))
        self.file.write(np.ascontiguousarray(rows).tobytes())
        self.index.append(len(self.index))

    def close(self) -> list:
        self._finish()
        return self.paths

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def read_avi(path):
    """-> (frames [n][height][width][3] top-down, dwRate, dwScale) of a file AviWriter wrote, checking the sizes that frame it."""
    blob = Path(path).read_bytes()
    riff, size, avi = struct.unpack("<4sI4s", blob[:12])
    assert riff == b"RIFF" and avi == b"AVI " and size == len(blob) - 8
    avih = struct.unpack("<14I", blob[32: 32 + 56])
    n, width, height = avih[4], avih[8], avih[9]
    strh = struct.unpack("<4s4sIHHIIIIIIII4h", blob[108: 108 + 56])
    assert strh[0] == b"vids" and strh[1] == b"DIB " and strh[9] == n
    scale, rate = strh[6], strh[7]
    strf = struct.unpack("<IiiHHIIiiII", blob[172: 172 + 40])
    assert strf[:6] == (40, width, height, 1, 24, 0)
    row = (3 * width + 3) & ~3
    off = AviWriter.HEADER
    assert blob[off - 12: off - 8] == b"LIST" and blob[off - 4: off] == b"movi"
    assert struct.unpack("<I", blob[off - 8: off - 4])[0] == 4 + n * (8 + row * height)
    frames = []
    for k in range(n):
        cid, nbytes = struct.unpack("<4sI", blob[off: off + 8])
        assert cid == b"00db" and nbytes == row * height
        rows = np.frombuffer(blob, np.uint8, nbytes, off + 8).reshape(height, row)[:, : 3 * width]
        frames.append(rows.reshape(height, width, 3)[::-1])
        off += 8 + nbytes
    cid, nbytes = struct.unpack("<4sI", blob[off: off + 8])
    assert cid == b"idx1" and nbytes == 16 * n and off + 8 + nbytes == len(blob)
    for k in range(n):
        assert struct.unpack("<4sIII", blob[off + 8 + 16 * k: off + 24 + 16 * k]) == (b"00db", 0x10, 4 + k * (8 + row * height), row * height)
    return np.stack(frames) if frames else np.zeros((0, height, width, 3), np.uint8), rate, scale


def bands_of_text(binding, text: str):
    """--bands' text -> (the bands' coefficients, lowest band first; the band shown in byte 0, 1, 2 of a B G R pixel)."""
    entries = [e for e in text.split(",")]
    if not 1 <= len(entries) <= 3:
        raise ValueError(f"bands '{text}': one to three LO:HI[:TAPS] entries, separated by commas")
    entries.sort(key=lambda e: float(e.split(":")[0]))  # (band_from_text judges the entry itself)
    bands = [binding.band_from_text(e) for e in entries]
    return bands, tuple(2 - c if 2 - c < len(bands) else -1 for c in range(3))  # red (byte 2) = band 0, green = band 1, blue = band 2


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
    ap.add_argument("--every", type=int, default=3, help="show every Nth block (3: 63.6 frames per second)")
    ap.add_argument("--size", type=int, default=1024, help="the video is size x size pixels (X_RES / Y_RES)")
    ap.add_argument("--flip", action="store_true", help="mirror left-right, cv::flip(frame, frame, 1)")
    ap.add_argument("--gray", action="store_true", help="levels as grey instead of the jet-like table")
    ap.add_argument("--chunk", type=int, default=96, help="blocks per engine call")
    ap.add_argument("--max-batch", type=int, default=32, help="frames per sweep launch (and per display piece held in memory)")
    ap.add_argument("--raw", action="store_true", help="headerless BGR24 frames into OUT.bgr instead of AVI parts")
    ap.add_argument("--out", default="heatmap", help="output prefix")
    ap.add_argument("--band", default=None, metavar="LO:HI[:TAPS]", help="limit the heatmaps to LO .. HI Hz (an FIR band of TAPS taps, 63 unless given)")
    ap.add_argument("--bands", default=None, metavar="LO:HI[:TAPS],...", help="one to three bands, each in a colour of its own: lowest red, next green, highest blue")
    ap.add_argument("--band-scale", default="common", choices=("common", "per-band"), help="--bands: one maximum per frame over the bands, or each band's own")
    ap.add_argument("--focus", type=float, default=None, metavar="METRES",
                    help="focus the delay table on points METRES away instead of on plane waves (include/awpu_hip_focus.h)")
    ap.add_argument("--exposure", type=int, default=None, metavar="L",
                    help="integrate every frame over the L blocks that end with its shown block, 1 <= L <= --every (include/awpu_hip_expose.h)")
    ap.add_argument("--peak-hold", action="store_true", help="--exposure: the per-pixel maximum of the L blocks instead of their mean")
    ap.add_argument("--coherence", nargs="?", const="weighted", default=None, choices=("weighted", "factor"),
                    help="show the coherence-weighted power, or the coherence factor itself (include/awpu_hip_cohere.h)")
    ap.add_argument("--peel", default=None, metavar="STEPS[:GAIN]",
                    help="show every frame peeled: the clean map plus the residual after STEPS steps (include/awpu_hip_peel.h)")
    ap.add_argument("--tone", default=None, metavar="LO:HI[:hann]",
                    help="show the power in the transform bins between LO and HI Hz of every pixel's beam (include/awpu_hip_tones.h)")
    ap.add_argument("--pitch", default=None, metavar="LO:HI[:hann]",
                    help="show every pixel's strongest bin between LO and HI Hz: brighter where the pitch is higher")
    ap.add_argument("--csm", default=None, metavar="LO:HI[:hann]",
                    help="show the cross-spectral map of the transform bins between LO and HI Hz, at most 8 (include/awpu_hip_csm_watch.h)")
    ap.add_argument("--csm-kind", default="conventional", metavar="conventional|diagonal-removed|capon[:LOADING]", help="--csm: which map")
    ap.add_argument("--csm-length", type=int, default=64, metavar="L", help="--csm: every frame's matrix is added up over the L blocks that end with it")
    ap.add_argument("--csm-clean", default=None, metavar="STEPS[:GAIN[:STOP]]",
                    help="--csm: show every frame deconvolved by CLEAN-SC, the clean map plus the residual after STEPS steps a bin (include/awpu_hip_csm_clean.h)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if a.csm and (a.band or a.bands or a.exposure is not None or a.coherence or a.peel or a.tone or a.pitch):
        ap.error("--csm together with --band, --bands, --exposure, --coherence, --peel, --tone or --pitch: the cross-spectral maps choose their bins themselves")
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
    if a.tone and a.pitch:
        ap.error("--tone together with --pitch: one row per frame")
    if (a.tone or a.pitch) and (a.bands or a.exposure is not None or a.coherence or a.peel):
        ap.error("--tone and --pitch together with --bands, --exposure, --coherence or --peel: those runs are not swept for tones")
    if a.tone or a.pitch:
        # (the one parser of LO:HI[:hann] is the binding's, and which bins a range takes is the library's to say: both are
        # asked here, before the capture is opened)
        sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
        try:
            tone_groups = importlib.import_module("beamforming-lk_amd").binding.tones_from_text(a.tone or a.pitch)
        except ValueError as e:
            ap.error(str(e))
    if a.peel and (a.bands or a.band or a.exposure is not None or a.coherence):
        ap.error("--peel together with --band, --bands, --exposure or --coherence: those runs are not peeled")
    if a.peel:
        try:
            peel = peel_of_text(a.peel)
        except ValueError as e:
            ap.error(str(e))
    if a.every < 1 or a.chunk < 1 or a.size < a.cols:
        ap.error("--every and --chunk are positive, --size is at least --cols")
    if a.exposure is not None and not 1 <= a.exposure <= a.every:
        ap.error("--exposure is between 1 and --every")
    if a.exposure is not None and a.bands:
        ap.error("--exposure together with --bands: spectral runs are not exposed")
    if a.peak_hold and a.exposure is None:
        ap.error("--peak-hold needs --exposure")
    if a.coherence and (a.bands or a.exposure is not None):
        ap.error("--coherence together with --bands or --exposure: those runs are not swept for coherence")
    if a.band and a.bands:
        ap.error("--bands together with --band: one band through the colour table, or several bands as colours")

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
    import torch

    xyz = pkg.create_tiled_antenna(a.arrays, a.rows)
    if a.focus is not None:
        off, frac = pkg.build_focus_table(xyz, a.cols, a.cols, a.focus, a.fov)
    else:
        off, frac = pkg.build_delay_table(xyz, a.cols, a.cols, a.fov)
    n = xyz.shape[1]
    if n > 256:
        print(f"{n} mics: the wire carries 256 streams per datagram")
        return 1
    table = torch.from_numpy(gray_table() if a.gray else jet_table()).to(f"cuda:{a.device}")
    if a.bands:
        bands, channel = bands_of_text(pkg.binding, a.bands)
        band_scale = pkg.binding.SPECTRAL_SCALE_COMMON if a.band_scale == "common" else pkg.binding.SPECTRAL_SCALE_PER_BAND
    rate, scale = frame_rate(a.every)
    shown, first, block_bytes, res = 0, 0, 256 * 1032, None
    carry, carried = None, 0
    if a.exposure is not None:
        first, mode = a.exposure - 1, pkg.binding.EXPOSE_PEAK if a.peak_hold else pkg.binding.EXPOSE_MEAN
    raw = open(f"{a.out}.bgr", "wb") if a.raw else None
    writer = None if a.raw else AviWriter(a.out, a.size, a.size, a.every)
    with pkg.Engine(n_pixels=a.cols * a.cols, n_streams=n, max_batch=a.max_batch, grid_columns=a.cols, device=a.device) as eng:
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        if a.band:
            eng.set_band(pkg.binding.band_from_text(a.band))
        for b in range(0, n_blocks, a.chunk):
            nb = min(a.chunk, n_blocks - b)
            if a.bands:
                res = eng.spectral_blocks(wire[b * block_bytes: (b + nb) * block_bytes], a.cols, a.cols, bands, channel, band_scale, first=first,
                                          every=a.every, out_rows=a.size, out_cols=a.size, flip=a.flip, want_image=False, want_dominant=False)
            elif a.exposure is not None:
                res = eng.expose_blocks(wire[b * block_bytes: (b + nb) * block_bytes], a.cols, a.cols, a.exposure, first=first, every=a.every,
                                        mode=mode, carry=carry, out_rows=a.size, out_cols=a.size, d_colormap_ptr=table.data_ptr(), flip=a.flip,
                                        want_image=False)
                carry = res.carry
            elif a.peel:
                res = eng.peel_blocks(wire[b * block_bytes: (b + nb) * block_bytes], a.cols, a.cols, peel[0], peel[1], first=first, every=a.every,
                                      out_rows=a.size, out_cols=a.size, d_colormap_ptr=table.data_ptr(), flip=a.flip, want_image=False)
            elif a.tone or a.pitch:
                res = eng.tones_blocks(wire[b * block_bytes: (b + nb) * block_bytes], a.cols, a.cols, tone_groups,
                                       show=0 if a.tone else pkg.binding.TONES_SHOW_PITCH, first=first, every=a.every, out_rows=a.size,
                                       out_cols=a.size, d_colormap_ptr=table.data_ptr(), flip=a.flip, want_image=False)
            elif a.csm and a.csm_clean:
                res = eng.csm_clean_blocks(wire[b * block_bytes: (b + nb) * block_bytes], a.cols, a.cols, csm_bins, *csm_clean, window=csm_window,
                                           length=a.csm_length, first=first, every=a.every, carry=carry, carried=carried, out_rows=a.size,
                                           out_cols=a.size, d_colormap_ptr=table.data_ptr(), flip=a.flip, want_image=False)
                carry, carried = res.carry, res.carried
            elif a.csm:
                res = eng.csm_watch_blocks(wire[b * block_bytes: (b + nb) * block_bytes], a.cols, a.cols, csm_bins, csm_window, csm_kind, csm_loading,
                                           a.csm_length, pkg.binding.CSM_SHOW_SUM, first=first, every=a.every, carry=carry, carried=carried,
                                           out_rows=a.size, out_cols=a.size, d_colormap_ptr=table.data_ptr(), flip=a.flip, want_image=False)
                carry, carried = res.carry, res.carried
            elif a.coherence:
                show = pkg.binding.COHERE_FACTOR if a.coherence == "factor" else pkg.binding.COHERE_WEIGHTED
                res = eng.cohere_blocks(wire[b * block_bytes: (b + nb) * block_bytes], a.cols, a.cols, first=first, every=a.every, show=show,
                                        out_rows=a.size, out_cols=a.size, d_colormap_ptr=table.data_ptr(), flip=a.flip, want_image=False)
            else:
                res = eng.watch_blocks(wire[b * block_bytes: (b + nb) * block_bytes], a.cols, a.cols, first=first, every=a.every,
                                       out_rows=a.size, out_cols=a.size, d_colormap_ptr=table.data_ptr(), flip=a.flip, want_image=False,
                                       out=res)  # (the frames of the chunk before are in the file)
            first = res.next_first
            for frame in res.big:
                raw.write(frame.tobytes()) if raw else writer.write(frame)
            shown += len(res.big)
    if raw:
        raw.close()
        files = [f"{a.out}.bgr"]
    else:
        files = writer.close()
    print(f"{shown} frames of {a.size} x {a.size} at {rate}/{scale} = {rate / scale:.3f} per second: {', '.join(files) or 'nothing written'}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
