#!/usr/bin/env python3
"""Listen to a recorded capture -- the reference's --miso mode (MISOWorker, src/dsp/miso.cpp:27-55, and AudioWrapper's
output.wav, src/audio/audio_wrapper.cpp:34-36, :76) over a .pcap instead of a live FPGA: every listener is a steered direction
that may follow its source, and its delayed-and-summed signal is one channel of a float32 WAV at 48 828 Hz
(Engine.listen_blocks, include/awpu_hip_listen.h).  The capture is read by tools/pcap_heatmaps.py's reader.

  tools/pcap_listen.py recording.pcap --port 21844 --listen 20,35 --listen 60,215 --steps 3 --out DIR [--heatmaps --cols 100]

--listen THETA,PHI in degrees, once per listener.  --steps gradient steps per block (0: fixed directions).  The first
--settle blocks are listened to with steps = 0: a new engine's history is zeros, and a tracker that divides its gradient by the
reference power of an empty block never recovers (awpu_hip_listen.h, "A hazard").
Writes DIR/listen.wav (one channel per listener), DIR/trail.npy [n_blocks][n] records (theta, phi, gradient, error, powers after
every block) and with --heatmaps DIR/power.npy [n_blocks][cols][cols]."""
from __future__ import annotations

import argparse
import importlib
import importlib.util
import struct
import sys
from pathlib import Path

import numpy as np

SAMPLE_RATE = 48828  # src/geometry/antenna.h:16-21
WAVE_FORMAT_IEEE_FLOAT = 3


def _reader():
    spec = importlib.util.spec_from_file_location("pcap_heatmaps", Path(__file__).resolve().parent / "pcap_heatmaps.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def wav_bytes(audio: np.ndarray, rate: int = SAMPLE_RATE) -> bytes:
    """audio [channels, frames] float32 -> a RIFF/WAVE file of IEEE float samples, interleaved: the 'fmt ' chunk with the
    extension size field and the 'fact' chunk that non-PCM formats carry, then 'data'."""
    audio = np.atleast_2d(np.asarray(audio, np.float32))
    channels, frames = audio.shape
    if not 1 <= channels <= 65535:
        raise ValueError("a WAV file holds 1 .. 65535 channels")
    data = np.ascontiguousarray(audio.T).astype("<f4").tobytes()
    if len(data) + 50 > 0xFFFFFFFF:
        raise ValueError("more than 4 GiB of samples: split the recording")
    block_align = 4 * channels
    fmt = struct.pack("<4sIHHIIHHH", b"fmt ", 18, WAVE_FORMAT_IEEE_FLOAT, channels, rate, rate * block_align, block_align, 32, 0)
    fact = struct.pack("<4sII", b"fact", 4, frames)
    body = b"WAVE" + fmt + fact + struct.pack("<4sI", b"data", len(data)) + data + (b"\0" if len(data) & 1 else b"")
    return struct.pack("<4sI", b"RIFF", len(body)) + body


def settle_split(n_blocks: int, settle: int, steps: int):
    """The run as [(first block, blocks, steps per block)]: the first `settle` blocks fixed, the rest tracked."""
    head = min(max(settle, 0), n_blocks) if steps > 0 else 0
    return [part for part in ((0, head, 0), (head, n_blocks - head, steps)) if part[1] > 0]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("pcap")
    ap.add_argument("--port", type=int, required=True, help="UDP destination port of the FPGA datagrams")
    ap.add_argument("--listen", action="append", required=True, metavar="THETA,PHI", help="a listener's start direction, degrees")
    ap.add_argument("--steps", type=int, default=3, help="gradient steps per block (MISOWorker: 3); 0 = fixed directions")
    ap.add_argument("--settle", type=int, default=4, help="blocks listened to without tracking first")
    ap.add_argument("--spread", type=float, default=2.0, help="monopulse spread, degrees (TRACKER_SPREAD)")
    ap.add_argument("--rate", type=float, default=5e-5, help="step size (MISOWorker: PARTICLE_RATE / 10)")
    ap.add_argument("--theta-limit", type=float, default=90.0, help="clip of theta, degrees")
    ap.add_argument("--arrays", type=int, default=1, help="8x8 arrays side by side (stream id = a*64 + r*8 + c)")
    ap.add_argument("--rows", type=int, default=1, help="rows of arrays")
    ap.add_argument("--heatmaps", action="store_true", help="the heatmaps of the same blocks too")
    ap.add_argument("--cols", type=int, default=100, help="heatmap resolution: cols x cols pixels")
    ap.add_argument("--fov", type=float, default=180.0, help="field of view in degrees")
    ap.add_argument("--max-batch", type=int, default=128, help="blocks per chunk")
    ap.add_argument("--out", default=".", help="directory for listen.wav, trail.npy and power.npy")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)

    reader = _reader()
    start = np.radians(np.array([[float(v) for v in d.split(",")] for d in a.listen], np.float64).reshape(-1, 2))
    payloads = reader.read_pcap_payloads(a.pcap, a.port)
    wire, n_blocks, gaps = reader.blocks_of(payloads)
    print(f"{len(payloads)} datagrams to port {a.port}: {n_blocks} blocks, {len(payloads) - 256 * n_blocks} left over")
    for i, missing in gaps:
        print(f"counter gap before datagram {i}: {missing} missing (not repaired)")
    if n_blocks == 0:
        print("no whole block of 256 datagrams")
        return 1

    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    pkg = importlib.import_module("beamforming-lk_amd")
    xyz = pkg.create_tiled_antenna(a.arrays, a.rows)
    n = xyz.shape[1]
    if n > 256:
        print(f"{n} mics: the wire carries 256 streams per datagram")
        return 1
    block = 256 * reader.DATAGRAM
    audio, trail, power = [], [], []
    with pkg.Engine(n_pixels=a.cols * a.cols, n_streams=n, max_batch=min(a.max_batch, n_blocks), grid_columns=a.cols,
                    device=a.device) as eng:
        eng.set_antenna(xyz)
        eng.set_active_mics(None)
        if a.heatmaps:
            eng.set_delay_table(*pkg.build_delay_table(xyz, a.cols, a.cols, a.fov))
        who = (start[:, 0], start[:, 1], np.radians(a.spread), a.rate)
        for first, count, steps in settle_split(n_blocks, a.settle, a.steps):
            got = eng.listen_blocks(wire[first * block: (first + count) * block], *who, steps, np.radians(a.theta_limit),
                                    want_power=a.heatmaps)
            who = (got.theta, got.phi, got.spread, got.rate)
            audio.append(got.audio)
            trail.append(got.trail)
            power.append(got.power)
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    audio = np.concatenate(audio, axis=1)
    (out / "listen.wav").write_bytes(wav_bytes(audio))
    np.save(out / "trail.npy", np.concatenate(trail))
    print(f"wrote {out / 'listen.wav'}: {audio.shape[0]} channels, {audio.shape[1] / SAMPLE_RATE:.2f} s, and {out / 'trail.npy'}")
    if a.heatmaps:
        np.save(out / "power.npy", np.concatenate(power).reshape(n_blocks, a.cols, a.cols))
        print(f"wrote {out / 'power.npy'}: {n_blocks} x {a.cols} x {a.cols}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
