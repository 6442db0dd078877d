#!/usr/bin/env python3
"""Heatmaps for every block of a recorded capture -- the reference's offline workflow (udp/README.md: FPGA datagrams recorded
to a .pcap and replayed) without the replay: the capture is read here, in pure Python, and handed to the engine in batched
sweeps (Engine.process_blocks, include/awpu_hip_blocks.h).

  tools/pcap_heatmaps.py recording.pcap --port 21844 --arrays 1 --rows 1 --cols 100 --fov 180 --out DIR

Reads classic libpcap files (either byte order, micro- or nanosecond stamps) with Ethernet, IPv4 and UDP; keeps the UDP payloads
of 1032 bytes (one datagram of the wire format, src/fpga/receiver.h:24-30) sent to --port, in capture order; cuts them into
blocks of 256 and drops a trailing partial block.  Counter gaps are reported, not repaired: the reference ignores the counter
(src/fpga/pipeline.cpp:264-267).  pcapng is refused (convert with `editcap -F pcap in.pcapng out.pcap`).
Writes DIR/power.npy [n_blocks][cols*cols] and DIR/u8.npy (heatmap_u8 of every row, MIMOWorker::populateHeatmap)."""
from __future__ import annotations

import argparse
import importlib
import struct
import sys
from pathlib import Path

import numpy as np

DATAGRAM = 1032
PCAP_MAGIC = {0xA1B2C3D4: "us", 0xA1B23C4D: "ns"}
PCAPNG_MAGIC = 0x0A0D0D0A
LINKTYPE_ETHERNET = 1


def read_pcap_payloads(path, port: int) -> list:
    """UDP payloads of DATAGRAM bytes to `port` (Ethernet / IPv4 / UDP, VLAN tags skipped), in capture order."""
    data = Path(path).read_bytes()
    if len(data) < 24:
        raise ValueError(f"{path}: too short for a pcap header")
    if struct.unpack("<I", data[:4])[0] == PCAPNG_MAGIC:
        raise ValueError(f"{path} is pcapng; convert it first: editcap -F pcap {path} out.pcap")
    for e in ("<", ">"):
        if struct.unpack(e + "I", data[:4])[0] in PCAP_MAGIC:
            break
    else:
        raise ValueError(f"{path}: not a libpcap capture (magic {data[:4].hex()})")
    linktype = struct.unpack(e + "I", data[20:24])[0]
    if linktype != LINKTYPE_ETHERNET:
        raise ValueError(f"{path}: link type {linktype}, only Ethernet (1) is read")
    out, off = [], 24
    while off + 16 <= len(data):
        incl = struct.unpack(e + "I", data[off + 8: off + 12])[0]
        frame = data[off + 16: off + 16 + incl]
        off += 16 + incl
        if len(frame) < 14:
            continue
        ethertype, p = struct.unpack("!H", frame[12:14])[0], 14
        while ethertype in (0x8100, 0x88A8) and len(frame) >= p + 4:  # VLAN tags
            ethertype, p = struct.unpack("!H", frame[p + 2: p + 4])[0], p + 4
        if ethertype != 0x0800 or len(frame) < p + 20:
            continue
        ihl = (frame[p] & 0x0F) * 4
        if frame[p] >> 4 != 4 or frame[p + 9] != 17:  # IPv4, UDP
            continue
        frag = struct.unpack("!H", frame[p + 6: p + 8])[0]
        if frag & 0x3FFF:  # fragments of a larger datagram: not the wire format's
            continue
        u = p + ihl
        if len(frame) < u + 8:
            continue
        dport, length = struct.unpack("!HH", frame[u + 2: u + 6])
        payload = frame[u + 8: u + length]
        if dport == port and length - 8 == DATAGRAM and len(payload) == DATAGRAM:
            out.append(payload)
    return out


def blocks_of(payloads: list):
    """-> (wire bytes of the whole blocks, number of blocks, counter gaps [(datagram index, datagrams missing)])."""
    gaps = []
    for i in range(1, len(payloads)):
        prev, cur = (struct.unpack("<I", p[4:8])[0] for p in (payloads[i - 1], payloads[i]))
        if cur != (prev + 1) & 0xFFFFFFFF:
            gaps.append((i, (cur - prev - 1) & 0xFFFFFFFF))
    n_blocks = len(payloads) // 256
    return b"".join(payloads[: 256 * n_blocks]), n_blocks, gaps


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("pcap")
    ap.add_argument("--port", type=int, required=True, help="UDP destination port of the FPGA datagrams")
    ap.add_argument("--arrays", type=int, default=1, help="8x8 arrays side by side (stream id = a*64 + r*8 + c)")
    ap.add_argument("--rows", type=int, default=1, help="rows of arrays")
    ap.add_argument("--cols", type=int, default=100, help="heatmap resolution: cols x cols pixels")
    ap.add_argument("--fov", type=float, default=180.0, help="field of view in degrees")
    ap.add_argument("--max-batch", type=int, default=128, help="frames per sweep launch")
    ap.add_argument("--out", default=".", help="directory for power.npy and u8.npy")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)

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
    with pkg.Engine(n_pixels=a.cols * a.cols, n_streams=n, max_batch=min(a.max_batch, n_blocks), grid_columns=a.cols,
                    device=a.device) as eng:
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        power = eng.process_blocks(wire)
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    np.save(out / "power.npy", power.reshape(n_blocks, a.cols, a.cols))
    np.save(out / "u8.npy", np.stack([pkg.heatmap_u8(p) for p in power]).reshape(n_blocks, a.cols, a.cols))
    print(f"wrote {out / 'power.npy'} and {out / 'u8.npy'}: {n_blocks} x {a.cols} x {a.cols}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
