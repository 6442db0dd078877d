"""Runs of consecutive blocks (include/awpu_hip_blocks.h) on a box without a GPU: the three entry points are exported beside
awpu_hip.h's and awpu_hip_track.h's, refuse bad arguments before touching the handle, their kernels compile for gfx950
without spills, and tools/pcap_heatmaps.py reads classic libpcap captures."""
import ctypes as C
import importlib.util
import re
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "beamforming-lk_amd" / "csrc"
NAMES = ["awpu_hip_process_blocks", "awpu_hip_process_samples", "awpu_hip_process_samples_device"]


def test_block_symbols_exported(pkg):
    lib = pkg.binding.load()
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "awpu_hip_blocks.h").read_text(), flags=re.S)
    assert sorted(set(re.findall(r"\b(awpu_hip_\w+)\s*\(", text))) == sorted(NAMES)
    assert sorted(pkg.binding.BLOCK_SYMBOLS) == sorted(NAMES)
    for name in NAMES:
        assert hasattr(lib, name)
    assert not set(pkg.binding.BLOCK_SYMBOLS) & set(pkg.binding.EXPORTED_SYMBOLS)
    assert not set(pkg.binding.BLOCK_SYMBOLS) & set(pkg.binding.TRACK_SYMBOLS)
    assert lib.awpu_hip_abi_version() == 4
    assert "awpu_hip_blocks.h" not in (REPO / "include" / "awpu_hip.h").read_text()


def test_block_entry_points_refuse_bad_arguments(pkg):
    """Null handle, null buffers, n_blocks < 1, a stride below one datagram, a pitch below 256 * n_blocks: a negative status,
    no dereference.  The handle is a zeroed buffer that is not an engine: touching it would crash or change it."""
    lib = pkg.binding.load()
    INV = pkg.binding.ERR_INVALID
    fake = (C.c_ubyte * 4096)()
    h = C.cast(fake, C.c_void_p)
    wire = (C.c_ubyte * (2 * 256 * 1032))()
    power = (C.c_float * 16)()
    samples = (C.c_float * (64 * 512))()
    fp = C.POINTER(C.c_float)
    pw = C.cast(power, fp)
    sp = C.cast(samples, fp)
    assert lib.awpu_hip_process_blocks(None, wire, 1032, 2, pw) == INV
    assert lib.awpu_hip_process_blocks(h, None, 1032, 2, pw) == INV
    assert lib.awpu_hip_process_blocks(h, wire, 1032, 2, None) == INV
    assert lib.awpu_hip_process_blocks(h, wire, 1032, 0, pw) == INV
    assert lib.awpu_hip_process_blocks(h, wire, 1032, -3, pw) == INV
    assert lib.awpu_hip_process_blocks(h, wire, 1031, 2, pw) == INV
    assert lib.awpu_hip_process_samples(None, sp, 512, 2, pw) == INV
    assert lib.awpu_hip_process_samples(h, None, 512, 2, pw) == INV
    assert lib.awpu_hip_process_samples(h, sp, 512, 2, None) == INV
    assert lib.awpu_hip_process_samples(h, sp, 512, 0, pw) == INV
    assert lib.awpu_hip_process_samples(h, sp, 511, 2, pw) == INV
    assert lib.awpu_hip_process_samples_device(None, sp, 512, 2, pw, None) == INV
    assert lib.awpu_hip_process_samples_device(h, None, 512, 2, pw, None) == INV
    assert lib.awpu_hip_process_samples_device(h, sp, 512, 2, None, None) == INV
    assert lib.awpu_hip_process_samples_device(h, sp, 512, 0, pw, None) == INV
    assert lib.awpu_hip_process_samples_device(h, sp, 767, 3, pw, None) == INV
    assert bytes(fake) == bytes(4096)


def test_block_kernels_compile_without_spills(pkg, tmp_path):
    out = tmp_path / "block_kernels.s"
    subprocess.run([pkg._build.hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{REPO / 'include'}", f"-I{CSRC}",
                    "-S", "--cuda-device-only", "-o", str(out), str(CSRC / "block_kernels.hip")], check=True, capture_output=True)
    meta = {}
    for block in out.read_text().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1))
                      for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")}
    names = {n for n in meta if re.search(r"unpack_blocks_kernel|copy_rows_kernel|cut_windows_kernel|ring_write_kernel", n)}
    assert len(names) == 4, sorted(meta)
    for name in names:
        m = meta[name]
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
    assert pkg._build.CSRC / "block_kernels.hip" in pkg._build.SOURCES
    assert REPO / "include" / "awpu_hip_blocks.h" in pkg._build.HEADERS


# ------------------------------------------------------------------------------------------------ tools/pcap_heatmaps.py

def load_tool():
    spec = importlib.util.spec_from_file_location("pcap_heatmaps", REPO / "tools" / "pcap_heatmaps.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def udp_frame(payload, dport, sport=5000):
    udp = struct.pack("!HHHH", sport, dport, 8 + len(payload), 0) + payload
    ip = struct.pack("!BBHHHBBH4s4s", 0x45, 0, 20 + len(udp), 0, 0, 64, 17, 0, bytes([10, 0, 0, 1]), bytes([10, 0, 0, 2]))
    return b"\xff" * 6 + b"\x02" * 6 + struct.pack("!H", 0x0800) + ip + udp


def write_pcap(path, frames, big_endian=False):
    e = ">" if big_endian else "<"
    with open(path, "wb") as f:
        f.write(struct.pack(e + "IHHiIII", 0xA1B2C3D4, 2, 4, 0, 0, 65535, 1))
        for i, fr in enumerate(frames):
            f.write(struct.pack(e + "IIII", 1000 + i, 0, len(fr), len(fr)) + fr)


def datagram(counter, fill):
    return struct.pack("<HBBI", 48828, 1, 2, counter) + struct.pack("<256i", *([fill] * 256))


@pytest.mark.parametrize("big_endian", [False, True])
def test_pcap_reader_recovers_payloads(tmp_path, big_endian):
    tool = load_tool()
    frames, want = [], []
    counter = 0
    for k in range(2 * 256 + 17):  # two whole blocks and an odd tail
        if k == 300:
            counter += 5  # a counter gap: reported, not repaired
        d = datagram(counter, k)
        counter += 1
        want.append(d)
        frames.append(udp_frame(d, 21844))
        if k % 50 == 0:
            frames.append(udp_frame(b"x" * 1032, 9999))  # another port
            frames.append(udp_frame(b"short", 21844))    # not a datagram of the wire format
    path = tmp_path / "rec.pcap"
    write_pcap(path, frames, big_endian)
    payloads = tool.read_pcap_payloads(path, 21844)
    assert payloads == want
    wire, n_blocks, gaps = tool.blocks_of(payloads)
    assert n_blocks == 2 and len(wire) == 2 * 256 * 1032 and wire == b"".join(want[:512])
    assert gaps == [(300, 5)]


def test_pcapng_is_refused(tmp_path):
    tool = load_tool()
    path = tmp_path / "rec.pcapng"
    path.write_bytes(struct.pack("<III", 0x0A0D0D0A, 28, 0x1A2B3C4D) + bytes(16))
    with pytest.raises(ValueError, match="editcap -F pcap"):
        tool.read_pcap_payloads(path, 21844)
