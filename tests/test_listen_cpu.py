"""Listening to runs of blocks (include/awpu_hip_listen.h) on a box without a GPU: the three entry points are exported beside
the other headers', the header compiles as C, bad arguments are refused before the handle is touched, the listen kernels
compile for gfx950 without scratch, and tools/pcap_listen.py writes float WAV files and splits a run for --settle."""
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
NAMES = ["awpu_hip_listen_blocks", "awpu_hip_listen_samples", "awpu_hip_listen_samples_device"]


def test_listen_symbols_exported(pkg):
    lib = pkg.binding.load()
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "awpu_hip_listen.h").read_text(), flags=re.S)
    assert sorted(set(re.findall(r"\b(awpu_hip_\w+)\s*\(", text))) == sorted(NAMES)
    assert sorted(pkg.binding.LISTEN_SYMBOLS) == sorted(NAMES)
    for name in NAMES:
        assert hasattr(lib, name)
    for other in (pkg.binding.EXPORTED_SYMBOLS, pkg.binding.TRACK_SYMBOLS, pkg.binding.BLOCK_SYMBOLS):
        assert not set(pkg.binding.LISTEN_SYMBOLS) & set(other)
    assert lib.awpu_hip_abi_version() == 4
    assert REPO / "include" / "awpu_hip_listen.h" in pkg._build.HEADERS
    for header in ("awpu_hip.h", "awpu_hip_track.h", "awpu_hip_blocks.h"):
        assert "awpu_hip_listen" not in (REPO / "include" / header).read_text()


def test_listen_header_compiles_as_c(tmp_path):
    src = tmp_path / "one.c"
    src.write_text('#include "awpu_hip_listen.h"\n'
                   "int main(void) { awpu_particle_t p; p.steps = 3; return awpu_hip_listen_blocks(0, 0, 0, 0, &p, 1, 1.0, 0.0, 0, 0, 0, 0) == 0; }\n")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", f"-I{REPO / 'include'}", str(src)], check=True,
                   capture_output=True)


def test_listen_entry_points_refuse_bad_arguments(pkg):
    """Null pointers, counts and pitches out of range, a listener awpu_hip_track would refuse: AWPU_ERR_INVALID, no dereference.
    The handle is a zeroed buffer that is not an engine: touching it would crash or change it."""
    lib = pkg.binding.load()
    B = pkg.binding
    INV = B.ERR_INVALID
    fake = (C.c_ubyte * 4096)()
    h = C.cast(fake, C.c_void_p)
    wire = (C.c_ubyte * (2 * 256 * 1032))()
    samples = (C.c_float * (64 * 512))()
    audio = (C.c_float * (2 * 512))()
    fp = C.POINTER(C.c_float)
    sp, au = C.cast(samples, fp), C.cast(audio, fp)

    def listeners(**field):
        p = (B.Particle * 2)()
        for k in range(2):
            p[k].theta, p[k].phi, p[k].spread, p[k].rate, p[k].steps = 0.3, 1.0, 0.03, 5e-5, 3
        for name, value in field.items():
            setattr(p[1], name, value)
        return p

    ok = listeners()
    forms = [
        lambda hh, src_ok, nb, p, n, lim, ref, a, ap: lib.awpu_hip_listen_blocks(hh, wire if src_ok else None, 1032, nb, p, n, lim, ref, a, ap,
                                                                                 None, None),
        lambda hh, src_ok, nb, p, n, lim, ref, a, ap: lib.awpu_hip_listen_samples(hh, sp if src_ok else None, 512, nb, p, n, lim, ref, a, ap,
                                                                                  None, None),
        lambda hh, src_ok, nb, p, n, lim, ref, a, ap: lib.awpu_hip_listen_samples_device(hh, sp if src_ok else None, 512, nb, p, n, lim,
                                                                                         ref, a, ap, None, None, None),
    ]
    for call in forms:
        assert call(None, True, 2, ok, 2, 1.5, 0.0, au, 512) == INV      # no handle
        assert call(h, False, 2, ok, 2, 1.5, 0.0, au, 512) == INV        # no input
        assert call(h, True, 2, None, 2, 1.5, 0.0, au, 512) == INV       # no listeners
        assert call(h, True, 2, ok, 2, 1.5, 0.0, None, 512) == INV       # no audio
        assert call(h, True, 0, ok, 2, 1.5, 0.0, au, 512) == INV         # n_blocks
        assert call(h, True, -1, ok, 2, 1.5, 0.0, au, 512) == INV
        assert call(h, True, 2, ok, 0, 1.5, 0.0, au, 512) == INV         # n
        assert call(h, True, 2, ok, 65536, 1.5, 0.0, au, 512) == INV
        assert call(h, True, 2, ok, 2, 0.0, 0.0, au, 512) == INV         # theta_limit
        assert call(h, True, 2, ok, 2, float("inf"), 0.0, au, 512) == INV
        assert call(h, True, 2, ok, 2, 1.5, float("nan"), au, 512) == INV  # reference
        assert call(h, True, 2, ok, 2, 1.5, 0.0, au, 511) == INV         # audio_pitch below 256 * n_blocks
        assert call(h, True, 2, listeners(steps=4097), 2, 1.5, 0.0, au, 512) == INV
        assert call(h, True, 2, listeners(steps=-1), 2, 1.5, 0.0, au, 512) == INV
        assert call(h, True, 2, listeners(theta=float("nan")), 2, 1.5, 0.0, au, 512) == INV
        assert call(h, True, 2, listeners(phi=float("inf")), 2, 1.5, 0.0, au, 512) == INV
        assert call(h, True, 2, listeners(spread=float("nan")), 2, 1.5, 0.0, au, 512) == INV
        assert call(h, True, 2, listeners(rate=float("inf")), 2, 1.5, 0.0, au, 512) == INV
    assert lib.awpu_hip_listen_blocks(h, wire, 1031, 2, ok, 2, 1.5, 0.0, au, 512, None, None) == INV  # datagram stride
    assert lib.awpu_hip_listen_samples(h, sp, 511, 2, ok, 2, 1.5, 0.0, au, 512, None, None) == INV    # sample pitch
    assert lib.awpu_hip_listen_samples_device(h, sp, 767, 3, ok, 2, 1.5, 0.0, au, 768, None, None, None) == INV
    assert bytes(fake) == bytes(4096)
    assert bytes(ok) == bytes(listeners())


@pytest.fixture(scope="module")
def track_metadata(tmp_path_factory, pkg):
    out = tmp_path_factory.mktemp("asm") / "track_kernels.s"
    subprocess.run([pkg._build.hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{REPO / 'include'}", f"-I{CSRC}",
                    "-S", "--cuda-device-only", "-o", str(out), str(CSRC / "track_kernels.hip")], check=True, capture_output=True)
    meta = {}
    for block in out.read_text().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1))
                      for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")}
    return meta


# listen_blocks_kernel carries a listener over the blocks of a piece around gradient_track_kernel's step loop, whose fp64 libm
# calls use nearly every scalar register: the pointers and counts of the block loop wait in VGPR lanes meanwhile (v_writelane /
# v_readlane: no memory traffic, no scratch).  The count is what the compiler gives, pinned so that any growth is seen.
LISTEN_SGPR_SPILLS_ACCEPTED = {"listen_blocks_kernel": 35, "listen_fixed_kernel": 0}


def test_listen_kernels_compile_without_scratch(track_metadata):
    """Both shapes -- one workgroup per tracking listener, one per (block, fixed listener): no register spilled to memory, no
    scratch, SGPR spills into VGPR lanes no more than pinned above."""
    names = {n for n in track_metadata if re.search(r"listen_blocks_kernel|listen_fixed_kernel", n)}
    assert len(names) == 2, sorted(track_metadata)
    for name in names:
        m = track_metadata[name]
        assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_count"] <= 256, (name, m)
        short = next(k for k in LISTEN_SGPR_SPILLS_ACCEPTED if k in name)
        assert m["sgpr_spill_count"] <= LISTEN_SGPR_SPILLS_ACCEPTED[short], (name, m)


# ------------------------------------------------------------------------------------------------ tools/pcap_listen.py

def load_tool():
    spec = importlib.util.spec_from_file_location("pcap_listen", REPO / "tools" / "pcap_listen.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def parse_wav(blob):
    """-> ({chunk id: payload}, in file order) of a RIFF/WAVE file, checking the sizes that frame it."""
    riff, size, wave = struct.unpack("<4sI4s", blob[:12])
    assert riff == b"RIFF" and wave == b"WAVE" and size == len(blob) - 8
    chunks, off = {}, 12
    while off < len(blob):
        cid, n = struct.unpack("<4sI", blob[off: off + 8])
        chunks[cid] = blob[off + 8: off + 8 + n]
        assert len(chunks[cid]) == n
        off += 8 + n + (n & 1)
    assert off == len(blob)
    return chunks


@pytest.mark.parametrize("channels", [1, 3])
def test_wav_writer_round_trips(channels):
    tool = load_tool()
    rng = np.random.default_rng(channels)
    audio = rng.standard_normal((channels, 777)).astype(np.float32)
    audio[0, :3] = [np.float32(np.nan), np.float32(-0.0), np.float32(1e-41)]  # bytes, not values: NaN and a subnormal survive
    chunks = parse_wav(tool.wav_bytes(audio))
    assert list(chunks) == [b"fmt ", b"fact", b"data"]
    tag, n_ch, rate, byte_rate, align, bits = struct.unpack("<HHIIHH", chunks[b"fmt "][:16])
    assert (tag, n_ch, rate, align, bits) == (3, channels, 48828, 4 * channels, 32)  # WAVE_FORMAT_IEEE_FLOAT
    assert byte_rate == 48828 * 4 * channels
    assert struct.unpack("<I", chunks[b"fact"])[0] == 777
    assert len(chunks[b"data"]) == 4 * channels * 777
    back = np.frombuffer(chunks[b"data"], "<f4").reshape(777, channels).T
    assert back.tobytes() == audio.tobytes()
    assert tool.SAMPLE_RATE == 48828
    if channels == 1:
        assert tool.wav_bytes(audio[0]) == tool.wav_bytes(audio)  # a 1-D row is one channel


def test_settle_split():
    tool = load_tool()
    assert tool.settle_split(40, 4, 3) == [(0, 4, 0), (4, 36, 3)]
    assert tool.settle_split(3, 4, 3) == [(0, 3, 0)]
    assert tool.settle_split(4, 4, 3) == [(0, 4, 0)]
    assert tool.settle_split(40, 0, 3) == [(0, 40, 3)]
    assert tool.settle_split(40, 4, 0) == [(0, 40, 0)]  # fixed listeners: nothing to settle
    for n, settle, steps in ((40, 4, 3), (3, 4, 3), (40, 0, 5), (7, 7, 1)):
        parts = tool.settle_split(n, settle, steps)
        assert sum(p[1] for p in parts) == n and parts[0][0] == 0
        assert all(a[0] + a[1] == b[0] for a, b in zip(parts, parts[1:]))
