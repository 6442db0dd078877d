"""Watching runs of blocks (include/awpu_hip_watch.h) on a box without a GPU: the five entry points are exported beside the
other headers', the header compiles as C, awpu_hip_watch_count equals a brute-force enumeration and chains over a split
recording, bad arguments are refused before the handle is touched, the kernels compile for gfx950 without spills and the
large-image kernel stores 16 bytes at a time, and tools/pcap_video.py writes AVI files that parse back."""
import ctypes as C
import importlib.util
import math
import re
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "beamforming-lk_amd" / "csrc"
NAMES = ["awpu_hip_watch_count", "awpu_hip_watch_blocks", "awpu_hip_watch_samples", "awpu_hip_watch_samples_device"]
TYPES = ["awpu_watch_t"]  # the fifth name the header declares


def test_watch_symbols_exported(pkg):
    lib = pkg.binding.load()
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "awpu_hip_watch.h").read_text(), flags=re.S)
    assert sorted(set(re.findall(r"\b(awpu_hip_\w+)\s*\(", text))) == sorted(NAMES)
    assert re.findall(r"\}\s*(\w+)\s*;", text) == TYPES
    assert sorted(pkg.binding.WATCH_SYMBOLS) == sorted(NAMES)
    for name in NAMES:
        assert hasattr(lib, name)
    for other in (pkg.binding.EXPORTED_SYMBOLS, pkg.binding.TRACK_SYMBOLS, pkg.binding.BLOCK_SYMBOLS, pkg.binding.LISTEN_SYMBOLS):
        assert not set(pkg.binding.WATCH_SYMBOLS) & set(other)
    assert lib.awpu_hip_abi_version() == 4
    assert REPO / "include" / "awpu_hip_watch.h" in pkg._build.HEADERS
    assert CSRC / "watch_kernels.hip" in pkg._build.SOURCES
    for header in ("awpu_hip.h", "awpu_hip_track.h", "awpu_hip_blocks.h", "awpu_hip_listen.h"):
        assert "awpu_hip_watch" not in (REPO / "include" / header).read_text()
    assert C.sizeof(pkg.binding.Watch) == 40


def test_watch_header_compiles_as_c(tmp_path):
    src = tmp_path / "one.c"
    src.write_text('#include "awpu_hip_watch.h"\n'
                   "int main(void) { awpu_watch_t w; int32_t n, next; w.every = 3; w.d_colormap = 0;\n"
                   "  return awpu_hip_watch_count(10, 0, w.every, &n, &next) + awpu_hip_watch_blocks(0, 0, 0, 0, &w, 0, 0, 0)\n"
                   "       + awpu_hip_watch_samples(0, 0, 0, 0, &w, 0, 0, 0) + awpu_hip_watch_samples_device(0, 0, 0, 0, &w, 0, 0, 0, 0); }\n")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", f"-I{REPO / 'include'}", str(src)], check=True,
                   capture_output=True)


def test_watch_count_against_enumeration(pkg):
    count = pkg.binding.watch_count
    for n_blocks in range(1, 41):
        for first in range(0, 46):
            for every in range(1, 10):
                shown = list(range(first, n_blocks, every))
                nxt = (shown[-1] + every if shown else first) - n_blocks
                assert count(n_blocks, first, every) == (len(shown), nxt), (n_blocks, first, every)
    rng = np.random.default_rng(11)
    for every in (1, 2, 3, 4, 7, 64, 499, 1024):
        for first0 in (0, 1, 5, 600):
            whole = list(range(first0, 500, every))
            cuts = np.sort(rng.choice(np.arange(1, 500), size=int(rng.integers(1, 40)), replace=False))
            got, first, begin = [], first0, 0
            for end in list(cuts) + [500]:
                n, nxt = count(int(end - begin), first, every)
                got += [begin + first + j * every for j in range(n)]
                assert nxt >= 0
                first, begin = nxt, int(end)
            assert got == whole, (every, first0)
    lib = pkg.binding.load()
    n, nxt = C.c_int32(7), C.c_int32(7)
    INV = pkg.binding.ERR_INVALID
    assert lib.awpu_hip_watch_count(10, 0, 0, C.byref(n), C.byref(nxt)) == INV   # every
    assert lib.awpu_hip_watch_count(10, 0, -2, C.byref(n), C.byref(nxt)) == INV
    assert lib.awpu_hip_watch_count(10, -1, 3, C.byref(n), C.byref(nxt)) == INV  # first
    assert lib.awpu_hip_watch_count(0, 0, 3, C.byref(n), C.byref(nxt)) == INV    # n_blocks
    assert lib.awpu_hip_watch_count(10, 0, 3, None, C.byref(nxt)) == INV
    assert lib.awpu_hip_watch_count(10, 0, 3, C.byref(n), None) == INV
    assert (n.value, nxt.value) == (7, 7)
    assert lib.awpu_hip_watch_count(2147483647, 0, 1, C.byref(n), C.byref(nxt)) == 0 and (n.value, nxt.value) == (2147483647, 0)


def test_watch_entry_points_refuse_bad_arguments(pkg):
    """AWPU_ERR_INVALID and no dereference: the handle is a zeroed buffer that is not an engine (touching it would crash or
    change it), and the outputs keep their bytes."""
    lib = pkg.binding.load()
    B = pkg.binding
    INV = B.ERR_INVALID
    fake = (C.c_ubyte * 4096)()
    h = C.cast(fake, C.c_void_p)
    wire = (C.c_ubyte * (2 * 256 * 1032))()
    samples = (C.c_float * (64 * 768))()
    sp = C.cast(samples, C.POINTER(C.c_float))
    image = (C.c_uint8 * (2 * 64))()
    big = (C.c_uint8 * (2 * 16 * 16 * 3))()
    power = (C.c_float * (2 * 64))()
    im, bg, pw = C.cast(image, C.POINTER(C.c_uint8)), C.cast(big, C.POINTER(C.c_uint8)), C.cast(power, C.POINTER(C.c_float))

    def watch(**field):
        w = B.Watch(0, 1, 8, 8, 16, 16, 0, None)
        for name, value in field.items():
            setattr(w, name, value)
        return w

    forms = [
        lambda hh, src_ok, nb, w, i, b, p: lib.awpu_hip_watch_blocks(hh, wire if src_ok else None, 1032, nb, w, i, b, p),
        lambda hh, src_ok, nb, w, i, b, p: lib.awpu_hip_watch_samples(hh, sp if src_ok else None, 512, nb, w, i, b, p),
        lambda hh, src_ok, nb, w, i, b, p: lib.awpu_hip_watch_samples_device(hh, sp if src_ok else None, 512, nb, w, i, b, p, None),
    ]
    ok = watch()
    for call in forms:
        assert call(None, True, 2, C.byref(ok), im, bg, pw) == INV       # no handle
        assert call(h, False, 2, C.byref(ok), im, bg, pw) == INV         # no input
        assert call(h, True, 2, None, im, bg, pw) == INV                 # no w
        assert call(h, True, 2, C.byref(ok), None, None, None) == INV    # no output
        assert call(h, True, 0, C.byref(ok), im, bg, pw) == INV          # n_blocks
        assert call(h, True, -1, C.byref(ok), im, bg, pw) == INV
        for bad in (dict(every=0), dict(every=-1), dict(every=1025), dict(first=-1), dict(flip=2), dict(flip=-1)):
            for outs in ((im, bg, pw), (im, None, None), (None, None, pw)):
                assert call(h, True, 2, C.byref(watch(**bad)), *outs) == INV, bad
        for bad in (dict(out_rows=7), dict(out_cols=7), dict(out_rows=0, out_cols=0)):  # a large image smaller than the compact one
            assert call(h, True, 2, C.byref(watch(**bad)), im, bg, pw) == INV, bad
            assert call(h, True, 2, C.byref(watch(**bad)), None, bg, None) == INV, bad
    assert lib.awpu_hip_watch_blocks(h, wire, 1031, 2, C.byref(ok), im, bg, pw) == INV            # datagram stride
    assert lib.awpu_hip_watch_samples(h, sp, 511, 2, C.byref(ok), im, bg, pw) == INV              # sample pitch
    assert lib.awpu_hip_watch_samples_device(h, sp, 767, 3, C.byref(ok), im, bg, pw, None) == INV
    assert bytes(fake) == bytes(4096)
    assert bytes(image) == bytes(len(image)) and bytes(big) == bytes(len(big)) and bytes(power) == bytes(4 * len(power))


@pytest.fixture(scope="module")
def watch_asm(tmp_path_factory, pkg):
    out = tmp_path_factory.mktemp("asm") / "watch_kernels.s"
    subprocess.run([pkg._build.hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{REPO / 'include'}", f"-I{CSRC}",
                    "-S", "--cuda-device-only", "-o", str(out), str(CSRC / "watch_kernels.hip")], check=True, capture_output=True)
    return out.read_text()


def test_watch_kernels_compile_without_spills(watch_asm):
    meta = {}
    for block in watch_asm.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1))
                      for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")}
    names = {n for n in meta if re.search(r"watch_gather_kernel|watch_cut_kernel|watch_upscale_kernel", n)}
    assert len(names) == 3 and len(meta) == 3, sorted(meta)
    for name in names:
        m = meta[name]
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
    # the kernels the existing suites count by name live elsewhere and keep their names to themselves
    for taken in ("unpack_blocks_kernel", "copy_rows_kernel", "cut_windows_kernel", "ring_write_kernel", "listen_blocks_kernel",
                  "listen_fixed_kernel", "gradient_track_kernel", "steer_table_kernel"):
        assert not any(taken in n for n in meta)


def test_large_image_kernel_stores_wide(watch_asm):
    """Between the kernel's label and its s_endpgm: 16-byte stores in the steady state, narrower ones only in the path of an
    image narrower than one lane's 16 pixels."""
    label = re.search(r"^(_Z\w*watch_upscale_kernel\w*):", watch_asm, flags=re.M).group(1)
    body = watch_asm.split(f"\n{label}:", 1)[1].split(".Lfunc_end", 1)[0]
    assert "s_endpgm" in body
    wide = len(re.findall(r"\bglobal_store_dwordx4\b", body))
    narrow = len(re.findall(r"\bglobal_store_(byte|short)\b", body))
    other = set(re.findall(r"\b((?:global|flat|buffer|scratch)_store_\w+)", body)) - {"global_store_dwordx4", "global_store_byte", "global_store_short"}
    print("watch_upscale_kernel stores: dwordx4", wide, "byte/short", narrow, "other", sorted(other))
    assert wide >= 1 and narrow < wide
    assert not other  # (nothing in between either: no dword-by-dword steady state)


# ------------------------------------------------------------------------------------------------ tools/pcap_video.py

def load_tool():
    spec = importlib.util.spec_from_file_location("pcap_video", REPO / "tools" / "pcap_video.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def parse_avi(blob):
    """-> (width, height, dwRate, dwScale, frames [n][height][width][3] top-down) of an uncompressed BGR24 AVI, walking the RIFF
    structure with struct alone (independently of the tool's own reader)."""
    riff, size, avi = struct.unpack("<4sI4s", blob[:12])
    assert riff == b"RIFF" and avi == b"AVI " and size == len(blob) - 8
    found, frames, index = {}, [], None

    def walk(lo, hi):
        nonlocal index
        off = lo
        while off < hi:
            cid, n = struct.unpack("<4sI", blob[off: off + 8])
            if cid == b"LIST":
                kind = blob[off + 8: off + 12]
                found[kind + b"@"] = off + 8
                walk(off + 12, off + 8 + n)
            elif cid == b"00db":
                frames.append(blob[off + 8: off + 8 + n])
            elif cid == b"idx1":
                index = blob[off + 8: off + 8 + n]
            else:
                found[cid] = blob[off + 8: off + 8 + n]
            off += 8 + n + (n & 1)
        assert off == hi

    walk(12, len(blob))
    avih = struct.unpack("<14I", found[b"avih"])
    total, streams, width, height = avih[4], avih[6], avih[8], avih[9]
    strh = struct.unpack("<4s4sIHHIIIIIIII4h", found[b"strh"])
    assert strh[0] == b"vids" and strh[1] == b"DIB " and streams == 1
    scale, rate, length = strh[6], strh[7], strh[9]
    size_, w, hgt, planes, bits, compression, image_bytes = struct.unpack("<IiiHHII", found[b"strf"][:24])
    row = (3 * width + 3) & ~3
    assert (size_, w, hgt, planes, bits, compression, image_bytes) == (40, width, height, 1, 24, 0, row * height)
    assert total == length == len(frames) and len(index) == 16 * len(frames)
    movi = found[b"movi@"]
    for k, f in enumerate(frames):
        cid, flags, off, n = struct.unpack("<4sIII", index[16 * k: 16 * k + 16])
        assert cid == b"00db" and flags & 0x10 and n == len(f) == row * height
        assert blob[movi + off: movi + off + 8] == b"00db" + struct.pack("<I", n)  # offsets count from the 'movi' fourcc
    micro = avih[0]
    assert abs(micro - 1e6 * scale / rate) <= 1
    out = [np.frombuffer(f, np.uint8).reshape(height, row)[:, : 3 * width].reshape(height, width, 3)[::-1] for f in frames]
    return width, height, rate, scale, np.stack(out)


@pytest.mark.parametrize("every,width", [(3, 10), (1, 7), (4, 8), (1024, 5)])
def test_avi_writer_round_trips(tmp_path, every, width):
    tool = load_tool()
    rng = np.random.default_rng(every)
    frames = rng.integers(0, 256, size=(3, 6, width, 3), dtype=np.uint8)  # (widths whose rows need padding to 4 bytes too)
    with tool.AviWriter(tmp_path / "v", width, 6, every) as wr:
        for f in frames:
            wr.write(f)
    assert wr.paths == [str(tmp_path / "v") + ".000.avi"]
    w, h, rate, scale, back = parse_avi(Path(wr.paths[0]).read_bytes())
    assert (w, h) == (width, 6) and back.shape == frames.shape and np.array_equal(back, frames)
    g = math.gcd(48828, 256 * every)
    assert (rate, scale) == (48828 // g, 256 * every // g) and math.gcd(rate, scale) == 1
    assert rate * 256 * every == 48828 * scale
    own, rate2, scale2 = tool.read_avi(wr.paths[0])
    assert np.array_equal(own, frames) and (rate2, scale2) == (rate, scale)
    assert tool.frame_rate(3) == (4069, 64)  # 63.578 frames per second


def test_avi_parts_roll_over(tmp_path):
    tool = load_tool()
    rng = np.random.default_rng(2)
    frames = rng.integers(0, 256, size=(7, 4, 8, 3), dtype=np.uint8)
    one = tool.AviWriter.HEADER + 8  # a part with no frame (idx1 is empty); every frame adds its chunk and its index entry
    per_frame = 8 + 4 * 8 * 3 + 16
    limit = one + 3 * per_frame + 5  # three frames fit, a fourth does not
    with tool.AviWriter(tmp_path / "p", 8, 4, 3, limit=limit) as wr:
        for f in frames:
            wr.write(f)
    assert [Path(p).name for p in wr.paths] == ["p.000.avi", "p.001.avi", "p.002.avi"]
    got = []
    for p in wr.paths:
        blob = Path(p).read_bytes()
        assert len(blob) <= limit
        got.append(parse_avi(blob)[4])
    assert [len(g) for g in got] == [3, 3, 1]
    assert np.array_equal(np.concatenate(got), frames)
    with pytest.raises(ValueError):
        tool.AviWriter(tmp_path / "q", 8, 4, 3, limit=one + per_frame - 1)
    assert tool.PART_LIMIT < (1 << 30)


def test_colour_tables():
    tool = load_tool()
    jet = tool.jet_table()
    assert jet.shape == (256, 3) and jet.dtype == np.uint8
    x = np.arange(256) / 255.0
    for ch, centre in enumerate((1.0, 2.0, 3.0)):  # B, G, R
        assert np.array_equal(jet[:, ch], np.rint(np.clip(1.5 - np.abs(4 * x - centre), 0, 1) * 255).astype(np.uint8))
    assert tuple(jet[0]) == (128, 0, 0) and tuple(jet[255]) == (0, 0, 128)  # dark blue to dark red
    gray = tool.gray_table()
    assert np.array_equal(gray, np.arange(256, dtype=np.uint8)[:, None].repeat(3, 1))
