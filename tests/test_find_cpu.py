"""Finding sources (include/awpu_hip_find.h) on a box without a GPU: the seven entry points are exported beside the other
headers', the header compiles as C, awpu_hip_find_peaks equals a numpy restatement of the header's rule (integers and powers
equal, doubles within 1e-12), its directions steer to the delay table's own rows, bad arguments are refused before any work, the
kernel compiles for gfx950 without spills or scratch, and tools/pcap_sources.py writes rows that parse back."""
import ctypes as C
import csv
import importlib.util
import itertools
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "beamforming-lk_amd" / "csrc"
NAMES = ["awpu_hip_find_peaks", "awpu_hip_find_peaks_device", "awpu_hip_find_blocks", "awpu_hip_find_samples", "awpu_hip_find_samples_device"]
TYPES = ["awpu_find_t", "awpu_source_t"]

GRIDS = [(1, 1), (1, 7), (5, 3), (8, 8), (33, 17), (100, 100)]
RADII = [1, 2, 8]
MAX_SOURCES = [1, 4, 32]
RATIOS = [0.0, 0.25, 1.0]
TOL = 1e-12  # doubles: libm against numpy, four orders above their rounding, eight below any grid's pitch


def test_find_symbols_exported(pkg):
    lib = pkg.binding.load()
    B = pkg.binding
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "awpu_hip_find.h").read_text(), flags=re.S)
    assert sorted(set(re.findall(r"\b(awpu_hip_\w+)\s*\(", text))) == sorted(NAMES)
    assert re.findall(r"\}\s*(\w+)\s*;", text) == TYPES
    assert '#include "awpu_hip_watch.h"' in text
    assert sorted(B.FIND_SYMBOLS) == sorted(NAMES)
    for name in NAMES:
        assert hasattr(lib, name)
    for other in (B.EXPORTED_SYMBOLS, B.TRACK_SYMBOLS, B.BLOCK_SYMBOLS, B.LISTEN_SYMBOLS, B.WATCH_SYMBOLS):
        assert not set(B.FIND_SYMBOLS) & set(other)
    assert lib.awpu_hip_abi_version() == 4
    assert REPO / "include" / "awpu_hip_find.h" in pkg._build.HEADERS and CSRC / "find_kernels.h" in pkg._build.HEADERS
    assert CSRC / "find_kernels.hip" in pkg._build.SOURCES
    for header in ("awpu_hip.h", "awpu_hip_track.h", "awpu_hip_blocks.h", "awpu_hip_listen.h", "awpu_hip_watch.h"):
        assert "awpu_hip_find" not in (REPO / "include" / header).read_text()
    assert C.sizeof(B.Source) == 40 == B.SOURCE_DTYPE.itemsize and C.sizeof(B.Find) == 28
    for name, _ in B.Source._fields_:
        assert getattr(B.Source, name).offset == B.SOURCE_DTYPE.fields[name][1]
    for macro, value in (("AWPU_FIND_MAX_RADIUS", 8), ("AWPU_FIND_MAX_SOURCES", 32), ("AWPU_FIND_MAX_PIXELS", B.FIND_MAX_PIXELS)):
        assert int(re.search(rf"#define {macro} (\d+)", text).group(1)) == value
    assert B.FIND_MAX_PIXELS >= 256 * 256


def test_find_header_compiles_as_c(tmp_path):
    src = tmp_path / "one.c"
    src.write_text('#include "awpu_hip_find.h"\n'
                   "int main(void) { awpu_watch_t w; awpu_find_t f; awpu_source_t s[AWPU_FIND_MAX_SOURCES]; int32_t n; w.every = 1; f.radius = AWPU_FIND_MAX_RADIUS;\n"
                   "  f.rows = AWPU_FIND_MAX_PIXELS; s[0].theta = 0.0; (void) sizeof(char[sizeof(awpu_source_t) == 40 ? 1 : -1]);\n"
                   "  return awpu_hip_find_peaks(0, 1, &f, s, &n) + awpu_hip_find_peaks_device(0, 0, 1, &f, s, &n, 0)\n"
                   "       + awpu_hip_find_blocks(0, 0, 0, 0, &w, &f, s, &n, 0) + awpu_hip_find_samples(0, 0, 0, 0, &w, &f, s, &n, 0)\n"
                   "       + awpu_hip_find_samples_device(0, 0, 0, 0, &w, &f, s, &n, 0, 0); }\n")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", f"-I{REPO / 'include'}", str(src)], check=True,
                   capture_output=True)


# ------------------------------------------------------------------------------------------------ the rule, restated in numpy

def all_peaks(frame, rows, cols, radius, min_power, min_ratio):
    """Keys of every peak of one frame, strongest first (the header's Order, Maximum and Peak)."""
    p = np.asarray(frame, np.float32).reshape(rows, cols)
    bits = p.view(np.uint32).astype(np.uint64)
    index = np.arange(rows * cols, dtype=np.uint64).reshape(rows, cols)
    key = (bits << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - index)  # a beats b <=> key[a] > key[b]
    m = p.reshape(-1)[int(np.argmax(key))]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):  # (m may be +inf or a NaN: the rule holds on every bit pattern)
        floor_ratio = np.float32(0.0) if np.float32(min_ratio) == 0 else np.float32(min_ratio) * m  # no threshold, or one fp32 multiply
    assert floor_ratio.dtype == np.float32
    padded = np.zeros((rows + 2 * radius, cols + 2 * radius), np.uint64)  # (0 is below every key of the grid)
    padded[radius: radius + rows, radius: radius + cols] = key
    best = np.zeros_like(key)
    for dr in range(2 * radius + 1):
        for dc in range(2 * radius + 1):
            best = np.maximum(best, padded[dr: dr + rows, dc: dc + cols])
    with np.errstate(invalid="ignore"):
        peak = (key == best) & (p > 0) & (p >= np.float32(min_power)) & (p >= floor_ratio)
    return np.sort(key[peak])[::-1]


def offset(a, b, c):
    a, b, c = np.float64(a), np.float64(b), np.float64(c)
    with np.errstate(invalid="ignore", over="ignore"):  # (a +inf peak: den is -inf or a NaN, and the offset 0)
        den = a - 2.0 * b + c
        d = 0.5 * (a - c) / den if den < 0 else np.float64(0.0)
    return min(max(d, -0.5), 0.5)


def describe(frame, rows, cols, pixel, fov_deg):
    """(pixel, power, row, col, theta, phi) of a peak (the header's Refinement and Direction)."""
    p = np.asarray(frame, np.float32).reshape(rows, cols)
    r, c = divmod(int(pixel), cols)
    d_row = offset(p[r - 1, c], p[r, c], p[r + 1, c]) if 0 < r < rows - 1 else 0.0
    d_col = offset(p[r, c - 1], p[r, c], p[r, c + 1]) if 0 < c < cols - 1 else 0.0
    row, col = np.float64(r) + d_row, np.float64(c) + d_col
    fov = np.float64(np.float32(fov_deg)) * (np.pi / 180.0)
    sep_rows, sep_cols = np.sin(fov / 2.0) / (rows / 2.0), np.sin(fov / 2.0) / (cols / 2.0)
    y = row * sep_rows - rows * sep_rows / 2.0 + sep_rows / 2.0
    x = col * sep_cols - cols * sep_cols / 2.0 + sep_cols / 2.0
    theta = np.arcsin(min(np.sqrt(x * x + y * y), 1.0))
    phi = 0.0 if x == 0.0 and y == 0.0 else np.arctan2(y, x)
    return int(pixel), p[r, c], row, col, theta, phi


def restated(frame, rows, cols, radius, max_sources, min_power, min_ratio, fov_deg, keys=None):
    """-> (records [max_sources], count) of one frame."""
    from importlib import import_module

    dtype = import_module("beamforming-lk_amd").binding.SOURCE_DTYPE
    keys = all_peaks(frame, rows, cols, radius, min_power, min_ratio) if keys is None else keys
    out = np.zeros(max_sources, dtype)
    out["pixel"] = -1
    found = min(max_sources, len(keys))
    for k in range(found):
        out[k] = describe(frame, rows, cols, 0xFFFFFFFF - (int(keys[k]) & 0xFFFFFFFF), fov_deg)
    return out, found


def assert_same(got, count, want, want_count, where):
    """Integers and powers equal, doubles within TOL."""
    assert int(count) == int(want_count), where
    assert np.array_equal(got["pixel"], want["pixel"]), where
    assert np.array_equal(got["power"].view(np.uint32), want["power"].view(np.uint32)), where
    for name in ("row", "col", "theta", "phi"):
        err = np.abs(got[name] - want[name]).max()
        assert err <= TOL, (where, name, err)


def contents(rows, cols, seed):
    """name -> frame [rows * cols] float32: the contents the tests share."""
    rng = np.random.default_rng(seed)
    n = rows * cols
    r, c = np.divmod(np.arange(n), cols)
    frames = {
        "random": rng.uniform(1e-6, 1.0, n),
        "ties": rng.integers(0, 4, n),                        # many ties and zeros
        "constant": np.full(n, 0.375),                        # only pixel 0
        "zero": np.zeros(n),                                  # nothing
        "ramp": 1.0 + np.arange(n),
        "ramp_down": 2.0 * n - np.arange(n) // 2,             # pairs of equal neighbours
        "smooth": 1.0 + np.cos(0.9 * r + 0.3) * np.sin(0.7 * c + 0.1) + 1e-3 * rng.uniform(size=n),  # a few peaks, real offsets
    }
    corners = np.zeros(n)
    corners[[0, cols - 1, n - cols, n - 1]] = [4.0, 3.0, 3.0, 5.0]  # a spike in each corner (the two equal ones: the lower index first)
    frames["corners"] = corners
    return {name: np.ascontiguousarray(f, np.float32) for name, f in frames.items()}


def thresholds(frame, rows, cols, radius):
    """(min_ratio, min_power): the three ratios, and a floor just above and just below the second peak where there is one."""
    out = [(ratio, 0.0) for ratio in RATIOS]
    keys = all_peaks(frame, rows, cols, radius, 0.0, 0.0)
    if len(keys) >= 2:
        second = np.array([int(keys[1]) >> 32], np.uint32).view(np.float32)[0]
        out += [(0.0, float(np.nextafter(second, np.float32(np.inf)))), (0.25, float(np.nextafter(second, np.float32(0.0))))]
    return out


def find_cases():
    """Every (rows, cols, name, frame, radius, min_ratio, min_power) the CPU and the GPU tests run, each for every MAX_SOURCES."""
    for (rows, cols), radius in itertools.product(GRIDS, RADII):
        for name, frame in contents(rows, cols, seed=rows * 131 + cols).items():
            for min_ratio, min_power in thresholds(frame, rows, cols, radius):
                yield rows, cols, name, frame, radius, min_ratio, min_power


@pytest.mark.parametrize("fov_deg", [180.0, 90.0])
def test_find_peaks_equals_the_rule(pkg, fov_deg):
    seen = {"cases": 0, "more": 0, "fewer": 0, "refined": 0}
    for rows, cols, name, frame, radius, min_ratio, min_power in find_cases():
        keys = all_peaks(frame, rows, cols, radius, min_power, min_ratio)
        for max_sources in MAX_SOURCES:
            where = (rows, cols, name, radius, max_sources, min_ratio, min_power)
            got = pkg.find_peaks(frame, rows, cols, radius=radius, max_sources=max_sources, min_power=min_power, min_ratio=min_ratio,
                                 fov_deg=fov_deg)
            want, want_count = restated(frame, rows, cols, radius, max_sources, min_power, min_ratio, fov_deg, keys)
            assert got.sources.shape == (1, max_sources) and got.count.shape == (1,)
            assert_same(got.sources[0], got.count[0], want, want_count, where)
            unused = got.sources[0][want_count:]
            assert np.all(unused["pixel"] == -1) and not unused["power"].any() and not unused["theta"].any() and not unused["row"].any()
            seen["cases"] += 1
            seen["more"] += len(keys) > max_sources
            seen["fewer"] += len(keys) < max_sources
            seen["refined"] += bool(np.any(want["row"][:want_count] != np.floor(want["row"][:want_count])))
        if name == "constant":
            assert list(keys & np.uint64(0xFFFFFFFF)) == [0xFFFFFFFF]  # pixel 0 alone
        if name == "zero":
            assert len(keys) == 0
    assert seen["cases"] > 1500 and seen["more"] > 100 and seen["fewer"] > 100 and seen["refined"] > 100, seen


def test_frames_are_independent(pkg):
    """A batch equals its frames one by one, whatever their neighbours in the batch."""
    for rows, cols in ((5, 3), (33, 17)):
        frames = np.stack(list(contents(rows, cols, seed=7).values()))
        whole = pkg.find_peaks(frames, rows, cols, radius=2, max_sources=4, min_ratio=0.25)
        assert whole.sources.shape == (len(frames), 4)
        for k, frame in enumerate(frames):
            one = pkg.find_peaks(frame, rows, cols, radius=2, max_sources=4, min_ratio=0.25)
            assert whole.sources[k].tobytes() == one.sources[0].tobytes() and whole.count[k] == one.count[0]


@pytest.mark.parametrize("rows,cols,fov_deg", [(32, 32, 180.0), (33, 17, 180.0), (20, 12, 90.0)])
def test_directions_steer_to_the_tables_rows(pkg, rows, cols, fov_deg):
    """At integer pixels -- a symmetric 3 x 3 bump refines by 0 -- steering_delays(theta, phi) is that pixel's row of
    build_delay_table within 5e-5 samples, the project's own bound for the table (tests/test_oracle_golden.py)."""
    xyz = pkg.create_antenna()
    off, frac = pkg.build_delay_table(xyz, rows, cols, fov_deg)
    table = (256 - off).astype(np.float64) + frac
    rng = np.random.default_rng(rows)
    pixels = [(0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1), (rows // 2 - 1, cols // 2 - 1), (3, cols - 1), (rows - 1, 5)]
    pixels += [(int(rng.integers(rows)), int(rng.integers(cols))) for _ in range(24)]
    worst = 0.0
    for r, c in pixels:
        if (2 * r + 1, 2 * c + 1) == (rows, cols):
            continue  # the centre of an odd grid: the table's own row is 0 / 0 there
        frame = np.zeros((rows, cols), np.float32)
        frame[max(r - 1, 0): r + 2, max(c - 1, 0): c + 2] = 1.0
        frame[r, c] = 2.0
        got = pkg.find_peaks(frame, rows, cols, radius=1, max_sources=2, fov_deg=fov_deg)
        assert got.count[0] == 1 and got.pixel[0, 0] == r * cols + c and got.row[0, 0] == r and got.col[0, 0] == c
        tau = pkg.steering_delays(xyz, got.theta[0, 0], got.phi[0, 0])
        worst = max(worst, float(np.abs(tau - table[r * cols + c]).max()))
    print(f"{rows} x {cols} fov {fov_deg}: worst |steering_delays(theta, phi) - table row| = {worst:.3g} samples")
    assert worst < 5e-5
    # the centre of an odd grid, where the reference divides 0 by 0: x = y = 0 exactly on a 1 x 1 grid (0 * sep - sep / 2 + sep / 2), and
    # phi = 0 there; on larger grids rounding leaves some 1e-17 of x and y, and any finite phi
    got = pkg.find_peaks(np.ones(1, np.float32), 1, 1)
    assert got.count[0] == 1 and got.pixel[0, 0] == 0 and got.theta[0, 0] == 0.0 and got.phi[0, 0] == 0.0
    centre = np.zeros((33, 17), np.float32)
    centre[16, 8] = 1.0
    got = pkg.find_peaks(centre, 33, 17)
    assert got.count[0] == 1 and 0.0 <= got.theta[0, 0] < 1e-15 and np.isfinite(got.phi[0, 0])


# ------------------------------------------------------------------------------------------------ refusals

BAD_FINDS = [dict(radius=0), dict(radius=9), dict(radius=-1), dict(max_sources=0), dict(max_sources=33), dict(min_ratio=-0.1),
             dict(min_ratio=1.5), dict(min_ratio=float("nan")), dict(min_power=-1.0), dict(min_power=float("inf")),
             dict(min_power=float("nan")), dict(fov_deg=0.0), dict(fov_deg=180.5), dict(fov_deg=-90.0), dict(fov_deg=float("nan")),
             dict(rows=0), dict(cols=0), dict(rows=-8), dict(rows=1024, cols=1024), dict(rows=65536, cols=65536)]


def find_request(pkg, **field):
    f = pkg.binding.Find(8, 8, 2, 4, 0.0, 0.25, 180.0)
    for name, value in field.items():
        setattr(f, name, value)
    return f


def test_find_entry_points_refuse_bad_arguments(pkg):
    """AWPU_ERR_INVALID before any work: the handle is a zeroed buffer that is not an engine (touching it would crash or change
    it), and the outputs keep their bytes."""
    lib = pkg.binding.load()
    B = pkg.binding
    INV = B.ERR_INVALID
    fake = (C.c_ubyte * 4096)()
    h = C.cast(fake, C.c_void_p)
    wire = (C.c_ubyte * (2 * 256 * 1032))()
    samples = (C.c_float * (64 * 768))()
    sp = C.cast(samples, C.POINTER(C.c_float))
    power = (C.c_float * (2 * 64))()
    pw = C.cast(power, C.POINTER(C.c_float))
    sources = (B.Source * (2 * 32))()
    count = (C.c_int32 * 2)()
    ok = find_request(pkg)
    w = B.Watch(0, 1, 8, 8, 0, 0, 0, None)

    assert lib.awpu_hip_find_peaks(pw, 1, C.byref(ok), sources, count) == 0  # the all-zero frame: no source
    assert count[0] == 0 and sources[0].pixel == -1
    C.memset(sources, 0, C.sizeof(sources))
    assert lib.awpu_hip_find_peaks(None, 1, C.byref(ok), sources, count) == INV
    assert lib.awpu_hip_find_peaks(pw, 1, None, sources, count) == INV
    assert lib.awpu_hip_find_peaks(pw, 1, C.byref(ok), None, count) == INV
    assert lib.awpu_hip_find_peaks(pw, 1, C.byref(ok), sources, None) == INV
    assert lib.awpu_hip_find_peaks(pw, 0, C.byref(ok), sources, count) == INV
    assert lib.awpu_hip_find_peaks(pw, -3, C.byref(ok), sources, count) == INV
    assert lib.awpu_hip_find_peaks_device(None, pw, 1, C.byref(ok), sources, count, None) == INV
    assert lib.awpu_hip_find_peaks_device(h, None, 1, C.byref(ok), sources, count, None) == INV
    assert lib.awpu_hip_find_peaks_device(h, pw, 1, None, sources, count, None) == INV
    assert lib.awpu_hip_find_peaks_device(h, pw, 1, C.byref(ok), None, count, None) == INV
    assert lib.awpu_hip_find_peaks_device(h, pw, 1, C.byref(ok), sources, None, None) == INV
    assert lib.awpu_hip_find_peaks_device(h, pw, 0, C.byref(ok), sources, count, None) == INV

    forms = [
        lambda hh, src_ok, nb, ww, f, s, c, p: lib.awpu_hip_find_blocks(hh, wire if src_ok else None, 1032, nb, ww, f, s, c, p),
        lambda hh, src_ok, nb, ww, f, s, c, p: lib.awpu_hip_find_samples(hh, sp if src_ok else None, 512, nb, ww, f, s, c, p),
        lambda hh, src_ok, nb, ww, f, s, c, p: lib.awpu_hip_find_samples_device(hh, sp if src_ok else None, 512, nb, ww, f, s, c, p, None),
    ]
    for call in forms:
        for p in (pw, None):
            assert call(None, True, 2, C.byref(w), C.byref(ok), sources, count, p) == INV   # no handle
            assert call(h, False, 2, C.byref(w), C.byref(ok), sources, count, p) == INV     # no input
            assert call(h, True, 2, None, C.byref(ok), sources, count, p) == INV            # no w
            assert call(h, True, 2, C.byref(w), None, sources, count, p) == INV             # no f
            assert call(h, True, 2, C.byref(w), C.byref(ok), None, count, p) == INV         # no sources
            assert call(h, True, 2, C.byref(w), C.byref(ok), sources, None, p) == INV       # no count
            assert call(h, True, 0, C.byref(w), C.byref(ok), sources, count, p) == INV      # n_blocks
            for bad in (dict(every=0), dict(every=1025), dict(first=-1)):
                ww = B.Watch(0, 1, 8, 8, 0, 0, 0, None)
                for name, value in bad.items():
                    setattr(ww, name, value)
                assert call(h, True, 2, C.byref(ww), C.byref(ok), sources, count, p) == INV, bad
            for grid in ((8, 4), (4, 8), (16, 16)):  # the find grid is not the watch grid
                assert call(h, True, 2, C.byref(B.Watch(0, 1, grid[0], grid[1], 0, 0, 0, None)), C.byref(ok), sources, count, p) == INV
    for bad in BAD_FINDS:
        f = find_request(pkg, **bad)
        ww = B.Watch(0, 1, f.rows, f.cols, 0, 0, 0, None)
        assert lib.awpu_hip_find_peaks(pw, 1, C.byref(f), sources, count) == INV, bad
        assert lib.awpu_hip_find_peaks_device(h, pw, 1, C.byref(f), sources, count, None) == INV, bad
        for call in forms:
            assert call(h, True, 2, C.byref(ww), C.byref(f), sources, count, pw) == INV, bad
    assert lib.awpu_hip_find_blocks(h, wire, 1031, 2, C.byref(w), C.byref(ok), sources, count, pw) == INV   # datagram stride
    assert lib.awpu_hip_find_samples(h, sp, 511, 2, C.byref(w), C.byref(ok), sources, count, pw) == INV     # sample pitch
    assert bytes(fake) == bytes(4096)
    assert bytes(sources) == bytes(C.sizeof(sources)) and bytes(count) == bytes(8) and bytes(power) == bytes(4 * len(power))
    # the limits themselves are accepted
    for good in (dict(radius=8, max_sources=32, min_ratio=1.0, fov_deg=180.0), dict(radius=1, max_sources=1, min_power=3.0e38, fov_deg=1e-3)):
        assert lib.awpu_hip_find_peaks(pw, 1, C.byref(find_request(pkg, **good)), sources, count) == 0, good
    with pytest.raises(pkg.AwpuError) as ei:
        pkg.find_peaks(np.zeros(64, np.float32), 8, 8, radius=9)
    assert ei.value.status == INV


# ------------------------------------------------------------------------------------------------ the kernel's build

def test_find_kernel_compiles_without_spills(tmp_path, pkg):
    out = tmp_path / "find_kernels.s"
    subprocess.run([pkg._build.hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{REPO / 'include'}", f"-I{CSRC}",
                    "-S", "--cuda-device-only", "-o", str(out), str(CSRC / "find_kernels.hip")], check=True, capture_output=True)
    meta = {}
    for block in out.read_text().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1))
                      for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    assert len(meta) == 1 and "find_peaks_kernel" in next(iter(meta)), sorted(meta)
    m = next(iter(meta.values()))
    print("find_peaks_kernel:", m)
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, m
    assert m["vgpr_count"] <= 128, m  # sixteen waves of a workgroup on one compute unit
    assert m["group_segment_fixed_size"] + pkg.binding.FIND_MAX_PIXELS // 8 <= 64 * 1024  # the LDS plan: static slots + a bit a pixel


# ------------------------------------------------------------------------------------------------ tools/pcap_sources.py

def load_tool():
    spec = importlib.util.spec_from_file_location("pcap_sources", REPO / "tools" / "pcap_sources.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_sources_csv_round_trips(pkg, tmp_path):
    """The tool's writer on the sources of a few frames: the lines parse back to the bits find_peaks returned."""
    tool = load_tool()
    frames = np.stack(list(contents(33, 17, seed=3).values()))
    res = pkg.find_peaks(frames, 33, 17, radius=2, max_sources=4, min_ratio=0.25, fov_deg=120.0)
    blocks = 5 + 3 * np.arange(len(frames))
    path = tmp_path / "sources.csv"
    with open(path, "w", newline="") as f:
        writer = csv.writer(f, lineterminator="\n")
        writer.writerow(tool.HEADER)
        lines = tool.write_rows(writer, blocks, res.sources, res.count)
    assert lines == int(res.count.sum()) > 8 and 0 in res.count  # (the all-zero frame writes no line)
    assert path.read_text().splitlines()[0] == "block,rank,pixel,power,row,col,theta,phi"
    back = tool.read_rows(path)
    k = 0
    for block, entries, n in zip(blocks, res.sources, res.count):
        for rank in range(n):
            row = back[k]
            assert (row["block"], row["rank"], row["pixel"]) == (block, rank, entries[rank]["pixel"])
            for name in ("power", "row", "col", "theta", "phi"):
                assert row[name] == entries[rank][name], name  # the same bits
            k += 1
    assert k == len(back)
    with pytest.raises(ValueError):
        tool.read_rows(REPO / "tools" / "pcap_sources.py")
