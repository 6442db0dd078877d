"""Spectral heatmaps (include/awpu_hip_spectral.h) on a box without a GPU: the entry points are exported beside the other headers'
and built from the listed files; awpu_hip_spectral_compose equals a numpy restatement made of heatmap_u8 alone, for every count of
bands, channel choice and both scales, and at its value edges; bad arguments are refused with nothing written; the host code runs
clean under the address and undefined-behaviour sanitizers as a program of its own; the kernels compile for gfx950 without spills
or scratch, the pre-pass with fused multiply-adds as its only float arithmetic."""
import ctypes as C
import itertools
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "beamforming-lk_amd" / "csrc"
NAMES = ["awpu_hip_spectral_compose", "awpu_hip_process_bands", "awpu_hip_process_bands_device", "awpu_hip_spectral_blocks",
         "awpu_hip_spectral_samples", "awpu_hip_spectral_samples_device"]


def test_spectral_symbols_exported_and_listed(pkg):
    lib = pkg.binding.load()
    B = pkg.binding
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "awpu_hip_spectral.h").read_text(), flags=re.S)
    assert sorted(set(re.findall(r"\b(awpu_hip_\w+)\s*\(", text))) == sorted(NAMES)
    assert '#include "awpu_hip_watch.h"' in text and '#include "awpu_hip_band.h"' in text
    assert int(re.search(r"#define AWPU_SPECTRAL_MAX_BANDS (\d+)", text).group(1)) == 4 == B.SPECTRAL_MAX_BANDS
    assert int(re.search(r"#define AWPU_SPECTRAL_SCALE_COMMON (\d+)", text).group(1)) == 0 == B.SPECTRAL_SCALE_COMMON
    assert int(re.search(r"#define AWPU_SPECTRAL_SCALE_PER_BAND (\d+)", text).group(1)) == 1 == B.SPECTRAL_SCALE_PER_BAND
    assert sorted(B.SPECTRAL_SYMBOLS) == sorted(NAMES)
    for name in NAMES:
        assert hasattr(lib, name)
    for other in (B.EXPORTED_SYMBOLS, B.TRACK_SYMBOLS, B.BLOCK_SYMBOLS, B.LISTEN_SYMBOLS, B.WATCH_SYMBOLS, B.FIND_SYMBOLS, B.BAND_SYMBOLS, B.FOCUS_SYMBOLS):
        assert not set(B.SPECTRAL_SYMBOLS) & set(other)
    assert lib.awpu_hip_abi_version() == 4
    assert "spectral" not in (REPO / "include" / "awpu_hip.h").read_text()
    assert C.sizeof(B.Spectral) == 72  # int32, int32[4], (pad), float *[4], int32[3], int32
    H, S = pkg._build.HEADERS, pkg._build.SOURCES
    assert REPO / "include" / "awpu_hip_spectral.h" in H and CSRC / "spectral_kernels.h" in H and CSRC / "spectral_rule.h" in H
    assert CSRC / "spectral_kernels.hip" in S and CSRC / "spectral_host.cpp" in S


def test_spectral_header_compiles_as_c(tmp_path):
    src = tmp_path / "one.c"
    src.write_text('#include "awpu_hip_spectral.h"\n'
                   "int main(void) { awpu_spectral_t sp; awpu_watch_t w; float p[4]; uint8_t i[12], d[4]; int32_t ch[3] = {0, -1, 0};\n"
                   "  sp.n_bands = AWPU_SPECTRAL_MAX_BANDS; w.first = 0;\n"
                   "  return awpu_hip_spectral_compose(p, 4, 1, 4, ch, AWPU_SPECTRAL_SCALE_PER_BAND, i, d) + awpu_hip_process_bands(0, p, 1, &sp, p)\n"
                   "    + awpu_hip_spectral_samples(0, p, 256, 1, &w, &sp, i, 0, d, p) + (int) sizeof(sp); }\n")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", f"-I{REPO / 'include'}", str(src)], check=True, capture_output=True)


def test_host_file_compiles_with_a_plain_host_compiler(tmp_path):
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{REPO / 'include'}", f"-I{CSRC}", "-c", str(CSRC / "spectral_host.cpp"),
                    "-o", str(tmp_path / "spectral_host.o")], check=True, capture_output=True)


# ------------------------------------------------------------------------------------------------ the display rule

def compose_np(B, power, channel, scale):
    """The header's rule out of heatmap_u8 alone: per plane, or of the shown planes laid end to end."""
    n = power.shape[1]
    image = np.zeros((n, 3), np.uint8)
    shown = [c for c in range(3) if channel[c] >= 0]
    if scale == B.SPECTRAL_SCALE_PER_BAND:
        for c in shown:
            image[:, c] = B.heatmap_u8(power[channel[c]])
    elif shown:
        image[:, shown] = B.heatmap_u8(np.concatenate([power[channel[c]] for c in shown])).reshape(len(shown), n).T
    return image


def dominant_np(power):
    """The greater bits as unsigned 32-bit numbers win; equal bits go to the lower band (argmax takes the first)."""
    return np.argmax(np.ascontiguousarray(power, np.float32).view(np.uint32), axis=0).astype(np.uint8)


CHANNELS = sorted(set(itertools.permutations((0, 1, 2))) | {(0, 1, -1), (-1, 2, 0), (-1, -1, -1), (1, 1, 0), (3, 3, 3), (2, -1, 2), (0, 3, 1), (0, 0, 0), (-1, 0, -1)})


@pytest.mark.parametrize("n", [1, 1024])
@pytest.mark.parametrize("n_bands", [1, 2, 3, 4])
def test_compose_equals_heatmap_u8(pkg, n_bands, n):
    B = pkg.binding
    rng = np.random.default_rng(10 * n_bands + n)
    power = (rng.uniform(0.0, 1.0, (n_bands, n)) * 10.0 ** rng.integers(-3, 3, (n_bands, 1))).astype(np.float32)
    tried = 0
    for channel in CHANNELS:
        if max(channel) >= n_bands:
            continue
        for scale in (B.SPECTRAL_SCALE_COMMON, B.SPECTRAL_SCALE_PER_BAND):
            image, dominant = B.spectral_compose(power, channel, scale)
            assert image.dtype == np.uint8 and image.shape == (n, 3) and dominant.shape == (n,)
            assert np.array_equal(image, compose_np(B, power, channel, scale)), (channel, scale)
            assert np.array_equal(dominant, dominant_np(power)), (channel, scale)
            tried += 1
    assert tried >= 6  # (one band: nothing shown, the band in every byte, in one byte; both scales)
    if n > 1 and n_bands > 1:
        image, _ = B.spectral_compose(power, (0, 1, -1), B.SPECTRAL_SCALE_COMMON)
        other, _ = B.spectral_compose(power, (0, 1, -1), B.SPECTRAL_SCALE_PER_BAND)
        assert image.max() == 255 and other[:, 0].max() == 255 and other[:, 1].max() == 255 and not np.array_equal(image, other)


def test_compose_planes_a_pitch_apart(pkg):
    """band_pitch wider than n: what lies between the planes is neither read nor shown."""
    lib, B = pkg.binding.load(), pkg.binding
    rng = np.random.default_rng(3)
    wide = np.full((3, 50), np.nan, np.float32)
    wide[:, :40] = rng.uniform(0.0, 2.0, (3, 40))
    image, dominant = np.zeros((40, 3), np.uint8), np.zeros(40, np.uint8)
    ch = (C.c_int32 * 3)(2, 0, 1)
    u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    assert lib.awpu_hip_spectral_compose(wide.ctypes.data_as(C.POINTER(C.c_float)), 50, 3, 40, ch, 0, u8(image), u8(dominant)) == B.OK
    want_image, want_dominant = B.spectral_compose(wide[:, :40], (2, 0, 1), 0)
    assert np.array_equal(image, want_image) and np.array_equal(dominant, want_dominant)
    # either output alone
    only = np.zeros((40, 3), np.uint8)
    assert lib.awpu_hip_spectral_compose(wide.ctypes.data_as(C.POINTER(C.c_float)), 50, 3, 40, ch, 0, u8(only), None) == B.OK
    assert np.array_equal(only, want_image)
    only_d = np.zeros(40, np.uint8)
    assert lib.awpu_hip_spectral_compose(wide.ctypes.data_as(C.POINTER(C.c_float)), 50, 3, 40, ch, 0, None, u8(only_d)) == B.OK
    assert np.array_equal(only_d, want_dominant)


def test_compose_value_edges(pkg):
    B = pkg.binding
    for scale in (B.SPECTRAL_SCALE_COMMON, B.SPECTRAL_SCALE_PER_BAND):
        # an all-zero frame: zero image, dominant 0
        image, dominant = B.spectral_compose(np.zeros((3, 16), np.float32), (0, 1, 2), scale)
        assert not image.any() and not dominant.any()
        # a NaN pixel in one band: level 0 there, the maximum and every other pixel as without it
        power = np.random.default_rng(5).uniform(0.1, 1.0, (3, 16)).astype(np.float32)
        clean, _ = B.spectral_compose(power, (0, 1, 2), scale)
        dirty = power.copy()
        dirty[1, 5] = np.nan
        assert int(np.argmax(power[1])) != 5
        image, dominant = B.spectral_compose(dirty, (0, 1, 2), scale)
        assert image[5, 1] == 0
        clean[5, 1] = 0
        assert np.array_equal(image, clean) and image.max() == 255
        # ... and dominant applies the order as written: a NaN's bits (0x7fc00000) beat every finite power's
        assert dominant[5] == 1 and np.array_equal(dominant, dominant_np(dirty))
    # ties go to the lower band
    power = np.array([[1.0, 2.0, 3.0, 0.0], [1.0, 2.5, 3.0, 0.0], [1.0, 2.5, 1.0, 0.0]], np.float32)
    assert list(B.spectral_compose(power, (0, 1, 2), 0)[1]) == [0, 1, 0, 0]
    # -0.0 against +0.0: by bits, 0x80000000 beats 0; and against 1.0 (0x3f800000) too
    power = np.array([[0.0, 0.0, 1.0], [-0.0, 0.0, -0.0]], np.float32)
    assert list(B.spectral_compose(power, (0, 1, -1), 0)[1]) == [1, 0, 1]
    # a negative power or an infinite one: the levels are heatmap_u8's
    power = np.array([[1.0, -2.0, 0.5, np.inf], [3.0, 0.25, -np.inf, 2.0]], np.float32)
    for scale in (B.SPECTRAL_SCALE_COMMON, B.SPECTRAL_SCALE_PER_BAND):
        with np.errstate(invalid="ignore"):
            assert np.array_equal(B.spectral_compose(power, (1, 0, -1), scale)[0], compose_np(B, power, (1, 0, -1), scale))


def test_compose_refusals_write_nothing(pkg):
    lib, B = pkg.binding.load(), pkg.binding
    fp, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    power = np.ones((2, 8), np.float32)
    image, dominant = np.full((8, 3), 7, np.uint8), np.full(8, 7, np.uint8)
    P, I, D = power.ctypes.data_as(fp), image.ctypes.data_as(u8p), dominant.ctypes.data_as(u8p)
    ch = lambda *v: (C.c_int32 * 3)(*v)
    good = ch(0, 1, -1)
    for args in ((None, 8, 2, 8, good, 0, I, D), (P, 8, 2, 8, None, 0, I, D), (P, 8, 2, 8, good, 0, None, None), (P, 8, 2, 0, good, 0, I, D),
                 (P, 8, 2, -1, good, 0, I, D), (P, 8, 0, 8, good, 0, I, D), (P, 8, 5, 8, good, 0, I, D), (P, 8, -1, 8, good, 0, I, D),
                 (P, 8, 2, 8, ch(0, 2, 1), 0, I, D), (P, 8, 2, 8, ch(-2, 0, 1), 0, I, D), (P, 8, 2, 8, ch(0, 1, 4), 0, I, D),
                 (P, 8, 2, 8, good, 2, I, D), (P, 8, 2, 8, good, -1, I, D)):
        assert lib.awpu_hip_spectral_compose(*args) == B.ERR_INVALID
    assert np.all(image == 7) and np.all(dominant == 7)
    with pytest.raises(pkg.AwpuError) as e:
        B.spectral_compose(power, (0, 2, 1))
    assert e.value.status == B.ERR_INVALID


def test_handle_entry_points_refuse_bad_arguments_before_the_handle(pkg):
    """Null handles, and for the runs everything that is judged before the handle is read: a fake handle of zero bytes keeps its
    bytes, the outputs theirs."""
    lib, B = pkg.binding.load(), pkg.binding
    INV = B.ERR_INVALID
    fake = (C.c_ubyte * 4096)()
    h = C.cast(fake, C.c_void_p)
    wire = (C.c_ubyte * (2 * 256 * 1032))()
    samples = (C.c_float * (64 * 768))()
    xs = C.cast(samples, C.POINTER(C.c_float))
    image, big, dominant, power = (C.c_uint8 * (2 * 64 * 3))(), (C.c_uint8 * (2 * 16 * 16 * 3))(), (C.c_uint8 * (2 * 64))(), (C.c_float * (2 * 2 * 64))()
    u8p = C.POINTER(C.c_uint8)
    im, bg, dm, pw = C.cast(image, u8p), C.cast(big, u8p), C.cast(dominant, u8p), C.cast(power, C.POINTER(C.c_float))
    good, keep = B.spectral_of([np.ones(3, np.float32), np.ones(128, np.float32)], (0, 1, -1), B.SPECTRAL_SCALE_PER_BAND)
    w = B.Watch(0, 1, 8, 8, 16, 16, 0, None)

    # the five entry points that take a handle, without one
    assert lib.awpu_hip_process_bands(None, xs, 1, C.byref(good), pw) == INV
    assert lib.awpu_hip_process_bands_device(None, xs, 1, C.byref(good), pw, None) == INV
    forms = [
        lambda hh, sp, ww, *outs: lib.awpu_hip_spectral_blocks(hh, wire, 1032, 2, ww, sp, *outs),
        lambda hh, sp, ww, *outs: lib.awpu_hip_spectral_samples(hh, xs, 512, 2, ww, sp, *outs),
        lambda hh, sp, ww, *outs: lib.awpu_hip_spectral_samples_device(hh, xs, 512, 2, ww, sp, *outs, None),
    ]

    def bands(**change):
        sp, arrays = B.spectral_of([np.ones(3, np.float32), np.ones(128, np.float32)], (0, 1, -1), B.SPECTRAL_SCALE_PER_BAND)
        for name, value in change.items():
            if name == "taps1":
                sp.taps[1] = value
            elif name == "coef1":
                arrays.append(np.ascontiguousarray(value, np.float32))
                sp.coef[1] = arrays[-1].ctypes.data_as(C.POINTER(C.c_float)) if value is not None else None
                sp.taps[1] = arrays[-1].size
            elif name == "channel2":
                sp.channel[2] = value
            else:
                setattr(sp, name, value)
        return sp, arrays

    bad_sets = [dict(n_bands=0), dict(n_bands=5), dict(n_bands=-1), dict(taps1=129), dict(taps1=0), dict(coef1=[1.0, np.inf, 1.0]), dict(coef1=[np.nan]),
                dict(channel2=2), dict(channel2=4), dict(channel2=-2), dict(scale=2), dict(scale=-1)]
    for call in forms:
        assert call(None, C.byref(good), C.byref(w), im, bg, dm, pw) == INV          # no handle
        assert call(h, None, C.byref(w), im, bg, dm, pw) == INV                      # no bands
        assert call(h, C.byref(good), None, im, bg, dm, pw) == INV                   # no w
        assert call(h, C.byref(good), C.byref(w), None, None, None, None) == INV     # no output
        for change in bad_sets:
            sp, arrays = bands(**change)
            assert call(h, C.byref(sp), C.byref(w), im, bg, dm, pw) == INV, change
            assert call(h, C.byref(sp), C.byref(w), None, None, None, pw) == INV, change
        sp, arrays = bands()
        sp.coef[1] = None                                                            # a band without coefficients
        assert call(h, C.byref(sp), C.byref(w), im, bg, dm, pw) == INV
        for field, value in (("every", 0), ("every", 1025), ("first", -1), ("flip", 2), ("out_rows", 7), ("out_cols", 7)):  # the watch run's checks
            ww = B.Watch(0, 1, 8, 8, 16, 16, 0, None)
            setattr(ww, field, value)
            assert call(h, C.byref(good), C.byref(ww), im, bg, dm, pw) == INV, field
        ww = B.Watch(0, 1, 8, 8, 16, 16, 0, C.c_void_p(4096))                        # a colour table
        assert call(h, C.byref(good), C.byref(ww), im, bg, dm, pw) == INV
    assert bytes(fake) == bytes(4096)
    for out in (image, big, dominant):
        assert bytes(out) == bytes(len(out))
    assert bytes(power) == bytes(4 * len(power))
    del keep


def test_the_video_tools_bands_option(pkg):
    """--bands of tools/pcap_video.py: band_from_text per entry, lowest band first, red = the lowest band in a B G R pixel; together
    with --band an error."""
    import importlib.util
    import sys

    B = pkg.binding
    spec = importlib.util.spec_from_file_location("pcap_video", REPO / "tools" / "pcap_video.py")
    tool = importlib.util.module_from_spec(spec)
    sys.modules["pcap_video"] = tool
    spec.loader.exec_module(tool)
    bands, channel = tool.bands_of_text(B, "6375:9000,1950:3541:31,3541:6375")
    assert channel == (2, 1, 0) and [len(c) for c in bands] == [31, 63, 63]
    assert np.array_equal(bands[0], B.band_design(1950, 3541, 31)) and np.array_equal(bands[2], B.band_design(6375, 9000, 63))
    assert tool.bands_of_text(B, "1950:3541,6375:9000")[1] == (-1, 1, 0) and tool.bands_of_text(B, "0:4000")[1] == (-1, -1, 0)
    for bad in ("", "1:2,3:4,5:6,7:8", "a:b,1:2"):
        with pytest.raises(ValueError):
            tool.bands_of_text(B, bad)
    with pytest.raises(SystemExit):
        tool.main(["nothing.pcap", "--port", "1", "--band", "1:2", "--bands", "1:2,3:4"])
    text = (REPO / "tools" / "pcap_video.py").read_text()
    assert '"--bands"' in text and "spectral_blocks" in text


# ------------------------------------------------------------------------------------------------ sanitizers, and the kernels' build

def test_host_code_runs_clean_under_sanitizers(tmp_path):
    """tests/host/spectral_rule_check.cpp with spectral_host.cpp: a program of its own under ASan and UBSan, largest and smallest sizes."""
    exe = tmp_path / "spectral_rule_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{REPO / 'include'}", f"-I{CSRC}", str(REPO / "tests" / "host" / "spectral_rule_check.cpp"), str(CSRC / "spectral_host.cpp"),
                    "-o", str(exe)], check=True, capture_output=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "spectral rule: ok" in out.stdout, out.stdout + out.stderr


def test_spectral_kernels_compile_without_spills(tmp_path, pkg):
    out = tmp_path / "spectral_kernels.s"
    subprocess.run([pkg._build.hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{REPO / 'include'}", f"-I{CSRC}",
                    "-S", "--cuda-device-only", "-o", str(out), str(CSRC / "spectral_kernels.hip")], check=True, capture_output=True)
    text = out.read_text()
    meta = {}
    for block in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1))
                      for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    kernels = ("spectral_filter_kernel", "spectral_max_kernel", "spectral_compose_kernel", "spectral_upscale_kernel")
    assert len(meta) == 4 and all(any(k in name for name in meta) for k in kernels), sorted(meta)
    for name, m in meta.items():
        print(name, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
    pre_pass = next(name for name in meta if "spectral_filter_kernel" in name)
    assert meta[pre_pass]["group_segment_fixed_size"] == 4 * 640 * 4  # the band kernel's rows: staged once, however many bands
    # the pre-pass's own code: from its label to the end of its program.  The rule's steps are fused multiply-adds (single or packed,
    # one rounding a lane) and nothing else: no separate multiply or add of floats anywhere in the kernel
    body = text.split(f"\n{pre_pass}:", 1)[1].split("s_endpgm", 1)[0]
    assert re.search(r"\bv_(pk_)?fmac?_f32", body) and not re.search(r"\bv_(pk_)?(mul|add|sub|mac)_f32", body)
    assert "ds_read" in body or "ds_load" in body
