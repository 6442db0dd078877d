"""Tone maps (include/awpu_hip_tones.h) on a box without a GPU: the entry points are exported beside the other headers' and built
from the globbed files; awpu_hip_tones_host equals a numpy restatement of the rule bit for bit, its out[] is the coherence rule's
sums, its bins meet an fp64 transform and add up to the power (Parseval); on the two-source scene the band maps and the pitch
find the weak source the power map loses; value edges, refusals that write nothing; the host code runs clean under the address
and undefined-behaviour sanitizers as a program of its own; the kernel compiles for gfx950 without spills or scratch; the tools'
new flags parse."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import tones_util as TU
import util

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "beamforming-lk_amd" / "csrc"
GOLDEN = REPO / "tests" / "golden"
NAMES = ["awpu_hip_tones_window", "awpu_hip_tones_twiddles", "awpu_hip_tones_linear", "awpu_hip_tones_host", "awpu_hip_tones",
         "awpu_hip_tones_device", "awpu_hip_tones_device_bins", "awpu_hip_tones_blocks", "awpu_hip_tones_samples", "awpu_hip_tones_samples_device"]
F32P, I32P, U8P = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
ALL = ("tone", "pitch", "bins", "spectrum")
UNEVEN = [3, 4, 40, 41, 127]  # edge[0] > 0, edge[n] < 129, groups of one bin beside wide ones


# ------------------------------------------------------------------------------------------------ wiring

def test_tones_symbols_exported_and_listed(pkg):
    lib = pkg.binding.load()
    B = pkg.binding
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "awpu_hip_tones.h").read_text(), flags=re.S)
    assert sorted(set(re.findall(r"\b(awpu_hip_\w+)\s*\(", text))) == sorted(NAMES)
    assert int(re.search(r"#define AWPU_TONES_BINS (\d+)", text).group(1)) == 129 == B.TONES_BINS
    assert int(re.search(r"#define AWPU_TONES_RECT (\d+)", text).group(1)) == 0 == B.TONES_RECT
    assert int(re.search(r"#define AWPU_TONES_HANN (\d+)", text).group(1)) == 1 == B.TONES_HANN
    assert int(re.search(r"#define AWPU_TONES_SHOW_PITCH \((-\d+)\)", text).group(1)) == -1 == B.TONES_SHOW_PITCH
    assert sorted(B.TONES_SYMBOLS) == sorted(NAMES)
    for name in NAMES:
        assert hasattr(lib, name)
    for other in (B.EXPORTED_SYMBOLS, B.TRACK_SYMBOLS, B.BLOCK_SYMBOLS, B.LISTEN_SYMBOLS, B.WATCH_SYMBOLS, B.FIND_SYMBOLS, B.BAND_SYMBOLS, B.FOCUS_SYMBOLS,
                  B.SPECTRAL_SYMBOLS, B.EXPOSE_SYMBOLS, B.COHERE_SYMBOLS, B.PEEL_SYMBOLS):
        assert not set(B.TONES_SYMBOLS) & set(other)
    assert lib.awpu_hip_abi_version() == 4
    main = (REPO / "include" / "awpu_hip.h").read_text()
    assert "awpu_hip_tones" not in main.replace("awpu_hip_tones.h", "") and "awpu_tones_t" not in main
    assert C.sizeof(B.Tones) == 528
    assert B.KERNEL_NAMES[19] == "tones" and len(B.KERNEL_NAMES) == 20 and "AWPU_KERNEL_TONES = 19" in main
    H, S = pkg._build.HEADERS, pkg._build.SOURCES
    assert REPO / "include" / "awpu_hip_tones.h" in H and CSRC / "tones_kernels.h" in H and CSRC / "tones_rule.h" in H
    assert CSRC / "tones_kernels.hip" in S and CSRC / "tones_host.cpp" in S and CSRC / "awpu_tones.cpp" in S
    # the rule is host-only and lives in one header; no device file may include it
    assert "tones_rule.h" in (CSRC / "tones_host.cpp").read_text() and "tones_rule.h" in (REPO / "tests" / "host" / "tones_rule_check.cpp").read_text()
    for device_file in list(CSRC.glob("*.hip")) + [CSRC / "tones_kernels.h"]:
        assert "tones_rule.h" not in device_file.read_text(), device_file
    for name in ("tones_host", "tones_linear", "tones_of", "tones_twiddles", "tones_window"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    for name in ("tones", "tones_device", "tones_device_bins", "tones_blocks", "tones_samples", "tones_samples_device"):
        assert callable(getattr(B.Engine, name))


def test_tones_header_compiles_as_c(tmp_path):
    src = tmp_path / "one.c"
    src.write_text('#include "awpu_hip_tones.h"\n'
                   "typedef char size_is_528[sizeof(awpu_tones_t) == 528 ? 1 : -1];\n"
                   "int main(void) { awpu_tones_t t; awpu_watch_t w; awpu_find_t f; awpu_source_t s[2]; float p[256]; float tw[128][2]; int32_t n[4]; uint8_t i[4];\n"
                   "  t.window = AWPU_TONES_HANN; t.n_groups = 1; t.edge[0] = 0; t.edge[AWPU_TONES_BINS] = 129; w.first = 0; f.rows = 1;\n"
                   "  return awpu_hip_tones_window(AWPU_TONES_RECT, p) + awpu_hip_tones_twiddles(tw) + awpu_hip_tones_linear(1.0f, 2.0f, 1, 3.0f, &t)\n"
                   "    + awpu_hip_tones_host(p, 1, 1, 257, n, p, 1, 1, n, 1, 0, &t, p, n, 0, 0) + awpu_hip_tones(0, p, 1, &t, p, n)\n"
                   "    + awpu_hip_tones_device(0, p, 1, &t, p, n, 0) + awpu_hip_tones_device_bins(0, p, 1, &t, p, n, p, p, 0)\n"
                   "    + awpu_hip_tones_blocks(0, p, 1032, 1, &w, &t, AWPU_TONES_SHOW_PITCH, &f, i, i, p, s, n)\n"
                   "    + awpu_hip_tones_samples(0, p, 256, 1, &w, &t, 0, &f, i, i, p, s, n)\n"
                   "    + awpu_hip_tones_samples_device(0, p, 256, 1, &w, &t, 0, &f, i, i, p, s, n, 0) + (int) sizeof(size_is_528); }\n")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", f"-I{REPO / 'include'}", str(src)], check=True, capture_output=True)


def test_host_file_compiles_with_a_plain_host_compiler(tmp_path):
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{REPO / 'include'}", f"-I{CSRC}", "-c", str(CSRC / "tones_host.cpp"),
                    "-o", str(tmp_path / "tones_host.o")], check=True, capture_output=True)


# ------------------------------------------------------------------------------------------------ the rule

@pytest.fixture(scope="module")
def c1(pkg):
    """The c1 table, the frame synthetic.make_frames(xyz, 1) makes and the two-source scene's, with the host rule's answers
    (computed once, never written)."""
    S = pkg.synthetic
    spec = S.WORKLOADS["c1"]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    frame = S.make_frames(xyz, 1)[0]
    rect = pkg.tones_host(frame, off, frac, [0, 129], want=ALL)
    power, _, _, sums, _ = pkg.cohere_host(frame, off, frac, want_sums=True)
    r, c = S.source_pixel(spec)
    scene = TU.scene_frame(pkg, xyz)
    return dict(spec=spec, xyz=xyz, off=off, frac=frac, frame=frame, rect=rect, power=power, sums=sums, source=r * spec.res + c, scene=scene,
                index51=np.load(GOLDEN / "sweep_c1_ragged.npz")["index"])


def assert_equals_restatement(pkg, frame, off, frac, edges, window, index=None, gain=None):
    got = pkg.tones_host(frame, off, frac, edges, window, index=index, gain=gain, want=ALL)
    want = TU.rule(pkg, frame, off, frac, edges, window, index, gain)
    for name in ("tone", "bins", "spectrum"):
        assert got[name].dtype == np.float32 and got[name].shape == want[name].shape and TU.same_bits(got[name], want[name]), name
    assert got["pitch"].dtype == np.int32 and np.array_equal(got["pitch"], want["pitch"])
    return got, want


def test_host_rule_equals_the_numpy_restatement_on_c1(pkg, c1):
    want = TU.rule(pkg, c1["frame"], c1["off"], c1["frac"], [0, 129])
    for name in ("tone", "bins", "spectrum"):
        assert TU.same_bits(c1["rect"][name], want[name]), name
    assert np.array_equal(c1["rect"]["pitch"], want["pitch"])
    assert TU.same_bits(want["sums"], c1["sums"])  # the restatement's out[] is the coherence rule's too


def test_host_rule_with_hann_and_129_groups(pkg, c1):
    pixels = np.arange(0, 1024, 13)
    got, _ = assert_equals_restatement(pkg, c1["frame"], c1["off"][pixels], c1["frac"][pixels], list(range(130)), 1)
    assert TU.same_bits(got["tone"], got["bins"].T)  # groups of one bin are the bins


def test_host_rule_on_the_ragged_51_mic_list_with_uneven_edges(pkg, c1):
    assert len(c1["index51"]) == 51
    pixels = np.arange(0, 1024, 7)
    for window in (0, 1):
        assert_equals_restatement(pkg, c1["frame"], c1["off"][pixels], c1["frac"][pixels], UNEVEN, window, index=c1["index51"])


def test_host_rule_with_gains_and_with_one_mic(pkg, c1):
    gain = (0.5 + np.random.default_rng(3).random(51)).astype(np.float32)
    pixels = np.arange(3, 1024, 11)
    with_gain, _ = assert_equals_restatement(pkg, c1["frame"], c1["off"][pixels], c1["frac"][pixels], UNEVEN, 1, index=c1["index51"], gain=gain)
    without = pkg.tones_host(c1["frame"], c1["off"][pixels], c1["frac"][pixels], UNEVEN, 1, index=c1["index51"], want=("bins",))
    assert not TU.same_bits(with_gain["bins"], without["bins"])
    assert_equals_restatement(pkg, c1["frame"], c1["off"][pixels], c1["frac"][pixels], [0, 129], 0, index=[37])


def test_host_rule_on_a_three_pixel_table_and_a_batch(pkg, c1):
    pixels = np.array([0, 517, 1023])
    frames = pkg.synthetic.make_frames(c1["xyz"], 3, seed=77)
    got = pkg.tones_host(frames, c1["off"][pixels], c1["frac"][pixels], UNEVEN, 1, want=ALL)
    assert got["tone"].shape == (3, 4, 3) and got["pitch"].shape == (3, 3) and got["bins"].shape == (3, 3, 129) and got["spectrum"].shape == (3, 3, 129, 2)
    for b in range(3):
        want = TU.rule(pkg, frames[b], c1["off"][pixels], c1["frac"][pixels], UNEVEN, 1)
        for name in ("tone", "bins", "spectrum"):
            assert TU.same_bits(got[name][b], want[name]), name
        assert np.array_equal(got["pitch"][b], want["pitch"])


def test_sums_are_the_coherence_rules(pkg, c1, tmp_path):
    """out[] is not an output of tones_host, so the C's own step 1 (tones_rule.h's tones_sums) is set beside cohere_rule.h's
    cohere_pixel in a small program: on c1's frame with the table rows of five pixels, the ragged 51-mic list and gains, out[] is
    the same bits.  (The restatement's out[] equals cohere_host's sums above, and tones_host's bins the restatement's.)"""
    pixels = np.array([0, 31, c1["source"], 700, 1023])
    gain = (0.5 + np.random.default_rng(4).random(51)).astype(np.float32)
    np.ascontiguousarray(c1["frame"], np.float32).tofile(tmp_path / "frame.f32")
    np.ascontiguousarray(c1["off"][pixels], np.int32).tofile(tmp_path / "off.i32")
    np.ascontiguousarray(c1["frac"][pixels], np.float32).tofile(tmp_path / "frac.f32")
    np.ascontiguousarray(c1["index51"], np.int32).tofile(tmp_path / "index.i32")
    gain.tofile(tmp_path / "gain.f32")
    src = tmp_path / "sums.cpp"
    src.write_text('#include "tones_rule.h"\n#include <cstdio>\n#include <string>\n#include <vector>\n'
                   'template <class T> std::vector<T> load(const std::string &path, size_t n) { std::vector<T> v(n); FILE *f = std::fopen(path.c_str(), "rb");\n'
                   '  if (!f || std::fread(v.data(), sizeof(T), n, f) != n) std::abort(); std::fclose(f); return v; }\n'
                   'int main(int, char **argv) { const std::string d = argv[1];\n'
                   '  const auto x = load<float>(d + "/frame.f32", 64 * 1024); const auto off = load<int32_t>(d + "/off.i32", 5 * 64);\n'
                   '  const auto frac = load<float>(d + "/frac.f32", 5 * 64); const auto index = load<int32_t>(d + "/index.i32", 51);\n'
                   '  const auto gain = load<float>(d + "/gain.f32", 51); std::vector<float> o(256), s(256), e(256);\n'
                   '  for (int p = 0; p < 5; p++) for (int g = 0; g < 2; g++) {\n'
                   '    awpu::tones_sums(x.data(), 1024, &off[p * 64], &frac[p * 64], index.data(), 51, g ? gain.data() : nullptr, o.data());\n'
                   '    awpu::cohere_pixel(x.data(), 1024, &off[p * 64], &frac[p * 64], index.data(), 51, g ? gain.data() : nullptr, s.data(), e.data());\n'
                   '    for (int i = 0; i < 256; i++) if (__builtin_memcmp(&o[i], &s[i], 4)) return 1; }\n'
                   '  std::puts("same"); return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", f"-I{REPO / 'include'}", f"-I{CSRC}", str(src), "-o", str(tmp_path / "sums")],
                   check=True, capture_output=True)
    assert subprocess.run([str(tmp_path / "sums"), str(tmp_path)], capture_output=True, text=True).stdout.strip() == "same"


def test_tables(pkg):
    """Within one unit in the last place of numpy's float64 values rounded to float32; wss is the sum of the window's squares."""
    i = np.arange(256, dtype=np.float64)
    hann64 = 0.5 - 0.5 * np.cos(2.0 * np.pi * i / 256.0)
    k = np.arange(128, dtype=np.float64)
    tw64 = np.stack([np.cos(2.0 * np.pi * k / 256.0), -np.sin(2.0 * np.pi * k / 256.0)], axis=1)

    def ulps(got, want64):
        want = want64.astype(np.float32)
        return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.maximum(np.spacing(np.abs(want)).astype(np.float64), 1e-45)

    assert TU.same_bits(pkg.tones_window(0), np.ones(256, np.float32))
    hann, tw = pkg.tones_window(1), pkg.tones_twiddles()
    assert hann.shape == (256,) and tw.shape == (128, 2)
    assert ulps(hann, hann64).max() <= 1.0 and ulps(tw, tw64).max() <= 1.0
    assert hann[0] == 0.0 and hann[128] == 1.0 and tw[0, 0] == 1.0 and tw[64, 1] == -1.0
    assert float((np.ones(256) ** 2).sum()) == 256.0
    assert abs(float((hann64 ** 2).sum()) - 96.0) <= 1e-12  # exact for the periodic Hann window: 256 * 3 / 8
    assert abs(float((hann.astype(np.float64) ** 2).sum()) - 96.0) <= 96.0 * 2.0 ** -23


def test_tones_linear_and_tones_of(pkg):
    B = pkg.binding
    t = pkg.tones_linear(2500.0, 3500.0, 2)
    assert t.n_groups == 2 and list(B.tones_edges(t)) == [14, 17, 19]  # centres 2670 .. 3433 Hz; the wider run first
    t = pkg.tones_linear(0.0, 1e9, 129, window=B.TONES_HANN)
    assert t.window == 1 and list(B.tones_edges(t)) == list(range(130))
    t = pkg.tones_linear(0.0, 25000.0, 4)
    assert list(np.diff(B.tones_edges(t))) == [33, 32, 32, 32]
    for bad in ((2500.0, 3500.0, 6), (3500.0, 2500.0, 1), (2500.0, 3500.0, 0), (0.0, 1e9, 130)):
        with pytest.raises(B.AwpuError) as err:
            pkg.tones_linear(*bad)
        assert err.value.status == B.ERR_INVALID
    assert list(B.tones_edges(pkg.tones_of((2500.0, 3500.0, 2)))) == [14, 17, 19]
    t = pkg.tones_of(UNEVEN, B.TONES_HANN)
    assert (t.window, t.n_groups, list(B.tones_edges(t))) == (1, 4, UNEVEN) and pkg.tones_of(t) is t


# ------------------------------------------------------------------------------------------------ against fp64, and Parseval

def frames_for_accuracy(pkg, xyz, seed):
    """Noise, a tone in noise (synthetic.make_frames), and an on-bin tone (bin 47, from make_frames' direction, amplitude 1e-2) on a
    DC offset of a quarter of full scale."""
    S = pkg.synthetic
    n = xyz.shape[1]
    t = np.arange(1024, dtype=np.float64)
    tau = pkg.binding.steering_delays(xyz, S.SOURCE_THETA, S.SOURCE_PHI).astype(np.float64)
    on_bin = (1e-2 * np.sin(2.0 * np.pi * 47.0 * (t[None, :] + tau[:, None]) / 256.0) + 0.25).astype(np.float32)
    return dict(noise=util.hash_frames(n, 1024, seed=seed, batch=1)[0], tone=S.make_frames(xyz, 1)[0], on_bin_dc=on_bin)


FLAT = 2e-6  # of the pixel's largest bin


def check_against_fp64(pkg, name, frame, off, frac, index, window, source):
    """Every pixel of `off`; `source` is the row of the pixel the frames' wave comes from.  -> the worst flat figure asserted."""
    usable = off.shape[1] if index is None else len(index)
    got = pkg.tones_host(frame, off, frac, [0, 129], window, index=index, want=("bins",))["bins"]
    out = TU.sums(frame, off, frac, index)
    want, floor = TU.bins64(out, pkg.tones_window(window), 96.0 if window else 256.0, usable, want_floor=True)
    top = want.max(axis=1)
    diff = np.abs(got - want)
    err = diff.max(axis=1) / top
    print(f"{name} {usable} mics: every pixel {err.max():.3g}, the source's pixel {err[source]:.3g}, "
          f"the stencil's floor at most {float((floor.max(axis=1) / top).max()):.3g} of the largest bin")
    if name != "on_bin_dc" or usable == 1:
        assert err.max() <= FLAT, (name, usable)
        return float(err.max())
    assert (diff <= FLAT * top[:, None] + floor).all(), (name, usable, float((diff - floor).max(axis=1).max()))
    assert err[source] <= FLAT, (name, usable)
    return float(err[source])


@pytest.mark.parametrize("window", [0, 1])
def test_bins_meet_an_fp64_transform_of_the_same_sums(pkg, c1, window):
    """|bins - bins64| <= 2e-6 of the pixel's largest bin at every pixel, bins64 numpy's rfft of the rule's own out[] in float64
    (steps 2 to 4), on noise and on a tone in noise with 1, 3, 51, 64 and 256 mics, and on the DC frame with one mic.  Measured
    worst: 9.5e-7 (the bound is five times the 4.2e-7 of the experiment behind the feature).

    The DC frame with more than one mic is asserted at every pixel too, against that bound PLUS the stencil's own floor,
    tones_util.stencil_floor, derived from the number format alone: the stencil adds out[i+1] + out[i-1] in fp32, on a DC offset
    of 0.25 over U mics that sum is near U / 2 and loses up to ulp(U / 2) / 2 whatever tone rides on it, and in the nulls of the
    array's pattern the pixel's largest bin sinks towards what that loss adds up to (measured 3.0e-4 of the largest bin at 64 mics,
    4.4e-6 at 3, 3.4e-3 at 256; the floor is a worst case, every sample's loss of one sign, and stands at 1.2e-2, 6.0e-5 and 0.12
    of the largest bin there: forty times what is measured, and still far under the order-one error of a wrong butterfly).  The flat bound cannot hold there for any implementation of the rule -- the loss is step 2's, the reference's
    stencil, not the transform's --, so the floor is added where it applies and nowhere else; at the pixel the wave comes from,
    where the mics' tones add up, the flat bound alone is asserted on the DC frame as well."""
    S = pkg.synthetic
    pixels = np.append(np.arange(0, 1024, 9), c1["source"])
    off, frac = c1["off"][pixels], c1["frac"][pixels]
    worst = 0.0
    for name, frame in frames_for_accuracy(pkg, c1["xyz"], 91).items():
        for index in (None, [5], [0, 9, 63], c1["index51"]):
            worst = max(worst, check_against_fp64(pkg, name, frame, off, frac, index, window, len(pixels) - 1))
    four = S.WorkloadSpec("four arrays, 16 x 16", 4, 1, 16)  # 256 mics
    xyz4 = S.geometry(four)
    off4, frac4 = S.delay_table(four, xyz4)
    r, c = S.source_pixel(four)
    for name, frame in frames_for_accuracy(pkg, xyz4, 93).items():
        worst = max(worst, check_against_fp64(pkg, name, frame, off4, frac4, None, window, r * four.res + c))
    print("worst", worst)


def test_parseval_the_bins_add_up_to_the_power(pkg, c1):
    """RECT, one group over all bins: within 1e-5 (the project's flat bound) of cohere_host's power at every pixel.  Measured 1.3e-6."""
    err = TU.rel_err(c1["rect"]["tone"][0], c1["power"])
    print("parseval", err)
    assert err <= 1e-5
    noise = util.hash_frames(64, 1024, seed=92, batch=1)[0]
    tone = pkg.tones_host(noise, c1["off"], c1["frac"], [0, 129], index=c1["index51"], want=("tone",))["tone"][0]
    err = TU.rel_err(tone, pkg.cohere_host(noise, c1["off"], c1["frac"], index=c1["index51"])[0])
    print("parseval, noise on 51 mics", err)
    assert err <= 1e-5


# ------------------------------------------------------------------------------------------------ the physics, on c1

def test_the_band_maps_find_the_source_the_power_map_loses(pkg, c1):
    """Source A: 9 kHz (bin 47), 1e-2, (20, 35) deg; source B: 3.05 kHz (bin 16), 3e-3, (40, 200) deg, 26.4 dB under A in the power
    map; uniform noise 1e-3."""
    A, B = TU.scene_pixels(pkg, c1["spec"])
    power = pkg.cohere_host(c1["scene"], c1["off"], c1["frac"])[0]
    print("B under A, dB", 10 * np.log10(power[B] / power[A]))
    assert int(power.argmax()) == A and power[B] < 0.01 * power[A]
    got = pkg.tones_host(c1["scene"], c1["off"], c1["frac"], [13, 20, 44, 51])
    assert int(got["tone"][0].argmax()) == B and int(got["tone"][2].argmax()) == A
    pitch = pkg.tones_host(c1["scene"], c1["off"], c1["frac"], [0, 129], want=("pitch",))["pitch"]
    assert pitch[A] == 47 and pitch[B] == 16


def test_make_frames_has_pitch_47_at_the_source(c1):
    assert c1["rect"]["pitch"][c1["source"]] == 47


# ------------------------------------------------------------------------------------------------ values

def test_silence_and_dc_have_no_tones(pkg, c1):
    pixels = np.arange(0, 1024, 31)
    off, frac = c1["off"][pixels], c1["frac"][pixels]
    for value in (0.0, -0.0, 0.25):  # (a DC bias cancels in the stencil: 0.5 s - 0.25 (s + s) = 0 whatever s the mics add up to)
        got = pkg.tones_host(np.full((64, 1024), value, np.float32), off, frac, UNEVEN, 1, want=ALL)
        assert TU.same_bits(got["bins"], np.zeros_like(got["bins"])) and TU.same_bits(got["tone"], np.zeros_like(got["tone"]))
        assert (got["pitch"] == UNEVEN[0]).all()


def test_powers_of_two_scale_the_spectrum_exactly(pkg, c1):
    pixels = np.arange(5, 1024, 41)
    off, frac = c1["off"][pixels], c1["frac"][pixels]
    base = pkg.tones_host(c1["frame"], off, frac, [0, 129], 1, want=("spectrum",))["spectrum"]
    assert np.abs(base).max() > 1e-3
    for scale in (2.0 ** -40, 2.0 ** 55):
        got = pkg.tones_host(c1["frame"] * np.float32(scale), off, frac, [0, 129], 1, want=("spectrum",))["spectrum"]
        assert np.isfinite(got).all() and TU.same_bits(got, base * np.float32(scale)), scale


def test_a_nan_reaches_only_the_pixels_that_read_it_and_only_its_frame(pkg, c1):
    pixels = np.arange(0, 1024, 9)
    off, frac = c1["off"][pixels], c1["frac"][pixels]
    at = int(np.median(off[:, 0])) + 256  # the last sample that half of these pixels read of mic 0
    frames = np.stack([c1["frame"], c1["frame"]])
    frames[1, 0, at] = np.nan
    got = pkg.tones_host(frames, off, frac, UNEVEN, 1, want=ALL)
    clean = pkg.tones_host(c1["frame"], off, frac, UNEVEN, 1, want=ALL)
    reads = (off[:, 0] <= at) & (at <= off[:, 0] + 256)
    assert reads.any() and not reads.all()
    for name in ALL:
        assert TU.same_bits(got[name][0].astype(np.float32), clean[name].astype(np.float32)), name
    assert TU.same_bits(got["bins"][1][~reads], clean["bins"][~reads]) and np.array_equal(got["pitch"][1][~reads], clean["pitch"][~reads])
    assert TU.same_bits(got["tone"][1][:, ~reads], clean["tone"][:, ~reads])
    # (with frac = 0 the lerp is 0 * (x0 - x1) + x1: the NaN reaches out[] from either side)
    assert np.isnan(got["bins"][1][reads]).all()
    want = TU.rule(pkg, frames[1], off, frac, UNEVEN, 1)
    assert TU.same_bits(got["bins"][1], want["bins"]) and np.array_equal(got["pitch"][1], want["pitch"])


# ------------------------------------------------------------------------------------------------ refusals

def test_host_rule_refusals_write_nothing(pkg, c1):
    lib, B = pkg.binding.load(), pkg.binding
    off, frac = c1["off"][:4].copy(), c1["frac"][:4].copy()
    frame = np.ascontiguousarray(c1["frame"])
    index = np.arange(64, dtype=np.int32)
    good = B.tones_of(UNEVEN, 1)
    tone, pitch = np.full((4, 4), -5.0, np.float32), np.full(4, -5, np.int32)
    bins, spectrum = np.full((4, 129), -5.0, np.float32), np.full((4, 129, 2), -5.0, np.float32)
    fp = lambda a: a.ctypes.data_as(F32P)
    ip = lambda a: a.ctypes.data_as(I32P)

    def call(frame_p=fp(frame), batch=1, n_streams=64, hist=1024, off_=off, frac_=frac, stride=64, n_pixels=4, index_=index, usable=64, t=good,
             outputs=True):
        outs = [fp(tone), ip(pitch), fp(bins), fp(spectrum)] if outputs else [None] * 4
        return lib.awpu_hip_tones_host(frame_p, batch, n_streams, hist, None if off_ is None else ip(off_), None if frac_ is None else fp(frac_),
                                       stride, n_pixels, None if index_ is None else ip(index_), usable, None, None if t is None else C.byref(t), *outs)

    for bad_off in (1024 - 256, 1024, -1):  # entries reading outside the history
        o = off.copy()
        o[3, 63] = bad_off
        assert call(off_=o) == B.ERR_RANGE, bad_off
    for bad_frac in (-1e-6, 1.0 + 1e-6, np.nan, np.inf):
        f = frac.copy()
        f[0, 0] = bad_frac
        assert call(frac_=f) == B.ERR_INVALID, bad_frac
    assert call(frame_p=None) == B.ERR_INVALID and call(off_=None) == B.ERR_INVALID and call(frac_=None) == B.ERR_INVALID
    assert call(index_=None) == B.ERR_INVALID and call(t=None) == B.ERR_INVALID and call(outputs=False) == B.ERR_INVALID
    for kw in (dict(batch=0), dict(n_streams=0), dict(hist=256), dict(stride=0), dict(n_pixels=0), dict(usable=0), dict(n_streams=63),
               dict(index_=np.full(64, 64, np.int32)), dict(index_=np.full(64, -1, np.int32))):
        assert call(**kw) == B.ERR_INVALID, kw
    bad_requests = [B.tones_of(UNEVEN, 2), B.tones_of(UNEVEN, -1), B.tones_of([3, 3, 5]), B.tones_of([5, 4]), B.tones_of([-1, 4]), B.tones_of([100, 130])]
    for n_groups in (0, -1, 130):
        t = B.tones_of(UNEVEN)
        t.n_groups = n_groups
        bad_requests.append(t)
    for t in bad_requests:
        assert call(t=t) == B.ERR_INVALID, (t.window, t.n_groups, list(t.edge[:4]))
    assert (tone == -5.0).all() and (pitch == -5).all() and (bins == -5.0).all() and (spectrum == -5.0).all()
    assert call() == B.OK and not (tone == -5.0).any() and not (pitch == -5).any()
    # an entry outside the history that belongs to a mic off the list is never read
    o = off.copy()
    o[:, 7] = 5000
    assert call(off_=o, index_=np.array([0, 1, 2], np.int32), usable=3) == B.OK


def test_handle_entry_points_refuse_bad_arguments_before_the_handle(pkg):
    """Null handles, and for the runs everything that is judged before the handle is read -- the watch run's refusals, a bad
    request and a show that names no group: a fake handle of zero bytes keeps its bytes, the outputs theirs."""
    lib, B = pkg.binding.load(), pkg.binding
    INV = B.ERR_INVALID
    fake = (C.c_ubyte * 4096)()
    h = C.cast(fake, C.c_void_p)
    wire = (C.c_ubyte * (4 * 256 * 1032))()
    samples = (C.c_float * (64 * 1024))()
    xs = C.cast(samples, F32P)
    image, big, power = (C.c_uint8 * (4 * 64))(), (C.c_uint8 * (4 * 16 * 16))(), (C.c_float * (4 * 64))()
    sources, count = (C.c_ubyte * (4 * 4 * 40))(), (C.c_int32 * 4)()
    im, bg, pw = C.cast(image, U8P), C.cast(big, U8P), C.cast(power, F32P)
    so, co = C.cast(sources, C.c_void_p), C.cast(count, C.c_void_p)
    forms = [
        lambda hh, *rest: lib.awpu_hip_tones_blocks(hh, wire, 1032, 4, *rest),
        lambda hh, *rest: lib.awpu_hip_tones_samples(hh, xs, 1024, 4, *rest),
        lambda hh, *rest: lib.awpu_hip_tones_samples_device(hh, xs, 1024, 4, *rest, None),
    ]
    w = B.Watch(1, 2, 8, 8, 16, 16, 0, None)
    f = B.Find(8, 8, 2, 4, 0.0, 0.0, 180.0)
    t = B.tones_of(UNEVEN, 1)
    W, T, F = C.byref(w), C.byref(t), C.byref(f)
    for call in forms:
        assert call(None, W, T, 0, F, im, bg, pw, so, co) == INV                # no handle
        assert call(h, None, T, 0, F, im, bg, pw, so, co) == INV                # no w
        assert call(h, W, None, 0, F, im, bg, pw, so, co) == INV                # no t
        assert call(h, W, T, 0, None, None, None, None, None, None) == INV      # no output
        assert call(h, W, T, 0, None, im, bg, pw, so, co) == INV                # sources without a find request
        assert call(h, W, T, 0, F, im, bg, pw, None, None) == INV               # a find request without sources
        for show in (4, -2, 129):
            assert call(h, W, T, show, F, im, bg, pw, so, co) == INV, show
        assert call(h, W, C.byref(B.tones_of(UNEVEN, 2)), 0, F, im, bg, pw, so, co) == INV
        assert call(h, W, C.byref(B.tones_of([4, 4])), B.TONES_SHOW_PITCH, F, im, bg, pw, so, co) == INV
        assert call(h, W, T, 0, C.byref(B.Find(8, 8, 0, 4, 0.0, 0.0, 180.0)), im, bg, pw, so, co) == INV   # the find request's own checks
        for field, value in (("every", 0), ("every", 1025), ("first", -1), ("flip", 2), ("out_rows", 7), ("out_cols", 7)):  # the watch run's checks
            ww = B.Watch(1, 2, 8, 8, 16, 16, 0, None)
            setattr(ww, field, value)
            assert call(h, C.byref(ww), T, 0, F, im, bg, pw, so, co) == INV, field
    assert lib.awpu_hip_tones_blocks(h, None, 1032, 4, W, T, 0, F, im, bg, pw, so, co) == INV
    assert lib.awpu_hip_tones_blocks(h, wire, 1031, 4, W, T, 0, F, im, bg, pw, so, co) == INV
    assert lib.awpu_hip_tones_samples(h, xs, 1023, 4, W, T, 0, F, im, bg, pw, so, co) == INV
    assert lib.awpu_hip_tones_samples(h, xs, 1024, 0, W, T, 0, F, im, bg, pw, so, co) == INV
    # the three handle forms without a handle (what they refuse of a real one: tests/test_gpu_tones.py)
    pi = C.cast(count, I32P)
    assert lib.awpu_hip_tones(None, xs, 1, T, pw, pi) == INV
    assert lib.awpu_hip_tones_device(None, xs, 1, T, pw, pi, None) == INV
    assert lib.awpu_hip_tones_device_bins(None, xs, 1, T, pw, pi, pw, pw, None) == INV
    assert bytes(fake) == bytes(4096)
    for out in (image, big, sources):
        assert bytes(out) == bytes(len(out))
    assert bytes(power) == bytes(4 * len(power)) and bytes(count) == bytes(16)


# ------------------------------------------------------------------------------------------------ the tools

def load_tool(name):
    import importlib.util
    import sys

    spec = importlib.util.spec_from_file_location(name, REPO / "tools" / f"{name}.py")
    tool = importlib.util.module_from_spec(spec)
    sys.modules[name] = tool
    spec.loader.exec_module(tool)
    return tool


def test_the_tools_tone_flags_parse(tmp_path):
    video, sources = load_tool("pcap_video"), load_tool("pcap_sources")
    missing = str(tmp_path / "nothing.pcap")
    # accepted: the tools get as far as opening the capture
    for tool, flags in ((video, ["--tone", "2500:3500"]), (video, ["--tone", "8000:10000:hann"]), (video, ["--pitch", "1000:12000"]),
                        (video, ["--tone", "2500:3500", "--band", "2000:4000"]), (sources, ["--tone", "2500:3500"]),
                        (sources, ["--tone", "2500:3500:hann", "--every", "4"])):
        with pytest.raises(OSError):
            tool.main([missing, "--port", "1", *flags])
    # refused by the parser
    for tool, flags in ((video, ["--tone", "2500"]), (video, ["--tone", "2500:3500:hamming"]), (video, ["--tone", "3500:2500"]),
                        (video, ["--tone", "2500:3500", "--pitch", "1000:12000"]), (video, ["--tone", "2500:3500", "--bands", "1:2,3:4"]),
                        (video, ["--every", "4", "--exposure", "2", "--tone", "2500:3500"]), (video, ["--tone", "2500:3500", "--coherence"]),
                        (video, ["--pitch", "1000:12000", "--peel", "3"]), (sources, ["--tone", "2500:3500", "--coherence"]),
                        (sources, ["--every", "4", "--exposure", "2", "--tone", "2500:3500"]), (sources, ["--tone", "2500:3500", "--peel", "3"]),
                        (sources, ["--tone", "2500:3500", "--range", "1:2:4"]), (sources, ["--tone", "-5:100"]),
                        (video, ["--tone", "10:20"]), (video, ["--pitch", "10:20:hann"]), (sources, ["--tone", "10:20"]), (sources, ["--tone", "a:b"])):
        with pytest.raises(SystemExit):
            tool.main([missing, "--port", "1", *flags])
    for name in ("pcap_video", "pcap_sources"):
        text = (REPO / "tools" / f"{name}.py").read_text()
        assert '"--tone"' in text and "tones_blocks" in text
    rate = (REPO / "tools" / "tones_rate.py").read_text()
    assert "tones_device" in rate and "cohere_device" in rate and "exact_verify" in rate


# ------------------------------------------------------------------------------------------------ sanitizers, and the kernel's build

def test_host_code_runs_clean_under_sanitizers(tmp_path):
    """tests/host/tones_rule_check.cpp with tones_host.cpp: a program of its own under ASan and UBSan, every buffer exactly as
    long as the header says, entries at both ends of the history."""
    exe = tmp_path / "tones_rule_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{REPO / 'include'}", f"-I{CSRC}", str(REPO / "tests" / "host" / "tones_rule_check.cpp"), str(CSRC / "tones_host.cpp"),
                    "-o", str(exe)], check=True, capture_output=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "tones rule: ok" in out.stdout, out.stdout + out.stderr


def test_tones_kernel_compiles_without_spills(tmp_path, pkg):
    """The metadata of the code object only: no spills, no private segment."""
    out = tmp_path / "tones_kernels.s"
    subprocess.run([pkg._build.hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{REPO / 'include'}", f"-I{CSRC}",
                    "-S", "--cuda-device-only", "-o", str(out), str(CSRC / "tones_kernels.hip")], check=True, capture_output=True)
    text = out.read_text()
    meta = {}
    for block in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1))
                      for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")}
    assert len(meta) == 1 and "tones_sweep_kernel" in next(iter(meta)), sorted(meta)
    for name, m in meta.items():
        print(name, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_count"] <= 168  # three waves a SIMD at the least; the LDS chunk allows two workgroups a CU anyway
