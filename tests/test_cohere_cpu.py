"""Coherence heatmaps (include/awpu_hip_cohere.h) on a box without a GPU: the entry points are exported beside the other headers'
and built from the listed files; awpu_hip_cohere_host equals a numpy restatement of the rule bit for bit and its power the oracle's;
one mic is coherent with itself, silence has no coherence, and on the synthetic plane wave the coherence-weighted map keeps the
source and drops its side lobes; bad arguments are refused with nothing written; the host code runs clean under the address and
undefined-behaviour sanitizers as a program of its own; the kernel compiles for gfx950 without spills or scratch; the tools' new
flag parses."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import cohere_util as CU
import util

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "beamforming-lk_amd" / "csrc"
GOLDEN = REPO / "tests" / "golden"
NAMES = ["awpu_hip_cohere_host", "awpu_hip_cohere", "awpu_hip_cohere_device", "awpu_hip_cohere_device_sums", "awpu_hip_cohere_blocks",
         "awpu_hip_cohere_samples", "awpu_hip_cohere_samples_device"]
F32P, I32P, U8P = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)


def test_cohere_symbols_exported_and_listed(pkg):
    lib = pkg.binding.load()
    B = pkg.binding
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "awpu_hip_cohere.h").read_text(), flags=re.S)
    assert sorted(set(re.findall(r"\b(awpu_hip_\w+)\s*\(", text))) == sorted(NAMES)
    assert int(re.search(r"#define AWPU_COHERE_WEIGHTED (\d+)", text).group(1)) == 0 == B.COHERE_WEIGHTED
    assert int(re.search(r"#define AWPU_COHERE_FACTOR (\d+)", text).group(1)) == 1 == B.COHERE_FACTOR
    assert sorted(B.COHERE_SYMBOLS) == sorted(NAMES)
    for name in NAMES:
        assert hasattr(lib, name)
    for other in (B.EXPORTED_SYMBOLS, B.TRACK_SYMBOLS, B.BLOCK_SYMBOLS, B.LISTEN_SYMBOLS, B.WATCH_SYMBOLS, B.FIND_SYMBOLS, B.BAND_SYMBOLS, B.FOCUS_SYMBOLS,
                  B.SPECTRAL_SYMBOLS, B.EXPOSE_SYMBOLS):
        assert not set(B.COHERE_SYMBOLS) & set(other)
    assert lib.awpu_hip_abi_version() == 4
    assert "awpu_hip_cohere(" not in (REPO / "include" / "awpu_hip.h").read_text() and "awpu_cohere_t" not in (REPO / "include" / "awpu_hip.h").read_text()
    assert C.sizeof(B.Cohere) == 4
    assert B.KERNEL_NAMES[18] == "cohere" and "AWPU_KERNEL_COHERE = 18" in (REPO / "include" / "awpu_hip.h").read_text()
    H, S = pkg._build.HEADERS, pkg._build.SOURCES
    assert REPO / "include" / "awpu_hip_cohere.h" in H and CSRC / "cohere_kernels.h" in H and CSRC / "cohere_rule.h" in H
    assert CSRC / "cohere_kernels.hip" in S and CSRC / "cohere_host.cpp" in S and CSRC / "awpu_cohere.cpp" in S
    # the rule is host-only and lives in one header; the kernel file may not include it
    assert "cohere_rule.h" in (CSRC / "cohere_host.cpp").read_text() and "cohere_rule.h" in (REPO / "tests" / "host" / "cohere_rule_check.cpp").read_text()
    assert "cohere_rule.h" not in (CSRC / "cohere_kernels.hip").read_text() + (CSRC / "cohere_kernels.h").read_text()


def test_cohere_header_compiles_as_c(tmp_path):
    src = tmp_path / "one.c"
    src.write_text('#include "awpu_hip_cohere.h"\n'
                   "typedef char size_is_4[sizeof(awpu_cohere_t) == 4 ? 1 : -1];\n"
                   "int main(void) { awpu_cohere_t co; awpu_watch_t w; awpu_find_t f; awpu_source_t s[2]; float p[4]; int32_t n[4]; uint8_t i[4];\n"
                   "  co.show = AWPU_COHERE_FACTOR; w.first = 0; f.rows = 1;\n"
                   "  return awpu_hip_cohere_host(p, 1, 1, 257, n, p, 1, 1, n, 1, 0, p, p, p, 0, 0) + awpu_hip_cohere(0, p, 1, p, p, p)\n"
                   "    + awpu_hip_cohere_device(0, p, 1, p, p, p, 0) + awpu_hip_cohere_device_sums(0, p, 1, p, p, p, p, p, 0)\n"
                   "    + awpu_hip_cohere_blocks(0, p, 1032, 1, &w, &co, &f, i, i, p, s, n) + awpu_hip_cohere_samples(0, p, 256, 1, &w, &co, &f, i, i, p, s, n)\n"
                   "    + awpu_hip_cohere_samples_device(0, p, 256, 1, &w, &co, &f, i, i, p, s, n, 0) + (int) sizeof(size_is_4); }\n")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", f"-I{REPO / 'include'}", str(src)], check=True, capture_output=True)


def test_host_file_compiles_with_a_plain_host_compiler(tmp_path):
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{REPO / 'include'}", f"-I{CSRC}", "-c", str(CSRC / "cohere_host.cpp"),
                    "-o", str(tmp_path / "cohere_host.o")], check=True, capture_output=True)


# ------------------------------------------------------------------------------------------------ the rule

@pytest.fixture(scope="module")
def c1(pkg):
    """The c1 table and the frame synthetic.make_frames(xyz, 1) makes, with the host rule's answer on it (computed once)."""
    S = pkg.synthetic
    spec = S.WORKLOADS["c1"]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    frame = S.make_frames(xyz, 1)[0]
    power, coherence, weighted, sums, energy = pkg.cohere_host(frame, off, frac, want_sums=True)
    r, c = S.source_pixel(spec)
    return dict(spec=spec, xyz=xyz, off=off, frac=frac, frame=frame, power=power, coherence=coherence, weighted=weighted, sums=sums,
                energy=energy, source=r * spec.res + c)


def assert_equals_restatement(pkg, frame, off, frac, index=None, gain=None):
    got = pkg.cohere_host(frame, off, frac, index=index, gain=gain, want_sums=True)
    want = CU.rule(frame, off, frac, index, gain)
    for name, g, w in zip(("power", "coherence", "weighted", "sums", "energy"), got, want):
        assert g.dtype == np.float32 and CU.same_bits(g, w), name
    assert not got[4][:, 0].any() and not got[4][:, 255].any()  # e[0] and e[255] are written as 0
    return got


def test_host_rule_equals_the_numpy_restatement_on_c1(pkg, c1):
    want = CU.rule(c1["frame"], c1["off"], c1["frac"])
    for name, w in zip(("power", "coherence", "weighted", "sums", "energy"), want):
        assert CU.same_bits(c1[name], w), name


def test_host_rule_on_the_ragged_51_mic_list(pkg, c1):
    index = np.load(GOLDEN / "sweep_c1_ragged.npz")["index"]
    assert len(index) == 51
    pixels = np.arange(0, 1024, 7)
    assert_equals_restatement(pkg, c1["frame"], c1["off"][pixels], c1["frac"][pixels], index=index)


def test_host_rule_with_gains(pkg, c1):
    index = np.load(GOLDEN / "sweep_c1_ragged.npz")["index"]
    gain = (0.5 + np.random.default_rng(3).random(len(index))).astype(np.float32)
    pixels = np.arange(3, 1024, 11)
    with_gain = assert_equals_restatement(pkg, c1["frame"], c1["off"][pixels], c1["frac"][pixels], index=index, gain=gain)
    without = pkg.cohere_host(c1["frame"], c1["off"][pixels], c1["frac"][pixels], index=index)
    assert not CU.same_bits(with_gain[0], without[0])


def test_host_rule_on_a_three_pixel_table_and_a_batch(pkg, c1):
    pixels = np.array([0, 517, 1023])
    frames = pkg.synthetic.make_frames(c1["xyz"], 3, seed=77)
    got = pkg.cohere_host(frames, c1["off"][pixels], c1["frac"][pixels], want_sums=True)
    for b in range(3):
        want = CU.rule(frames[b], c1["off"][pixels], c1["frac"][pixels])
        for g, w in zip(got, want):
            assert CU.same_bits(g[b], w)


def test_power_equals_the_oracle(pkg, oracle, c1):
    power, out = oracle.das_f32(c1["frame"], c1["off"], c1["frac"], want_out=True)
    assert CU.same_bits(c1["power"], power) and CU.same_bits(c1["sums"], out)
    index = np.load(GOLDEN / "sweep_c1_ragged.npz")["index"]
    got = pkg.cohere_host(c1["frame"], c1["off"], c1["frac"], index=index)
    assert CU.same_bits(got[0], oracle.das_f32(c1["frame"], c1["off"], c1["frac"], index=index))


def test_one_mic_is_coherent_with_itself(pkg, c1):
    for mic in (0, 37):
        power, coherence, weighted, sums, energy = pkg.cohere_host(c1["frame"], c1["off"], c1["frac"], index=[mic], want_sums=True)
        den = energy.astype(np.float64).sum(axis=1)
        assert (den > 0).all()
        assert CU.same_bits(coherence, np.ones(1024, np.float32))
        assert CU.same_bits(weighted, power)
    # ... and where den is 0 the coherence is 0: a silent mic
    frame = c1["frame"].copy()
    frame[5] = 0.0
    power, coherence, weighted = pkg.cohere_host(frame, c1["off"], c1["frac"], index=[5])
    assert not power.any() and not coherence.any() and not weighted.any()


def test_silence_has_no_coherence(pkg, c1):
    for maps in (pkg.cohere_host(np.zeros((64, 1024), np.float32), c1["off"], c1["frac"]),
                 pkg.cohere_host(np.full((64, 1024), -0.0, np.float32), c1["off"], c1["frac"])):
        for m in maps:
            assert CU.same_bits(m, np.zeros(1024, np.float32))


def test_coherence_lies_in_the_unit_interval_on_random_frames(pkg, c1):
    pixels = np.arange(0, 1024, 5)
    frames = np.concatenate([util.hash_frames(64, 1024, seed=91, batch=2), util.hash_frames(64, 1024, seed=92, batch=1) + np.float32(0.25)])
    power, coherence, weighted = pkg.cohere_host(frames, c1["off"][pixels], c1["frac"][pixels])
    assert np.isfinite(coherence).all() and (coherence >= 0).all() and (coherence <= 1).all()
    assert (weighted <= power).all() and (power > 0).all()


def test_non_finite_input_takes_the_rule_as_written(pkg, c1):
    """A NaN den gives 0; a NaN num over a positive den gives NaN: the restatement and the C agree on both."""
    pixels = np.arange(0, 1024, 9)
    at = int(np.median(c1["off"][pixels, 0])) + 256  # the last sample that half of these pixels read of mic 0
    for bad in (np.nan, np.inf):
        frame = c1["frame"].copy()
        frame[0, at] = bad
        got = assert_equals_restatement(pkg, frame, c1["off"][pixels], c1["frac"][pixels])
        reached = ~np.isfinite(got[3]).all(axis=1)
        assert reached.any() and not reached.all()
        assert not got[1][reached].any()  # den is NaN there: coherence 0


# ------------------------------------------------------------------------------------------------ the physics, on c1

def test_the_source_is_coherent_and_the_maximum(c1):
    """Predicted S / (S + N) behind the stencil: 4.5e-6 / (4.5e-6 + 1.25e-7) = 0.97; measured 0.953."""
    c = c1["coherence"]
    print("coherence at the source", c[c1["source"]])
    assert c[c1["source"]] >= 0.9
    assert int(c.argmax()) == c1["source"]


def test_the_weighted_map_has_one_peak_where_the_power_map_has_many(pkg, c1):
    """radius 2, min_ratio 0.01: measured 12 peaks on power, 1 on weighted."""
    res = c1["spec"].res
    on_power = pkg.find_peaks(c1["power"], res, res, radius=2, max_sources=32, min_ratio=0.01)
    on_weighted = pkg.find_peaks(c1["weighted"], res, res, radius=2, max_sources=32, min_ratio=0.01)
    print("peaks", int(on_power.count[0]), int(on_weighted.count[0]))
    assert int(on_power.count[0]) > 1
    assert int(on_weighted.count[0]) == 1 and int(on_weighted.sources[0, 0]["pixel"]) == c1["source"]


def test_the_weighted_map_is_20_db_cleaner(c1):
    """Median over maximum: measured -32.3 dB on power and -64.6 dB on weighted, 32 dB apart."""
    p, w = CU.median_over_max_db(c1["power"]), CU.median_over_max_db(c1["weighted"])
    print("median over maximum, dB", p, w)
    assert w <= p - 20.0


def test_noise_alone_has_coherence_one_over_usable(pkg, c1):
    """Measured 0.0155 against 1 / 64 = 0.0156."""
    noise = (1e-3 * (np.random.RandomState(5).rand(64, 1024) * 2 - 1)).astype(np.float32)
    coherence = pkg.cohere_host(noise, c1["off"], c1["frac"])[1]
    print("median coherence of noise", np.median(coherence))
    assert 0.5 / 64 <= np.median(coherence) <= 2.0 / 64


# ------------------------------------------------------------------------------------------------ refusals

def test_host_rule_refusals_write_nothing(pkg, c1):
    lib, B = pkg.binding.load(), pkg.binding
    off, frac = c1["off"][:4].copy(), c1["frac"][:4].copy()
    frame = np.ascontiguousarray(c1["frame"])
    index = np.arange(64, dtype=np.int32)
    outs = [np.full(4, -5.0, np.float32) for _ in range(3)] + [np.full((4, 256), -5.0, np.float32) for _ in range(2)]
    fp = lambda a: a.ctypes.data_as(F32P)
    ip = lambda a: a.ctypes.data_as(I32P)

    def call(frame_p=fp(frame), batch=1, n_streams=64, hist=1024, off_=off, frac_=frac, stride=64, n_pixels=4, index_=index, usable=64):
        return lib.awpu_hip_cohere_host(frame_p, batch, n_streams, hist, None if off_ is None else ip(off_), None if frac_ is None else fp(frac_),
                                        stride, n_pixels, None if index_ is None else ip(index_), usable, None, *[fp(o) for o in outs])

    for bad_off in (1024 - 256, 1024, -1):  # entries reading outside the history
        o = off.copy()
        o[3, 63] = bad_off
        assert call(off_=o) == B.ERR_RANGE, bad_off
    o = off.copy()
    o[3, 63] = 1024 - 257
    assert call(off_=o) == B.OK  # the last entry that fits
    for o_ in outs:
        o_.fill(-5.0)
    for bad_frac in (-1e-6, 1.0 + 1e-6, np.nan, np.inf):
        f = frac.copy()
        f[0, 0] = bad_frac
        assert call(frac_=f) == B.ERR_INVALID, bad_frac
    assert call(frame_p=None) == B.ERR_INVALID and call(off_=None) == B.ERR_INVALID and call(frac_=None) == B.ERR_INVALID
    assert call(index_=None) == B.ERR_INVALID
    for kw in (dict(batch=0), dict(n_streams=0), dict(hist=256), dict(stride=0), dict(n_pixels=0), dict(usable=0), dict(n_streams=63),
               dict(index_=np.full(64, 64, np.int32)), dict(index_=np.full(64, -1, np.int32))):
        assert call(**kw) == B.ERR_INVALID, kw
    assert all((o_ == -5.0).all() for o_ in outs)
    # an entry outside the history that belongs to a mic off the list is never read
    o = off.copy()
    o[:, 7] = 5000
    assert call(off_=o, index_=np.array([0, 1, 2], np.int32), usable=3) == B.OK


def test_handle_entry_points_refuse_bad_arguments_before_the_handle(pkg):
    """Null handles, and for the runs everything that is judged before the handle is read -- the watch run's refusals and a show
    outside {0, 1}: a fake handle of zero bytes keeps its bytes, the outputs theirs."""
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
        lambda hh, *rest: lib.awpu_hip_cohere_blocks(hh, wire, 1032, 4, *rest),
        lambda hh, *rest: lib.awpu_hip_cohere_samples(hh, xs, 1024, 4, *rest),
        lambda hh, *rest: lib.awpu_hip_cohere_samples_device(hh, xs, 1024, 4, *rest, None),
    ]
    w = B.Watch(1, 2, 8, 8, 16, 16, 0, None)
    f = B.Find(8, 8, 2, 4, 0.0, 0.0, 180.0)
    W, K, F = C.byref(w), C.byref(B.Cohere(B.COHERE_WEIGHTED)), C.byref(f)
    for call in forms:
        assert call(None, W, K, F, im, bg, pw, so, co) == INV                # no handle
        assert call(h, None, K, F, im, bg, pw, so, co) == INV                # no w
        assert call(h, W, None, F, im, bg, pw, so, co) == INV                # no co
        assert call(h, W, K, None, None, None, None, None, None) == INV      # no output
        assert call(h, W, K, None, im, bg, pw, so, co) == INV                # sources without a find request
        assert call(h, W, K, F, im, bg, pw, None, None) == INV               # a find request without sources
        assert call(h, W, K, F, im, bg, pw, so, None) == INV                 # sources without count
        assert call(h, W, K, F, im, bg, pw, None, co) == INV
        for show in (2, -1, 7):
            assert call(h, W, C.byref(B.Cohere(show)), F, im, bg, pw, so, co) == INV, show
        assert call(h, W, K, C.byref(B.Find(8, 8, 0, 4, 0.0, 0.0, 180.0)), im, bg, pw, so, co) == INV   # the find request's own checks
        assert call(h, W, K, C.byref(B.Find(4, 16, 2, 4, 0.0, 0.0, 180.0)), im, bg, pw, so, co) == INV  # another grid
        for field, value in (("every", 0), ("every", 1025), ("first", -1), ("flip", 2), ("out_rows", 7), ("out_cols", 7)):  # the watch run's checks
            ww = B.Watch(1, 2, 8, 8, 16, 16, 0, None)
            setattr(ww, field, value)
            assert call(h, C.byref(ww), K, F, im, bg, pw, so, co) == INV, field
    assert lib.awpu_hip_cohere_blocks(h, None, 1032, 4, W, K, F, im, bg, pw, so, co) == INV
    assert lib.awpu_hip_cohere_blocks(h, wire, 1031, 4, W, K, F, im, bg, pw, so, co) == INV
    assert lib.awpu_hip_cohere_samples(h, xs, 1023, 4, W, K, F, im, bg, pw, so, co) == INV
    assert lib.awpu_hip_cohere_samples(h, xs, 1024, 0, W, K, F, im, bg, pw, so, co) == INV
    # the three handle forms without a handle (what they refuse of a real one: tests/test_gpu_cohere.py)
    assert lib.awpu_hip_cohere(None, xs, 1, pw, pw, pw) == INV
    assert lib.awpu_hip_cohere_device(None, xs, 1, pw, pw, pw, None) == INV
    assert lib.awpu_hip_cohere_device_sums(None, xs, 1, pw, pw, pw, pw, pw, None) == INV
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


def test_the_tools_coherence_flag_parses(tmp_path):
    video, sources = load_tool("pcap_video"), load_tool("pcap_sources")
    missing = str(tmp_path / "nothing.pcap")
    # accepted: the tools get as far as opening the capture
    for tool, flags in ((video, ["--coherence"]), (video, ["--coherence", "weighted"]), (video, ["--coherence", "factor", "--band", "6000:9000"]),
                        (sources, ["--coherence"]), (sources, ["--coherence", "factor", "--every", "4"])):
        with pytest.raises(OSError):
            tool.main([missing, "--port", "1", *flags])
    # refused by the parser
    for tool, flags in ((video, ["--coherence", "power"]), (video, ["--coherence", "--bands", "1:2,3:4"]),
                        (video, ["--every", "4", "--exposure", "2", "--coherence"]), (sources, ["--coherence", "both"]),
                        (sources, ["--every", "4", "--exposure", "2", "--coherence"]), (sources, ["--coherence", "--range", "1:2:4"])):
        with pytest.raises(SystemExit):
            tool.main([missing, "--port", "1", *flags])
    for name in ("pcap_video", "pcap_sources"):
        text = (REPO / "tools" / f"{name}.py").read_text()
        assert '"--coherence"' in text and "cohere_blocks" in text
    rate = (REPO / "tools" / "cohere_rate.py").read_text()
    assert "cohere_device" in rate and "exact_verify" in rate


# ------------------------------------------------------------------------------------------------ sanitizers, and the kernel's build

def test_host_code_runs_clean_under_sanitizers(tmp_path):
    """tests/host/cohere_rule_check.cpp with cohere_host.cpp: a program of its own under ASan and UBSan, every buffer exactly as
    long as the header says, entries at both ends of the history."""
    exe = tmp_path / "cohere_rule_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{REPO / 'include'}", f"-I{CSRC}", str(REPO / "tests" / "host" / "cohere_rule_check.cpp"), str(CSRC / "cohere_host.cpp"),
                    "-o", str(exe)], check=True, capture_output=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "cohere rule: ok" in out.stdout, out.stdout + out.stderr


def test_cohere_kernel_compiles_without_spills(tmp_path, pkg):
    """The metadata of the code object only: no spills, no private segment."""
    out = tmp_path / "cohere_kernels.s"
    subprocess.run([pkg._build.hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{REPO / 'include'}", f"-I{CSRC}",
                    "-S", "--cuda-device-only", "-o", str(out), str(CSRC / "cohere_kernels.hip")], check=True, capture_output=True)
    text = out.read_text()
    meta = {}
    for block in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1))
                      for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")}
    assert len(meta) == 1 and "cohere_sweep_kernel" in next(iter(meta)), sorted(meta)
    for name, m in meta.items():
        print(name, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_count"] <= 128  # four waves a SIMD at the least
