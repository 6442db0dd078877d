"""Exposure (include/awpu_hip_expose.h) on a box without a GPU: the entry points are exported beside the other headers' and built
from the listed files; awpu_hip_expose_count equals a brute-force enumeration and chains; awpu_hip_expose_rows equals a numpy
restatement bit for bit, at its value edges too, and is invariant under every split of its input; bad arguments are refused with
nothing written; the host code runs clean under the address and undefined-behaviour sanitizers as a program of its own; the
kernels compile for gfx950 without spills or scratch; the tools' new flags parse."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import expose_util as X
import value_edges as V

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "beamforming-lk_amd" / "csrc"
NAMES = ["awpu_hip_expose_count", "awpu_hip_expose_rows", "awpu_hip_expose_rows_device", "awpu_hip_expose_blocks", "awpu_hip_expose_samples",
         "awpu_hip_expose_samples_device"]
F32P, U8P = C.POINTER(C.c_float), C.POINTER(C.c_uint8)


def test_expose_symbols_exported_and_listed(pkg):
    lib = pkg.binding.load()
    B = pkg.binding
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "awpu_hip_expose.h").read_text(), flags=re.S)
    assert sorted(set(re.findall(r"\b(awpu_hip_\w+)\s*\(", text))) == sorted(NAMES)
    assert '#include "awpu_hip_find.h"' in text
    assert int(re.search(r"#define AWPU_EXPOSE_MEAN (\d+)", text).group(1)) == 0 == B.EXPOSE_MEAN
    assert int(re.search(r"#define AWPU_EXPOSE_PEAK (\d+)", text).group(1)) == 1 == B.EXPOSE_PEAK
    assert sorted(B.EXPOSE_SYMBOLS) == sorted(NAMES)
    for name in NAMES:
        assert hasattr(lib, name)
    for other in (B.EXPORTED_SYMBOLS, B.TRACK_SYMBOLS, B.BLOCK_SYMBOLS, B.LISTEN_SYMBOLS, B.WATCH_SYMBOLS, B.FIND_SYMBOLS, B.BAND_SYMBOLS, B.FOCUS_SYMBOLS,
                  B.SPECTRAL_SYMBOLS):
        assert not set(B.EXPOSE_SYMBOLS) & set(other)
    assert lib.awpu_hip_abi_version() == 4
    assert "awpu_hip_expose" not in (REPO / "include" / "awpu_hip.h").read_text() and "awpu_expose" not in (REPO / "include" / "awpu_hip.h").read_text()
    assert C.sizeof(B.Expose) == 8
    H, S = pkg._build.HEADERS, pkg._build.SOURCES
    assert REPO / "include" / "awpu_hip_expose.h" in H and CSRC / "expose_kernels.h" in H and CSRC / "expose_rule.h" in H
    assert CSRC / "expose_kernels.hip" in S and CSRC / "expose_host.cpp" in S
    # the rule lives in one header that the host definition, the kernel and the run all include
    for user in ("expose_host.cpp", "expose_kernels.h", "awpu_expose.cpp"):
        assert "expose_rule.h" in (CSRC / user).read_text() or "expose_kernels.h" in (CSRC / user).read_text(), user


def test_expose_header_compiles_as_c(tmp_path):
    src = tmp_path / "one.c"
    src.write_text('#include "awpu_hip_expose.h"\n'
                   "typedef char size_is_8[sizeof(awpu_expose_t) == 8 ? 1 : -1];\n"
                   "int main(void) { awpu_expose_t e; awpu_watch_t w; awpu_find_t f; awpu_source_t s[2]; float p[4], c[2]; uint8_t i[4]; int32_t n[5];\n"
                   "  e.length = 1; e.mode = AWPU_EXPOSE_PEAK; w.first = 0; f.rows = 1;\n"
                   "  return awpu_hip_expose_count(1, 0, 1, 1, n, n + 1, n + 2, n + 3, n + 4) + awpu_hip_expose_rows(p, 2, 2, 0, 1, &e, c, p)\n"
                   "    + awpu_hip_expose_rows_device(0, p, 2, 2, 0, 1, &e, c, p, 0) + awpu_hip_expose_blocks(0, p, 1032, 1, &w, &e, &f, c, i, i, p, s, n)\n"
                   "    + awpu_hip_expose_samples(0, p, 256, 1, &w, &e, &f, c, i, i, p, s, n)\n"
                   "    + awpu_hip_expose_samples_device(0, p, 256, 1, &w, &e, &f, c, i, i, p, s, n, 0) + (int) sizeof(size_is_8); }\n")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", f"-I{REPO / 'include'}", str(src)], check=True, capture_output=True)


def test_host_file_compiles_with_a_plain_host_compiler(tmp_path):
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{REPO / 'include'}", f"-I{CSRC}", "-c", str(CSRC / "expose_host.cpp"),
                    "-o", str(tmp_path / "expose_host.o")], check=True, capture_output=True)


# ------------------------------------------------------------------------------------------------ the counts

def brute_count(n_blocks, first, every, L):
    """(the blocks of the call whose frames close in it, next_first, carry_in, carry_out, n_swept) straight from the rule's words."""
    shown = list(range(first, n_blocks, every))
    nxt = (shown[-1] + every if shown else first) - n_blocks
    window = lambda b: range(b - L + 1, b + 1)
    carry_in = sum(1 for k in window(first) if k < 0)
    carry_out = sum(1 for k in window(n_blocks + nxt) if k < n_blocks)
    swept = sum(1 for j in range(len(shown) + 1) for k in window(first + j * every) if 0 <= k < n_blocks)
    return shown, nxt, carry_in, carry_out, swept


def test_expose_count_equals_a_brute_force_enumeration(pkg):
    lib = pkg.binding.load()
    out = [C.c_int32(0) for _ in range(5)]
    refs = [C.byref(v) for v in out]
    for every in range(1, 10):
        for L in range(1, every + 1):
            for first in range(0, 46):
                for n_blocks in range(1, 41):
                    assert lib.awpu_hip_expose_count(n_blocks, first, every, L, *refs) == 0
                    shown, nxt, c_in, c_out, swept = brute_count(n_blocks, first, every, L)
                    assert [v.value for v in out] == [len(shown), nxt, c_in, c_out, swept], (n_blocks, first, every, L)
    assert pkg.expose_count(23, 2, 3, 3) == (7, 0, 0, 2, 23)


def test_expose_count_chained_calls_give_the_single_calls_frames(pkg):
    total = 40
    for every in range(1, 10):
        for L in range(1, every + 1):
            for first in (0, L - 1, every + 2):
                whole = pkg.expose_count(total, first, every, L)
                want = list(range(first, total, every))
                for cuts in ([1], [5, 6, 15, 23], [every], [L, 2 * L + 1], list(range(1, total))):
                    got, at, f, swept, c_out = [], 0, first, 0, None
                    for end in [c for c in cuts if c < total] + [total]:
                        if end == at:
                            continue
                        n_frames, nxt, c_in, c_out_now, n_swept = pkg.expose_count(end - at, f, every, L)
                        assert c_out is None or c_in == c_out  # what one call leaves open, the next finds open
                        got += [at + f + j * every for j in range(n_frames)]
                        at, f, swept, c_out = end, nxt, swept + n_swept, c_out_now
                    assert got == want and swept == whole[4] and f == whole[1] and c_out == whole[3], (every, L, first, cuts)


# ------------------------------------------------------------------------------------------------ the rule

CASES = [(0, 1, 1), (2, 3, 3), (1, 3, 2), (6, 7, 4), (3, 4, 4), (0, 5, 1), (0, 3, 3), (40, 2, 2), (22, 23, 23)]


def call_rows(pkg, power, first, every, L, mode, carry):
    """awpu_hip_expose_rows with a carry that is always there -> (frames, next_first); carry is written in place."""
    return pkg.expose_rows(power, first, every, L, mode, carry)


@pytest.mark.parametrize("mode", [X.MEAN, X.PEAK])
@pytest.mark.parametrize("edges", [False, True])
def test_expose_rows_equals_the_numpy_restatement(pkg, mode, edges):
    assert not V.host_flushes()
    rng = np.random.default_rng(11)
    for n_blocks, n_pixels in ((23, 37), (1, 1), (7, 4)):
        power = X.edge_rows(n_blocks, n_pixels) if edges else rng.random((n_blocks, n_pixels), dtype=np.float32) * np.float32(100.0)
        for first, every, L in CASES:
            carry0 = rng.random(n_pixels, dtype=np.float32)
            want, acc = X.expose_np(power, first, every, L, mode, carry0)
            n_frames, nxt, c_in, c_out, _ = pkg.expose_count(n_blocks, first, every, L)
            carry = carry0.copy()
            got, next_first = call_rows(pkg, power, first, every, L, mode, carry)
            assert next_first == nxt and got.shape == (n_frames, n_pixels) == want.shape
            assert X.same_bits(got, want), (n_blocks, n_pixels, first, every, L)
            assert X.same_bits(carry, acc if c_out > 0 else carry0)  # the open window, or not written
            if c_in == 0 and c_out == 0:  # then it may be left out
                assert X.same_bits(pkg.expose_rows(power, first, every, L, mode, None)[0], want)


@pytest.mark.parametrize("mode", [X.MEAN, X.PEAK])
def test_expose_rows_every_split_of_23_rows(pkg, mode):
    power = X.edge_rows(23, 9, seed=3)
    power[:, 2:6] = np.random.default_rng(2).random((23, 4), dtype=np.float32)
    for first, every, L in CASES:
        carry0 = np.full(9, 0.25, np.float32)
        whole_carry = carry0.copy()
        whole, nxt = call_rows(pkg, power, first, every, L, mode, whole_carry)
        for cut in range(1, 23):
            carry = carry0.copy()
            a, f = call_rows(pkg, power[:cut], first, every, L, mode, carry)
            b, f = call_rows(pkg, power[cut:], f, every, L, mode, carry)
            assert f == nxt and X.same_bits(np.concatenate([a, b]), whole), (first, every, L, cut)
            if pkg.expose_count(23, first, every, L)[3] > 0:
                assert X.same_bits(carry, whole_carry)


def test_length_1_returns_the_shown_rows_bits(pkg):
    power = X.edge_rows(23, 16)
    for first, every in ((0, 1), (0, 5), (3, 4), (30, 2)):
        for mode in (X.MEAN, X.PEAK):
            got, _ = pkg.expose_rows(power, first, every, 1, mode, None)
            assert X.same_bits(got, power[first::every])


def test_expose_rows_refusals_write_nothing(pkg):
    lib, B = pkg.binding.load(), pkg.binding
    INV = B.ERR_INVALID
    power = np.arange(12, dtype=np.float32).reshape(6, 2)
    carry, frames = np.full(2, 7.0, np.float32), np.full((6, 2), 9.0, np.float32)
    p, c, f = (a.ctypes.data_as(F32P) for a in (power, carry, frames))
    good = B.Expose(2, B.EXPOSE_MEAN)
    call = lambda *a: lib.awpu_hip_expose_rows(*a)
    assert call(p, 6, 2, 1, 2, C.byref(good), c, f) == 0 and frames[0, 0] == 1.0  # the good call, for contrast
    frames[:] = 9.0
    bad = [
        (None, 6, 2, 1, 2, C.byref(good), c, f),                          # no rows
        (p, 0, 2, 1, 2, C.byref(good), c, f), (p, -1, 2, 1, 2, C.byref(good), c, f),
        (p, 6, 0, 1, 2, C.byref(good), c, f),                             # no pixels
        (p, 6, 2, -1, 2, C.byref(good), c, f),                            # first below 0
        (p, 6, 2, 1, 0, C.byref(good), c, f),                             # every below 1
        (p, 6, 2, 1, 2, None, c, f),                                      # no request
        (p, 6, 2, 1, 2, C.byref(B.Expose(0, 0)), c, f),                   # length outside [1, every]
        (p, 6, 2, 1, 2, C.byref(B.Expose(3, 0)), c, f),
        (p, 6, 2, 1, 2, C.byref(B.Expose(-1, 0)), c, f),
        (p, 6, 2, 1, 2, C.byref(B.Expose(2, 2)), c, f), (p, 6, 2, 1, 2, C.byref(B.Expose(2, -1)), c, f),  # an unknown mode
        (p, 6, 2, 0, 2, C.byref(good), None, f),                          # carry_in = 1 and no carry
        (p, 5, 2, 1, 2, C.byref(good), None, f),                          # carry_out = 1 and no carry
        (p, 6, 2, 1, 2, C.byref(good), c, None),                          # frames and nowhere to put them
    ]
    for args in bad:
        assert call(*args) == INV, args[1:5]
    assert np.all(carry == 7.0) and np.all(frames == 9.0)
    out = [C.c_int32(-5) for _ in range(5)]
    refs = [C.byref(v) for v in out]
    for args in ((0, 0, 1, 1), (1, -1, 1, 1), (1, 0, 0, 1), (1, 0, 1, 0), (1, 0, 1, 2), (1, 0, 3, 4)):
        assert lib.awpu_hip_expose_count(*args, *refs) == INV, args
    for k in range(5):
        assert lib.awpu_hip_expose_count(4, 0, 2, 1, *[None if j == k else r for j, r in enumerate(refs)]) == INV
    assert [v.value for v in out] == [-5] * 5
    with pytest.raises(B.AwpuError):
        pkg.expose_rows(power, 1, 2, 3)


def test_handle_entry_points_refuse_bad_arguments_before_the_handle(pkg):
    """Null handles, and for the runs everything that is judged before the handle is read: a fake handle of zero bytes keeps its
    bytes, the outputs and the carry theirs."""
    lib, B = pkg.binding.load(), pkg.binding
    INV = B.ERR_INVALID
    fake = (C.c_ubyte * 4096)()
    h = C.cast(fake, C.c_void_p)
    wire = (C.c_ubyte * (4 * 256 * 1032))()
    samples = (C.c_float * (64 * 1024))()
    xs = C.cast(samples, F32P)
    image, big, power, carry = (C.c_uint8 * (4 * 64))(), (C.c_uint8 * (4 * 16 * 16))(), (C.c_float * (4 * 64))(), (C.c_float * 64)()
    sources, count = (C.c_ubyte * (4 * 4 * 40))(), (C.c_int32 * 4)()
    im, bg, pw, cy = C.cast(image, U8P), C.cast(big, U8P), C.cast(power, F32P), C.cast(carry, F32P)
    so, co = C.cast(sources, C.c_void_p), C.cast(count, C.c_void_p)
    forms = [
        lambda hh, *rest: lib.awpu_hip_expose_blocks(hh, wire, 1032, 4, *rest),
        lambda hh, *rest: lib.awpu_hip_expose_samples(hh, xs, 1024, 4, *rest),
        lambda hh, *rest: lib.awpu_hip_expose_samples_device(hh, xs, 1024, 4, *rest, None),
    ]
    w = B.Watch(1, 2, 8, 8, 16, 16, 0, None)
    e = B.Expose(2, B.EXPOSE_MEAN)
    f = B.Find(8, 8, 2, 4, 0.0, 0.0, 180.0)
    W, E, F = C.byref(w), C.byref(e), C.byref(f)
    for call in forms:
        assert call(None, W, E, F, cy, im, bg, pw, so, co) == INV                # no handle
        assert call(h, None, E, F, cy, im, bg, pw, so, co) == INV                # no w
        assert call(h, W, None, F, cy, im, bg, pw, so, co) == INV                # no e
        assert call(h, W, E, None, cy, None, None, None, None, None) == INV      # no output
        assert call(h, W, E, None, cy, im, bg, pw, so, co) == INV                # sources without a find request
        assert call(h, W, E, F, cy, im, bg, pw, None, None) == INV               # a find request without sources
        assert call(h, W, E, F, cy, im, bg, pw, so, None) == INV                 # sources without count
        assert call(h, W, E, F, cy, im, bg, pw, None, co) == INV
        for length, mode in ((0, 0), (3, 0), (-2, 0), (2, 2), (2, -1)):
            assert call(h, W, C.byref(B.Expose(length, mode)), F, cy, im, bg, pw, so, co) == INV, (length, mode)
        assert call(h, W, E, C.byref(B.Find(8, 8, 0, 4, 0.0, 0.0, 180.0)), cy, im, bg, pw, so, co) == INV   # the find request's own checks
        assert call(h, W, E, C.byref(B.Find(4, 16, 2, 4, 0.0, 0.0, 180.0)), cy, im, bg, pw, so, co) == INV  # another grid
        assert call(h, C.byref(B.Watch(2, 3, 8, 8, 16, 16, 0, None)), C.byref(B.Expose(3, 0)), F, None, im, bg, pw, so, co) == INV  # carry_out = 1 and no carry
        assert call(h, C.byref(B.Watch(0, 2, 8, 8, 16, 16, 0, None)), E, F, None, im, bg, pw, so, co) == INV  # carry_in = 1 and no carry
        for field, value in (("every", 0), ("every", 1025), ("first", -1), ("flip", 2), ("out_rows", 7), ("out_cols", 7)):  # the watch run's checks
            ww = B.Watch(1, 2, 8, 8, 16, 16, 0, None)
            setattr(ww, field, value)
            assert call(h, C.byref(ww), E, F, cy, im, bg, pw, so, co) == INV, field
    assert lib.awpu_hip_expose_rows_device(None, xs, 4, 4, 1, 2, E, cy, pw, None) == INV
    for args in ((h, None, 4, 4, 1, 2, E, cy, pw), (h, xs, 0, 4, 1, 2, E, cy, pw), (h, xs, 4, 0, 1, 2, E, cy, pw), (h, xs, 4, 4, -1, 2, E, cy, pw),
                 (h, xs, 4, 4, 1, 0, E, cy, pw), (h, xs, 4, 4, 1, 2, None, cy, pw), (h, xs, 4, 4, 1, 1, E, cy, pw),
                 (h, xs, 4, 4, 0, 2, E, None, pw), (h, xs, 3, 4, 1, 2, E, None, pw), (h, xs, 4, 4, 1, 2, E, cy, None)):
        assert lib.awpu_hip_expose_rows_device(*args, None) == INV, args[2:6]
    assert bytes(fake) == bytes(4096)
    for out in (image, big, sources):
        assert bytes(out) == bytes(len(out))
    assert bytes(power) == bytes(4 * len(power)) and bytes(carry) == bytes(4 * len(carry)) and bytes(count) == bytes(16)


# ------------------------------------------------------------------------------------------------ the tools

def load_tool(name):
    import importlib.util
    import sys

    spec = importlib.util.spec_from_file_location(name, REPO / "tools" / f"{name}.py")
    tool = importlib.util.module_from_spec(spec)
    sys.modules[name] = tool
    spec.loader.exec_module(tool)
    return tool


def test_the_tools_exposure_flags_parse(tmp_path):
    video, sources = load_tool("pcap_video"), load_tool("pcap_sources")
    missing = str(tmp_path / "nothing.pcap")
    # accepted: the tools get as far as opening the capture
    for tool, flags in ((video, ["--every", "6", "--exposure", "6"]), (video, ["--every", "6", "--exposure", "2", "--peak-hold"]),
                        (video, ["--exposure", "1"]), (sources, ["--every", "4", "--exposure", "4"]), (sources, ["--exposure", "1"])):
        with pytest.raises(OSError):
            tool.main([missing, "--port", "1", *flags])
    # refused by the parser
    for tool, flags in ((video, ["--exposure", "4"]), (video, ["--exposure", "0"]), (video, ["--peak-hold"]),
                        (video, ["--exposure", "2", "--bands", "1:2,3:4"]), (sources, ["--exposure", "2"]), (sources, ["--exposure", "0"]),
                        (sources, ["--every", "4", "--exposure", "2", "--range", "1:2:4"])):
        with pytest.raises(SystemExit):
            tool.main([missing, "--port", "1", *flags])
    for name, call in (("pcap_video", "expose_blocks"), ("pcap_sources", "expose_blocks")):
        text = (REPO / "tools" / f"{name}.py").read_text()
        assert '"--exposure"' in text and call in text and "carry=carry" in text


# ------------------------------------------------------------------------------------------------ sanitizers, and the kernels' build

def test_host_code_runs_clean_under_sanitizers(tmp_path):
    """tests/host/expose_rule_check.cpp with expose_host.cpp: a program of its own under ASan and UBSan, smallest (1 pixel, length 1)
    and largest (every = length = 1024) sizes."""
    exe = tmp_path / "expose_rule_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{REPO / 'include'}", f"-I{CSRC}", str(REPO / "tests" / "host" / "expose_rule_check.cpp"), str(CSRC / "expose_host.cpp"),
                    "-o", str(exe)], check=True, capture_output=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "expose rule: ok" in out.stdout, out.stdout + out.stderr


def test_expose_kernels_compile_without_spills(tmp_path, pkg):
    out = tmp_path / "expose_kernels.s"
    subprocess.run([pkg._build.hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{REPO / 'include'}", f"-I{CSRC}",
                    "-S", "--cuda-device-only", "-o", str(out), str(CSRC / "expose_kernels.hip")], check=True, capture_output=True)
    text = out.read_text()
    meta = {}
    for block in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1))
                      for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    kernels = ("expose_kernel", "expose_gather_kernel")
    assert len(meta) == 2 and all(any(k in name for name in meta) for k in kernels), sorted(meta)
    for name, m in meta.items():
        print(name, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
        assert m["group_segment_fixed_size"] == 0
    # the exposure kernel's own code: rows and frames go 16 bytes a lane, the mean is closed by a true division (the scale / fmas /
    # fixup sequence, not a bare reciprocal times acc), and no float multiply-add can have been contracted out of acc + p
    name = next(n for n in meta if "expose_kernel" in n)
    body = text.split(f"\n{name}:", 1)[1].split("s_endpgm", 1)[0]
    assert "global_load_dwordx4" in body and "global_store_dwordx4" in body
    assert "v_div_fixup_f32" in body and "v_div_fmas_f32" in body
    assert re.search(r"\bv_(pk_)?add_f32", body)
