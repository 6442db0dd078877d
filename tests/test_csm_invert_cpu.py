"""Step 6a of include/awpu_hip_csm.h, the loaded inverse with a written arithmetic, on a box without a GPU: the entry points are
exported in a list of their own and declared by the header that awpu_hip_csm.h includes; awpu_hip_csm_invert_rule_host meets
numpy.linalg.inv and the existing awpu_hip_csm_invert_host within one float rounding of the bin's largest entry; G has an exactly
real diagonal and exactly conjugate mirrors; an unsolved bin is +0 with solved 0 and leaves the other bins alone; refusals write
nothing; the host code runs clean under the address and undefined-behaviour sanitizers as a program of its own; the kernels
compile for gfx950 without spills or scratch.  And the wiring of the cross-spectral runs (include/awpu_hip_csm_watch.h): symbols, the
header as C, the block source's refusals, the tools' --csm flags."""
import ctypes as C
import importlib
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import csm_util as CU

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "beamforming-lk_amd" / "csrc"
NAMES = ["awpu_hip_csm_invert_rule_host", "awpu_hip_csm_invert", "awpu_hip_csm_invert_device"]
LOADING = 1e-2
# Entries agree within 2^-22 of the bin's largest |entry|: cond(A) <= U / loading + 1 = 6.5e3 at 65 mics (A = B + load I with B
# positive semi-definite and load = loading trace(B) / U >= loading max_eig(B) / U), so two double results lie within ~1e-10 of the
# truth relative to |G|, and rounded to float they differ by at most one float rounding of the largest entry (2^-23 relative: the
# roundings are 2^-24 each).  The factor 2 is slack.
BOUND = 2.0 ** -22


def random_matrix(rng, K, U, n_blocks):
    """C = sum over blocks of X X^H, as step 2 lays it out: [K, U, U, 2] float32, Hermitian, with an exactly real diagonal."""
    X = rng.standard_normal((K, U, n_blocks)) + 1j * rng.standard_normal((K, U, n_blocks))
    Cc = X @ np.conj(np.swapaxes(X, 1, 2))
    out = np.stack([Cc.real, Cc.imag], axis=-1).astype(np.float32)
    out[:, np.arange(U), np.arange(U), 1] = 0.0
    return out


def loaded(Cm, n, loading):
    """A of the rule, in complex128, from the entries the rule reads (the lower triangle and the diagonal's real parts)."""
    U = Cm.shape[1]
    Cc = CU.as_complex(Cm)
    low = np.tril(Cc, -1)
    A = (low + np.conj(np.swapaxes(low, 1, 2))) / n
    d = np.diagonal(Cm[..., 0], axis1=1, axis2=2).astype(np.float64) / n
    load = np.float64(np.float32(loading)) * (d.sum(axis=1) / U)
    return A + (d + load[:, None])[:, :, None] * np.eye(U)


def test_invert_symbols_exported_and_listed(pkg):
    lib = pkg.binding.load()
    B = pkg.binding
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "awpu_hip_csm_invert.h").read_text(), flags=re.S)
    assert sorted(set(re.findall(r"\b(awpu_hip_\w+)\s*\(", text))) == sorted(NAMES) == sorted(B.CSM_INVERT_SYMBOLS)
    assert int(re.search(r"#define AWPU_CSM_INVERT_MAX_MICS (\d+)", text).group(1)) == 512 == B.CSM_INVERT_MAX_MICS
    assert '#include "awpu_hip_csm_invert.h"' in (REPO / "include" / "awpu_hip_csm.h").read_text()
    for name in NAMES:
        assert hasattr(lib, name)
    assert not set(B.CSM_INVERT_SYMBOLS) & set(B.CSM_SYMBOLS)
    H, S = pkg._build.HEADERS, pkg._build.SOURCES
    assert REPO / "include" / "awpu_hip_csm_invert.h" in H and CSRC / "csm_invert_rule.h" in H and CSRC / "csm_invert_kernels.h" in H
    assert CSRC / "csm_invert_kernels.hip" in S and CSRC / "csm_invert_host.cpp" in S
    # one statement of the arithmetic: the host rule, the kernels and the checker compile the same header
    for user in (CSRC / "csm_invert_host.cpp", CSRC / "csm_invert_kernels.h", REPO / "tests" / "host" / "csm_invert_check.cpp"):
        assert '#include "csm_invert_rule.h"' in user.read_text(), user
    assert "csm_invert_rule_host" in pkg.__all__ and callable(pkg.csm_invert_rule_host)
    assert callable(B.Engine.csm_invert) and callable(B.Engine.csm_invert_device)
    # the std::complex inverse stays as it was, beside the rule
    assert "awpu_hip_csm_invert_host" in (CSRC / "csm_host.cpp").read_text() and "awpu_hip_csm_invert_host" in B.CSM_SYMBOLS


def test_header_compiles_as_c_from_either_include(tmp_path):
    for first in ("awpu_hip_csm.h", "awpu_hip_csm_invert.h"):
        src = tmp_path / "one.c"
        src.write_text(f'#include "{first}"\n'
                       "int main(void) { awpu_csm_t c; float p[8]; int32_t s[1];\n"
                       "  c.window = AWPU_TONES_RECT; c.n_bins = 1; c.bin[0] = 3; c.kind = AWPU_CSM_CAPON; c.loading = 0.5f; p[0] = 1.0f;\n"
                       "  return awpu_hip_csm_invert_rule_host(p, 1, 1, &c, p + 2, s) + awpu_hip_csm_invert(0, p, 1, &c, p + 2)\n"
                       "    + awpu_hip_csm_invert_device(0, p, 1, &c, p + 2, s, 0) + AWPU_CSM_INVERT_MAX_MICS; }\n")
        subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", f"-I{REPO / 'include'}", str(src)], check=True, capture_output=True)


def test_host_file_compiles_with_a_plain_host_compiler(tmp_path):
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{REPO / 'include'}", f"-I{CSRC}", "-c", str(CSRC / "csm_invert_host.cpp"),
                    "-o", str(tmp_path / "csm_invert_host.o")], check=True, capture_output=True)


@pytest.mark.parametrize("U", [1, 2, 5, 64, 65])
def test_rule_host_against_numpy_and_the_existing_inverse(pkg, U):
    """Random Hermitian positive-definite inputs, loading 1e-2, three bins: against numpy.linalg.inv of the loaded matrix in
    complex128 and against awpu_hip_csm_invert_host, within BOUND of the bin's largest |entry| (derived above)."""
    rng = np.random.default_rng(100 + U)
    bins = [3, 16, 128]
    n = 2 * U + 3
    Cm = random_matrix(rng, 3, U, n)
    Gf, solved = pkg.csm_invert_rule_host(Cm, n, bins, loading=LOADING)
    assert Gf.dtype == np.float32 and Gf.shape == Cm.shape and solved.tolist() == [1, 1, 1]
    G = CU.as_complex(Gf)
    inv = np.linalg.inv(loaded(Cm, n, LOADING))
    old = CU.as_complex(pkg.csm_invert_host(Cm, n, bins, loading=LOADING))
    largest = np.abs(inv).max(axis=(1, 2))
    worst = {"numpy": np.abs(G - inv).max(axis=(1, 2)) / largest, "invert_host": np.abs(G - old).max(axis=(1, 2)) / largest}
    print(U, {k: float(v.max()) for k, v in worst.items()}, "bound", BOUND)
    assert (worst["numpy"] <= BOUND).all() and (worst["invert_host"] <= BOUND).all(), worst


def test_structure_of_g(pkg):
    rng = np.random.default_rng(7)
    bins = [0, 5, 47, 128]
    Cm = random_matrix(rng, 4, 9, 30)
    Cm[:, np.arange(9), np.arange(9), 1] = 5.0   # never read: the diagonal's imaginary parts ...
    upper = np.triu(np.ones((9, 9), bool), 1)
    spoiled = Cm.copy()
    spoiled[:, upper] = np.nan                   # ... and the entries above the diagonal
    Gf, solved = pkg.csm_invert_rule_host(spoiled, 30, bins, loading=LOADING)
    assert solved.tolist() == [1, 1, 1, 1] and np.isfinite(Gf).all()
    assert CU.same_bits(Gf, pkg.csm_invert_rule_host(Cm, 30, bins, loading=LOADING)[0])
    diag_im = np.diagonal(Gf[..., 1], axis1=1, axis2=2)
    assert not diag_im.any() and not np.signbit(diag_im).any()  # +0
    assert (np.diagonal(Gf[..., 0], axis1=1, axis2=2) > 0).all()
    G = Gf[..., 0] + 1j * Gf[..., 1]
    assert np.array_equal(G, np.conj(np.swapaxes(G, 1, 2)))
    low = np.tril(np.ones((9, 9), bool), -1)
    assert CU.same_bits(np.swapaxes(Gf[..., 0], 1, 2)[:, low], Gf[..., 0][:, low])
    assert CU.same_bits(np.swapaxes(Gf[..., 1], 1, 2)[:, low], -Gf[..., 1][:, low])


@pytest.mark.parametrize("what", ["zeros", "nan_lower", "nan_diagonal", "negative"])
def test_unsolved_bins(pkg, what):
    """An all-zero matrix with loading 0, and a matrix with a NaN entry: that bin +0 with solved 0, the other bins untouched,
    AWPU_OK overall."""
    rng = np.random.default_rng(11)
    bins = [3, 16, 128]
    U, n = 6, 20
    Cm = random_matrix(rng, 3, U, n)
    loading = 0.0 if what == "zeros" else LOADING
    want, ok = pkg.csm_invert_rule_host(Cm, n, bins, loading=loading)
    assert ok.tolist() == [1, 1, 1]
    bad = Cm.copy()
    if what == "zeros":
        bad[1] = 0.0
    elif what == "nan_lower":
        bad[1, 4, 2, 1] = np.nan
    elif what == "nan_diagonal":
        bad[1, 3, 3, 0] = np.nan
    else:
        bad[1, 0, 0, 0] = -1e6
    got, solved = pkg.csm_invert_rule_host(bad, n, bins, loading=loading)
    assert solved.tolist() == [1, 0, 1]
    assert not got[1].any() and not np.signbit(got[1]).any()
    assert CU.same_bits(got[0], want[0]) and CU.same_bits(got[2], want[2])
    assert not np.isnan(got).any()


def test_refusals_write_nothing(pkg):
    B = pkg.binding
    lib = B.load()
    bins = [3, 47]
    Cm = random_matrix(np.random.default_rng(3), 2, 4, 9)
    canary = np.float32(-3.0)
    out = np.full(2 * 4 * 4 * 2, canary, np.float32)
    solved = np.full(2, -7, np.int32)
    f, i = B._f32, B._i32

    def status(c, matrix=Cm, blocks=9, usable=4, inverse=True):
        return lib.awpu_hip_csm_invert_rule_host(None if matrix is None else f(matrix), blocks, usable, None if c is None else C.byref(c),
                                                 f(out) if inverse else None, i(solved))

    def bad(**changes):
        c = B.csm_of(bins, 0, CU.CAPON, 0.01)
        for k, v in changes.items():
            if k == "bin":
                c.bin[v[0]] = v[1]
            else:
                setattr(c, k, v)
        return c

    assert status(bad()) == B.OK and (out != canary).all() and solved.tolist() == [1, 1]
    out[:] = canary
    solved[:] = -7
    for c in (None, bad(window=2), bad(n_bins=0), bad(n_bins=9), bad(bin=(1, 129)), bad(bin=(0, -1)), bad(bin=(1, 3)), bad(kind=3), bad(kind=-1),
              bad(loading=-1e-3), bad(loading=float("nan")), bad(loading=float("inf"))):
        assert status(c) == B.ERR_INVALID
    good = bad()
    assert status(good, matrix=None) == B.ERR_INVALID and status(good, inverse=False) == B.ERR_INVALID
    assert status(good, blocks=0) == B.ERR_INVALID and status(good, usable=0) == B.ERR_INVALID
    assert (out == canary).all() and solved.tolist() == [-7, -7]
    with pytest.raises(pkg.AwpuError) as ei:
        pkg.csm_invert_rule_host(Cm, 9, [47, 3])
    assert ei.value.status == B.ERR_INVALID


def test_host_code_runs_clean_under_sanitizers(tmp_path):
    """tests/host/csm_invert_check.cpp with csm_invert_host.cpp: a program of its own under ASan and UBSan, every buffer exactly as
    long as the header says."""
    exe = tmp_path / "csm_invert_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{REPO / 'include'}", f"-I{CSRC}", str(REPO / "tests" / "host" / "csm_invert_check.cpp"), str(CSRC / "csm_invert_host.cpp"),
                    "-o", str(exe)], check=True, capture_output=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "csm invert rule: ok" in out.stdout, out.stdout + out.stderr


def test_invert_kernels_compile_without_spills(tmp_path, pkg):
    """The metadata of the code object only: no spills, no private segment; the factor kernel's 1024 threads leave it 128
    registers."""
    out = tmp_path / "csm_invert_kernels.s"
    subprocess.run([pkg._build.hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{REPO / 'include'}", f"-I{CSRC}",
                    "-S", "--cuda-device-only", "-o", str(out), str(CSRC / "csm_invert_kernels.hip")], check=True, capture_output=True)
    text = out.read_text()
    assert "v_fma_f64" in text and "v_div_scale_f64" in text  # fused steps as written, and the full-precision division
    meta = {}
    for block in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1))
                      for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")}
    assert len(meta) == 5 and all(any(k in name for name in meta) for k in ("factor_kernelILb0", "factor_kernelILb1", "solve", "gram", "finish")), sorted(meta)
    for name, m in meta.items():
        print(name, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_count"] <= 128, (name, m)


# ------------------------------------------------------------------------------------------------ the runs' wiring

WATCH_NAMES = ["awpu_hip_csm_watch_blocks", "awpu_hip_csm_watch_samples", "awpu_hip_csm_watch_samples_device"]


def test_watch_symbols_exported_and_listed(pkg):
    lib = pkg.binding.load()
    B = pkg.binding
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "awpu_hip_csm_watch.h").read_text(), flags=re.S)
    assert sorted(set(re.findall(r"\b(awpu_hip_\w+)\s*\(", text))) == sorted(WATCH_NAMES) == sorted(B.CSM_WATCH_SYMBOLS)
    assert "#define AWPU_CSM_SHOW_SUM (-1)" in text and B.CSM_SHOW_SUM == -1
    assert int(re.search(r"#define AWPU_CSM_MAX_LENGTH (\d+)", text).group(1)) == 1024 == B.CSM_MAX_LENGTH
    assert '#include "awpu_hip_csm_watch.h"' in (REPO / "include" / "awpu_hip_csm.h").read_text()
    for name in WATCH_NAMES:
        assert hasattr(lib, name)
    assert not set(B.CSM_WATCH_SYMBOLS) & (set(B.CSM_SYMBOLS) | set(B.CSM_INVERT_SYMBOLS))
    assert CSRC / "csm_show_kernels.hip" in pkg._build.SOURCES and REPO / "include" / "awpu_hip_csm_watch.h" in pkg._build.HEADERS
    for name in ("csm_watch_blocks", "csm_watch_samples", "csm_watch_samples_device"):
        assert callable(getattr(B.Engine, name))


def test_watch_header_compiles_as_c(tmp_path):
    src = tmp_path / "one.c"
    src.write_text('#include "awpu_hip_csm.h"\n'
                   "int main(void) { awpu_csm_t c; awpu_watch_t w; float p[8]; int32_t n = 0;\n"
                   "  c.n_bins = 1; w.first = 0; p[0] = 0.0f;\n"
                   "  return awpu_hip_csm_watch_blocks(0, p, 1032, 1, &w, &c, 1, AWPU_CSM_SHOW_SUM, 0, 0, &n, 0, 0, p, 0, 0, 0, 0)\n"
                   "    + awpu_hip_csm_watch_samples(0, p, 256, 1, &w, &c, 1, 0, 0, 0, &n, 0, 0, p, 0, 0, 0, 0)\n"
                   "    + awpu_hip_csm_watch_samples_device(0, p, 256, 1, &w, &c, AWPU_CSM_MAX_LENGTH, 0, 0, 0, &n, 0, 0, p, 0, 0, 0, 0, 0); }\n")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", f"-I{REPO / 'include'}", str(src)], check=True, capture_output=True)


def test_a_run_without_a_handle_is_refused(pkg):
    """The block source's refusals come first, as in every run: a null handle, null samples, a pitch below the blocks."""
    B = pkg.binding
    lib = B.load()
    x = np.zeros((2, 512), np.float32)
    power = np.zeros((2, 4), np.float32)
    carry = np.zeros((2, 1, 2, 2), np.float32)
    held = C.c_int32(0)
    w, c = B.Watch(0, 1, 2, 2, 0, 0, 0, None), B.csm_of([16], 0, CU.CAPON, 0.01)
    rest = (C.byref(w), C.byref(c), 3, -1, None, B._f32(carry), C.cast(C.byref(held), B._i32p), None, None, B._f32(power), None, None, None, None)
    assert lib.awpu_hip_csm_watch_samples(None, B._f32(x), 512, 2, *rest) == B.ERR_INVALID and b"null handle" in lib.awpu_hip_last_error()
    assert lib.awpu_hip_csm_watch_blocks(None, x.ctypes.data_as(C.c_void_p), 1032, 2, *rest) == B.ERR_INVALID
    assert lib.awpu_hip_csm_watch_samples_device(None, None, 512, 2, *rest[:7], *([None] * 8)) == B.ERR_INVALID
    assert not power.any() and not carry.any() and held.value == 0


def test_tools_take_the_csm_flags():
    B = importlib.import_module("beamforming-lk_amd").binding
    assert B.csm_from_text("2900:3300:hann") == ([16, 17], B.TONES_HANN) and B.csm_from_text("0:100") == ([0], B.TONES_RECT)
    assert B.csm_kind_from_text("capon:0.05") == (B.CSM_CAPON, 0.05) and B.csm_kind_from_text("capon") == (B.CSM_CAPON, 1e-2)
    assert B.csm_kind_from_text("diagonal-removed")[0] == B.CSM_DIAGONAL_REMOVED and B.csm_kind_from_text("conventional")[0] == B.CSM_CONVENTIONAL
    for bad in ("1000:9000", "5:6", "3:2", "1:2:hamming"):
        with pytest.raises(ValueError):
            B.csm_from_text(bad)
    with pytest.raises(ValueError, match="at most 8"):
        B.csm_from_text("0:9000")
    for bad in ("mvdr", "conventional:1", "capon:-1"):
        with pytest.raises(ValueError):
            B.csm_kind_from_text(bad)
    for tool in ("pcap_video.py", "pcap_sources.py"):
        out = subprocess.run([sys.executable, str(REPO / "tools" / tool), "--help"], capture_output=True, text=True)
        assert out.returncode == 0 and "--csm " in out.stdout and "--csm-kind" in out.stdout and "--csm-length" in out.stdout, tool
        out = subprocess.run([sys.executable, str(REPO / "tools" / tool), "none.pcap", "--port", "1", "--csm", "0:9000"], capture_output=True, text=True)
        assert out.returncode == 2 and "at most 8" in out.stderr, (tool, out.stderr)
        out = subprocess.run([sys.executable, str(REPO / "tools" / tool), "none.pcap", "--port", "1", "--csm", "3000:3200", "--csm-length", "2000"],
                             capture_output=True, text=True)
        assert out.returncode == 2 and "--csm-length" in out.stderr, (tool, out.stderr)
    out = subprocess.run([sys.executable, str(REPO / "tools" / "csm_rate.py"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--repeats" in out.stdout
