"""Cross-spectral maps (include/awpu_hip_csm.h) on a box without a GPU: the entry points are exported in a list of their own and
built from the globbed files; every host function equals a numpy restatement of the rule bit for bit (tests/csm_util.py); C is
exactly Hermitian and a recording split over two calls gives one call's bits; steering, spectra, the quadratic form and the
inverse meet fp64; a unit sine gives 0.5 in the conventional and the diagonal-removed map and 0.5 (1 + loading / usable) in Capon's; on the two-source scene delay-and-sum's conventional plane shows one
source, Capon's both, and the diagonal-removed plane a lower floor; refusals write nothing; the host code runs clean under the
address and undefined-behaviour sanitizers as a program of its own; the kernels compile for gfx950 without spills or scratch.
The accuracy of q and of the loaded inverse at 545 to 2048 and at 512 mics: test_csm_large_cpu.py."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import csm_util as CU

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "beamforming-lk_amd" / "csrc"
GOLDEN = REPO / "tests" / "golden"
NAMES = ["awpu_hip_csm_spectra_host", "awpu_hip_csm_accumulate_host", "awpu_hip_csm_steer_host", "awpu_hip_csm_map_host",
         "awpu_hip_csm_invert_host", "awpu_hip_csm_samples", "awpu_hip_csm_samples_device", "awpu_hip_csm_map", "awpu_hip_csm_map_device"]
KINDS = (CU.CONVENTIONAL, CU.DIAGONAL_REMOVED, CU.CAPON)
BINS = [0, 3, 16, 47, 100, 127, 128]  # the accuracy tests': both ends, odd and even bins

# Accuracy against fp64, measured on this build's host rule over c1's table and the frames below; each is asserted at 4 x the
# measured worst, a margin for other seeds and not for another arithmetic:
STEER_MEASURED = 1.65e-7    # |s - exp(-2 pi i k tau / 256)|, every pixel, mic and bin of BINS
SPECTRA_MEASURED = 9.6e-7   # |X - rfft(w x)| over the largest |rfft| of the call
Q_MEASURED = 6.2e-7         # |q - s^H C s (complex128)| over the largest q of the bin's map
GA_MEASURED = 1.93e-7       # |G A - I|, largest entry
INVERSE_MEASURED = 4.6e-8   # |G - numpy.linalg.inv(A)| over the largest entry of the inverse


# ------------------------------------------------------------------------------------------------ wiring

def test_csm_symbols_exported_and_listed(pkg):
    lib = pkg.binding.load()
    B = pkg.binding
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "awpu_hip_csm.h").read_text(), flags=re.S)
    assert sorted(set(re.findall(r"\b(awpu_hip_\w+)\s*\(", text))) == sorted(NAMES)
    assert int(re.search(r"#define AWPU_CSM_MAX_BINS (\d+)", text).group(1)) == 8 == B.CSM_MAX_BINS
    assert int(re.search(r"#define AWPU_CSM_CONVENTIONAL (\d+)", text).group(1)) == 0 == B.CSM_CONVENTIONAL
    assert int(re.search(r"#define AWPU_CSM_DIAGONAL_REMOVED (\d+)", text).group(1)) == 1 == B.CSM_DIAGONAL_REMOVED
    assert int(re.search(r"#define AWPU_CSM_CAPON (\d+)", text).group(1)) == 2 == B.CSM_CAPON
    assert sorted(B.CSM_SYMBOLS) == sorted(NAMES)
    for name in NAMES:
        assert hasattr(lib, name)
    for other in (B.EXPORTED_SYMBOLS, B.TRACK_SYMBOLS, B.BLOCK_SYMBOLS, B.LISTEN_SYMBOLS, B.WATCH_SYMBOLS, B.FIND_SYMBOLS, B.BAND_SYMBOLS, B.FOCUS_SYMBOLS,
                  B.SPECTRAL_SYMBOLS, B.EXPOSE_SYMBOLS, B.COHERE_SYMBOLS, B.PEEL_SYMBOLS, B.TONES_SYMBOLS):
        assert not set(B.CSM_SYMBOLS) & set(other)
    assert lib.awpu_hip_abi_version() == 4
    main = (REPO / "include" / "awpu_hip.h").read_text()
    assert "awpu_hip_csm" not in main and "awpu_csm_t" not in main and "AWPU_CSM" not in main
    assert C.sizeof(B.Csm) == 48 and len(B.KERNEL_NAMES) == 20
    H, S = pkg._build.HEADERS, pkg._build.SOURCES
    assert REPO / "include" / "awpu_hip_csm.h" in H and CSRC / "csm_kernels.h" in H and CSRC / "csm_rule.h" in H
    assert CSRC / "csm_kernels.hip" in S and CSRC / "csm_host.cpp" in S and CSRC / "awpu_csm.cpp" in S
    # one statement of the arithmetic: the host rule, the kernels and the checker compile the same header
    for user in (CSRC / "csm_host.cpp", CSRC / "csm_kernels.hip", REPO / "tests" / "host" / "csm_rule_check.cpp"):
        assert '#include "csm_rule.h"' in user.read_text(), user
    for name in ("csm_spectra_host", "csm_accumulate_host", "csm_steer_host", "csm_map_host", "csm_invert_host"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    for name in ("csm_samples", "csm_samples_device", "csm_map", "csm_map_device"):
        assert callable(getattr(B.Engine, name))


def test_csm_header_compiles_as_c(tmp_path):
    src = tmp_path / "one.c"
    src.write_text('#include "awpu_hip_csm.h"\n'
                   "typedef char size_is_48[sizeof(awpu_csm_t) == 48 ? 1 : -1];\n"
                   "int main(void) { awpu_csm_t c; float p[512]; int32_t n[4]; int32_t count = 0;\n"
                   "  c.window = AWPU_TONES_HANN; c.n_bins = 1; c.bin[AWPU_CSM_MAX_BINS - 1] = 0; c.bin[0] = 3; c.kind = AWPU_CSM_CAPON; c.loading = 0.5f;\n"
                   "  n[0] = 0; p[0] = 0.0f;\n"
                   "  return awpu_hip_csm_spectra_host(p, 256, 1, 1, n, 1, 0, &c, p) + awpu_hip_csm_accumulate_host(p, 256, 1, 1, n, 1, 0, &c, p, &count)\n"
                   "    + awpu_hip_csm_steer_host(n, p, 1, 1, n, 1, &c, p) + awpu_hip_csm_map_host(p, 1, n, p, 1, 1, n, 1, &c, p, 0)\n"
                   "    + awpu_hip_csm_invert_host(p, 1, 1, &c, p) + awpu_hip_csm_samples(0, p, 256, 1, &c, p, &count, 0)\n"
                   "    + awpu_hip_csm_samples_device(0, p, 256, 1, &c, p, &count, 0, 0) + awpu_hip_csm_map(0, p, 1, &c, p, 0)\n"
                   "    + awpu_hip_csm_map_device(0, p, 1, &c, p, 0, 0) + (int) sizeof(size_is_48); }\n")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", f"-I{REPO / 'include'}", str(src)], check=True, capture_output=True)


def test_host_file_compiles_with_a_plain_host_compiler(tmp_path):
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{REPO / 'include'}", f"-I{CSRC}", "-c", str(CSRC / "csm_host.cpp"),
                    "-o", str(tmp_path / "csm_host.o")], check=True, capture_output=True)


# ------------------------------------------------------------------------------------------------ the rule

@pytest.fixture(scope="module")
def c1(pkg):
    """The c1 table, a recording of 5 blocks with 40 samples of slack in its pitch, the ragged 51-mic list with gains, and the
    scene with the host rule's planes (computed once, never written)."""
    S = pkg.synthetic
    spec = S.WORKLOADS["c1"]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    frames = S.make_frames(xyz, 2, seed=99)
    samples = np.ascontiguousarray(np.concatenate([frames[0], frames[1]], axis=1)[:, :5 * 256 + 40])
    index51 = np.load(GOLDEN / "sweep_c1_ragged.npz")["index"]
    gain = (0.5 + np.random.default_rng(3).random(51)).astype(np.float32)
    x, levels = CU.scene_samples(pkg, spec, xyz)
    b = [CU.SCENE_BIN]
    C_scene, n = pkg.csm_accumulate_host(x, b, 1)
    planes = {CU.CONVENTIONAL: pkg.csm_map_host(C_scene, n, off, frac, b, 1, CU.CONVENTIONAL)["map"][0],
              CU.DIAGONAL_REMOVED: pkg.csm_map_host(C_scene, n, off, frac, b, 1, CU.DIAGONAL_REMOVED)["map"][0],
              CU.CAPON: pkg.csm_map_host(pkg.csm_invert_host(C_scene, n, b, loading=CU.SCENE_LOADING), n, off, frac, b, 1, CU.CAPON)["map"][0]}
    for a in (samples, off, frac, *planes.values()):
        a.setflags(write=False)
    return dict(spec=spec, xyz=xyz, off=off, frac=frac, samples=samples, index51=index51, gain=gain, planes=planes, levels=levels)


SETTINGS = [([0, 1, 2, 3, 4, 5, 6, 7], 0, False), ([3, 47, 128], 1, True), ([128], 1, False), ([0], 0, True)]


@pytest.mark.parametrize("bins,window,ragged", SETTINGS)
def test_host_functions_equal_the_numpy_restatement(pkg, c1, bins, window, ragged):
    """Spectra, C, steering, q and the three kinds of plane, bit for bit; with the ragged list come gains and a pixel subset."""
    index, gain = (c1["index51"], c1["gain"]) if ragged else (None, None)
    pixels = np.arange(0, 1024, 7) if ragged else np.arange(1024)
    off, frac = c1["off"][pixels], c1["frac"][pixels]
    X = pkg.csm_spectra_host(c1["samples"], bins, window, index=index, gain=gain)
    want_X = CU.spectra(pkg, c1["samples"], bins, window, index, gain)
    assert X.shape == want_X.shape == (5, len(bins), 51 if ragged else 64, 2) and CU.same_bits(X, want_X)
    Cm, n = pkg.csm_accumulate_host(c1["samples"], bins, window, index=index, gain=gain)
    assert n == 5 and CU.same_bits(Cm, CU.accumulate(want_X))
    assert CU.same_bits(pkg.csm_steer_host(off, frac, bins, index=index), CU.steer(pkg, off, frac, bins, index))
    G = pkg.csm_invert_host(Cm, n, bins, loading=0.05)
    for kind in KINDS:
        H = G if kind == CU.CAPON else Cm
        got = pkg.csm_map_host(H, n, off, frac, bins, window, kind, index=index, want=("map", "q"))
        want = CU.rule_map(pkg, H, n, off, frac, bins, window, kind, index)
        assert got["q"].shape == (len(bins), len(pixels)) and CU.same_bits(got["q"], want["q"]), kind
        assert CU.same_bits(got["map"], want["map"]), kind
        assert CU.same_bits(pkg.csm_map_host(H, n, off, frac, bins, window, kind, index=index)["map"], got["map"])  # alone: the same bits
    if ragged:  # gains change the bits
        assert not CU.same_bits(Cm, pkg.csm_accumulate_host(c1["samples"], bins, window, index=index)[0])


def test_matrix_is_exactly_hermitian_and_a_split_recording_gives_one_calls_bits(pkg, c1):
    bins = [3, 47, 128]
    whole, n = pkg.csm_accumulate_host(c1["samples"], bins, 1)
    Cc = whole[..., 0] + 1j * whole[..., 1]
    assert np.array_equal(Cc, np.conj(np.swapaxes(Cc, 1, 2))) and not np.diagonal(whole[..., 1], axis1=1, axis2=2).any()
    assert not np.signbit(np.diagonal(whole[..., 1], axis1=1, axis2=2)).any()  # +0
    first, n2 = pkg.csm_accumulate_host(c1["samples"], bins, 1, n_blocks=2)
    both, n5 = pkg.csm_accumulate_host(c1["samples"][:, 512:], bins, 1, matrix=first, block_count=n2, n_blocks=3)
    assert (n, n2, n5) == (5, 2, 5) and both is first and CU.same_bits(both, whole)
    # the restatement adds into a matrix the same way
    X = CU.spectra(pkg, c1["samples"], bins, 1)
    assert CU.same_bits(CU.accumulate(X[2:], CU.accumulate(X[:2])), whole)


def test_accuracy_against_fp64(pkg, c1):
    """Measured here (worst over c1's table, BINS, both windows and three seeds of synthetic.make_frames, 8 blocks each):
    steering 1.65e-7, spectra 9.6e-7 of the largest bin, q 6.2e-7 of the map's largest q.  Asserted at 4 x."""
    S = pkg.synthetic
    steer = CU.as_complex(pkg.csm_steer_host(c1["off"], c1["frac"], BINS))
    tau = (256.0 - c1["off"]) + c1["frac"].astype(np.float64)
    exact = np.exp(-2j * np.pi * np.array(BINS)[None, :, None] * tau[:, None, :] / 256.0)
    worst = {"steer": float(np.abs(steer - exact).max()), "spectra": 0.0, "q": 0.0}
    for seed in (1, 2, 3):
        fr = S.make_frames(c1["xyz"], 2, seed=seed)
        x = np.concatenate([fr[0], fr[1]], axis=1)
        for window in (0, 1):
            X = CU.as_complex(pkg.csm_spectra_host(x, BINS, window))
            w = pkg.tones_window(window).astype(np.float64)
            ref = np.fft.rfft(x.astype(np.float64).reshape(64, 8, 256) * w, axis=2)[:, :, BINS].transpose(1, 2, 0)
            worst["spectra"] = max(worst["spectra"], float(np.abs(X - ref).max() / np.abs(ref).max()))
            Cm, n = pkg.csm_accumulate_host(x, BINS, window)
            q = pkg.csm_map_host(Cm, n, c1["off"], c1["frac"], BINS, window, want=("q",))["q"]
            q64 = np.einsum("pka,kab,pkb->kp", steer, CU.as_complex(Cm), np.conj(steer)).real
            worst["q"] = max(worst["q"], float((np.abs(q - q64).max(axis=1) / np.abs(q64).max(axis=1)).max()))
    print(worst)
    assert worst["steer"] <= 4 * STEER_MEASURED and worst["spectra"] <= 4 * SPECTRA_MEASURED and worst["q"] <= 4 * Q_MEASURED, worst


def test_inverse_against_fp64(pkg):
    """G A against the identity and G against numpy.linalg.inv(A), A formed in fp64 from the fp32 matrix as step 6 says: 64 mics
    of white noise, 100 blocks, bins 3, 16 and 128, loading 1e-3 and 1e-1, two seeds.  Measured here: 1.93e-7 and 4.6e-8 of the
    inverse's largest entry.  Asserted at 4 x."""
    rng = np.random.default_rng(5)
    bins = [3, 16, 128]
    worst = {"ga": 0.0, "inverse": 0.0}
    for _ in range(2):
        x = rng.standard_normal((64, 256 * 100)).astype(np.float32)
        Cm, n = pkg.csm_accumulate_host(x, bins, 1)
        for loading in (1e-3, 1e-1):
            Gf = pkg.csm_invert_host(Cm, n, bins, loading=loading)
            G = CU.as_complex(Gf)
            assert np.array_equal(G, np.conj(np.swapaxes(G, 1, 2))) and not np.diagonal(Gf[..., 1], axis1=1, axis2=2).any()
            A = CU.as_complex(Cm) / n
            A = A + np.float64(np.float32(loading)) * (np.trace(A, axis1=1, axis2=2).real[:, None, None] / 64.0) * np.eye(64)
            inv = np.linalg.inv(A)
            worst["ga"] = max(worst["ga"], float(np.abs(G @ A - np.eye(64)).max()))
            worst["inverse"] = max(worst["inverse"], float((np.abs(G - inv).max(axis=(1, 2)) / np.abs(inv).max(axis=(1, 2))).max()))
    print(worst)
    assert worst["ga"] <= 4 * GA_MEASURED and worst["inverse"] <= 4 * INVERSE_MEASURED, worst


def test_a_unit_sine_gives_one_half_and_in_capons_map_one_half_times_its_loading_factor(pkg):
    """Eight mics, integer delays (frac = 0: the steering values are table entries), the rectangular window, a unit sine at the
    centre of bin k arriving from pixel 0 of a two-pixel table, 2 blocks.  Every term s_a C[a][b] conj(s_b) of pixel 0 is then
    the same positive number, so every partial sum of the rule is no larger than its total and each rounding is relative to the
    result.  |X| = 128: step 1 adds 256 terms into a partial sum below 256, each fmaf off by at most 2^-17, so X is within
    2^-9 / 128 = 2^-16 of its value and a product of two spectra within 2^-15; behind it come 2 n_blocks fmaf per entry, 4 U + 2 U
    per pixel, the twiddles' own roundings (4) and the division's (4): (2 n_blocks + 6 U + 8) 2^-24.  Capon's map is
    0.5 (1 + loading / U) by the rule; G's rounding to float adds U^2 2^-24 / loading."""
    U_, k, n_blocks = 8, 16, 2
    rel = 2.0 ** -15 + (2 * n_blocks + 6 * U_ + 8) * 2.0 ** -24
    off = np.array([[40, 3, 17, 0, 255, 90, 128, 77], [41, 9, 3, 11, 200, 60, 100, 7]], np.int32)
    frac = np.zeros((2, U_), np.float32)
    tau = 256.0 - off[0]
    t = np.arange(256 * n_blocks)
    for bin_ in (k, 0, 128):
        amp = 1.0
        x = (amp * np.cos(2.0 * np.pi * bin_ * (t[None, :] + tau[:, None]) / 256.0 + (0.3 if 0 < bin_ < 128 else 0.0))).astype(np.float32)
        want = 0.5 if 0 < bin_ < 128 else 1.0  # (a cosine at DC or at the Nyquist bin has all its power in one bin: c_k = 1, |X| = 256)
        Cm, n = pkg.csm_accumulate_host(x, [bin_], 0)
        for kind in (CU.CONVENTIONAL, CU.DIAGONAL_REMOVED):
            got = float(pkg.csm_map_host(Cm, n, off, frac, [bin_], 0, kind)["map"][0, 0])
            print(bin_, kind, got, abs(got / want - 1.0), rel)
            assert abs(got / want - 1.0) <= rel, (bin_, kind, got)
        loading = 1.0
        G = pkg.csm_invert_host(Cm, n, [bin_], loading=loading)
        got = float(pkg.csm_map_host(G, n, off, frac, [bin_], 0, CU.CAPON)["map"][0, 0])
        print(bin_, "capon", got, abs(got / (want * (1.0 + loading / U_)) - 1.0))
        assert abs(got / (want * (1.0 + loading / U_)) - 1.0) <= rel + U_ * U_ * 2.0 ** -24 / loading, (bin_, got)


def test_the_scene_that_justifies_the_feature(pkg, c1):
    """csm_util's scene on c1 (32 x 32 pixels, 64 mics): two independent noise sources within 100 Hz of bin 16's centre
    (3.05 kHz), rms 1.0 and 0.8 at the mics, at pixels (16, 12) and (16, 19) -- 7 pixels, 0.44 in sine space, where the array's
    beam is about 0.8 wide --, 256 blocks, white self-noise of rms 0.5 to 2.0, a level of its own on every mic, the Hann window,
    loading 1e-2, find_peaks with radius 2 and min_ratio 0.25.  Picked on the host rule alone: the conventional plane shows ONE
    source (at column 14, between the two), Capon's both at their pixels, and the diagonal-removed plane's median lies 21.5 dB
    under its maximum where the conventional plane's lies 15.5 dB under."""
    planes = c1["planes"]
    found = {kind: pkg.find_peaks(planes[kind], 32, 32, **CU.SCENE_FIND) for kind in KINDS}
    count = {kind: int(np.ravel(found[kind].count)[0]) for kind in KINDS}
    pixels = {kind: [int(p) for p in np.ravel(found[kind].sources)["pixel"][:count[kind]]] for kind in KINDS}
    floor = {kind: CU.median_over_max_db(planes[kind]) for kind in KINDS}
    print(count, pixels, floor)
    assert count[CU.CONVENTIONAL] == 1
    assert count[CU.CAPON] == 2
    for true in CU.scene_pixels(c1["spec"]):
        assert any(abs(p // 32 - true // 32) <= 1 and abs(p % 32 - true % 32) <= 1 for p in pixels[CU.CAPON]), (true, pixels)
    assert floor[CU.DIAGONAL_REMOVED] < floor[CU.CONVENTIONAL]
    assert c1["levels"].max() / c1["levels"].min() > 2.0  # the mics' self-noise does differ


# ------------------------------------------------------------------------------------------------ refusals

def test_refusals_write_nothing(pkg, c1):
    B = pkg.binding
    lib = B.load()
    bins = [3, 47]
    x = np.ascontiguousarray(c1["samples"][:4, :512])
    off, frac = np.ascontiguousarray(c1["off"][:3, :4]), np.ascontiguousarray(c1["frac"][:3, :4])
    index = np.arange(4, dtype=np.int32)
    Cm, n = pkg.csm_accumulate_host(x, bins)
    canary = np.float32(-3.0)
    out = np.full(2 * 4 * 4 * 2 * 4, canary, np.float32)
    count = C.c_int32(7)
    good = B.csm_of(bins, 0, CU.CONVENTIONAL, 0.0)
    f, i = B._f32, B._i32

    def bad(**changes):
        c = B.csm_of(bins, 0, CU.CONVENTIONAL, 0.0)
        for k, v in changes.items():
            if k == "bin":
                c.bin[v[0]] = v[1]
            else:
                setattr(c, k, v)
        return c

    def calls(c, which=slice(0, 5), samples=x, matrix=Cm, pitch=512, blocks=n, idx=index, fr=frac, of=off, usable=4, map_out=True):
        """The statuses of the host functions `which` (spectra, accumulate, steer, map, invert), all writing into `out`."""
        cp = None if c is None else C.byref(c)
        o = f(out)
        five = [lambda: lib.awpu_hip_csm_spectra_host(None if samples is None else f(samples), pitch, 4, 2, i(idx), usable, None, cp, o),
                lambda: lib.awpu_hip_csm_accumulate_host(None if samples is None else f(samples), pitch, 4, 2, i(idx), usable, None, cp, o, C.byref(count)),
                lambda: lib.awpu_hip_csm_steer_host(i(of), f(fr), 4, 3, i(idx), usable, cp, o),
                lambda: lib.awpu_hip_csm_map_host(None if matrix is None else f(matrix), blocks, i(of), f(fr), 4, 3, i(idx), usable, cp,
                                                  o if map_out else None, None),
                lambda: lib.awpu_hip_csm_invert_host(None if matrix is None else f(matrix), blocks, usable, cp, o)]
        return [call() for call in five[which]]

    for c in (None, bad(window=2), bad(n_bins=0), bad(n_bins=9), bad(bin=(1, 129)), bad(bin=(0, -1)), bad(bin=(1, 3)), bad(kind=3), bad(kind=-1),
              bad(loading=-1e-3), bad(loading=float("nan")), bad(loading=float("inf"))):
        assert calls(c) == [B.ERR_INVALID] * 5, None if c is None else (c.window, c.n_bins, list(c.bin), c.kind, c.loading)
    assert calls(good, slice(0, 2), samples=None) == [B.ERR_INVALID] * 2 and calls(good, slice(3, 5), matrix=None) == [B.ERR_INVALID] * 2
    assert calls(good, slice(0, 2), pitch=511) == [B.ERR_INVALID] * 2
    assert calls(good, slice(3, 5), blocks=0) == [B.ERR_INVALID] * 2
    assert calls(good, slice(0, 4), idx=np.array([0, 1, 2, 4], np.int32)) == [B.ERR_INVALID] * 4
    assert calls(good, usable=0) == [B.ERR_INVALID] * 5
    nan_frac = frac.copy()
    nan_frac[2, 3] = np.nan
    assert calls(good, slice(2, 4), fr=nan_frac) == [B.ERR_INVALID] * 2
    neg_off = off.copy()
    neg_off[0, 0] = -1
    assert calls(good, slice(2, 4), of=neg_off) == [B.ERR_INVALID] * 2
    assert calls(good, slice(3, 4), map_out=False) == [B.ERR_INVALID]  # no output asked for
    # diagonal removal needs two mics
    assert lib.awpu_hip_csm_map_host(f(Cm), n, i(off), f(frac), 4, 3, i(index), 1, C.byref(bad(kind=CU.DIAGONAL_REMOVED)), f(out), None) == B.ERR_INVALID
    # not positive definite: AWPU_ERR_RANGE
    indefinite = Cm.copy()
    indefinite[0, 0, 0, 0] = -1e6
    assert lib.awpu_hip_csm_invert_host(f(indefinite), n, 4, C.byref(bad(kind=CU.CAPON, loading=0.01)), f(out)) == B.ERR_RANGE
    silence = np.zeros_like(Cm)  # singular, and no loading lifts it
    assert lib.awpu_hip_csm_invert_host(f(silence), n, 4, C.byref(bad(kind=CU.CAPON)), f(out)) == B.ERR_RANGE
    full = C.c_int32(2 ** 31 - 2)
    assert lib.awpu_hip_csm_accumulate_host(f(x), 512, 4, 2, i(index), 4, None, C.byref(good), f(out), C.byref(full)) == B.ERR_INVALID
    assert (out == canary).all() and count.value == 7 and full.value == 2 ** 31 - 2
    with pytest.raises(pkg.AwpuError) as ei:
        pkg.csm_map_host(Cm, n, off, frac, [47, 3])
    assert ei.value.status == B.ERR_INVALID


# ------------------------------------------------------------------------------------------------ sanitizers, and the kernels' build

def test_host_code_runs_clean_under_sanitizers(tmp_path):
    """tests/host/csm_rule_check.cpp with csm_host.cpp: a program of its own under ASan and UBSan, every buffer exactly as long as
    the header says."""
    exe = tmp_path / "csm_rule_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{REPO / 'include'}", f"-I{CSRC}", str(REPO / "tests" / "host" / "csm_rule_check.cpp"), str(CSRC / "csm_host.cpp"),
                    "-o", str(exe)], check=True, capture_output=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "csm rule: ok" in out.stdout, out.stdout + out.stderr


def test_csm_kernels_compile_without_spills(tmp_path, pkg):
    """The metadata of the code object only: no spills, no private segment.  The map kernel's design keeps the steering vectors in
    LDS and the matrix entries in SGPRs: its lanes hold four rows' sums, one steering value and the running totals, well inside 64
    VGPRs -- LDS, not registers, sets how many waves a compute unit holds."""
    out = tmp_path / "csm_kernels.s"
    subprocess.run([pkg._build.hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{REPO / 'include'}", f"-I{CSRC}",
                    "-S", "--cuda-device-only", "-o", str(out), str(CSRC / "csm_kernels.hip")], check=True, capture_output=True)
    text = out.read_text()
    meta = {}
    for block in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1))
                      for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")}
    assert len(meta) == 3 and all(any(k in name for name in meta) for k in ("csm_spectra_kernel", "csm_accumulate_kernel", "csm_map_kernel")), sorted(meta)
    for name, m in meta.items():
        print(name, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_count"] <= 64, (name, m)


def test_rate_tool_parses():
    out = subprocess.run([sys.executable, str(REPO / "tools" / "csm_rate.py"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--repeats" in out.stdout
