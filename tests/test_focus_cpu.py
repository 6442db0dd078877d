"""Focus and range (include/awpu_hip_focus.h) without a GPU: the symbols are a set of their own and the ABI version stays 4; the
focus rule equals its fp64 closed form within the builders' 5e-5 samples and has the properties the header states (inf = the
plane-wave builders bit for bit, min tau 0, max tau within the aperture, row slices, refusals); awpu_hip_range_pick picks and
refines as the header says; and on the CPU oracle's sweep a table focused on a point source 2 m from the 32 x 8 tile has its
maximum at the source's pixel, where the plane-wave table keeps less than half of the power; the range kernels compile for gfx950
without spills or scratch."""
import ctypes as C

import numpy as np
import pytest

ARRAYS = [(1, 1), (4, 1), (4, 2)]  # 8 x 8, 32 x 8, 32 x 16
FS_C = 48828.0 / 340.0
TOL = 5e-5  # samples: the project's figure for the plane-wave builders against their fp64 closed form (tests/test_oracle_golden.py)


def closed_form(xyz, theta, phi, distance):
    """(max d - d_m) * fs / c in fp64, with w = (sin t cos p, -sin t sin p, cos t): the unit vector whose plane-wave delay is
    (fs / c) w . p_m."""
    w = np.array([np.sin(theta) * np.cos(phi), -np.sin(theta) * np.sin(phi), np.cos(theta)])
    d = np.linalg.norm(distance * w[:, None] - xyz.astype(np.float64), axis=0)
    return (d.max() - d) * FS_C


def aperture_samples(xyz):
    p = xyz.astype(np.float64).T
    return float(np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)).max()) * FS_C


def test_symbols_are_a_set_of_their_own(pkg):
    B = pkg.binding
    lib = B.load()
    focus = set(B.FOCUS_SYMBOLS)
    assert len(focus) == 9
    for other in (B.EXPORTED_SYMBOLS, B.TRACK_SYMBOLS, B.BLOCK_SYMBOLS, B.LISTEN_SYMBOLS, B.WATCH_SYMBOLS, B.FIND_SYMBOLS, B.BAND_SYMBOLS):
        assert not focus & set(other)
    for name in focus:
        assert hasattr(lib, name), name
    assert lib.awpu_hip_abi_version() == 4
    assert C.sizeof(B.Range) == 16 and B.RANGE_MAX_CANDIDATES == 64


@pytest.mark.parametrize("arrays", ARRAYS)
def test_rule_equals_the_closed_form(pkg, arrays):
    """300 random (theta, phi, d) per array, d log-uniform in [0.05 m, 1e6 m]: |tau - closed form| <= 5e-5 samples."""
    xyz = pkg.create_tiled_antenna(*arrays)
    rng = np.random.default_rng(sum(arrays))
    worst = 0.0
    for _ in range(300):
        theta, phi, d = rng.uniform(0.0, np.pi / 2), rng.uniform(-np.pi, np.pi), 10.0 ** rng.uniform(np.log10(0.05), 6.0)
        worst = max(worst, float(np.abs(pkg.focus_delays(xyz, theta, phi, d) - closed_form(xyz, theta, phi, d)).max()))
    print(f"{arrays}: worst |tau - closed form| = {worst:.3g} samples")
    assert worst <= TOL


@pytest.mark.parametrize("arrays", ARRAYS)
def test_infinity_is_the_plane_wave_bit_for_bit(pkg, arrays):
    xyz = pkg.create_tiled_antenna(*arrays)
    for fov in (180.0, 90.0):
        got, want = pkg.build_focus_table(xyz, 12, 10, np.inf, fov), pkg.build_delay_table(xyz, 12, 10, fov)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    theta, phi = np.array([0.0, 0.3, 1.2, np.pi / 2]), np.array([0.0, 1.1, -2.5, 0.7])
    got, want = pkg.focus_steer_table(xyz, theta, phi, np.inf), pkg.steer_table(xyz, theta, phi)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    for t, p in zip(theta, phi):
        assert np.array_equal(pkg.focus_delays(xyz, t, p, np.inf).view(np.uint32), pkg.steering_delays(xyz, t, p).view(np.uint32))
    # a mixed batch: the infinite entries are the plane wave's, the finite ones the rule's
    mixed = pkg.focus_steer_table(xyz, theta, phi, np.array([np.inf, 2.0, np.inf, 0.5]))
    assert np.array_equal(mixed[0][[0, 2]], want[0][[0, 2]]) and np.array_equal(mixed[1][[0, 2]], want[1][[0, 2]])
    one = pkg.focus_steer_table(xyz, theta[1], phi[1], 2.0)
    assert np.array_equal(mixed[0][1], one[0][0]) and np.array_equal(mixed[1][1], one[1][0])
    tau = pkg.focus_delays(xyz, theta[1], phi[1], 2.0)
    assert np.array_equal(one[0][0], 256 - np.trunc(tau).astype(np.int32)) and np.array_equal(one[1][0], tau - np.trunc(tau))


@pytest.mark.parametrize("arrays", ARRAYS)
def test_table_properties(pkg, arrays):
    """Far away the rule tends to the plane wave (5e-5 for each builder + aperture^2 / 2r * fs / c = 3e-6 at 1e7 m); min tau = 0;
    max tau <= the aperture; row slices are the rows of the whole table."""
    xyz = pkg.create_tiled_antenna(*arrays)
    aperture = aperture_samples(xyz)
    rng = np.random.default_rng(7)
    for _ in range(40):
        theta, phi = rng.uniform(0.0, np.pi / 2), rng.uniform(-np.pi, np.pi)
        assert float(np.abs(pkg.focus_delays(xyz, theta, phi, 1e7) - pkg.steering_delays(xyz, theta, phi)).max()) <= 1.1e-4
        for d in (0.05, 0.3, 2.0, 50.0, 1e6):
            tau = pkg.focus_delays(xyz, theta, phi, d)
            assert tau.min() == 0.0 and tau.max() <= aperture, (theta, phi, d, tau.max(), aperture)
    for d, fov in ((0.3, 180.0), (2.0, 90.0)):
        off, frac = pkg.build_focus_table(xyz, 10, 12, d, fov)
        assert off.shape == (120, xyz.shape[1]) and off.min() >= 0 and off.max() == 256 and frac.min() >= 0.0 and frac.max() < 1.0
        a, b = pkg.build_focus_table(xyz, 10, 12, d, fov, 0, 3), pkg.build_focus_table(xyz, 10, 12, d, fov, 3, 7)
        assert np.array_equal(np.concatenate([a[0], b[0]]), off) and np.array_equal(np.concatenate([a[1], b[1]]), frac)
        assert pkg.build_focus_table(xyz, 10, 12, d, fov, 4, 0)[0].shape == (0, xyz.shape[1])


def test_focused_pixel_equals_the_steered_direction(pkg):
    """A pixel of the focused table is focus_steer_table at that pixel's theta / phi (mimo.cpp:34-43)."""
    xyz = pkg.create_tiled_antenna(4, 1)
    rows, cols, fov, d = 6, 8, 120.0, 1.5
    off, frac = pkg.build_focus_table(xyz, rows, cols, d, fov)
    sep_r, sep_c = np.sin(np.deg2rad(fov) / 2) / (rows / 2.0), np.sin(np.deg2rad(fov) / 2) / (cols / 2.0)
    for r, c in ((0, 0), (2, 5), (5, 7)):
        y, x = r * sep_r - rows * sep_r / 2.0 + sep_r / 2.0, c * sep_c - cols * sep_c / 2.0 + sep_c / 2.0
        norm = np.sqrt(x * x + y * y)
        one = pkg.focus_steer_table(xyz, np.arcsin(min(norm, 1.0)), np.arctan2(y / norm, x / norm), d)
        assert np.array_equal(one[0][0], off[r * cols + c]) and np.array_equal(one[1][0], frac[r * cols + c])


def test_refusals(pkg):
    B = pkg.binding
    lib = B.load()
    xyz = pkg.create_antenna()
    INV = B.ERR_INVALID
    tau = np.full(64, 7.0, np.float32)
    off, frac = np.full((4, 64), 7, np.int32), np.full((4, 64), 7.0, np.float32)
    f32, i32, f64 = (lambda a: a.ctypes.data_as(B._f32p)), (lambda a: a.ctypes.data_as(B._i32p)), (lambda a: a.ctypes.data_as(B._f64p))
    ang = np.array([0.1, 0.2, 0.3, 0.4])
    for bad in (0.0, -1.0, -np.inf, np.nan):
        assert lib.awpu_hip_focus_delays(f32(xyz), 64, 0.3, 1.1, bad, f32(tau)) == INV
        assert lib.awpu_hip_focus_steer_table(f32(xyz), 64, f64(ang), f64(ang), f64(np.array([1.0, 2.0, bad, np.inf])), 4, i32(off), f32(frac)) == INV
        assert lib.awpu_hip_build_focus_table(f32(xyz), 64, 2, 2, 180.0, bad, 0, 2, i32(off), f32(frac)) == INV
        assert lib.awpu_hip_build_focus_table_device(0, f32(xyz), 64, 2, 2, 180.0, bad, 0, 2, i32(off), f32(frac)) == INV
    assert lib.awpu_hip_focus_delays(None, 64, 0.3, 1.1, 1.0, f32(tau)) == INV and lib.awpu_hip_focus_delays(f32(xyz), 0, 0.3, 1.1, 1.0, f32(tau)) == INV
    assert lib.awpu_hip_focus_steer_table(f32(xyz), 64, f64(ang), f64(ang), None, 4, i32(off), f32(frac)) == INV
    assert lib.awpu_hip_build_focus_table(f32(xyz), 64, 2, 2, 180.0, 1.0, 1, 2, i32(off), f32(frac)) == INV  # rows outside the grid
    assert lib.awpu_hip_build_focus_table_device(0, None, 64, 2, 2, 180.0, 1.0, 0, 2, i32(off), f32(frac)) == INV
    assert np.all(tau == 7.0) and np.all(off == 7) and np.all(frac == 7.0)  # nothing written
    # the calls that need a handle refuse a null one; range_pick its own arguments
    p, best = np.ones((2, 3), np.float32), np.zeros(2, B.RANGE_DTYPE)
    d3 = np.array([1.0, 2.0, 4.0])
    void = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.awpu_hip_range(None, None, f64(ang), f64(ang), 1, f64(d3), 3, f32(p), void(best)) == INV
    assert lib.awpu_hip_locate_blocks(None, None, 1032, 1, None, None, None, None, None, f64(d3), 3, void(best), None) == INV
    assert lib.awpu_hip_locate_samples(None, f32(p), 256, 1, None, None, None, None, None, f64(d3), 3, void(best), None) == INV
    assert lib.awpu_hip_locate_samples_device(None, None, 256, 1, None, None, None, None, None, f64(d3), 3, void(best), None, None) == INV
    assert lib.awpu_hip_range_pick(None, 2, f64(d3), 3, void(best)) == INV and lib.awpu_hip_range_pick(f32(p), 0, f64(d3), 3, void(best)) == INV
    assert lib.awpu_hip_range_pick(f32(p), 2, f64(d3), 0, void(best)) == INV and lib.awpu_hip_range_pick(f32(p), 2, f64(d3), 65, void(best)) == INV
    assert lib.awpu_hip_range_pick(f32(p), 2, f64(np.array([1.0, 0.0, 4.0])), 3, void(best)) == INV
    assert lib.awpu_hip_range_pick(f32(p), 2, f64(d3), 3, None) == INV


def test_focus_table_device_without_device(pkg):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the no-device path is exercised on CPU-only boxes")
    with pytest.raises(pkg.AwpuError) as ei:
        pkg.build_focus_table_device(pkg.create_antenna(), 8, 8, 2.0)
    assert ei.value.status == pkg.binding.ERR_NO_DEVICE


def test_range_pick(pkg):
    cand = pkg.range_candidates(np.inf, 1.0 / 3.0, 61)  # 1 / d = 0, 0.05, ..., 3
    u = np.linspace(0.0, 3.0, 61)
    assert np.isinf(cand[0]) and np.allclose(1.0 / cand[1:], u[1:], rtol=1e-15)
    # ties go to the lower index; equal powers everywhere: index 0, an end, unrefined -- and 1 / inf = 0 gives distance inf
    best = pkg.range_pick(np.ones((1, 61), np.float32), cand)[0]
    assert best["index"] == 0 and best["power"] == 1.0 and np.isinf(best["distance"])
    p = np.zeros(61, np.float32)
    p[[7, 30]] = 2.0
    best = pkg.range_pick(p, cand)[0]
    assert best["index"] == 7 and best["distance"] == 1.0 / (1.0 / cand[7])  # a - 2b + c < 0, a == c: delta 0
    # winners at either end are unrefined, whatever their neighbours
    p = np.linspace(1.0, 2.0, 61).astype(np.float32)
    best = pkg.range_pick(p, cand)[0]
    assert best["index"] == 60 and best["distance"] == 1.0 / (1.0 / cand[60])
    best = pkg.range_pick(p[::-1].copy(), cand)[0]
    assert best["index"] == 0 and np.isinf(best["distance"])
    best = pkg.range_pick(p[:0:-1].copy(), cand[1:])[0]  # (60 candidates from 20 m down)
    assert best["index"] == 0 and best["distance"] == cand[1]
    # an inf candidate as a neighbour: the winner at index 1 is refined towards u = 0
    best = pkg.range_pick(np.array([0.9, 1.0, 0.8], np.float32), cand[:3])[0]
    a, b, c = np.float64(np.float32(0.9)), 1.0, np.float64(np.float32(0.8))
    delta = 0.5 * (a - c) / (a - 2 * b + c)
    assert best["index"] == 1 and delta < 0 and best["distance"] == 1.0 / (u[1] + delta * (u[1] - 0.0)) > cand[1]
    # a plateau behind the winner: refined towards it (den = 0.5 - 2 + 1 < 0), never past half a step
    best = pkg.range_pick(np.array([0.5, 1.0, 1.0, 1.0, 0.5], np.float32), cand[10:15])[0]
    assert best["index"] == 1 and 1.0 / best["distance"] == u[11] + 0.5 * (u[12] - u[11])
    # den >= 0 gives no refinement.  An interior winner of finite non-negative powers beats its lower neighbour strictly and its
    # upper one at least by the tie, so den < 0 there; den >= 0 needs bit patterns outside that domain -- a negative power, whose
    # bits beat every positive one's: winner 1 of (1, -1, 2), den = 1 + 2 + 2
    best = pkg.range_pick(np.array([1.0, -1.0, 2.0], np.float32), cand[10:13])[0]
    assert best["index"] == 1 and best["power"] == -1.0 and best["distance"] == 1.0 / (1.0 / cand[11])
    # a parabola sampled on the uniform 1 / d grid (step h = 0.05) returns its vertex.  The powers are rounded to fp32: half an
    # ulp in [8, 16) is 4.8e-7, so 0.5 (a - c) is off by <= 4.8e-7 and den = -2 h^2 = -0.005 by <= 1.9e-6; with |delta| <= 0.5
    # that is <= 2.9e-4 of a step in delta, 1.45e-5 in u: the bound below is 2e-5
    for vertex in (0.5, 1.0 / 3.0, 1.2345, 2.93, 0.031):
        p = (10.0 - (u - vertex) ** 2).astype(np.float32)
        best = pkg.range_pick(p, cand)[0]
        assert best["index"] == int(np.argmax(p)) and abs(1.0 / best["distance"] - vertex) <= 2e-5, (vertex, best)
    # several sources at once, one row each
    rows = np.stack([(10.0 - (u - v) ** 2).astype(np.float32) for v in (0.5, 1.0, 2.0)])
    best = pkg.range_pick(rows, cand)
    assert list(best["index"]) == [10, 20, 40] and np.allclose(best["distance"], [2.0, 1.0, 0.5], rtol=1e-4)


def test_focusing_matters_on_the_oracle(pkg, oracle):
    """The 32 x 8 tile, a 32 x 32 grid at fov 180, a point source 2 m away at the synthetic direction: through the oracle's sweep
    the focused table's maximum is at source_pixel, and the plane-wave table keeps less than 0.5 of the focused power there
    (the numpy model of the issue: 0.09-0.10; 0.5 is the condition that focusing matters, not a measurement)."""
    S = pkg.synthetic
    spec = S.WorkloadSpec("tile 32 x 8 on 32 x 32", 4, 1, 32)
    xyz = S.geometry(spec)
    frame = S.make_point_frames(xyz, 1, 2.0)[0]
    focused = oracle.das_f32(frame, *pkg.build_focus_table(xyz, 32, 32, 2.0))
    plane = oracle.das_f32(frame, *S.delay_table(spec, xyz))
    r, c = S.source_pixel(spec)
    at = r * 32 + c
    print(f"focused maximum at {divmod(int(focused.argmax()), 32)}, source pixel {(r, c)}; plane / focused there = {plane[at] / focused[at]:.3f}")
    assert int(focused.argmax()) == at
    assert plane[at] < 0.5 * focused[at]


def test_range_kernels_compile_without_scratch(tmp_path, pkg):
    """range_kernel and range_pick_kernel for gfx950: no register spilled, no scratch (the candidates are indexed out of the kernel
    arguments, not out of a private copy), and at most 128 VGPRs -- four workgroups of four waves a SIMD set."""
    import re
    import subprocess
    from pathlib import Path

    repo = Path(__file__).resolve().parent.parent
    csrc = repo / "beamforming-lk_amd" / "csrc"
    out = tmp_path / "track_kernels.s"
    subprocess.run([pkg._build.hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{repo / 'include'}", f"-I{csrc}", "-S",
                    "--cuda-device-only", "-o", str(out), str(csrc / "track_kernels.hip")], check=True, capture_output=True)
    meta = {}
    for block in out.read_text().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1))
                      for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")}
    names = [n for n in meta if re.search(r"range_kernel|range_pick_kernel", n)]
    assert len(names) == 2, sorted(meta)
    for name in names:
        m = meta[name]
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_count"] <= 128, (name, m)
