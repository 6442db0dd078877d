"""Particle tracking (include/awpu_hip_track.h) on a box without a GPU: the three entry points are exported and refuse
null arguments, the kernels compile for gfx950 without spills, and a float64 restatement of the reference's direction
arithmetic -- Spherical::quadrant, GradientParticle::step, Particle::step, normalizeSpherical -- that the GPU tests
compare the device against.  The same restatement, driven by the reference's own compiled delay() on the synthetic
9 kHz source, pins the convergence parameters the GPU test uses."""
import ctypes as C
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "beamforming-lk_amd" / "csrc"

# ------------------------------------------------------------------------------------------------ the restatement

Q_DEG = (45.0, 315.0, 225.0, 135.0)  # Spherical::quadrant's offsets q1..q4, src/geometry/geometry.cpp:184-187
TRACKER_SPREAD = math.radians(2.0)  # gradient_ascend.h TRACKER_SPREAD
SEEKER_SPREAD = math.radians(7.0)   # gradient_ascend.h SEEKER_SPREAD
PARTICLE_RATE = 5e-4                # gradient_ascend.h PARTICLE_RATE

# Convergence on the synthetic source (synthetic.make_frames(create_antenna(), 1, seed=1234)[0], source at 20 deg, 35 deg),
# pinned by test_single_tracker_converges_on_the_reference_delay below.  The reference's quadrant monopulse does NOT settle
# on the beam's peak: its four neighbours are centred on a point mirrored in phi (rotateTo multiplies row vectors by
# Ry Rz, i.e. rotates by the transpose), and the balance point of the four powers lies 3.03 deg from the source for every
# spread (0.5 .. 7 deg), rate (5e-5 .. 2.5e-4) and start tried.  What is pinned is therefore that fixed point.
CONVERGE_START = (math.radians(28.0), math.radians(30.0))
CONVERGE_RATE = PARTICLE_RATE / 2
CONVERGE_STEPS = 40
CONVERGE_FIXED_POINT = (math.radians(18.2712), math.radians(27.3873))
SOURCE = (math.radians(20.0), math.radians(35.0))


def normalize(theta, phi, limit):
    """normalizeSpherical (particle.h:24-27): wrapAngle (geometry.cpp:11-20) then clip (:7-9)."""
    r = math.fmod(phi, 2.0 * math.pi)
    phi = 2.0 * math.pi + r if r < 0.0 else r
    return max(0.0, min(theta, limit)), phi


def quadrant(theta, phi, spread, limit):
    """Spherical::quadrant (geometry.cpp:181-216) + normalizeSpherical of each neighbour (gradient_ascend.cpp:18-28)
    -> (the particle's theta after quadrant's side effect, [(theta, phi)] * 4)."""
    rot = theta
    if rot + spread > math.pi / 2.0:
        rot -= spread
        theta -= spread / 2.0
    st, ct, sp, cp = math.sin(rot), math.cos(rot), math.sin(phi), math.cos(phi)
    # rotateTo (geometry.cpp:120-142): row vector times Ry Rz = {{ct cp, -ct sp, st}, {sp, cp, 0}, {-st cp, st sp, ct}}
    r00, r01, r20, r21 = ct * cp, -(ct * sp), -st * cp, st * sp
    near = []
    for q in Q_DEG:
        a = q * (math.pi / 180.0)
        v0, v1, v2 = 1.0 * math.sin(spread) * math.cos(a), 1.0 * math.sin(spread) * math.sin(a), 1.0 * math.cos(spread)
        x = v0 * r00 + v1 * sp + v2 * r20
        y = v0 * r01 + v1 * cp + v2 * r21
        z = v0 * st + v2 * ct
        near.append(normalize(math.acos(z), math.atan2(y, x) - math.pi, limit))
    return theta, near


def gradient(power, reference):
    """gradient_ascend.cpp:53-78 (quadrant mode, RELATIVE 1) -> (error, grad_theta, grad_phi, radius)."""
    q1, q2, q3, q4 = (float(v) for v in power)
    total = q1 + q2 + q3 + q4
    d_phi = (q1 + q4) - (q2 + q3)
    d_theta = (q3 + q4) - (q1 + q2)
    error = float(np.float32((abs(d_phi) + abs(d_theta)) / total))
    return error, d_theta / reference, d_phi / reference, total / 4


def particle_step(theta, phi, rate, grad_theta, grad_phi, limit):
    """Particle::step (particle.cpp:22-27): phi's step uses the updated theta."""
    theta = theta + rate * grad_theta
    phi = phi + (rate * grad_phi) / math.sin(1e-9 + theta)
    return normalize(theta, phi, limit)


def reference_power(frame):
    """The block's reference power (gradient_ascend.cpp:301-313): stream 0's zero-delay window, fp32 in sample order."""
    out = np.asarray(frame[0, 256:512], np.float32)
    acc = np.float32(0.0)
    for i in range(1, 255):
        ma = np.float32(out[i] * np.float32(0.5)) - np.float32(np.float32(0.25) * np.float32(out[i + 1] + out[i - 1]))
        acc = np.float32(acc + np.float32(ma * ma))
    return float(np.float32(acc / np.float32(254.0)))


def track_host(beams_fn, steer_fn, theta, phi, spread, rate, steps, limit, reference):
    """`steps` gradient steps of one particle, composed on the host: quadrant -> steer_fn(thetas, phis) -> beams_fn(off,
    frac) -> gradient -> step.  Returns the state after the last step (and the trajectory of directions)."""
    state = None
    path = []
    for _ in range(steps):
        theta, near = quadrant(theta, phi, spread, limit)
        off, frac = steer_fn([t for t, _ in near], [p for _, p in near])
        power = beams_fn(off, frac)
        error, g_theta, g_phi, radius = gradient(power, reference)
        theta, phi = particle_step(theta, phi, rate, g_theta, g_phi, limit)
        state = dict(theta=theta, phi=phi, error=error, grad_theta=g_theta, grad_phi=g_phi, radius=radius,
                     power=np.asarray(power, np.float32))
        path.append((theta, phi))
    return state, path


def angle(a, b):
    """Spherical::angle (geometry.cpp:109-118)."""
    s1, s2 = math.sin(math.pi / 2 - a[0]), math.sin(math.pi / 2 - b[0])
    c1, c2 = math.cos(math.pi / 2 - a[0]), math.cos(math.pi / 2 - b[0])
    return math.acos(min(1.0, s1 * s2 + c1 * c2 * math.cos(a[1] - b[1])))


# ------------------------------------------------------------------------------------------------ restatement checks


def test_quadrant_at_the_pole():
    """theta = 0: the neighbours sit at theta = spread, phi = q + 180 deg (atan2(y, x) - pi, wrapped)."""
    s = math.radians(3.0)
    theta, near = quadrant(0.0, 0.0, s, math.pi / 2)
    assert theta == 0.0
    for (t, p), q in zip(near, Q_DEG):
        assert abs(t - s) < 1e-12
        assert abs(p - math.radians((q + 180.0) % 360.0)) < 1e-12


def test_quadrant_moves_the_particle_near_the_horizon():
    """theta + spread > pi/2: the particle's own theta drops by spread / 2 and the neighbours are built around theta - spread."""
    s, limit = math.radians(2.0), math.pi / 2
    theta0 = math.pi / 2 - math.radians(1.0)
    theta, near = quadrant(theta0, 0.3, s, limit)
    assert theta == theta0 - s / 2.0
    _, ref_near = quadrant(theta0 - s, 0.3, s, limit)  # the same rotation, without the side effect
    assert near == ref_near
    assert all(t <= limit for t, _ in near)
    theta, _ = quadrant(math.pi / 2 - math.radians(3.0), 0.3, s, limit)  # below the threshold: untouched
    assert theta == math.pi / 2 - math.radians(3.0)


def test_quadrant_neighbours_straddle_the_clip():
    """Neighbours are clipped to [0, limit] (normalizeSpherical with the particle's thetaLimit)."""
    _, near = quadrant(math.radians(30.0), 1.0, math.radians(7.0), math.radians(31.0))
    assert max(t for t, _ in near) == math.radians(31.0)
    assert min(t for t, _ in near) < math.radians(31.0)


def test_step_wraps_phi_through_zero_and_two_pi():
    limit = math.pi / 2
    theta, phi = particle_step(0.5, 2.0 * math.pi - 1e-3, 1.0, 0.0, 2e-3 * math.sin(1e-9 + 0.5), limit)
    assert theta == 0.5 and abs(phi - 1e-3) < 1e-12
    theta, phi = particle_step(0.5, 1e-3, 1.0, 0.0, -2e-3 * math.sin(1e-9 + 0.5), limit)
    assert abs(phi - (2.0 * math.pi - 1e-3)) < 1e-12
    theta, phi = particle_step(0.1, 0.0, 1.0, -0.3, 0.0, limit)  # theta clipped at 0, then phi's step divides by sin(1e-9)
    assert theta == 0.0 and phi == 0.0
    theta, _ = particle_step(1.5, 0.0, 1.0, 0.2, 0.0, limit)
    assert theta == limit


def test_gradient_quadrant_signs():
    error, g_t, g_p, radius = gradient([1.0, 2.0, 3.0, 4.0], 0.5)
    assert (g_t, g_p, radius) == ((3.0 + 4.0 - 1.0 - 2.0) / 0.5, (1.0 + 4.0 - 2.0 - 3.0) / 0.5, 2.5)
    assert error == pytest.approx(0.4)


def test_single_tracker_converges_on_the_reference_delay(pkg, oracle):
    """The restatement driven by the reference's own delay() (oracle/_ref, when the reference tree was there to build it;
    the oracle's restatement of Particle::beam otherwise -- the two are bit-identical, tests/test_oracle_golden.py) on
    the synthetic source: one tracker from CONVERGE_START settles on CONVERGE_FIXED_POINT, 3.03 deg from the source."""
    xyz = pkg.create_antenna()
    frame = pkg.synthetic.make_frames(xyz, 1, seed=1234)[0]
    reference = reference_power(frame)
    # the reference's own delay() whenever its tree is there to compile it from (oracle/_ref); a checkout without the tree
    # (it may not be readable to the user that runs the tests) has the oracle's restatement of Particle::beam only
    if oracle._in_reference_tree("src/dsp/delay.cpp") and not oracle.ref_available():
        oracle.build(ref=True)
    if oracle._in_reference_tree("src/dsp/delay.cpp"):
        assert oracle.ref_available(), "the reference tree is present but oracle/_ref was not built from it"
    impls = ["oracle"] + (["ref"] if oracle.ref_available() else [])
    finals = []
    for impl in impls:
        state, path = track_host(lambda off, frac: oracle.particle_beams(frame, off, frac, impl=impl)[0],
                                 lambda t, p: pkg.steer_table(xyz, t, p), *CONVERGE_START, TRACKER_SPREAD, CONVERGE_RATE,
                                 CONVERGE_STEPS, math.pi / 2, reference)
        finals.append((state["theta"], state["phi"]))
        assert angle(path[-1], CONVERGE_FIXED_POINT) < math.radians(0.01), [math.degrees(v) for v in path[-1]]
        assert angle(path[-1], path[-2]) < math.radians(1e-3)  # settled
        assert math.radians(2.9) < angle(path[-1], SOURCE) < math.radians(3.2)
        assert angle(CONVERGE_START, SOURCE) > math.radians(8.0)  # it did travel
    assert all(angle(f, finals[0]) < 1e-6 for f in finals)  # (their powers agree to rounding, the beams bit for bit)


# ------------------------------------------------------------------------------------------------ the library


def test_track_symbols_exported(pkg):
    lib = pkg.binding.load()
    for name in ("awpu_hip_set_antenna", "awpu_hip_steer_table_device", "awpu_hip_track"):
        assert hasattr(lib, name), name
    assert set(pkg.binding.TRACK_SYMBOLS) == {"awpu_hip_set_antenna", "awpu_hip_steer_table_device", "awpu_hip_track"}
    assert not set(pkg.binding.TRACK_SYMBOLS) & set(pkg.binding.EXPORTED_SYMBOLS)
    assert lib.awpu_hip_abi_version() == 4
    header = (REPO / "include" / "awpu_hip_track.h").read_text()
    assert '#include "awpu_hip.h"' in header
    assert C.sizeof(pkg.binding.Particle) == 80


def test_track_entry_points_refuse_null_arguments(pkg):
    """A null handle or null buffers give a negative status without being dereferenced (a dereference would crash)."""
    lib = pkg.binding.load()
    xyz = np.zeros((3, 64), np.float32)
    d = np.zeros(4, np.float64)
    off = np.zeros(256, np.int32)
    frac = np.zeros(256, np.float32)
    parts = (pkg.binding.Particle * 2)()
    dp = C.POINTER(C.c_double)
    fp = frac.ctypes.data_as(C.POINTER(C.c_float))
    ip = off.ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.awpu_hip_set_antenna(None, xyz.ctypes.data_as(C.POINTER(C.c_float)), 64) == pkg.binding.ERR_INVALID
    assert lib.awpu_hip_set_antenna(None, None, 64) == pkg.binding.ERR_INVALID
    assert lib.awpu_hip_steer_table_device(None, d.ctypes.data_as(dp), d.ctypes.data_as(dp), 4, ip, fp) == pkg.binding.ERR_INVALID
    assert lib.awpu_hip_steer_table_device(None, None, None, 4, None, None) == pkg.binding.ERR_INVALID
    assert lib.awpu_hip_track(None, None, parts, 2, 1.0, 0.0, None, None) == pkg.binding.ERR_INVALID
    assert lib.awpu_hip_track(None, None, None, 2, 1.0, 0.0, None, None) == pkg.binding.ERR_INVALID


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


# gradient_track_kernel's fp64 libm calls (sincos, acos, atan2, fmod) keep their constants and branch masks in scalar
# registers, and the compiler parks 6 of those across the step loop in VGPR lanes (v_writelane / v_readlane: no memory
# traffic, no scratch).  That count is pinned, so that any growth is seen.
TRACK_SGPR_SPILLS_ACCEPTED = {"gradient_track_kernel": 6, "steer_table_kernel": 0}


def test_track_kernels_compile_without_scratch(track_metadata):
    """gradient_track_kernel and steer_table_kernel: no register spilled to memory, no scratch, SGPR spills into VGPR lanes
    no more than pinned above."""
    names = {n for n in track_metadata if re.search(r"gradient_track_kernel|steer_table_kernel", n)}
    assert len(names) == 2, sorted(track_metadata)
    for name in names:
        m = track_metadata[name]
        assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_count"] <= 256, (name, m)
        short = next(k for k in TRACK_SGPR_SPILLS_ACCEPTED if k in name)
        assert m["sgpr_spill_count"] <= TRACK_SGPR_SPILLS_ACCEPTED[short], (name, m)


def build_spherical_gradient(pkg, out_dir):
    """g++ build of the SphericalGradientHip driver (tests/host/test_spherical_gradient.cpp) against libawpu_hip.so."""
    pkg.binding.load()  # (builds the library when it is stale)
    pkgdir = REPO / "beamforming-lk_amd"
    exe = Path(out_dir) / "test_spherical_gradient"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    f"-I{REPO / 'include'}", f"-I{pkgdir / 'host'}", str(REPO / "tests" / "host" / "test_spherical_gradient.cpp"),
                    str(pkgdir / "host" / "spherical_gradient_hip.cpp"), f"-L{pkgdir}", "-lawpu_hip", "-L/opt/rocm/lib", "-lamdhip64",
                    f"-Wl,-rpath,{pkgdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True, capture_output=True, text=True)
    return exe


def test_spherical_gradient_mirror_builds_and_refuses_without_a_device(pkg, tmp_path):
    """SphericalGradientHip builds with g++ against the library; with no gfx950 device its constructor throws -- there is
    no CPU path behind it."""
    import torch

    exe = build_spherical_gradient(pkg, tmp_path)
    if torch.cuda.is_available():
        return  # a GPU is present: tests/test_gpu_tracker.py runs the mirror on it
    out = subprocess.run([str(exe), "--nogpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "refused:" in out.stdout and "no CPU path" in out.stdout
