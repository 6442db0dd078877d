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


def listen_host(oracle, steer_fn, snaps, theta, phi, spread, rate, steps, limit, index, impl="oracle", das_impl=None, reference=None):
    """MISOWorker::update (src/dsp/miso.cpp:27-55) for every snapshot of snaps [n_blocks, n_streams, hist], on the host: per
    block the reference power of the block's own snapshot (unless given), per listener `steps` gradient steps (track_host on
    Particle::beam over the mics `index`, in that order), then Particle::das where the listener then points.  The steps use
    `impl` (oracle | ref), the audio `das_impl` (default: the same).
    -> (audio [n, 256 * n_blocks], trail [n_blocks][n] of (theta, phi, state of the block's last step or None))."""
    das_impl = das_impl or impl
    n = len(theta)
    where = [(float(theta[l]), float(phi[l])) for l in range(n)]
    audio = np.empty((n, 256 * len(snaps)), np.float32)
    trail = []
    for k, snap in enumerate(snaps):
        ref_power = reference_power(snap) if reference is None else reference
        row = []
        for l in range(n):
            state = None
            if steps[l] > 0:
                state, _ = track_host(lambda off, frac: oracle.particle_beams(snap, off, frac, index=index, impl=impl)[0], steer_fn,
                                      *where[l], float(spread[l]), float(rate[l]), int(steps[l]), limit, ref_power)
                where[l] = (state["theta"], state["phi"])
            off, frac = steer_fn([where[l][0]], [where[l][1]])
            audio[l, 256 * k: 256 * (k + 1)] = oracle.particle_beams(snap, off, frac, index=index, impl=das_impl)[1][0]
            row.append((where[l][0], where[l][1], state))
        trail.append(row)
    return audio, trail


# ------------------------------------------------------------------------------------------------ ragged mic lists
# AWProcessingUnit::calibrate leaves an active-mic list that is shorter than the array and not in id order.  The lists the
# GPU tests (tests/test_gpu_active_mics.py) run the tracker, the listeners and the block runs on; seeded, and pinned by
# test_mic_list_premises below.  The element with the lowest delay of a direction is a corner of the array
# (MIN_HOLDERS): a list tells "minimum over every element" from "minimum over the active ones" only if it leaves them out.


def _shuffled(ids, seed):
    return np.random.default_rng(seed).permutation(np.asarray(list(ids), np.int32)).astype(np.int32)


MIN_HOLDERS = {64: (0, 7, 56, 63), 100: (0, 56, 63, 71, 95), 256: (0, 56, 199, 255), 512: (0, 199, 312, 511)}  # by element count
_INNER64 = [s for s in range(64) if s not in MIN_HOLDERS[64]]
ONE = np.asarray([37], np.int32)
THREE = np.asarray([60, 2, 33], np.int32)
FIFTEEN = _shuffled(_INNER64, 41)[:15]
SEVENTEEN = _shuffled(_INNER64, 41)[:17]
NO_CORNERS60 = np.asarray(_INNER64, np.int32)                      # ascending; 60 = 15 * 4 = 3 * 16 + 12
KEEP57_PERM = _shuffled([s for s in range(64) if s % 9 != 4], 42)  # the goldens' ragged list, shuffled; 57 = 14 * 4 + 1 = 3 * 16 + 9
TILED205 = _shuffled([s for s in range(256) if s not in MIN_HOLDERS[256]], 43)[:205]  # create_tiled_antenna(4, 1); 205 = 51 * 4 + 1
_ALL_BUT_THREE = [s for s in range(512) if s not in (0, 199, 511)]
TILED509 = np.asarray(_ALL_BUT_THREE[300:] + _ALL_BUT_THREE[:300], np.int32)          # create_tiled_antenna(4, 2); not ascending
CUT100_37 = _shuffled([s for s in range(100) if s not in MIN_HOLDERS[100]], 44)[:37]  # create_tiled_antenna(2, 1)'s first 100
MIC_LISTS = {"one": ONE, "three": THREE, "fifteen": FIFTEEN, "seventeen": SEVENTEEN, "no_corners60": NO_CORNERS60,
             "keep57_perm": KEEP57_PERM, "tiled205": TILED205, "tiled509": TILED509, "cut100_37": CUT100_37}
# by element count: the lists that leave out every element of MIN_HOLDERS (keep57_perm keeps all four, tiled509 keeps 312)
LISTS_WITHOUT_THE_HOLDERS = {64: ("one", "three", "fifteen", "seventeen", "no_corners60"), 100: ("cut100_37",), 256: ("tiled205",), 512: ()}


def min_holders(off, frac):
    """Per direction of a steering table over ALL elements: the ids of the elements whose delay is the minimum that
    steering_vector_spherical removes (delay 0: off 256, frac 0)."""
    zero = (np.asarray(off) == 256) & (np.asarray(frac) == 0.0)
    return [np.nonzero(row)[0] for row in zero]


def minimum_is_inactive(off, frac, index):
    """The premise of a test that claims to tell the minimum over every element from the minimum over the active ones: in
    every direction of the table no active mic has the lowest delay."""
    active = set(int(s) for s in index)
    return all(len(ids) > 0 and not active.intersection(ids.tolist()) for ids in min_holders(off, frac))


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


def seeded_directions(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.02, math.pi / 2, n), rng.uniform(0.0, 2 * math.pi, n)


@pytest.mark.parametrize("elements", sorted(MIN_HOLDERS))
def test_the_lowest_delay_sits_in_a_corner(pkg, elements):
    """32 seeded directions and their monopulse neighbours (both spreads): one element holds the lowest delay, and it is one of
    MIN_HOLDERS.  The `s % 9 != 4` list of the goldens keeps all four corners of the reference's array."""
    xyz = {64: lambda: pkg.create_antenna(), 100: lambda: np.ascontiguousarray(pkg.create_tiled_antenna(2, 1)[:, :100]),
           256: lambda: pkg.create_tiled_antenna(4, 1), 512: lambda: pkg.create_tiled_antenna(4, 2)}[elements]()
    assert xyz.shape == (3, elements)
    theta, phi = seeded_directions(32, 77)
    near = [d for t, p in zip(theta, phi) for s in (TRACKER_SPREAD, SEEKER_SPREAD) for d in quadrant(t, p, s, math.pi / 2)[1]]
    off, frac = pkg.steer_table(xyz, np.r_[theta, [t for t, _ in near]], np.r_[phi, [p for _, p in near]])
    holders = min_holders(off, frac)
    assert all(len(ids) == 1 for ids in holders)
    assert {int(ids[0]) for ids in holders} <= set(MIN_HOLDERS[elements])
    assert set(MIN_HOLDERS[64]) <= {s for s in range(64) if s % 9 != 4}
    for name in LISTS_WITHOUT_THE_HOLDERS[elements]:
        assert minimum_is_inactive(off, frac, MIC_LISTS[name]), name
    assert not minimum_is_inactive(off, frac, np.arange(elements))


def test_mic_lists_are_what_the_kernels_tails_need():
    """Lengths around the 4-wide and 16-wide loops of the beams, ids unique, and which lists are out of id order."""
    assert {k: v.size for k, v in MIC_LISTS.items()} == {"one": 1, "three": 3, "fifteen": 15, "seventeen": 17, "no_corners60": 60,
                                                         "keep57_perm": 57, "tiled205": 205, "tiled509": 509, "cut100_37": 37}
    for name, index in MIC_LISTS.items():
        assert index.dtype == np.int32 and np.unique(index).size == index.size, name
        ascending = bool((np.diff(index) > 0).all())
        assert ascending == (name in ("one", "no_corners60")), name
    assert np.array_equal(SEVENTEEN[:15], FIFTEEN) and sorted(KEEP57_PERM.tolist()) == [s for s in range(64) if s % 9 != 4]


@pytest.mark.parametrize("name", ["three", "fifteen", "seventeen", "keep57_perm"])
def test_mic_order_and_rows_change_the_beams(pkg, oracle, name):
    """The reference sums the mics in index[] order: on the synthetic frame a list and its sorted self give different beam
    samples, and reading row s instead of row index[s] changes them too.  So a GPU test on these lists is not vacuous."""
    index = MIC_LISTS[name]
    xyz = pkg.create_antenna()
    frame = pkg.synthetic.make_frames(xyz, 1, seed=1234)[0]
    off, frac = pkg.steer_table(xyz, *seeded_directions(32, 78))
    _, beams = oracle.particle_beams(frame, off, frac, index=index)
    _, ordered = oracle.particle_beams(frame, off, frac, index=np.sort(index))
    differing = int((beams.view(np.uint32) != ordered.view(np.uint32)).sum())
    print(f"{name}: {differing} of {beams.size} samples differ from the sorted list's")
    assert differing > beams.size // 8
    _, by_slot = oracle.particle_beams(frame, off, frac, index=np.arange(index.size))  # row s and delay s for index[s]
    assert int((beams.view(np.uint32) != by_slot.view(np.uint32)).sum()) > beams.size // 2


@pytest.mark.parametrize("name", ["keep57_perm", "three"])
def test_listen_host_on_the_oracle_and_the_reference(pkg, oracle, name):
    """listen_host on 6 blocks of a recording of the synthetic source, two tracking listeners and a fixed one on a ragged
    list: the trackers move and stay finite, a fixed listener's rows are Particle::das of the snapshots, the first tracking
    step is track_host's, and -- where the reference's delay() is built -- its audio is the oracle's bit for bit (the steps
    taken on the oracle's powers: the two agree on a beam's samples to the bit, on the 254-term power sum to rounding)."""
    index = MIC_LISTS[name]
    xyz = pkg.create_antenna()
    n_blocks = 6
    rec = pkg.synthetic.make_frames(xyz, 1, seed=1234, hist=1024 + 256 * n_blocks)[0]
    snaps = np.stack([rec[:, 256 * (k + 1): 256 * (k + 1) + 1024] for k in range(n_blocks)])
    steer = lambda t, p: pkg.steer_table(xyz, t, p)
    who = dict(theta=[0.5, 0.9, SOURCE[0] + 0.05], phi=[1.0, 4.0, SOURCE[1]], spread=[TRACKER_SPREAD, SEEKER_SPREAD, TRACKER_SPREAD],
               rate=[PARTICLE_RATE / 10] * 3, steps=[3, 0, 1])
    audio, trail = listen_host(oracle, steer, snaps, **who, limit=math.pi / 2, index=index)
    assert np.isfinite(audio).all() and all(math.isfinite(t) and math.isfinite(p) for row in trail for t, p, _ in row)
    assert (trail[-1][0][0], trail[-1][0][1]) != (0.5, 1.0) and trail[-1][1][:2] == (0.9, 4.0) and trail[-1][1][2] is None
    off, frac = steer([0.9], [4.0])
    for k in range(n_blocks):
        assert np.array_equal(audio[1, 256 * k: 256 * (k + 1)], oracle.particle_beams(snaps[k], off, frac, index=index)[1][0])
    first, _ = track_host(lambda o, f: oracle.particle_beams(snaps[0], o, f, index=index)[0], steer, 0.5, 1.0, TRACKER_SPREAD,
                          PARTICLE_RATE / 10, 3, math.pi / 2, reference_power(snaps[0]))
    assert (first["theta"], first["phi"]) == trail[0][0][:2]
    if oracle._in_reference_tree("src/dsp/delay.cpp") and not oracle.ref_available():
        oracle.build(ref=True)
    if oracle.ref_available():
        heard, _ = listen_host(oracle, steer, snaps, **who, limit=math.pi / 2, index=index, das_impl="ref")
        assert heard.tobytes() == audio.tobytes()
        _, by_ref = listen_host(oracle, steer, snaps, **who, limit=math.pi / 2, index=index, impl="ref")
        assert all(angle(a[:2], b[:2]) < 1e-6 for ra, rb in zip(trail, by_ref) for a, b in zip(ra, rb))


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
