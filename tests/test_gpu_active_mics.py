"""The tracker, the listeners and the block / listen / watch runs on the active-mic lists AWProcessingUnit::calibrate leaves:
shorter than the array and not in id order (the lists of test_tracker_cpu: lengths around the 4-wide and 16-wide loops of the
beams, with and without the corner elements that hold a direction's lowest delay).  Every claim is anchored on the CPU: the
oracle's Particle::beam / Particle::das with index= (bit-identical to the reference's compiled delay(), which is used as well
where it is built), the fp64 restatement of the direction arithmetic (test_tracker_cpu), the host steer_table.  Bounds are
the project's own: bytes for beam samples and for runs against their definitions, 2e-6 on beam powers against the reference
(the order of the 254-term power sum is not pinned), 1e-12 on the fp64 step arithmetic, 1e-6 on the reference power, the flat
1e-5 of util.parity_report on heatmaps."""
import math

import numpy as np
import pytest

import test_tracker_cpu as R
import util
from test_gpu_blocks import chunked_process, recording, snapshots
from test_gpu_blocks import engine as sweep_engine
from test_gpu_listen import B, fields, listen_engine, listeners, per_block_loop, prime, same, wire_recording
from test_gpu_parity import check_full_grid
from test_gpu_tracker import _seeded_particles, cut_antenna
from test_gpu_watch import colour_table, compose

pytestmark = pytest.mark.gpu

LIMIT = math.pi / 2
MISO_LIMIT = 90.0  # MISOWorker hands its fov in DEGREES to thetaLimit (src/dsp/miso.cpp:6): theta is never clipped
L = R.MIC_LISTS
OTHER57 = R._shuffled([s for s in range(64) if s % 9 != 2], 45)  # as long as keep57_perm, other ids
INNER16 = R._shuffled([8 * r + c for r in range(2, 6) for c in range(2, 6)], 46)  # the middle of the array: a shorter delay window
ANTENNAS = {64: lambda pkg: pkg.create_antenna(), 100: lambda pkg: cut_antenna(pkg), 256: lambda pkg: pkg.create_tiled_antenna(4, 1),
            512: lambda pkg: pkg.create_tiled_antenna(4, 2)}


def impls(oracle):
    return ["oracle"] + (["ref"] if oracle.ref_available() else [])


def track_engine(pkg, xyz, index, n_streams=None, hist=1024):
    eng = pkg.Engine(n_pixels=16, n_streams=n_streams or xyz.shape[1], hist=hist)
    eng.set_antenna(xyz)
    eng.set_active_mics(index)
    return eng


def frame_for(pkg, n_streams, hist=1024, seed=1234):
    """The synthetic source + noise on n_streams streams (the antenna's elements are the first of them)."""
    full = {64: (1, 1), 100: (2, 1), 128: (2, 1), 256: (4, 1), 512: (4, 2)}[n_streams]
    return np.ascontiguousarray(pkg.synthetic.make_frames(pkg.create_tiled_antenna(*full), 1, seed=seed, hist=hist)[0][:n_streams])


def order_matters(oracle, frame, off, frac, index):
    """The premise of an order-sensitive check: the oracle's beams for the list and for its sorted self differ."""
    a = oracle.particle_beams(frame, off, frac, index=index)[1]
    b = oracle.particle_beams(frame, off, frac, index=np.sort(index))[1]
    return a.tobytes() != b.tobytes()


def check_steps_against_the_cpu(pkg, oracle, xyz, frame, index, before, after, limit, reference, premise):
    """One gradient step of every particle, piece by piece.  `before`, `after`: PARTICLE_DTYPE records around the step;
    `reference`: the power the gradient was divided by, or None = not known (the run took it from the snapshot): then the
    one the gradients imply is held against stream 0's, within the 1e-6 of test_reference_on_device_and_ring.
      neighbours + steering   R.quadrant on the direction before, the host steer_table over ALL elements
      beams                   the four powers against the oracle's Particle::beam on `index`, util.power_rel_err < 2e-6
      gradient + step         R.gradient / R.particle_step of the GPU's own four powers, the 1e-12 bounds of
                              test_gpu_tracker.test_one_step_equals_the_host_composition
    `premise`: assert that no active mic holds a neighbour's lowest delay.  -> the neighbours' tables (off, frac) of every particle."""
    tables = []
    stream0 = R.reference_power(frame)
    for k in range(before.size):
        th, near = R.quadrant(float(before["theta"][k]), float(before["phi"][k]), float(before["spread"][k]), limit)
        off, frac = pkg.steer_table(xyz, [t for t, _ in near], [p for _, p in near])
        tables.append((off, frac))
        if premise:
            assert R.minimum_is_inactive(off, frac, index), k
        want_power = oracle.particle_beams(frame, off, frac, index=index)[0]
        got_power = after["power"][k]
        err = util.power_rel_err(got_power, want_power)
        assert err < 2e-6, (k, err, got_power, want_power)
        ref = reference
        if ref is None:  # (d / ref = g: the reference the device divided by, from the larger of the two gradients)
            q1, q2, q3, q4 = (float(v) for v in got_power)
            d, g = max((((q3 + q4) - (q1 + q2)), float(after["grad_theta"][k])), (((q1 + q4) - (q2 + q3)), float(after["grad_phi"][k])),
                       key=lambda dg: abs(dg[0]))
            assert d != 0.0 and g != 0.0, k
            ref = d / g
            assert abs(ref - stream0) <= 1e-6 * stream0, (k, ref, stream0)
        error, g_t, g_p, radius = R.gradient(got_power, ref)
        t1, p1 = R.particle_step(th, float(before["phi"][k]), float(before["rate"][k]), g_t, g_p, limit)
        assert abs(after["theta"][k] - t1) < 1e-12 and abs(after["phi"][k] - p1) < 1e-12, (k, after["theta"][k], t1, after["phi"][k], p1)
        for name, want in (("grad_theta", g_t), ("grad_phi", g_p), ("radius", radius), ("error", error)):
            assert abs(after[name][k] - want) <= 1e-12 * max(abs(want), 1e-300) + (1e-7 * abs(want) if name == "error" else 0), (k, name)
    return tables


def check_das_against_the_cpu(pkg, oracle, xyz, frame, index, where, rows, premise=False):
    """rows [n, 256] = Particle::das on `index` at where's directions, byte for byte: the oracle, and the reference's delay()."""
    off, frac = pkg.steer_table(xyz, where["theta"], where["phi"])
    if premise:
        assert R.minimum_is_inactive(off, frac, index)
    for impl in impls(oracle):
        want = oracle.particle_beams(frame, off, frac, index=index, impl=impl)[1]
        assert same(np.ascontiguousarray(rows), want), impl
    return off, frac


def particles(pkg, theta, phi, spread, rate=R.PARTICLE_RATE, steps=1):
    p = np.zeros(len(theta), pkg.binding.PARTICLE_DTYPE)
    p["theta"], p["phi"], p["spread"], p["rate"], p["steps"] = theta, phi, spread, rate, steps
    return p


# ------------------------------------------------------------------------------------------------ 1. one tracker step

TRACK_CASES = [(64, "one"), (64, "three"), (64, "fifteen"), (64, "seventeen"), (64, "no_corners60"), (64, "keep57_perm"), (256, "tiled205")]


@pytest.mark.parametrize("elements,name", TRACK_CASES)
@pytest.mark.parametrize("limit", [LIMIT, MISO_LIMIT], ids=["limit_half_pi", "limit_as_miso"])
def test_one_step_piece_by_piece_against_the_cpu(pkg, oracle, elements, name, limit):
    """32 seeded particles with the corner cases of test_gpu_tracker (theta 0, theta either side of pi/2 - spread, phi at 0 and
    2 pi), one step.  With MISO's limit of 90.0 four more sit within 0.02 of the horizon and stay unclipped."""
    import torch

    index = L[name]
    xyz = ANTENNAS[elements](pkg)
    frame = frame_for(pkg, elements)
    d_frame = torch.from_numpy(frame).cuda()
    theta, phi, spread = _seeded_particles(32, 11)
    if limit == MISO_LIMIT:
        theta[8:12] = LIMIT - np.asarray([0.01, 0.002, 0.015, 0.0])
    before = particles(pkg, theta, phi, spread)
    premise = name in R.LISTS_WITHOUT_THE_HOLDERS[elements]
    with track_engine(pkg, xyz, index) as eng:
        given = R.reference_power(frame)
        got = eng.track(before, None, None, None, None, limit, given, d_frame.data_ptr(), want_beams=True)
        assert got.reference == given
        tables = check_steps_against_the_cpu(pkg, oracle, xyz, frame, index, before, got.particles, limit, given, premise)
        check_das_against_the_cpu(pkg, oracle, xyz, frame, index, got.particles, got.beams)
        if index.size > 1 and not (np.diff(index) > 0).all():
            assert any(order_matters(oracle, frame, off, frac, index) for off, frac in tables)
        if limit == MISO_LIMIT:  # (quadrant's side effect moved them down by spread / 2 first: below pi / 2 the two limits do the same)
            near = particles(pkg, [LIMIT - 0.01], [1.0], [R.TRACKER_SPREAD])
            moved = eng.track(near, None, None, None, None, limit, given, d_frame.data_ptr())
            again = eng.track(near, None, None, None, None, LIMIT, given, d_frame.data_ptr())
            assert same(moved.particles, again.particles) and moved.theta[0] < LIMIT
        # the reference power on the device: stream 0's, whether mic 0 is active or not
        own = eng.track(before[:3], None, None, None, None, limit, None, d_frame.data_ptr())
        assert abs(own.reference - given) <= 1e-6 * given
        check_steps_against_the_cpu(pkg, oracle, xyz, frame, index, before[:3], own.particles, limit, own.reference, premise)


def test_theta_beyond_the_horizon_is_not_clipped_by_misos_limit(pkg, oracle):
    """A particle that a large step carries past pi / 2: with MISO's 90.0 its theta stays there (and the CPU restatement agrees),
    with pi / 2 it is clipped."""
    import torch

    index = L["no_corners60"]
    xyz = pkg.create_antenna()
    frame = frame_for(pkg, 64)
    d_frame = torch.from_numpy(frame).cuda()
    given = R.reference_power(frame)
    before = particles(pkg, [LIMIT - 0.2] * 4, [0.3, 1.9, 3.5, 5.1], [R.SEEKER_SPREAD] * 4, rate=[0.5, -0.5, 2.0, -2.0])
    with track_engine(pkg, xyz, index) as eng:
        free = eng.track(before, None, None, None, None, MISO_LIMIT, given, d_frame.data_ptr(), want_beams=True)
        held = eng.track(before, None, None, None, None, LIMIT, given, d_frame.data_ptr())
    check_steps_against_the_cpu(pkg, oracle, xyz, frame, index, before, free.particles, MISO_LIMIT, given, True)
    check_steps_against_the_cpu(pkg, oracle, xyz, frame, index, before, held.particles, LIMIT, given, True)
    check_das_against_the_cpu(pkg, oracle, xyz, frame, index, free.particles, free.beams)
    assert free.theta.max() > LIMIT and held.theta.max() == LIMIT


@pytest.mark.parametrize("elements,n_streams,name", [(512, 512, "tiled509"), (100, 128, "cut100_37"), (100, 100, "cut100_37")])
def test_one_step_on_other_element_counts(pkg, oracle, elements, n_streams, name):
    """512 elements: a second trip of the loops over the elements and over the mics; 100 elements (of 128 or 100 streams): the
    second wave half idle, the third and fourth idle."""
    import torch

    index = L[name]
    xyz = ANTENNAS[elements](pkg)
    frame = frame_for(pkg, n_streams)
    d_frame = torch.from_numpy(frame).cuda()
    theta, phi, spread = _seeded_particles(16, 13)
    before = particles(pkg, theta, phi, spread)
    given = R.reference_power(frame)
    with track_engine(pkg, xyz, index, n_streams=n_streams) as eng:
        got = eng.track(before, None, None, None, None, LIMIT, given, d_frame.data_ptr(), want_beams=True)
    tables = check_steps_against_the_cpu(pkg, oracle, xyz, frame, index, before, got.particles, LIMIT, given, name == "cut100_37")
    check_das_against_the_cpu(pkg, oracle, xyz, frame, index, got.particles, got.beams)
    assert any(order_matters(oracle, frame, off, frac, index) for off, frac in tables)


@pytest.mark.parametrize("hist", [513, 640])
def test_one_step_on_other_frame_pitches(pkg, oracle, hist):
    """A d_frame's rows are cfg.hist floats apart: the shortest history a steered delay fits in, and one between it and 1024."""
    import torch

    index = L["keep57_perm"]
    xyz = pkg.create_antenna()
    frame = frame_for(pkg, 64, hist=hist)
    assert frame.shape == (64, hist)
    d_frame = torch.from_numpy(frame).cuda()
    theta, phi, spread = _seeded_particles(16, 14)
    before = particles(pkg, theta, phi, spread)
    given = R.reference_power(frame)
    with track_engine(pkg, xyz, index, hist=hist) as eng:
        got = eng.track(before, None, None, None, None, LIMIT, None, d_frame.data_ptr(), want_beams=True)
    assert abs(got.reference - given) <= 1e-6 * given
    check_steps_against_the_cpu(pkg, oracle, xyz, frame, index, before, got.particles, LIMIT, got.reference, False)
    check_das_against_the_cpu(pkg, oracle, xyz, frame, index, got.particles, got.beams)


# ------------------------------------------------------------------------------------------------ 2. listening


@pytest.fixture(scope="module")
def recordings(oracle):
    """16 blocks of zero-mean samples on the wire, unpacked for 64 and for 256 streams, and their snapshots."""
    wire, s256 = wire_recording(oracle, 16, 256, seed=41)
    out = {}
    for n in (64, 256):
        samples = np.ascontiguousarray(s256[:n])
        out[n] = (wire, samples, snapshots(samples))
    assert same(out[64][1], wire_recording(oracle, 16, 64, seed=41)[1])
    return out


@pytest.mark.parametrize("elements,name", [(64, "three"), (64, "seventeen"), (64, "keep57_perm"), (256, "tiled205")])
def test_listening_equals_the_per_block_loop(pkg, recordings, elements, name):
    """The definition, bit for bit: 12 blocks after a 4-block primer in pieces of 4, 6 listeners (steps 0, 3, 5; two spreads)."""
    wire = recordings[elements][0]
    xyz = ANTENNAS[elements](pkg)
    p0 = listeners(pkg, 6, 3, [0, 3, 5, 0, 5, 3])
    with listen_engine(pkg, xyz, 4, index=L[name]) as eng, listen_engine(pkg, xyz, 4, index=L[name]) as loop:
        prime(eng, wire)
        prime(loop, wire)
        want_audio, want_trail, want_p = per_block_loop(loop, wire[4 * B:], 12, p0)
        assert np.isfinite(want_p["theta"]).all() and np.isfinite(want_p["phi"]).all() and np.isfinite(want_audio).all()
        moving = [1, 2, 4, 5]
        assert all(want_trail[0]["theta"][l] != p0["theta"][l] and want_trail[-1]["theta"][l] != want_trail[0]["theta"][l] for l in moving)
        got = eng.listen_blocks(wire[4 * B: 16 * B], p0, None, None, None, None, LIMIT)
        assert same(got.audio, want_audio)
        assert same(got.trail, want_trail)
        assert same(got.listeners, want_p)
        assert same(eng.ring_snapshot(), loop.ring_snapshot())


@pytest.mark.parametrize("dc", [0, 1 << 21])
@pytest.mark.parametrize("name", ["one", "fifteen", "seventeen", "keep57_perm"])
def test_fixed_listeners_on_ragged_lists_equal_the_reference_delay(pkg, oracle, name, dc):
    """Every audio row of a fixed listener is Particle::das of that block's snapshot over the list, in the list's order: 1 and
    15 mics (the 16-wide loop never runs), 17 (once, and one mic), 57 (three times, and nine).  Zero-mean samples and samples
    biased by 0.25 of full scale."""
    index = L[name]
    xyz = pkg.create_antenna()
    wire, samples = wire_recording(oracle, 8, 64, seed=23, dc=dc)
    snaps = snapshots(samples)
    p0 = listeners(pkg, 5, 8, [0])
    off, frac = pkg.steer_table(xyz, p0["theta"], p0["phi"])
    if name in R.LISTS_WITHOUT_THE_HOLDERS[64]:
        assert R.minimum_is_inactive(off, frac, index)
    if index.size > 1:
        assert order_matters(oracle, snaps[5], off, frac, index)
    with listen_engine(pkg, xyz, 4, index=index) as eng:
        got = eng.listen_blocks(wire, *fields(p0), LIMIT)
    assert same(got.listeners, p0) and same(got.trail, np.stack([p0] * 8))
    for k in range(8):
        for impl in impls(oracle):
            _, want = oracle.particle_beams(snaps[k], off, frac, index=index, impl=impl)
            assert same(got.audio[:, 256 * k: 256 * (k + 1)], want), (k, impl)


def check_tracking_listeners_block_by_block(pkg, oracle, xyz, snaps, index, p0, got, reference, premise):
    """Teacher-forced: the state before block k is the GPU's own trail[k - 1]; the step of block k is checked against the CPU
    on snapshot k as one awpu_hip_track step is, and audio row k is the oracle's das where trail[k] points."""
    before = p0
    for k in range(len(snaps)):
        after = got.trail[k]
        check_steps_against_the_cpu(pkg, oracle, xyz, snaps[k], index, before, after, LIMIT, reference, premise)
        for f in ("spread", "rate", "steps"):
            assert same(after[f], p0[f])
        check_das_against_the_cpu(pkg, oracle, xyz, snaps[k], index, after, got.audio[:, 256 * k: 256 * (k + 1)])
        before = after
    assert same(got.listeners, got.trail[-1])
    assert not same(got.trail[-1]["theta"], p0["theta"]) and np.isfinite(got.trail["theta"]).all() and np.isfinite(got.trail["phi"]).all()


@pytest.mark.parametrize("elements,name", [(64, "seventeen"), (64, "no_corners60"), (64, "keep57_perm"), (256, "tiled205")])
@pytest.mark.parametrize("reference", ["given", "from_each_block"])
def test_tracking_listeners_against_the_cpu(pkg, oracle, recordings, elements, name, reference):
    """4 listeners of one step per block, 8 blocks after the 4-block primer, the trail asked for.  With the reference power
    given the whole chain is checked; taken from each block's snapshot, the one the gradients imply is stream 0's."""
    wire, _, snaps = recordings[elements]
    index = L[name]
    xyz = ANTENNAS[elements](pkg)
    p0 = listeners(pkg, 4, 19, [1])
    p0["rate"] = R.PARTICLE_RATE
    given = R.reference_power(snaps[6]) if reference == "given" else None
    with listen_engine(pkg, xyz, 4, index=index) as eng:
        prime(eng, wire)
        got = eng.listen_blocks(wire[4 * B: 12 * B], p0, None, None, None, None, LIMIT, reference=given)
    check_tracking_listeners_block_by_block(pkg, oracle, xyz, snaps[4:12], index, p0, got, given, name in R.LISTS_WITHOUT_THE_HOLDERS[elements])


def test_512_streams_on_a_ragged_list_through_the_samples_form(pkg, oracle):
    """Two FPGAs, 509 mics out of id order, 4 + 6 blocks: fixed listeners on every block, tracking ones once the ring is full."""
    index = L["tiled509"]
    xyz = pkg.create_tiled_antenna(4, 2)
    rng = np.random.default_rng(9)
    big = (rng.integers(-(1 << 21), 1 << 21, size=(512, 256 * 10)) / 8388608.0).astype(np.float32)
    snaps = snapshots(big)
    still = listeners(pkg, 3, 12, [0])
    late = listeners(pkg, 3, 12, [0, 1, 1])
    late["rate"] = R.PARTICLE_RATE
    with listen_engine(pkg, xyz, 4, index=index) as eng:
        head = eng.listen_samples(big[:, : 256 * 4], still, None, None, None, None, LIMIT)
        got = eng.listen_samples(big[:, 256 * 4:], late, None, None, None, None, LIMIT)
        assert same(eng.ring_snapshot(), snaps[-1])
    off, frac = pkg.steer_table(xyz, still["theta"], still["phi"])
    assert order_matters(oracle, snaps[7], off, frac, index)
    for k in range(10):
        rows = head.audio[:, 256 * k: 256 * (k + 1)] if k < 4 else got.audio[:1, 256 * (k - 4): 256 * (k - 3)]
        check_das_against_the_cpu(pkg, oracle, xyz, snaps[k], index, still[: len(rows)], rows)
    assert same(got.trail["theta"][:, 0], np.repeat(late["theta"][:1], 6))
    moving = type(got)(got.audio[1:], got.listeners[1:], got.trail[:, 1:], None)
    check_tracking_listeners_block_by_block(pkg, oracle, xyz, snaps[4:], index, late[1:], moving, None, False)


# ------------------------------------------------------------------------------------------------ 3. the list changes on a live handle

CHANGES = ["keep57_perm", OTHER57, "three", None, "keep57_perm"]  # same length and other ids; shorter; longer than any before; back


def list_of(entry):
    return L[entry] if isinstance(entry, str) else entry


def test_track_follows_the_list_on_a_live_handle(pkg, oracle, recordings):
    """awpu_hip_track after every set_active_mics on one handle == a fresh handle given that list, byte for byte; the ring
    (four blocks) is what it was."""
    wire, _, snaps = recordings[64]
    xyz = pkg.create_antenna()
    theta, phi, spread = _seeded_particles(16, 31)
    before = particles(pkg, theta, phi, spread, steps=3)
    results = []
    with listen_engine(pkg, xyz, 4, mics=False) as live:
        prime(live, wire)
        for entry in CHANGES:
            live.set_active_mics(list_of(entry))
            got = live.track(before, None, None, None, None, LIMIT, None, 0, want_beams=True)
            with listen_engine(pkg, xyz, 4, index=list_of(entry)) as fresh:
                prime(fresh, wire)
                want = fresh.track(before, None, None, None, None, LIMIT, None, 0, want_beams=True)
            assert same(got.particles, want.particles) and same(got.beams, want.beams) and got.reference == want.reference
            assert same(live.ring_snapshot(), snaps[3])
            results.append(got)
        assert same(results[0].particles, results[4].particles) and same(results[0].beams, results[4].beams)
        assert not same(results[0].beams, results[1].beams) and not same(results[1].beams, results[2].beams)
    # ... and the first of them against the CPU, so that "equal to a fresh handle" is not two handles wrong alike
    check_das_against_the_cpu(pkg, oracle, xyz, snaps[3], L["keep57_perm"], results[0].particles, results[0].beams)
    check_das_against_the_cpu(pkg, oracle, xyz, snaps[3], OTHER57, results[1].particles, results[1].beams)


def test_listening_follows_the_list_on_a_live_handle(pkg, oracle, recordings):
    """listen_blocks of two blocks after every set_active_mics on one handle == a fresh handle given that list and the same
    ring, byte for byte; the listeners carry on from stage to stage."""
    wire, _, snaps = recordings[64]
    xyz = pkg.create_antenna()
    p = listeners(pkg, 4, 27, [0, 3, 1, 0])
    with listen_engine(pkg, xyz, 4, mics=False) as live:
        prime(live, wire)
        for stage, entry in enumerate(CHANGES):
            a, b = 4 + 2 * stage, 6 + 2 * stage
            live.set_active_mics(list_of(entry))
            got = live.listen_blocks(wire[a * B: b * B], p, None, None, None, None, LIMIT)
            with listen_engine(pkg, xyz, 4, index=list_of(entry)) as fresh:
                prime(fresh, wire, a)
                want = fresh.listen_blocks(wire[a * B: b * B], p, None, None, None, None, LIMIT)
                assert same(got.audio, want.audio) and same(got.trail, want.trail) and same(got.listeners, want.listeners), stage
                assert same(live.ring_snapshot(), fresh.ring_snapshot()) and same(live.ring_snapshot(), snaps[b - 1])
            index = np.arange(64) if entry is None else list_of(entry)
            fixed = [0, 3]
            for k in range(a, b):  # the fixed listeners against the CPU
                check_das_against_the_cpu(pkg, oracle, xyz, snaps[k], index, p[fixed], got.audio[fixed, 256 * (k - a): 256 * (k - a + 1)])
            p = got.listeners
        assert np.isfinite(p["theta"]).all()


def test_a_list_change_after_an_enqueued_device_run(pkg, oracle, recordings):
    """listen_samples_device enqueued on another stream, no synchronisation by the caller, then at once a new list and the next
    call: the device run's audio is the old list's, the next call's the new list's (later calls are ordered after the run)."""
    import torch

    wire, samples, snaps = recordings[64]
    xyz = pkg.create_antenna()
    p0 = listeners(pkg, 4, 29, [0, 1, 3, 0])
    n = 6
    with listen_engine(pkg, xyz, 4, index=L["keep57_perm"]) as old, listen_engine(pkg, xyz, 4, index=OTHER57) as new, \
            listen_engine(pkg, xyz, 4, index=L["keep57_perm"]) as live:
        for e in (old, new, live):
            prime(e, wire)
        want_old = old.listen_blocks(wire[4 * B: (4 + n) * B], p0, None, None, None, None, LIMIT)
        prime(new, wire[4 * B:], n)
        want_new = new.listen_blocks(wire[(4 + n) * B: (6 + n) * B], want_old.listeners, None, None, None, None, LIMIT)
        want_track = new.track(want_new.listeners, None, None, None, None, LIMIT, None, 0, want_beams=True)
        d_in = torch.from_numpy(np.ascontiguousarray(samples[:, 256 * 4: 256 * (4 + n)])).cuda()
        d_audio = torch.zeros((4, 256 * n), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            after = live.listen_samples_device(d_in.data_ptr(), 256 * n, n, p0, None, None, None, None, LIMIT, d_audio.data_ptr(), 256 * n,
                                               stream=side.cuda_stream)
        live.set_active_mics(OTHER57)
        got_new = live.listen_blocks(wire[(4 + n) * B: (6 + n) * B], after, None, None, None, None, LIMIT)
        got_track = live.track(got_new.listeners, None, None, None, None, LIMIT, None, 0, want_beams=True)
        torch.cuda.synchronize()
        assert same(d_audio.cpu().numpy(), want_old.audio) and same(after, want_old.listeners)
        assert same(got_new.audio, want_new.audio) and same(got_new.listeners, want_new.listeners)
        assert same(got_track.particles, want_track.particles) and same(got_track.beams, want_track.beams)
        assert same(live.ring_snapshot(), snaps[5 + n])
    fixed = [0, 3]
    check_das_against_the_cpu(pkg, oracle, xyz, snaps[4 + n], OTHER57, p0[fixed], got_new.audio[fixed, :256])
    check_das_against_the_cpu(pkg, oracle, xyz, snaps[3 + n], L["keep57_perm"], p0[fixed], d_audio.cpu().numpy()[fixed, 256 * (n - 1):])


# ------------------------------------------------------------------------------------------------ 4. block, listen and watch runs

MODES = ["exact", "fast", "fir8"]


def mode_kw(pkg, mode):
    if mode == "fast":
        return dict(math=pkg.MATH_F32_FAST)
    if mode == "fir8":
        return dict(interp=pkg.binding.INTERP_FIR8, fir=util.synthetic_fir_table())
    return {}


@pytest.fixture(scope="module")
def run_scene(oracle):
    """The reference's array, 4 + 9 blocks of zero-mean samples, seeded gains in [0.5, 1.5], delay tables of both grids."""
    xyz = oracle.create_antenna()
    wire, samples = recording(oracle, 13, 64, seed=51)
    gains = np.random.default_rng(52).uniform(0.5, 1.5, 64).astype(np.float32)
    tables = {res: oracle.compute_delay_lut(xyz, res, res) for res in (16, 32)}
    return xyz, wire, snapshots(samples), gains, tables


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("res", [16, 32])
@pytest.mark.parametrize("name", ["keep57_perm", "inner16"])
def test_runs_of_blocks_on_a_ragged_list_with_gains(pkg, oracle, run_scene, name, res, mode):
    """9 blocks after a 4-block primer, max_batch 4 (pieces of 4 + 4 + 1): process_blocks == Engine.process of the snapshots in
    chunks of 4, and every pixel of every frame is within the flat 1e-5 of the oracle on the list, the gains on the samples;
    listen_blocks with heatmaps returns the same powers and the audio and trail of the run without them; watch_blocks shows
    every second block: the same powers, and the images of the composition.  inner16 touches a shorter window of the history than
    the full list does, so the compact cut of a piece starts elsewhere and is narrower."""
    xyz, wire, snaps, gains, tables = run_scene
    index = INNER16 if name == "inner16" else L[name]
    off, frac = tables[res]
    full = int(off.max() - off.min())
    active = int(off[:, index].max() - off[:, index].min())
    assert active < full if name == "inner16" else active == full
    kw = mode_kw(pkg, mode)
    fir = kw.get("fir")
    run = wire[4 * B: 13 * B]
    p0 = listeners(pkg, 3, 33, [0, 3, 1])
    with sweep_engine(pkg, off, frac, 64, res, 4, index=index, gains=gains, **kw) as eng:
        prime(eng, wire)
        power = eng.process_blocks(run)
        assert np.array_equal(power, chunked_process(eng, snaps[4:13], 4))
        assert np.array_equal(eng.ring_snapshot(), snaps[12])
    for k in range(9):
        check_full_grid(oracle, power[k], snaps[4 + k] * gains[:, None], off, frac, f"{name} {mode} {res}x{res} block {k}", index=index, fir_table=fir)
    lkw = dict(kw)
    with listen_engine(pkg, xyz, 4, (off, frac), res, lkw.pop("math", None), index=index, gains=gains, **lkw) as eng, \
            listen_engine(pkg, xyz, 4, index=index) as quiet:
        prime(eng, wire)
        prime(quiet, wire)
        got = eng.listen_blocks(run, p0, None, None, None, None, LIMIT, want_power=True)
        heard = quiet.listen_blocks(run, p0, None, None, None, None, LIMIT)
        assert same(got.power, power)
        assert same(got.audio, heard.audio) and same(got.trail, heard.trail) and same(got.listeners, heard.listeners)
        assert np.isfinite(got.trail["theta"]).all() and not same(got.trail[-1]["theta"], p0["theta"])
    fixed = [0]
    for k in (0, 8):  # (the audio takes no gains: it is Particle::das of the snapshot as it is)
        check_das_against_the_cpu(pkg, oracle, xyz, snaps[4 + k], index, p0[fixed], got.audio[fixed, 256 * k: 256 * (k + 1)])
    table, d_table = colour_table(5)
    shown = list(range(1, 9, 2))
    with sweep_engine(pkg, off, frac, 64, res, 4, index=index, gains=gains, **kw) as eng:
        prime(eng, wire)
        seen = eng.watch_blocks(run, res, res, first=1, every=2, out_rows=40, out_cols=56, d_colormap_ptr=d_table.data_ptr(), flip=True,
                                want_power=True)
        assert np.array_equal(eng.ring_snapshot(), snaps[12])
        assert np.array_equal(seen.power, chunked_process(eng, snaps[4:13][shown], 4))
    for j, k in enumerate(shown):
        check_full_grid(oracle, seen.power[j], snaps[4 + k] * gains[:, None], off, frac, f"{name} {mode} {res}x{res} shown block {k}", index=index,
                        fir_table=fir)
    image, big = compose(pkg, oracle, seen.power, res, res, 40, 56, table, True)
    assert np.array_equal(seen.image, image) and np.array_equal(seen.big, big)
