"""Listening to runs of blocks (include/awpu_hip_listen.h) on the device: audio, trail and final listeners equal the per-block
loop awpu_hip_ingest_block + awpu_hip_track bit for bit (NaN-safe: bytes are compared, never values with a tolerance), fixed
listeners equal the reference's delay() on every snapshot, consecutive rows are continuous audio, the heatmaps of the same pass
equal awpu_hip_process_blocks, and the ingest ring is left where the loop leaves it.  Tracking runs start on a ring primed with
four blocks: on a zeroed ring the reference power is 0 and a tracker's direction becomes NaN (the header's "hazard")."""
import ctypes as C
import math

import numpy as np
import pytest

import test_tracker_cpu as R
from test_gpu_blocks import engine as sweep_engine
from test_gpu_blocks import make_datagrams, snapshots

pytestmark = pytest.mark.gpu

B = 256 * 1032  # bytes of a block on the wire
LIMIT = math.pi / 2
SHAPES = {"reference": (1, 1), "tiled256": (4, 1)}  # arrays of 64 mics: the reference's antenna, and 256 mics on one wire


def wire_recording(oracle, n_blocks, n_streams, seed, dc=0):
    """(wire bytes, unpacked samples [n_streams, 256 * n_blocks]) of random 24-bit samples around `dc` (wire integers)."""
    rng = np.random.default_rng(seed)
    wire, blocks = [], []
    for b in range(n_blocks):
        stream = rng.integers(-(1 << 21), 1 << 21, size=(256, 256), dtype=np.int32) + np.int32(dc)
        wire.append(make_datagrams(stream, counter0=256 * b))
        blocks.append(oracle.unpack_exposure(stream, n_streams))
    return b"".join(wire), np.concatenate(blocks, axis=1)


def listen_engine(pkg, xyz, max_batch, table=None, res=32, math=None, mics=True, index=None, gains=None, **kw):
    """`index`: the active mics (None = all, in id order); `gains`: per-mic gains of the heatmaps; kw: interp, fir (the sweep's)."""
    fir = kw.pop("fir", None)
    eng = pkg.Engine(n_pixels=res * res, n_streams=xyz.shape[1], max_batch=max_batch, grid_columns=res, math=math, **kw)
    eng.set_antenna(xyz)
    if mics:
        eng.set_active_mics(index)
    if gains is not None:
        eng.set_mic_gains(gains)
    if fir is not None:
        eng.set_fir_table(fir)
    if table is not None:
        eng.set_delay_table(*table)
    return eng


def listeners(pkg, n, seed, steps):
    """n listeners at seeded directions; `steps` per listener (cycled), two spreads."""
    rng = np.random.default_rng(seed)
    p = np.zeros(n, pkg.binding.PARTICLE_DTYPE)
    p["theta"] = rng.uniform(0.05, 1.2, n)
    p["phi"] = rng.uniform(0.0, 2 * math.pi, n)
    p["spread"] = np.where(np.arange(n) % 2 == 0, R.TRACKER_SPREAD, R.SEEKER_SPREAD)
    p["rate"] = R.PARTICLE_RATE / 10
    p["steps"] = np.resize(np.asarray(steps, np.int32), n)
    return p


def fields(p):
    return p["theta"], p["phi"], p["spread"], p["rate"], p["steps"]


def per_block_loop(eng, wire, n_blocks, p, reference=None):
    """The definition: ingest_block + track(want_beams) per block -> (audio [n, 256 * n_blocks], trail [n_blocks, n], listeners)."""
    audio, trail = [], []
    for b in range(n_blocks):
        eng.ingest_block(wire[B * b: B * (b + 1)])
        got = eng.track(*fields(p), LIMIT, reference, 0, want_beams=True)
        p = got.particles
        audio.append(got.beams)
        trail.append(p.copy())
    return np.concatenate(audio, axis=1), np.stack(trail), p


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.fixture(scope="module", params=list(SHAPES))
def scene(request, pkg, oracle):
    xyz = pkg.create_tiled_antenna(*SHAPES[request.param])
    wire, samples = wire_recording(oracle, 44, xyz.shape[1], seed=17)
    return xyz, wire, samples


def prime(eng, wire, n=4):
    for b in range(n):
        eng.ingest_block(wire[B * b: B * (b + 1)])


@pytest.mark.parametrize("max_batch,calls", [(32, (40,)), (1, (40,)), (32, (7, 22, 11))])
def test_equals_the_per_block_loop(pkg, scene, max_batch, calls):
    """40 blocks after a 4-block primer, 6 listeners of mixed kind (steps 0, 3, 5; two spreads), the wire form: in one call
    over pieces of 32 + 8 blocks, block by block (max_batch 1: 40 pieces), and split over three calls of unequal length."""
    xyz, wire, _ = scene
    p0 = listeners(pkg, 6, 3, [0, 3, 5, 0, 5, 3])
    with listen_engine(pkg, xyz, max_batch) as eng, listen_engine(pkg, xyz, max_batch) as loop:
        prime(eng, wire)
        prime(loop, wire)
        want_audio, want_trail, want_p = per_block_loop(loop, wire[4 * B:], 40, p0)
        assert np.isfinite(want_p["theta"]).all()  # (the primer did its work: this run is not a comparison of NaNs)
        assert not same(want_trail[0]["theta"][1:3], p0["theta"][1:3])  # ... and the trackers moved
        audio, trail, p, k = [], [], p0, 4
        for n in calls:
            got = eng.listen_blocks(wire[k * B: (k + n) * B], p, None, None, None, None, LIMIT)
            audio.append(got.audio)
            trail.append(got.trail)
            p, k = got.listeners, k + n
        assert same(np.concatenate(audio, axis=1), want_audio)
        assert same(np.concatenate(trail), want_trail)
        assert same(p, want_p)
        assert same(eng.ring_snapshot(), loop.ring_snapshot())


def test_a_zeroed_ring_gives_the_loops_nans(pkg, scene):
    """Without the primer the reference power of the first block is 0 and a tracker's direction becomes NaN: in the loop's first
    block and here alike.  The loop ends there (awpu_hip_track refuses a NaN direction); a listen call carries the NaN to its
    end, the fixed listener beside it is not touched by it, and the next call refuses the NaN listener like awpu_hip_track."""
    xyz, wire, _ = scene
    p0 = listeners(pkg, 3, 4, [3, 0, 5])
    with listen_engine(pkg, xyz, 4) as eng, listen_engine(pkg, xyz, 4) as loop, listen_engine(pkg, xyz, 4) as long:
        want_audio, want_trail, want_p = per_block_loop(loop, wire, 1, p0)
        assert np.isnan(want_p["phi"][0]) and np.isnan(want_audio[0]).any() and np.isfinite(want_audio[1]).all()
        with pytest.raises(pkg.AwpuError):
            per_block_loop(loop, wire[B:], 1, want_p)
        got = eng.listen_blocks(wire[:B], *fields(p0), LIMIT)
        assert same(got.audio, want_audio) and same(got.trail, want_trail) and same(got.listeners, want_p)
        six = long.listen_blocks(wire[: 6 * B], *fields(p0), LIMIT)
        assert same(six.audio[:, :256], want_audio) and same(six.trail[0], want_trail[0])
        assert np.isnan(six.trail["phi"][:, 0]).all() and np.isnan(six.trail["phi"][:, 2]).all()
        fixed = p0[1:2].copy()
        with listen_engine(pkg, xyz, 4) as alone:
            assert same(alone.listen_blocks(wire[: 6 * B], fixed, None, None, None, None, LIMIT).audio[0], six.audio[1])
        with pytest.raises(pkg.AwpuError) as ei:
            long.listen_blocks(wire[6 * B: 7 * B], six.listeners, None, None, None, None, LIMIT)
        assert ei.value.status == pkg.binding.ERR_INVALID


@pytest.mark.parametrize("dc", [0, 1 << 21])
def test_fixed_listeners_equal_the_reference_delay(pkg, oracle, scene, dc):
    """Every audio row of a fixed listener is Particle::das on that block's snapshot: the oracle's restatement and, where it is
    built, the reference's own compiled delay().  Zero-mean samples and samples biased by 0.25 of full scale."""
    xyz, _, _ = scene
    n = xyz.shape[1]
    wire, samples = wire_recording(oracle, 12, n, seed=23, dc=dc)
    snaps = snapshots(samples)
    p0 = listeners(pkg, 5, 8, [0])
    p0["theta"][0] = 0.0
    off, frac = pkg.steer_table(xyz, p0["theta"], p0["phi"])
    with listen_engine(pkg, xyz, 8) as eng:
        got = eng.listen_blocks(wire, *fields(p0), LIMIT)
    assert same(got.listeners, p0) and same(got.trail, np.stack([p0] * 12))  # fixed: the state is left as passed
    impls = ["oracle"] + (["ref"] if oracle.ref_available() else [])
    for k in range(12):
        for impl in impls:
            _, want = oracle.particle_beams(snaps[k], off, frac, impl=impl)
            assert same(got.audio[:, 256 * k: 256 * (k + 1)], want), (k, impl)


def test_consecutive_rows_are_continuous_audio(pkg, oracle, scene):
    """Every stream carries the same signal s of 16 significant bits and the listener looks straight up (every delay equal:
    offset 256, fraction 0), so every partial sum is exact in fp32.  delay() with fraction 0 returns signal[i + 1]
    (src/dsp/delay.cpp:16-26), so sample i of row k is snapshot sample 257 + i, and the snapshot after block k holds blocks
    k-3 .. k: row k is usable * s over samples 1 .. 256 of block k-2 (the last of them block k-1's first).  Laid end to end the
    rows are usable * the recording from index 511 on, with no gap or repeat at block, piece, chunk or call boundaries."""
    xyz, _, _ = scene
    n = xyz.shape[1]
    n_blocks = 37
    rng = np.random.default_rng(31)
    m = rng.integers(-(1 << 14), 1 << 14, size=256 * n_blocks, dtype=np.int32) * 256
    s = m.astype(np.float32) / np.float32(8388608.0)
    wire = b"".join(make_datagrams(np.repeat(m[256 * b: 256 * (b + 1), None], 256, axis=1), counter0=256 * b) for b in range(n_blocks))
    up = listeners(pkg, 1, 0, [0])
    up["theta"], up["phi"] = 0.0, 0.0
    off, frac = pkg.steer_table(xyz, up["theta"], up["phi"])
    assert (off == 256).all() and (frac == 0.0).all()
    # the expected values on the CPU first: the per-block loop's arithmetic (the oracle's das) on the snapshots
    want = np.zeros(256 * n_blocks, np.float32)
    want[511:] = np.float32(n) * s[: 256 * n_blocks - 511]
    snaps = snapshots(np.repeat(s[None, :], n, axis=0))
    for k in (0, 1, 2, 3, 20, 36):
        assert same(oracle.particle_beams(snaps[k], off, frac)[1][0], want[256 * k: 256 * (k + 1)]), k
    with listen_engine(pkg, xyz, 8) as eng:  # chunks of 8 blocks; calls of 5 + 20 + 12
        rows = [eng.listen_blocks(wire[a * B: b * B], *fields(up), LIMIT).audio[0] for a, b in ((0, 5), (5, 25), (25, 37))]
    assert same(np.concatenate(rows), want)


@pytest.mark.parametrize("math", ["default", "fast"])
def test_heatmaps_in_the_same_pass(pkg, oracle, scene, math):
    """power = process_blocks of the same run on a second engine, bit for bit, and the audio does not depend on it."""
    xyz, wire, _ = scene
    n = xyz.shape[1]
    res = 48
    table = oracle.compute_delay_lut(xyz, res, res)
    mode = pkg.MATH_F32_FAST if math == "fast" else None
    p0 = listeners(pkg, 4, 5, [3, 0, 0, 5])
    with listen_engine(pkg, xyz, 16, table, res, mode) as eng, sweep_engine(pkg, *table, n, res, 16, math=mode) as sweep, \
            listen_engine(pkg, xyz, 16) as quiet:
        for e in (eng, sweep, quiet):
            prime(e, wire)
        got = eng.listen_blocks(wire[4 * B: 41 * B], *fields(p0), LIMIT, want_power=True)
        want = sweep.process_blocks(wire[4 * B: 41 * B])
        assert same(got.power, want)
        assert eng.stats().frames == sweep.stats().frames == 37 and eng.stats().launches == sweep.stats().launches
        # audio only: nothing swept, no table needed
        heard = quiet.listen_blocks(wire[4 * B: 41 * B], *fields(p0), LIMIT)
        assert heard.power is None and quiet.stats().launches == 0 and quiet.stats().frames == 0
        assert same(heard.audio, got.audio) and same(heard.trail, got.trail) and same(heard.listeners, got.listeners)
        assert same(quiet.ring_snapshot(), eng.ring_snapshot())


def test_ring_continuity_and_mixing(pkg, oracle, scene):
    """After a listen call the ring, process_ring and a following process_blocks are what the same number of ingests leave."""
    xyz, wire, samples = scene
    n = xyz.shape[1]
    res = 32
    table = oracle.compute_delay_lut(xyz, res, res)
    p0 = listeners(pkg, 2, 6, [0, 3])
    with listen_engine(pkg, xyz, 8, table, res) as eng, sweep_engine(pkg, *table, n, res, 8) as loop:
        head = eng.process_blocks(wire[: 5 * B])                        # a heatmap call, then a listen call, then ingests ...
        got = eng.listen_blocks(wire[5 * B: 18 * B], *fields(p0), LIMIT)
        for b in range(18):
            loop.ingest_block(wire[b * B: (b + 1) * B])
        assert same(eng.ring_snapshot(), loop.ring_snapshot())
        assert same(eng.ring_snapshot(), snapshots(samples[:, : 256 * 18])[-1])
        assert same(eng.process_ring(), loop.process_ring())
        assert same(eng.process_blocks(wire[18 * B: 27 * B]), loop.process_blocks(wire[18 * B: 27 * B]))
        # ... and a listen call continues a ring that ingests and heatmap calls have filled
        loop.set_antenna(xyz)
        tail = loop.listen_blocks(wire[27 * B: 30 * B], got.listeners, None, None, None, None, LIMIT)
        want = eng.listen_blocks(wire[27 * B: 30 * B], got.listeners, None, None, None, None, LIMIT)
        assert same(tail.audio, want.audio) and same(tail.listeners, want.listeners)
        assert head.shape == (5, res * res)


def test_samples_forms(pkg, oracle, scene):
    """listen_samples (host) and listen_samples_device (on the handle's stream and on another one, odd pitches) equal the wire form."""
    import torch

    xyz, wire, samples = scene
    n_mics, n, nl = xyz.shape[1], 21, 4
    p0 = listeners(pkg, nl, 7, [3, 0, 5, 0])
    PARTICLE = pkg.binding.PARTICLE_DTYPE
    with listen_engine(pkg, xyz, 8) as a, listen_engine(pkg, xyz, 8) as b:
        prime(a, wire)
        prime(b, wire)
        want = a.listen_blocks(wire[4 * B: (4 + n) * B], *fields(p0), LIMIT)
        got = b.listen_samples(samples[:, 256 * 4: 256 * (4 + n)], *fields(p0), LIMIT)
        assert same(got.audio, want.audio) and same(got.trail, want.trail) and same(got.listeners, want.listeners)
    for where in ("handle_stream", "other_stream"):
        with listen_engine(pkg, xyz, 8) as c:
            prime(c, wire)
            wide = np.zeros((n_mics, 256 * n + 101), np.float32)  # pitch above 256 * n_blocks, and odd
            wide[:, : 256 * n] = samples[:, 256 * 4: 256 * (4 + n)]
            d_in = torch.from_numpy(wide).cuda()
            d_audio = torch.zeros((nl, 256 * n + 7), dtype=torch.float32, device="cuda")
            d_trail = torch.zeros(n * nl * PARTICLE.itemsize, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            args = (d_in.data_ptr(), wide.shape[1], n, *fields(p0), LIMIT, d_audio.data_ptr(), d_audio.shape[1])
            if where == "other_stream":
                side = torch.cuda.Stream()
                with torch.cuda.stream(side):
                    after = c.listen_samples_device(*args, d_trail_ptr=d_trail.data_ptr(), stream=side.cuda_stream)
            else:
                after = c.listen_samples_device(*args, d_trail_ptr=d_trail.data_ptr())
            torch.cuda.synchronize()
            assert same(d_audio.cpu().numpy()[:, : 256 * n], want.audio), where
            assert (d_audio.cpu().numpy()[:, 256 * n:] == 0).all()
            assert same(d_trail.cpu().numpy().view(PARTICLE).reshape(n, nl), want.trail), where
            assert same(after, want.listeners), where
            assert same(c.ring_snapshot(), a_ring(pkg, xyz, wire, 4 + n)), where


def a_ring(pkg, xyz, wire, n_blocks):
    with listen_engine(pkg, xyz, 1) as eng:
        prime(eng, wire, n_blocks)
        return eng.ring_snapshot()


def test_512_streams_through_the_samples_form(pkg):
    """Two FPGAs: more streams than the wire carries.  The loop is awpu_hip_track on every snapshot, uploaded as a frame."""
    import torch

    xyz = pkg.create_tiled_antenna(4, 2)
    rng = np.random.default_rng(9)
    n = 11
    big = (rng.integers(-(1 << 21), 1 << 21, size=(512, 256 * n)) / 8388608.0).astype(np.float32)
    snaps = snapshots(big)
    p0 = listeners(pkg, 3, 12, [0, 3, 3])
    p0["steps"] = 0  # (a tracker would start on the zeroed ring: the first four blocks are only listened to)
    late = listeners(pkg, 3, 12, [0, 3, 3])
    with listen_engine(pkg, xyz, 4) as eng, listen_engine(pkg, xyz, 4) as loop:
        got = eng.listen_samples(big[:, : 256 * 4], *fields(p0), LIMIT)
        more = eng.listen_samples(big[:, 256 * 4:], *fields(late), LIMIT, want_trail=False)
        assert more.trail is None
        audio, p = [], p0
        for k in range(n):
            if k == 4:
                p = late
            d_frame = torch.from_numpy(snaps[k]).cuda()
            step = loop.track(*fields(p), LIMIT, None, d_frame.data_ptr(), want_beams=True)
            p = step.particles
            audio.append(step.beams)
        assert same(np.concatenate([got.audio, more.audio], axis=1), np.concatenate(audio, axis=1))
        assert same(more.listeners, p) and np.isfinite(p["theta"]).all()
        assert same(eng.ring_snapshot(), snaps[-1])


def test_refusals_leave_ring_and_listeners(pkg, scene):
    xyz, wire, samples = scene
    lib = pkg.binding.load()
    Bn = pkg.binding

    def refused(eng, status, p, n_blocks=2, audio_pitch=None, wire_bytes=None):
        before_ring = eng.ring_snapshot()
        before_p = p.copy()
        audio = np.zeros((p.size, 256 * max(n_blocks, 1)), np.float32)
        buf = np.frombuffer(wire[B: 3 * B] if wire_bytes is None else wire_bytes, np.uint8)
        rc = lib.awpu_hip_listen_blocks(eng._h, buf.ctypes.data_as(C.c_void_p), 1032, n_blocks, p.ctypes.data_as(C.POINTER(Bn.Particle)),
                                        p.size, LIMIT, -1.0, audio.ctypes.data_as(C.POINTER(C.c_float)),
                                        audio.shape[1] if audio_pitch is None else audio_pitch, None, None)
        assert rc == status, (rc, status)
        assert same(p, before_p) and same(eng.ring_snapshot(), before_ring)
        assert (audio == 0).all()

    good = listeners(pkg, 2, 1, [3, 0])
    with listen_engine(pkg, xyz, 4) as eng:
        prime(eng, wire, 1)
        for field, value in (("steps", 4097), ("steps", -1), ("theta", math.nan), ("phi", math.inf), ("rate", math.nan)):
            bad = good.copy()
            bad[field][0] = value
            refused(eng, Bn.ERR_INVALID, bad)
        refused(eng, Bn.ERR_INVALID, good.copy(), audio_pitch=511)
        refused(eng, Bn.ERR_INVALID, good.copy(), n_blocks=0)
        with pytest.raises(pkg.AwpuError) as ei:  # the binding's own range check of steps (before the int32 field wraps)
            eng.listen_blocks(wire[B: 3 * B], 0.1, 0.1, 0.1, 1e-5, 1 << 32, LIMIT)
        assert ei.value.status == Bn.ERR_INVALID
        after = eng.listen_blocks(wire[B: 3 * B], *fields(good), LIMIT)  # the handle still works
        assert after.audio.shape == (2, 512)
    # antenna unset, active mics unset: AWPU_ERR_STATE
    with pkg.Engine(n_pixels=16, n_streams=xyz.shape[1], max_batch=4) as bare:
        prime(bare, wire, 1)
        refused(bare, Bn.ERR_STATE, good.copy())
        bare.set_antenna(xyz)
        refused(bare, Bn.ERR_STATE, good.copy())
        # heatmaps asked for without a delay table: AWPU_ERR_STATE too
        bare.set_active_mics(None)
        with pytest.raises(pkg.AwpuError) as ei:
            bare.listen_blocks(wire[B: 3 * B], *fields(good), LIMIT, want_power=True)
        assert ei.value.status == Bn.ERR_STATE
    # hist != 1024: AWPU_ERR_INVALID
    with pkg.Engine(n_pixels=16, n_streams=xyz.shape[1], hist=2048, max_batch=4) as eng:
        eng.set_antenna(xyz)
        eng.set_active_mics(None)
        with pytest.raises(pkg.AwpuError) as ei:
            eng.listen_blocks(wire[: 2 * B], *fields(good), LIMIT)
        assert ei.value.status == Bn.ERR_INVALID
    # a device group (one device listed twice): AWPU_ERR_STATE, its ring untouched
    with pkg.Engine(n_pixels=32 * 32, n_streams=xyz.shape[1], max_batch=4, grid_columns=32, devices=[0, 0]) as group:
        group.set_antenna(xyz)
        group.set_active_mics(None)
        prime(group, wire, 1)
        refused(group, Bn.ERR_STATE, good.copy())


def test_a_tracker_finds_the_synthetic_source(pkg):
    """The scene of test_gpu_tracker.test_tracker_converges_like_the_cpu_restatement (the synthetic source at 20 deg, 35 deg on
    the reference antenna) as a recording: a tracker started 4 degrees off ends within that test's distance of the source (the
    reference's quadrant monopulse settles about 3 degrees off it), and hears more of it than a fixed listener pointed away."""
    xyz = pkg.create_antenna()
    n_blocks = 44
    rec = pkg.synthetic.make_frames(xyz, 1, seed=1234, hist=256 * n_blocks)[0]
    start = (R.SOURCE[0] + math.radians(4.0), R.SOURCE[1])
    away = (math.radians(60.0), R.SOURCE[1] + math.pi)
    who = ([start[0], away[0]], [start[1], away[1]], R.TRACKER_SPREAD, R.CONVERGE_RATE)
    with listen_engine(pkg, xyz, 16) as eng:
        settle = eng.listen_samples(rec[:, : 256 * 4], *who, 0, LIMIT)
        got = eng.listen_samples(rec[:, 256 * 4:], *who, [3, 0], LIMIT)
    assert same(settle.listeners["theta"], np.asarray(who[0]))
    end = (float(got.theta[0]), float(got.phi[0]))
    off_source = [math.degrees(R.angle((float(t["theta"][0]), float(t["phi"][0])), R.SOURCE)) for t in got.trail]
    print("LISTEN tracker, degrees off the source after blocks 0, 9, 19, 29, 39:", [round(off_source[k], 3) for k in (0, 9, 19, 29, 39)])
    power = (got.audio.astype(np.float64) ** 2).mean(axis=1)
    print("LISTEN audio power, tracker / fixed away:", power)
    assert R.angle(end, R.SOURCE) < math.radians(3.2)
    assert (got.theta[1], got.phi[1]) == (who[0][1], who[1][1])  # the fixed one stayed
    assert power[0] > power[1]
