"""Value edges behind the sweep, on the device: the display step (heatmap_max_kernel, heatmap_scale_kernel, peak_given), the peak
finder, calibration (stream_power_kernel and the host's decisions), the two unpack kernels of the ingest, the range sweep and one
run of blocks, on the frames of test_behind_sweep_cpu.py: subnormal powers, +inf, NaN of both signs, -0.0 and negative pixels.
Every device result lands in canary-filled buffers and is compared with the host entry point bit for bit and with the plain numpy
restatement of the rule (test_behind_sweep_cpu.py).  Non-finite and subnormal values are ordinary data here."""
import numpy as np
import pytest

import test_behind_sweep_cpu as E
import util
import value_edges as V
from test_find_cpu import TOL
from test_gpu_blocks import engine, make_datagrams, snapshots
from test_gpu_find import device_find
from test_gpu_focus import directions

pytestmark = pytest.mark.gpu


def same_u64(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


# ------------------------------------------------------------------------------------------------ B1: display

def device_display(eng, frames, given=None):
    """heatmap_device of frames [b, n] -> (pix [b, n], peak [b]); with `given` [b] the peaks are handed in (peak_given) and must
    come back untouched.  Nothing is written past either buffer."""
    import torch

    frames = np.ascontiguousarray(frames, np.float32)
    b, n = frames.shape
    d_power = torch.from_numpy(frames).cuda()
    d_pix = torch.full((b * n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    peak0 = np.full(b + 4, -7.0, np.float32)
    if given is not None:
        peak0[:b] = given
    d_peak = torch.from_numpy(peak0).cuda()
    torch.cuda.synchronize()
    eng.heatmap_device(d_power.data_ptr(), n, b, d_peak.data_ptr(), d_pix.data_ptr(), peak_given=given is not None)
    eng.synchronize()
    pix, peak = d_pix.cpu().numpy(), d_peak.cpu().numpy()
    assert np.all(pix[b * n:] == 0xA5) and np.all(peak[b:] == -7.0)
    assert given is None or V.same_bits(peak[:b], peak0[:b])
    return pix[: b * n].reshape(b, n), peak[:b]


@pytest.mark.parametrize("n", E.DISPLAY_N)
def test_display(pkg, n):
    assert not V.host_flushes()
    frames = E.display_frames(n)
    with pkg.Engine(n_pixels=16) as eng:
        for name, (frame, M) in frames.items():
            pix, peak = device_display(eng, frame[None])
            m = E.restated_max(frame)
            assert V.same_bits(peak, m), (n, name, peak, m)
            assert np.array_equal(pix[0], pkg.heatmap_u8(frame)), (n, name, "device and host", np.flatnonzero(pix[0] != pkg.heatmap_u8(frame))[:4])
            assert np.array_equal(pix[0], E.restated_levels(frame, m)), (n, name, "device and the restatement")
        # one batch of three different frames, then every frame in one batch: a frame's image does not depend on its neighbours
        names = list(frames)
        for batch in (["stairs_tiny", "nans", "inf_among_finite"], names):
            stack = np.stack([frames[k][0] for k in batch])
            pix, peak = device_display(eng, stack)
            want_peak = np.array([E.restated_max(f) for f in stack], np.float32)
            assert V.same_bits(peak, want_peak), (n, batch)
            for j, k in enumerate(batch):
                assert np.array_equal(pix[j], E.restated_levels(stack[j], want_peak[j])), (n, k, "in a batch")
        # peak_given: above and below the frame's peak, +0, +inf, NaN, -1, every frame with its own
        stack = np.stack([frames[k][0] for k in names])
        for g in range(6):
            given = np.array([E.given_peaks(frames[k][1])[g] for k in names], np.float32)
            pix, _ = device_display(eng, stack, given)
            for j, k in enumerate(names):
                want = E.restated_levels(stack[j], given[j])
                assert np.array_equal(pix[j], want), (n, k, "peak_given", given[j], np.flatnonzero(pix[j] != want)[:4])


# ------------------------------------------------------------------------------------------------ B2: find

def assert_device_is_host(got, count, want, where):
    """count, pixel, power, row and col the same bits; theta and phi within TOL (two maths libraries)."""
    assert np.array_equal(count, want.count), where
    assert np.array_equal(got["pixel"], want.sources["pixel"]), where
    assert V.same_bits(got["power"], want.sources["power"]), where
    assert same_u64(got["row"], want.sources["row"]) and same_u64(got["col"], want.sources["col"]), where
    for name in ("theta", "phi"):
        err = float(np.abs(got[name] - want.sources[name]).max())
        assert err <= TOL, (where, name, err)


def test_find(pkg):
    assert not V.host_flushes()
    cases = 0
    with pkg.Engine(n_pixels=16) as eng:
        for rows, cols, name, frame, kw in E.find_edge_cases():
            got, count = device_find(pkg, eng, frame, rows, cols, **kw)
            assert_device_is_host(got, count, pkg.find_peaks(frame, rows, cols, **kw), (rows, cols, name, kw))
            cases += 1
        assert cases == 324
        # every content of a grid in one launch: each frame's result is its result alone
        for rows, cols in E.FIND_GRIDS:
            contents = E.find_contents(rows, cols)
            stack = np.stack([f for f, _ in contents.values()])
            for min_ratio in E.FIND_RATIOS:
                for radius in E.FIND_RADII:
                    kw = dict(radius=radius, max_sources=4, min_ratio=min_ratio)
                    got, count = device_find(pkg, eng, stack, rows, cols, **kw)
                    for k, frame in enumerate(stack):
                        one = pkg.find_peaks(frame, rows, cols, **kw)
                        assert_device_is_host(got[k: k + 1], count[k: k + 1], one, (rows, cols, list(contents)[k], kw, "in a batch"))
        # the defect: a constant +inf frame has its one source at min_ratio = 0 as at 0.25
        frame = E.find_contents(33, 17)["all_inf"][0]
        for min_ratio in (0.0, 0.25):
            got, count = device_find(pkg, eng, frame, 33, 17, radius=2, max_sources=4, min_ratio=min_ratio)
            assert count[0] == 1 and got["pixel"][0, 0] == 0 and np.isposinf(got["power"][0, 0])


# ------------------------------------------------------------------------------------------------ B3: calibration

def test_calibration(pkg, oracle):
    import torch

    assert not V.host_flushes()
    xyz = pkg.create_antenna()
    off, frac = pkg.build_delay_table(xyz, 4, 4)
    frames = E.calibration_frames()
    for row in E.NAN_ROWS:  # the same 64 rows with the NaN row at each of the five places: one median
        frames[f"nan_row_at_{row}"] = frames["nan_row_0"].copy()
        frames[f"nan_row_at_{row}"][[0, row]] = frames["nan_row_0"][[row, 0]]
    medians = set()
    with engine(pkg, off, frac, 64, 4, 4) as eng:
        for name, X in frames.items():
            want = oracle.calibrate(X)
            d_X = torch.from_numpy(X).cuda()
            torch.cuda.synchronize()
            got = eng.calibrate_device(d_X.data_ptr())
            assert E.same_calibration(got, want), (name, "calibrate_device", got[0].size, want[0].size, got[2], want[2])
            got = eng.calibrate_host(X)
            assert E.same_calibration(got, want), (name, "calibrate_host", got[0].size, want[0].size, got[2], want[2])
            eng.process_samples(X)  # four blocks: the ring is X
            assert V.same_bits(eng.ring_snapshot(), X), name
            got = eng.calibrate_ring()
            assert E.same_calibration(got, want), (name, "calibrate_ring", got[0].size, want[0].size, got[2], want[2])
            if name.startswith("nan_row_at_"):
                medians.add(np.float32(got[2]).view(np.uint32).item())
                assert int(name.rsplit("_", 1)[1]) not in got[0] and got[0].size == 63
            if name.startswith("nan_row_"):
                assert np.isfinite(got[2]) and np.isfinite(got[1]).all()
    assert len(medians) == 1
    assert oracle.calibrate(frames["nan_in_33_rows"])[0].size == 0 and oracle.calibrate(frames["silence"])[0].size == 64


# ------------------------------------------------------------------------------------------------ B4: ingest

def test_ingest_of_extreme_words(pkg, oracle):
    """Raw words INT32_MIN, INT32_MAX, +-2^23, 2^24 + 1 and -1 among 24-bit ones, through awpu_hip_ingest_block (unpack_block_kernel)
    and through awpu_hip_process_blocks (unpack_blocks_kernel): the ring is the restated unpack's bits."""
    rng = np.random.default_rng(14)
    special = np.array([-(1 << 31), (1 << 31) - 1, 1 << 23, -(1 << 23), (1 << 24) + 1, -1, 0, (1 << 23) - 1], np.int64)
    xyz = pkg.create_antenna()
    off, frac = pkg.build_delay_table(xyz, 4, 4)
    wire, blocks = [], []
    for b in range(4):
        stream = rng.integers(-(1 << 23), 1 << 23, size=(256, 256), dtype=np.int64)
        at = rng.integers(0, 256 * 64, 200)
        stream[at // 64, at % 64] = special[np.arange(200) % len(special)]  # (the first 64 channels are the array's)
        stream[b, b] = special[b]
        stream = stream.astype(np.int32)
        wire.append(make_datagrams(stream, counter0=256 * b))
        blocks.append(oracle.unpack_exposure(stream, 64))
    want = np.concatenate(blocks, axis=1)
    assert want.min() == -256.0 and want.max() == 256.0 and (want == 2.0).any()  # INT32_MIN, INT32_MAX (rounded up), 2^24 + 1 (rounded)
    with engine(pkg, off, frac, 64, 4, 4) as one, engine(pkg, off, frac, 64, 4, 4) as run:
        for b in range(4):
            one.ingest_block(wire[b])
        assert V.same_bits(one.ring_snapshot(), want)
        run.process_blocks(b"".join(wire))
        assert V.same_bits(run.ring_snapshot(), want)


# ------------------------------------------------------------------------------------------------ B5: range

@pytest.mark.parametrize("tier", ["dim", "top", "nonfinite"])
def test_range(pkg, tier):
    """5 sources x 7 distances, +inf among the distances: every power is awpu_hip_beams' of awpu_hip_focus_steer_table's entry and
    `best` is awpu_hip_range_pick of those powers."""
    import torch

    assert not V.host_flushes()
    xyz = pkg.create_antenna()
    x = util.hash_frames(64, 1024, seed=33)[0]
    if tier == "nonfinite":
        x = x.copy()
        # (a beam reads 256 samples from its offset on, and the offsets are a little below 256: sample 300 is in every beam, 505 and
        # 232 at the far edges, inside some beams' windows and outside others')
        x[3, 300], x[20, 505], x[40, 232], x[40, 233] = np.inf, np.nan, 3e38, -3e38
    else:
        x = V.scale_pow2(x, V.SCALED[tier])
    theta, phi = directions(5, 17)
    dist = np.array([np.inf, 0.3, 0.7, 1.5, 4.0, np.inf, 40.0])
    d_x = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    torch.cuda.synchronize()
    with pkg.Engine(n_pixels=16, n_streams=64) as eng:
        eng.set_antenna(xyz)
        eng.set_active_mics(None)
        power, best = eng.range(theta, phi, dist, d_frame_ptr=d_x.data_ptr())
        off, frac = pkg.focus_steer_table(xyz, np.repeat(theta, 7), np.repeat(phi, 7), np.tile(dist, 5))
        want, _ = eng.beams(off, frac, d_frame_ptr=d_x.data_ptr(), want_beams=False)
    want = want.reshape(5, 7)
    if tier == "dim":
        assert V.subnormal(power).all()
    if tier == "top":
        assert np.isposinf(power).all()
    if tier == "nonfinite":
        assert not np.isfinite(power).any()  # (the +inf sample is in every beam)
    assert V.same_bits(power, want), (tier, int((V.bits(power) != V.bits(want)).sum()))
    assert best.tobytes() == pkg.range_pick(power, dist).tobytes(), tier


# ------------------------------------------------------------------------------------------------ B6: one run

def test_one_run_through_huge_and_tiny_blocks(pkg):
    """The default mode, 16 x 16, four frames a launch, 12 blocks of samples with blocks 4 and 5 scaled by 2^120 and blocks 8 and 9
    by 2^-64: the watch run and the find run equal their composition -- awpu_hip_process of every shown snapshot, then the host's
    awpu_hip_heatmap_u8 and awpu_hip_find_peaks -- and a frame whose 1024 samples hold no scaled block is the unscaled recording's."""
    assert not V.host_flushes()
    xyz = pkg.create_antenna()
    off, frac = pkg.build_delay_table(xyz, 16, 16)
    plain = util.hash_frames(64, 256 * 12, seed=77)[0]
    samples = plain.copy()
    samples[:, 256 * 4: 256 * 6] = V.scale_pow2(plain[:, 256 * 4: 256 * 6], 120)
    samples[:, 256 * 8: 256 * 10] = V.scale_pow2(plain[:, 256 * 8: 256 * 10], -64)
    snaps = snapshots(samples)
    with engine(pkg, off, frac, 64, 16, 4) as eng:
        want = np.concatenate([eng.process(snaps[k: k + 1]) for k in range(12)])
    assert np.isposinf(want[4:9]).any() and np.isfinite(want[:4]).all() and np.isfinite(want[9:]).all() and (want[9:] > 0).all()
    with engine(pkg, off, frac, 64, 16, 4) as eng:
        watched = eng.watch_samples(samples, 16, 16, want_image=True, want_power=True)
        assert V.same_bits(eng.ring_snapshot(), snaps[-1])
    assert V.same_bits(watched.power, want)
    for k in range(12):
        assert np.array_equal(watched.image[k].reshape(-1), pkg.heatmap_u8(want[k])), k
        assert np.array_equal(watched.image[k].reshape(-1), E.restated_levels(want[k], E.restated_max(want[k]))), k
    for min_ratio in (0.0, 0.25):
        kw = dict(radius=2, max_sources=4, min_ratio=min_ratio)
        with engine(pkg, off, frac, 64, 16, 4) as eng:
            found = eng.find_samples(samples, 16, 16, want_power=True, **kw)
        assert V.same_bits(found.power, want)
        host = pkg.find_peaks(want, 16, 16, **kw)
        assert_device_is_host(found.sources, found.count, host, ("find_samples", min_ratio))
        assert (found.count[3:] >= 1).all(), found.count  # frames of +inf pixels included, at either ratio
    with engine(pkg, off, frac, 64, 16, 4) as eng:
        unscaled = eng.watch_samples(plain, 16, 16, want_image=True, want_power=True)
    clean = [k for k in range(12) if not {4, 5, 8, 9} & set(range(max(k - 3, 0), k + 1))]
    assert clean == [0, 1, 2, 3]  # (with 12 blocks every later frame's window holds a scaled block)
    for k in clean:
        assert V.same_bits(watched.power[k], unscaled.power[k]) and np.array_equal(watched.image[k], unscaled.image[k]), k
    assert not V.same_bits(watched.power[11], unscaled.power[11])  # (the last frame reads the blocks scaled by 2^-64)
