"""Focus and range (include/awpu_hip_focus.h) on the device: the device table builder gives the host builder's bits; a sweep
with a focused table matches the oracle on that table within the project's 1e-5 per pixel; awpu_hip_range equals its
composition -- awpu_hip_focus_steer_table, then awpu_hip_beams -- bit for bit, and its `best` is awpu_hip_range_pick of its
powers; point sources 0.5, 1 and 2 m from the 32 x 8 tile are ranged to the true candidate +-1 and a plane wave to 1 / d <= 0.1;
the three locate runs equal the find run of the same form followed by awpu_hip_range on every shown block's raw snapshot;
refusals leave the ring alone; tools/pcap_sources.py --range writes the distance column."""
import importlib.util

import numpy as np
import pytest

import test_tracker_cpu as R
import util
from test_find_cpu import REPO
from test_gpu_blocks import engine, make_datagrams, snapshots

pytestmark = pytest.mark.gpu

B = 256 * 1032
# (the scene below through the oracle's sweep: the maxima of a shown block are 1, 0.98, 0.60, 0.59, 0.10, ... of its strongest, and
# the first block's snapshot sweeps to an all-zero frame: two sources a block, none in block 0, two unused entries everywhere)
FIND = dict(radius=2, max_sources=4, min_ratio=0.7)
U61 = np.linspace(0.0, 3.0, 61)  # 1 / d of the ranging candidates: 0 (a plane wave), 0.05, ..., 3


def candidates(pkg):
    return pkg.range_candidates(np.inf, 1.0 / 3.0, 61)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ------------------------------------------------------------------------------------------------ tables

@pytest.mark.parametrize("arrays,res", [((1, 1), 16), ((4, 1), 32)])
def test_device_builder_equals_host_builder(pkg, arrays, res):
    """off and frac bit-equal: the 8 x 8 array on 16 x 16 and the 32 x 8 tile on 32 x 32, distance 0.3, 2, 50 and inf, fov 180
    and 90, the whole table and a slice that does not start at row 0."""
    xyz = pkg.create_tiled_antenna(*arrays)
    differing = []
    for fov in (180.0, 90.0):
        for distance in (0.3, 2.0, 50.0, np.inf):
            want = pkg.build_focus_table(xyz, res, res, distance, fov)
            got = pkg.build_focus_table_device(xyz, res, res, distance, fov)
            part = pkg.build_focus_table_device(xyz, res, res, distance, fov, 3, res // 2)
            n_off, n_frac = int((got[0] != want[0]).sum()), int((got[1].view(np.uint32) != want[1].view(np.uint32)).sum())
            print(f"{arrays} fov {fov} d {distance}: {n_off} offsets and {n_frac} fractions of {want[0].size} differ")
            if n_off or n_frac or not np.array_equal(part[0], want[0][3 * res: (3 + res // 2) * res]) or \
                    not same_bits(part[1], want[1][3 * res: (3 + res // 2) * res]):
                differing.append((fov, distance, n_off, n_frac))
    assert not differing, differing


def test_sweep_with_a_focused_table_matches_the_oracle(pkg, oracle):
    """Engine.set_delay_table takes the focused table as it is; the default arithmetic, a point source 2 m from the 32 x 8 tile, a
    32 x 32 grid: every pixel within 1e-5 of the oracle on that table, and the maximum at the source's pixel."""
    S = pkg.synthetic
    spec = S.WorkloadSpec("tile 32 x 8 on 32 x 32", 4, 1, 32)
    xyz = S.geometry(spec)
    off, frac = pkg.build_focus_table(xyz, 32, 32, 2.0)
    frames = S.make_point_frames(xyz, 2, 2.0)
    with engine(pkg, off, frac, 256, 32, 2) as eng:
        power = eng.process(frames)
    for b in range(2):
        rep = util.parity_report(power[b], oracle.das_f32(frames[b], off, frac))
        print(f"frame {b}: max rel err {rep['max_rel_unfloored']:.3g}")
        assert rep["ok"], rep
    assert divmod(int(power[0].argmax()), 32) == S.source_pixel(spec)


# ------------------------------------------------------------------------------------------------ awpu_hip_range

def directions(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 1.4, n), rng.uniform(-np.pi, np.pi, n)


def distances(n, seed):
    """n candidates log-uniform in [0.05 m, 100 m], unsorted, +inf among them: a lone candidate on odd seeds, the first of
    several, and the sixth as well -- the second of a workgroup's four beams."""
    rng = np.random.default_rng(seed)
    d = 10.0 ** rng.uniform(np.log10(0.05), 2.0, n)
    if n > 1 or seed % 2:
        d[0] = np.inf
    if n >= 7:
        d[5] = np.inf
    return d


def check_range_against_composition(pkg, eng, xyz, frame_ptr, n_src, n_dist, seed):
    theta, phi = directions(n_src, seed)
    dist = distances(n_dist, seed + (1 if frame_ptr else 2))  # (a lone candidate: finite on the snapshot, inf on the ring)
    power, best = eng.range(theta, phi, dist, d_frame_ptr=frame_ptr)
    assert power.shape == (n_src, n_dist)
    off, frac = pkg.focus_steer_table(xyz, np.repeat(theta, n_dist), np.repeat(phi, n_dist), np.tile(dist, n_src))
    want, _ = eng.beams(off, frac, d_frame_ptr=frame_ptr, want_beams=False)
    assert same_bits(power, want.reshape(n_src, n_dist)), (n_src, n_dist, int((power.reshape(-1).view(np.uint32) != want.view(np.uint32)).sum()))
    assert best.tobytes() == pkg.range_pick(power, dist).tobytes()
    assert power.min() > 0.0
    return power


@pytest.mark.parametrize("mics", ["all", "keep57_perm", "gains"])
def test_range_equals_the_composition(pkg, oracle, mics):
    """n_src 1, 5 and 32, n_dist 1, 7 and 64 (+inf among the candidates), on a snapshot in device memory and on the ring: every
    power is awpu_hip_beams' of awpu_hip_focus_steer_table's entry, bit for bit, and best is range_pick(power)."""
    import torch

    xyz = pkg.create_antenna()
    frame = pkg.synthetic.make_point_frames(xyz, 1, 1.0, seed=5)[0]
    d_frame = torch.from_numpy(frame).cuda()
    stream = np.zeros((256, 256), np.int32)
    with pkg.Engine(n_pixels=16, n_streams=64) as eng:
        eng.set_antenna(xyz)
        eng.set_active_mics(R.MIC_LISTS["keep57_perm"] if mics == "keep57_perm" else None)
        if mics == "gains":
            eng.set_mic_gains(np.linspace(0.5, 1.5, 64).astype(np.float32))
        for b in range(4):  # the ring: the same wave, quantised to the wire's 24 bits
            stream[:, :64] = np.rint(frame[:, 256 * b: 256 * (b + 1)].astype(np.float64) * 8388608.0).astype(np.int32).T
            eng.ingest_block(make_datagrams(stream, counter0=256 * b))
        seed = 100
        for n_src in (1, 5, 32):
            for n_dist in (1, 7, 64):
                for ptr in (d_frame.data_ptr(), 0):
                    check_range_against_composition(pkg, eng, xyz, ptr, n_src, n_dist, seed)
                    seed += 2


def test_range_on_the_tile_with_a_ragged_list(pkg):
    """256 elements, 205 active mics out of id order, more elements than lanes' first pass covers in one go (n > 256 is the 512
    case below): the maxima and minima run over ALL elements, the beams over the active ones."""
    import torch

    for arrays, name in (((4, 1), "tiled205"), ((4, 2), "tiled509")):
        xyz = pkg.create_tiled_antenna(*arrays)
        n = xyz.shape[1]
        frame = pkg.synthetic.make_point_frames(xyz, 1, 0.7, seed=6)[0]
        d_frame = torch.from_numpy(frame).cuda()
        with pkg.Engine(n_pixels=16, n_streams=n) as eng:
            eng.set_antenna(xyz)
            eng.set_active_mics(R.MIC_LISTS[name])
            check_range_against_composition(pkg, eng, xyz, d_frame.data_ptr(), 5, 7, 300 + n)


def test_ranging_works(pkg):
    """The 32 x 8 tile, candidates 1 / d = linspace(0, 3, 61): point sources at 0.5, 1 and 2 m give the true candidate +-1 (the
    numpy model of the issue: exact hits), a make_frames plane wave an index with 1 / d <= 0.1 (the model: index 0)."""
    import torch

    S = pkg.synthetic
    xyz = pkg.create_tiled_antenna(4, 1)
    cand = candidates(pkg)
    with pkg.Engine(n_pixels=16, n_streams=256) as eng:
        eng.set_antenna(xyz)
        eng.set_active_mics(None)
        for d, want in ((0.5, 40), (1.0, 20), (2.0, 10)):
            d_frame = torch.from_numpy(S.make_point_frames(xyz, 1, d)[0]).cuda()
            power, best = eng.range(S.SOURCE_THETA, S.SOURCE_PHI, cand, d_frame_ptr=d_frame.data_ptr())
            j = int(best["index"][0])
            print(f"source at {d} m: candidate {j} (1 / d = {U61[j]:.2f}), refined {best['distance'][0]:.4f} m, neighbours "
                  f"{power[0, j - 1] / power[0, j]:.3f} {power[0, j + 1] / power[0, j]:.3f} of the peak")
            assert abs(j - want) <= 1, (d, j)
        d_frame = torch.from_numpy(S.make_frames(xyz, 1)[0]).cuda()
        power, best = eng.range(S.SOURCE_THETA, S.SOURCE_PHI, cand, d_frame_ptr=d_frame.data_ptr())
        print(f"plane wave: candidate {int(best['index'][0])}, refined {best['distance'][0]} m")
        assert U61[int(best["index"][0])] <= 0.1


# ------------------------------------------------------------------------------------------------ the locate runs

@pytest.fixture(scope="module")
def scene(pkg, oracle):
    """The reference's array on a 32 x 32 grid, 12 blocks of a point source 1 m away in noise (one long history), quantised to the
    wire's 24 bits and put on the wire stream by stream -- the ingest mirrors every other group of eight, so what the array hears
    is a scrambled wave with several maxima: (off, frac, xyz, wire, samples, candidates)."""
    S = pkg.synthetic
    xyz = pkg.create_antenna()
    off, frac = pkg.build_delay_table(xyz, 32, 32)
    wave = S.make_point_frames(xyz, 1, 1.0, seed=9, hist=256 * 12)[0]
    ints = np.rint(wave.astype(np.float64) * 8388608.0).astype(np.int32)
    wire, blocks = [], []
    for b in range(12):
        stream = np.zeros((256, 256), np.int32)
        stream[:, :64] = ints[:, 256 * b: 256 * (b + 1)].T
        wire.append(make_datagrams(stream, counter0=256 * b))
        blocks.append(oracle.unpack_exposure(stream, 64))
    cand = np.r_[np.inf, 1.0 / np.linspace(0.25, 3.0, 6)]  # 7 candidates: three of a workgroup's four beams in the second
    return off, frac, xyz, b"".join(wire), np.concatenate(blocks, axis=1), cand


def locate_engine(pkg, scene, max_batch, band=None):
    off, frac, xyz = scene[:3]
    eng = engine(pkg, off, frac, 64, 32, max_batch)
    eng.set_antenna(xyz)
    if band is not None:
        eng.set_band(band)
    return eng


def composition(pkg, scene, max_batch, first, every, band=None):
    """The find run of the samples form, then range on every shown block's raw snapshot at the directions the run reports."""
    import torch

    samples, cand = scene[4], scene[5]
    snaps = snapshots(samples)
    with locate_engine(pkg, scene, max_batch, band) as eng:
        found = eng.find_samples(samples, 32, 32, first=first, every=every, want_power=True, **FIND)
        after = eng.ring_snapshot()
        ranges = np.zeros((len(found), 4), pkg.binding.RANGE_DTYPE)
        ranges["index"] = -1
        rpower = np.zeros((len(found), 4, cand.size), np.float32)
        for j in range(len(found)):
            n = int(found.count[j])
            if n:
                d_frame = torch.from_numpy(np.ascontiguousarray(snaps[first + j * every])).cuda()
                rpower[j, :n], ranges[j, :n] = eng.range(found.sources["theta"][j, :n], found.sources["phi"][j, :n], cand, d_frame_ptr=d_frame.data_ptr())
    return found, ranges, rpower, after


def assert_located(got, want, where):
    found, ranges, rpower, _ = want
    assert got.sources.tobytes() == found.sources.tobytes() and np.array_equal(got.count, found.count), where
    assert got.next_first == found.next_first, where
    assert got.ranges.tobytes() == ranges.tobytes(), (where, got.ranges, ranges)
    assert got.range_power is None or same_bits(got.range_power, rpower), where


@pytest.mark.parametrize("max_batch", [2, 32])
@pytest.mark.parametrize("first,every", [(0, 1), (1, 3)])
def test_locate_runs_equal_the_composition(pkg, scene, max_batch, first, every):
    """locate_blocks, locate_samples and locate_samples_device == find_samples, then range on each shown snapshot; max_batch 2
    cuts the run into several pieces; the powers are the find run's and so is the ring; unused entries have index -1 and zeros."""
    import torch

    off, frac, xyz, wire, samples, cand = scene
    want = composition(pkg, scene, max_batch, first, every)
    found, ranges, rpower, ring = want
    n_frames = len(found)
    assert n_frames == len(range(first, 12, every)) and found.count[-1] >= 1 and found.count.min() < 4
    unused = np.arange(4)[None, :] >= found.count[:, None]
    assert np.all(ranges["index"][unused] == -1) and np.all(ranges["index"][~unused] >= 0)
    with locate_engine(pkg, scene, max_batch) as eng:
        got = eng.locate_blocks(wire, 32, 32, cand, first=first, every=every, want_power=True, want_range_power=True, **FIND)
        assert_located(got, want, "blocks")
        assert np.array_equal(got.power, found.power) and np.array_equal(eng.ring_snapshot(), ring)
        assert np.all(got.ranges["power"][unused] == 0.0) and np.all(got.ranges["distance"][unused] == 0.0) and not got.range_power[unused].any()
    with locate_engine(pkg, scene, max_batch) as eng:
        got = eng.locate_samples(samples, 32, 32, cand, first=first, every=every, **FIND)  # the ranges alone
        assert got.power is None and got.range_power is None
        assert_located(got, want, "samples")
        assert np.array_equal(eng.ring_snapshot(), ring)
    d_in = torch.from_numpy(np.ascontiguousarray(samples)).cuda()
    for with_power in (True, False):
        d_sources = torch.full((n_frames * 4 * 40 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        d_count = torch.full((n_frames + 4,), -7, dtype=torch.int32, device="cuda")
        d_ranges = torch.full((n_frames * 4 * 16 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        d_rpower = torch.full((n_frames * 4 * cand.size + 16,), -7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        with locate_engine(pkg, scene, max_batch) as eng:
            nxt = eng.locate_samples_device(d_in.data_ptr(), samples.shape[1], 12, 32, 32, cand, d_sources.data_ptr(), d_count.data_ptr(),
                                            d_ranges.data_ptr(), first=first, every=every,
                                            d_range_power_ptr=d_rpower.data_ptr() if with_power else 0, **FIND)
            eng.synchronize()
            raw, count, rraw, rp = d_sources.cpu().numpy(), d_count.cpu().numpy(), d_ranges.cpu().numpy(), d_rpower.cpu().numpy()
            assert np.all(raw[n_frames * 160:] == 0xA5) and np.all(count[n_frames:] == -7) and np.all(rraw[n_frames * 64:] == 0xA5)
            assert np.all(rp[n_frames * 4 * cand.size:] == -7.0) and (with_power or np.all(rp == -7.0))
            dev = pkg.binding.LocateResult(raw[: n_frames * 160].view(pkg.binding.SOURCE_DTYPE).reshape(n_frames, 4), count[:n_frames], None, nxt,
                                           rraw[: n_frames * 64].view(pkg.binding.RANGE_DTYPE).reshape(n_frames, 4),
                                           rp[: n_frames * 4 * cand.size].reshape(n_frames, 4, cand.size) if with_power else None)
            assert_located(dev, want, "device")
            assert np.array_equal(eng.ring_snapshot(), ring)


def test_split_runs_and_a_band(pkg, scene):
    """One run == the recording split at block 5 and continued with next_first; a band on the handle changes the sources -- they
    are the band's -- and leaves the ranges' definition: raw samples at the directions the run reports."""
    off, frac, xyz, wire, samples, cand = scene
    want = composition(pkg, scene, 4, 1, 3)
    with locate_engine(pkg, scene, 4) as eng:
        a = eng.locate_blocks(wire[: 5 * B], 32, 32, cand, first=1, every=3, want_range_power=True, **FIND)
        b = eng.locate_samples(samples[:, 256 * 5:], 32, 32, cand, first=a.next_first, every=3, want_range_power=True, **FIND)
        assert len(a) == 2 and len(b) == 2 and b.next_first == want[0].next_first
        assert np.concatenate([a.sources, b.sources]).tobytes() == want[0].sources.tobytes()
        assert np.concatenate([a.ranges, b.ranges]).tobytes() == want[1].tobytes()
        assert same_bits(np.concatenate([a.range_power, b.range_power]), want[2])
        assert np.array_equal(eng.ring_snapshot(), want[3])
    band = pkg.band_design(6375.0, 9000.0)
    banded = composition(pkg, scene, 4, 0, 2, band=band)
    plain = composition(pkg, scene, 4, 0, 2)
    assert banded[0].sources.tobytes() != plain[0].sources.tobytes() and banded[0].count[-1] >= 1
    with locate_engine(pkg, scene, 4, band=band) as eng:
        got = eng.locate_blocks(wire, 32, 32, cand, first=0, every=2, want_range_power=True, **FIND)
        assert_located(got, banded, "band")


def test_refusals_leave_the_ring(pkg, scene):
    """No antenna: AWPU_ERR_STATE; bad candidates, a null ranges pointer, the find run's own refusals: AWPU_ERR_INVALID; the ring
    and the outputs as they were, and the handle still works."""
    import torch

    off, frac, xyz, wire, samples, cand = scene
    ST, INV = pkg.binding.ERR_STATE, pkg.binding.ERR_INVALID

    def refused(eng, status, distance=cand, rows=32, cols=32, **kw):
        before = eng.ring_snapshot()
        with pytest.raises(pkg.AwpuError) as ei:
            eng.locate_blocks(wire[B: 4 * B], rows, cols, distance, every=2, **kw)
        assert ei.value.status == status
        with pytest.raises(pkg.AwpuError) as ei:
            eng.locate_samples(samples[:, 256: 1024], rows, cols, distance, every=2, **kw)
        assert ei.value.status == status
        d_in = torch.from_numpy(np.ascontiguousarray(samples[:, 256: 1024])).cuda()
        d_sources = torch.full((2 * 4 * 40,), 0xA5, dtype=torch.uint8, device="cuda")
        d_count = torch.full((2,), -7, dtype=torch.int32, device="cuda")
        d_ranges = torch.full((2 * 4 * 16,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(pkg.AwpuError) as ei:
            eng.locate_samples_device(d_in.data_ptr(), 768, 3, rows, cols, distance, d_sources.data_ptr(), d_count.data_ptr(), d_ranges.data_ptr(),
                                      every=2, **kw)
        assert ei.value.status == status
        eng.synchronize()
        assert bool((d_sources == 0xA5).all()) and bool((d_count == -7).all()) and bool((d_ranges == 0xA5).all())
        assert np.array_equal(eng.ring_snapshot(), before)

    with engine(pkg, off, frac, 64, 32, 4) as eng:
        eng.ingest_block(wire[:B])
        refused(eng, ST)  # no antenna
        with pytest.raises(pkg.AwpuError) as ei:
            eng.range(0.3, 1.0, cand)
        assert ei.value.status == ST
        eng.set_antenna(xyz)
        for bad in (np.array([1.0, 0.0]), np.array([1.0, -2.0]), np.array([np.nan]), np.ones(65), np.ones(0)):
            refused(eng, INV, distance=bad)
            with pytest.raises(pkg.AwpuError) as ei:
                eng.range(0.3, 1.0, bad)
            assert ei.value.status == INV
        for theta, phi in ((np.nan, 0.0), (0.1, np.inf), (np.zeros(33), np.zeros(33))):
            with pytest.raises(pkg.AwpuError) as ei:
                eng.range(theta, phi, cand)
            assert ei.value.status == INV
        refused(eng, INV, rows=16, cols=32)  # the find run's: rows x cols is not the grid
        refused(eng, INV, radius=9)
        ring = eng.ring_snapshot()
        power, best = eng.range(0.3, 1.0, cand)  # the ring form, after all that
        assert power.shape == (1, 7) and best["index"][0] >= 0 and np.array_equal(eng.ring_snapshot(), ring)
        assert len(eng.locate_blocks(wire[B: 4 * B], 32, 32, cand, every=2, **FIND)) == 2
    with pkg.Engine(n_pixels=1024, n_streams=64, hist=512) as eng:  # a d_frame of fewer than 513 samples a stream
        eng.set_antenna(xyz)
        eng.set_active_mics(None)
        d_frame = torch.zeros((64, 512), dtype=torch.float32, device="cuda")
        with pytest.raises(pkg.AwpuError) as ei:
            eng.range(0.3, 1.0, cand, d_frame_ptr=d_frame.data_ptr())
        assert ei.value.status == pkg.binding.ERR_RANGE


def test_pcap_sources_tool_ranges(pkg, tmp_path):
    """tools/pcap_sources.py --focus 1 --range 0.33333:inf:13 on a 6-block capture of a point source 1 m from the reference's array:
    the lines parse back to what locate_blocks returns for the same blocks, distance column included."""
    from test_blocks_cpu import udp_frame, write_pcap

    spec = importlib.util.spec_from_file_location("pcap_sources", REPO / "tools" / "pcap_sources.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    xyz = pkg.create_antenna()
    wave = pkg.synthetic.make_point_frames(xyz, 1, 1.0, seed=9, hist=256 * 6)[0]
    ints = np.rint(wave.astype(np.float64) * 8388608.0).astype(np.int32)
    wire = []
    for b in range(6):
        stream = np.zeros((256, 256), np.int32)
        stream[:, :64] = ints[:, 256 * b: 256 * (b + 1)].T
        wire.append(make_datagrams(stream, counter0=256 * b))
    wire = b"".join(wire)
    write_pcap(tmp_path / "rec.pcap", [udp_frame(wire[k: k + 1032], 21844) for k in range(0, 6 * B, 1032)])
    out = tmp_path / "sources.csv"
    assert tool.main([str(tmp_path / "rec.pcap"), "--port", "21844", "--cols", "32", "--every", "2", "--chunk", "4", "--max-batch", "4",
                      "--max-sources", "3", "--focus", "1.0", "--range", "0.25:inf:13", "--out", str(out)]) == 0
    back = tool.read_rows(out)
    assert "distance" in back.dtype.names
    cand = pkg.range_candidates(0.25, np.inf, 13)
    off, frac = pkg.build_focus_table(xyz, 32, 32, 1.0)
    with engine(pkg, off, frac, 64, 32, 4) as eng:
        eng.set_antenna(xyz)
        want = eng.locate_blocks(wire, 32, 32, cand, every=2, radius=2, max_sources=3, min_ratio=0.25)
    assert len(back) == int(want.count.sum()) >= 2
    k = 0
    for j, n in enumerate(want.count):
        for rank in range(n):
            assert (back[k]["block"], back[k]["rank"], back[k]["pixel"]) == (2 * j, rank, want.sources[j, rank]["pixel"])
            assert back[k]["theta"] == want.sources[j, rank]["theta"] and back[k]["distance"] == want.ranges[j, rank]["distance"]
            k += 1
