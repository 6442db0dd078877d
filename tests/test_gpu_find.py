"""Finding sources (include/awpu_hip_find.h) on the device: awpu_hip_find_peaks_device equals the host definition (integers
and powers equal, doubles within 1e-12) on every case of tests/test_find_cpu.py and on batches and large tie-heavy frames; the
three run forms equal their composition -- the watch run asked for powers, then awpu_hip_find_peaks of every shown row -- with
the watch run's powers and ring, however the recording is split or mixed with the other run calls; two plane waves are found
where they come from; refusals leave the ring and the outputs alone."""
import importlib.util

import numpy as np
import pytest

from test_find_cpu import MAX_SOURCES, REPO, TOL, contents, find_cases
from test_gpu_blocks import engine, make_datagrams
from test_gpu_watch import ref100  # noqa: F401  (the reference's array on a 100 x 100 grid, 37 blocks)

pytestmark = pytest.mark.gpu

B = 256 * 1032
FIND = dict(radius=2, max_sources=4, min_ratio=0.25)


def device_find(pkg, eng, frames, rows, cols, **find):
    """find_peaks_device of frames [n, rows * cols] -> (sources [n, max_sources], count [n]); nothing is written past either."""
    import torch

    frames = np.ascontiguousarray(frames, np.float32).reshape(-1, rows * cols)
    n, ms = len(frames), find.get("max_sources", 4)
    d_power = torch.from_numpy(frames).cuda()
    d_sources = torch.full((n * ms * 40 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    d_count = torch.full((n + 4,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.find_peaks_device(d_power.data_ptr(), n, rows, cols, d_sources.data_ptr(), d_count.data_ptr(), **find)
    eng.synchronize()
    raw, count = d_sources.cpu().numpy(), d_count.cpu().numpy()
    assert np.all(raw[n * ms * 40:] == 0xA5) and np.all(count[n:] == -7)
    return raw[: n * ms * 40].view(pkg.binding.SOURCE_DTYPE).reshape(n, ms), count[:n]


def assert_equal_to_host(got, count, want, where):
    assert np.array_equal(count, want.count), where
    assert np.array_equal(got["pixel"], want.sources["pixel"]), where
    assert np.array_equal(got["power"].view(np.uint32), want.sources["power"].view(np.uint32)), where
    for name in ("row", "col", "theta", "phi"):
        err = float(np.abs(got[name] - want.sources[name]).max())
        assert err <= TOL, (where, name, err)


def test_device_equals_host_on_every_cpu_case(pkg):
    """Item 1: every (grid, content, radius, thresholds, max_sources) of tests/test_find_cpu.py."""
    worst, cases = 0.0, 0
    with pkg.Engine(n_pixels=16) as eng:  # (no delay table, no mic list: the peak pass needs neither)
        for rows, cols, name, frame, radius, min_ratio, min_power in find_cases():
            for max_sources in MAX_SOURCES:
                kw = dict(radius=radius, max_sources=max_sources, min_power=min_power, min_ratio=min_ratio)
                got, count = device_find(pkg, eng, frame, rows, cols, **kw)
                want = pkg.find_peaks(frame, rows, cols, **kw)
                assert_equal_to_host(got, count, want, (rows, cols, name, kw))
                worst = max([worst] + [float(np.abs(got[f] - want.sources[f]).max()) for f in ("row", "col", "theta", "phi")])
                cases += 1
    print(f"{cases} cases: worst |device - host| over row, col, theta, phi = {worst:.3g}")
    assert cases > 1500


@pytest.mark.parametrize("n_frames", [1, 3, 130])
def test_batches_of_frames(pkg, n_frames):
    """Item 1: frames are independent -- a batch of every content, repeated with other seeds, on an odd grid and at fov 90."""
    rows, cols = 33, 17
    frames = np.stack([f for seed in range(-(-n_frames // 8)) for f in contents(rows, cols, seed=50 + seed).values()])[:n_frames]
    with pkg.Engine(n_pixels=16) as eng:
        for kw in (dict(radius=1, max_sources=32), dict(radius=2, max_sources=4, min_ratio=0.25, fov_deg=90.0), dict(radius=8, max_sources=1)):
            got, count = device_find(pkg, eng, frames, rows, cols, **kw)
            assert_equal_to_host(got, count, pkg.find_peaks(frames, rows, cols, **kw), (n_frames, kw))


@pytest.mark.parametrize("res", [128, 256])
def test_large_tie_heavy_frames(pkg, res):
    """Item 1: one frame of integers 0 .. 3 -- thousands of equal neighbours, more peaks than entries -- at 128 x 128 and 256 x 256
    (sixteen and sixty-four pixels a lane), and a device group answering from its first device."""
    frame = np.random.default_rng(res).integers(0, 4, res * res).astype(np.float32)
    with pkg.Engine(n_pixels=16) as eng, pkg.Engine(n_pixels=256, n_streams=64, max_batch=4, grid_columns=16, devices=[0, 0]) as group:
        for kw in (dict(radius=1, max_sources=32), dict(radius=3, max_sources=32, min_ratio=1.0), dict(radius=8, max_sources=4, min_power=2.5)):
            want = pkg.find_peaks(frame, res, res, **kw)
            assert want.count[0] == 32 if kw["radius"] == 1 else want.count[0] >= 1
            got, count = device_find(pkg, eng, frame, res, res, **kw)
            assert_equal_to_host(got, count, want, (res, kw))
        got, count = device_find(pkg, group, frame, res, res, **kw)
        assert_equal_to_host(got, count, want, (res, "group"))


# ------------------------------------------------------------------------------------------------ the runs

def c1_recording(pkg, oracle):
    """c1 (64 mics, 32 x 32): table, antenna, and 23 blocks of a plane wave in noise (synthetic.make_frames, one long history),
    quantised to the wire's 24 bits: (off, frac, xyz, wire, samples)."""
    S = pkg.synthetic
    spec = S.WORKLOADS["c1"]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    wave = S.make_frames(xyz, 1, seed=77, hist=256 * 23)[0]
    ints = np.rint(wave.astype(np.float64) * 8388608.0).astype(np.int32)
    wire, blocks = [], []
    for b in range(23):
        stream = np.zeros((256, 256), np.int32)
        stream[:, :64] = ints[:, 256 * b: 256 * (b + 1)].T
        wire.append(make_datagrams(stream, counter0=256 * b))
        blocks.append(oracle.unpack_exposure(stream, 64))
    return off, frac, xyz, b"".join(wire), np.concatenate(blocks, axis=1)


@pytest.fixture(scope="module")
def c1(pkg, oracle):
    return c1_recording(pkg, oracle)


def same_sources(a, b):
    return a.sources.tobytes() == b.sources.tobytes() and np.array_equal(a.count, b.count)


@pytest.mark.parametrize("max_batch", [1, 4, 32])
@pytest.mark.parametrize("first,every", [(0, 1), (2, 3), (5, 7)])
def test_run_forms_equal_the_composition(pkg, c1, max_batch, first, every):
    """Item 2: find_blocks, find_samples and find_samples_device == watch_samples(power) then find_peaks; the powers, when asked
    for, are the watch run's bits; the ring afterwards is the watch run's."""
    import torch

    off, frac, _, wire, samples = c1
    n_frames = len(range(first, 23, every))
    with engine(pkg, off, frac, 64, 32, max_batch) as ref:
        watched = ref.watch_samples(samples, 32, 32, first=first, every=every, want_image=False, want_power=True)
        ring, frames_swept = ref.ring_snapshot(), ref.stats().frames
    want = pkg.find_peaks(watched.power, 32, 32, **FIND)
    assert len(watched.power) == n_frames and want.count[-1] >= 1  # (the first blocks' snapshots may sweep to all-zero frames: count 0)

    def check(got, eng, power):
        assert got.next_first == watched.next_first and len(got) == n_frames
        assert_equal_to_host(got.sources, got.count, want, (max_batch, first, every))
        assert np.array_equal(got.sources["row"], want.sources["row"]) and np.array_equal(got.sources["col"], want.sources["col"])
        assert power is None or np.array_equal(power, watched.power)
        assert np.array_equal(eng.ring_snapshot(), ring) and eng.stats().frames == frames_swept

    with engine(pkg, off, frac, 64, 32, max_batch) as eng:
        got = eng.find_blocks(wire, 32, 32, first=first, every=every, want_power=True, **FIND)
        check(got, eng, got.power)
    with engine(pkg, off, frac, 64, 32, max_batch) as eng:
        got = eng.find_samples(samples, 32, 32, first=first, every=every, want_power=True, **FIND)
        check(got, eng, got.power)
    with engine(pkg, off, frac, 64, 32, max_batch) as eng:  # the sources alone: no power crosses PCIe
        alone = eng.find_blocks(wire, 32, 32, first=first, every=every, **FIND)
        assert alone.power is None and same_sources(alone, got)
        check(alone, eng, None)
    d_in = torch.from_numpy(np.ascontiguousarray(samples)).cuda()
    for with_power in (True, False):
        d_sources = torch.full((n_frames * 4 * 40 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        d_count = torch.full((n_frames + 4,), -7, dtype=torch.int32, device="cuda")
        d_power = torch.zeros((n_frames, 32 * 32), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        with engine(pkg, off, frac, 64, 32, max_batch) as eng:
            nxt = eng.find_samples_device(d_in.data_ptr(), samples.shape[1], 23, 32, 32, d_sources.data_ptr(), d_count.data_ptr(),
                                          first=first, every=every, d_power_ptr=d_power.data_ptr() if with_power else 0, **FIND)
            eng.synchronize()
            raw, count = d_sources.cpu().numpy(), d_count.cpu().numpy()
            assert np.all(raw[n_frames * 160:] == 0xA5) and np.all(count[n_frames:] == -7)
            dev = pkg.binding.FindResult(raw[: n_frames * 160].view(pkg.binding.SOURCE_DTYPE).reshape(n_frames, 4), count[:n_frames], None, nxt)
            assert same_sources(dev, got)
            check(dev, eng, d_power.cpu().numpy() if with_power else None)


def test_split_and_interleaved_runs(pkg, ref100):  # noqa: F811
    """Item 3: one call == the recording split at random points and continued with next_first == a run whose skipped blocks go to
    process_blocks and listen_blocks instead (the exact mode on the reference's 100 x 100 grid, where a frame's bits do not
    depend on its batch: tests/test_gpu_watch.py::test_split_and_interleaved_runs)."""
    off, frac, wire, samples, xyz = ref100
    kw = dict(radius=3, max_sources=8, min_ratio=0.1)
    rng = np.random.default_rng(43)
    for first0, every in ((2, 3), (0, 1), (5, 7)):
        with engine(pkg, off, frac, 64, 100, 4) as one:
            whole = one.find_blocks(wire, 100, 100, first=first0, every=every, want_power=True, **kw)
            ring = one.ring_snapshot()
        assert whole.count[-1] >= 1
        for _ in range(2):
            cuts = [0] + sorted(rng.choice(np.arange(1, 37), size=int(rng.integers(1, 9)), replace=False).tolist()) + [37]
            with engine(pkg, off, frac, 64, 100, 4) as eng:
                parts, first = [], first0
                for a, b in zip(cuts, cuts[1:]):
                    parts.append(eng.find_blocks(wire[a * B: b * B], 100, 100, first=first, every=every, want_power=(a % 2 == 0), **kw))
                    first = parts[-1].next_first
                assert np.concatenate([p.sources for p in parts]).tobytes() == whole.sources.tobytes(), (every, cuts)
                assert np.array_equal(np.concatenate([p.count for p in parts]), whole.count)
                assert first == whole.next_first and np.array_equal(eng.ring_snapshot(), ring)
    # shown: 2, 5, ..., 35; blocks 9-10 and 21-22 are skipped ones, given to the other calls
    with engine(pkg, off, frac, 64, 100, 4) as one:
        whole = one.find_blocks(wire, 100, 100, first=2, every=3, **kw)
        ring = one.ring_snapshot()
    with engine(pkg, off, frac, 64, 100, 4) as eng:
        eng.set_antenna(xyz)
        a = eng.find_blocks(wire[: 9 * B], 100, 100, first=2, every=3, **kw)
        assert a.next_first == 2 and len(a) == 3
        eng.process_blocks(wire[9 * B: 11 * B])
        b = eng.find_samples(samples[:, 256 * 11: 256 * 21], 100, 100, first=0, every=3, **kw)
        assert b.next_first == 2 and len(b) == 4
        eng.listen_blocks(wire[21 * B: 23 * B], 0.3, 1.0, 0.03, 5e-5, 0, 1.5, want_trail=False)
        c = eng.watch_blocks(wire[23 * B: 30 * B], 100, 100, first=0, every=3, want_power=True)  # a watch run in between: the same frames
        assert c.next_first == 2 and len(c) == 3
        d = eng.find_blocks(wire[30 * B:], 100, 100, first=2, every=3, **kw)
        assert d.next_first == 1 and len(d) == 2
        got = np.concatenate([a.sources, b.sources, pkg.find_peaks(c.power, 100, 100, **kw).sources, d.sources])
        assert np.array_equal(got["pixel"], whole.sources["pixel"]) and np.array_equal(got["power"], whole.sources["power"])
        assert np.array_equal(got["row"], whole.sources["row"]) and np.abs(got["theta"] - whole.sources["theta"]).max() <= TOL
        assert np.array_equal(eng.ring_snapshot(), ring)


def test_two_plane_waves_are_found(pkg, oracle):
    """Item 4, on the CPU oracle's heatmap: c1 at fov 180, the synthetic source plus 0.7 of a second wave from theta 0.5,
    phi -2.0; radius 2, four entries, min_ratio 0.25 -> two sources, at pixels (19, 20) and (9, 12) +- 1.  (On that heatmap the
    third maximum is 8.5 x below the second: the threshold has room on both sides.)  The device finds the same two in the
    engine's own heatmap, and their directions are the waves'."""
    S = pkg.synthetic
    spec = S.WORKLOADS["c1"]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    frame = S.make_frames(xyz, 1, seed=1)[0] + np.float32(0.7) * S.make_frames(xyz, 1, seed=2, theta=0.5, phi=-2.0)[0]
    heat = oracle.das_f32(frame, off, frac).astype(np.float32)
    got = pkg.find_peaks(heat, 32, 32, **FIND)
    every = pkg.find_peaks(heat, 32, 32, radius=2, max_sources=4)
    print("sources (pixel, power):", [(divmod(int(s["pixel"]), 32), float(s["power"])) for s in every.sources[0][: every.count[0]]])
    assert got.count[0] == 2
    for s, (r, c) in zip(got.sources[0], ((19, 20), (9, 12))):
        pr, pc = divmod(int(s["pixel"]), 32)
        assert abs(pr - r) <= 1 and abs(pc - c) <= 1, (pr, pc)
        assert abs(s["row"] - pr) <= 0.5 and abs(s["col"] - pc) <= 0.5
    with engine(pkg, off, frac, 64, 32, 1) as eng:
        power = eng.process(frame)
        dev, count = device_find(pkg, eng, power, 32, 32, **FIND)
    assert count[0] == 2 and np.array_equal(dev["pixel"], got.sources["pixel"])
    # a pixel is 1 / 16 in sine space: the refined directions are within one pixel of the waves'
    for s, (theta, phi) in zip(dev[0], ((S.SOURCE_THETA, S.SOURCE_PHI), (0.5, -2.0))):
        want = np.sin(theta) * np.array([np.cos(phi), np.sin(phi)])
        have = np.sin(s["theta"]) * np.array([np.cos(s["phi"]), np.sin(s["phi"])])
        assert np.abs(have - want).max() <= 1.0 / 16.0, (have, want)


def test_refusals_leave_the_ring(pkg, c1):
    """Item 5: a device group and a missing table / mic list: AWPU_ERR_STATE; a handle that holds a slab of the grid, a grid that is
    not the handle's, hist != 1024, a bad request: AWPU_ERR_INVALID; the ring and the outputs as they were."""
    import torch

    off, frac, _, wire, samples = c1
    ST, INV = pkg.binding.ERR_STATE, pkg.binding.ERR_INVALID

    def refused(eng, status, rows=32, cols=32, **kw):
        before = eng.ring_snapshot()
        with pytest.raises(pkg.AwpuError) as ei:
            eng.find_blocks(wire[B: 4 * B], rows, cols, every=2, **kw)
        assert ei.value.status == status
        with pytest.raises(pkg.AwpuError) as ei:
            eng.find_samples(samples[:, 256: 1024], rows, cols, every=2, **kw)
        assert ei.value.status == status
        d_in = torch.from_numpy(np.ascontiguousarray(samples[:, 256: 1024])).cuda()
        d_sources = torch.full((2 * 4 * 40,), 0xA5, dtype=torch.uint8, device="cuda")
        d_count = torch.full((2,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(pkg.AwpuError) as ei:
            eng.find_samples_device(d_in.data_ptr(), 768, 3, rows, cols, d_sources.data_ptr(), d_count.data_ptr(), every=2, **kw)
        assert ei.value.status == status
        eng.synchronize()
        assert bool((d_sources == 0xA5).all()) and bool((d_count == -7).all())
        assert np.array_equal(eng.ring_snapshot(), before)

    with pkg.Engine(n_pixels=1024, n_streams=64, max_batch=4) as eng:  # no table, then no mic list
        eng.ingest_block(wire[:B])
        refused(eng, ST)
        eng.set_delay_table(off, frac)
        refused(eng, ST)
        eng.set_active_mics(None)
        refused(eng, INV, rows=16, cols=32)    # rows x cols is not the grid
        refused(eng, INV, rows=64, cols=64)
        for bad in (dict(radius=0), dict(radius=9), dict(max_sources=33), dict(min_ratio=1.5), dict(min_power=-1.0), dict(fov_deg=0.0)):
            refused(eng, INV, **bad)
        assert len(eng.find_blocks(wire[B: 4 * B], 32, 32, every=2, **FIND)) == 2  # the handle still works
    with pkg.Engine(n_pixels=1024, n_streams=64, max_batch=4, grid_columns=32, devices=[0, 0]) as eng:  # a device group
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        eng.ingest_block(wire[:B])
        refused(eng, ST)
    with pkg.Engine(n_pixels=1024, n_streams=64, max_batch=4, pixel_begin=256, pixel_count=512) as eng:  # a slab of the grid
        eng.set_delay_table(off[256:768], frac[256:768])
        eng.set_active_mics(None)
        eng.ingest_block(wire[:B])
        refused(eng, INV)
    with pkg.Engine(n_pixels=1024, n_streams=64, hist=2048, max_batch=4) as eng:
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        with pytest.raises(pkg.AwpuError) as ei:
            eng.find_blocks(wire[: 2 * B], 32, 32)
        assert ei.value.status == INV


def test_device_run_then_host_run_are_ordered(pkg):
    """Item 6: a long asynchronous device-form find run on another stream, then at once a host-form run on the same handle: the
    host run continues the ring the device run leaves.  Both equal one call over the whole recording."""
    import torch

    S = pkg.synthetic
    spec = S.WORKLOADS["headline"]
    off, frac = S.delay_table(spec, S.geometry(spec))
    rng = np.random.default_rng(6)
    n, cut, every, res = 130, 121, 2, spec.res
    samples = (rng.integers(-(1 << 21), 1 << 21, size=(spec.n_mics, 256 * n)) / 8388608.0).astype(np.float32)
    kw = dict(radius=2, max_sources=8)
    with engine(pkg, off, frac, spec.n_mics, res, 32) as one, engine(pkg, off, frac, spec.n_mics, res, 32) as two:
        want = one.find_samples(samples, res, res, first=1, every=every, want_power=True, **kw)
        assert want.count[-1] >= 1
        n_dev, nxt = pkg.binding.watch_count(cut, 1, every)
        d_in = torch.from_numpy(np.ascontiguousarray(samples[:, : 256 * cut])).cuda()
        d_sources = torch.zeros((n_dev * 8 * 40,), dtype=torch.uint8, device="cuda")
        d_count = torch.zeros((n_dev,), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            assert two.find_samples_device(d_in.data_ptr(), 256 * cut, cut, res, res, d_sources.data_ptr(), d_count.data_ptr(), first=1,
                                           every=every, stream=side.cuda_stream, **kw) == nxt
        tail = two.find_samples(samples[:, 256 * cut:], res, res, first=nxt, every=every, want_power=True, **kw)  # while the device run is going
        torch.cuda.synchronize()
        assert tail.sources.tobytes() == want.sources[n_dev:].tobytes() and np.array_equal(tail.count, want.count[n_dev:])
        assert np.array_equal(tail.power, want.power[n_dev:])
        assert d_sources.cpu().numpy().tobytes() == want.sources[:n_dev].tobytes()
        assert np.array_equal(d_count.cpu().numpy(), want.count[:n_dev])
        assert np.array_equal(two.ring_snapshot(), one.ring_snapshot())


def test_pcap_sources_tool(pkg, c1, tmp_path):
    """tools/pcap_sources.py on a synthetic capture: the lines parse back to what find_blocks returns for the same blocks."""
    from test_blocks_cpu import udp_frame, write_pcap

    spec = importlib.util.spec_from_file_location("pcap_sources", REPO / "tools" / "pcap_sources.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    off, frac, _, wire, _ = c1
    write_pcap(tmp_path / "rec.pcap", [udp_frame(wire[k: k + 1032], 21844) for k in range(0, 11 * B, 1032)])
    out = tmp_path / "sources.csv"
    assert tool.main([str(tmp_path / "rec.pcap"), "--port", "21844", "--cols", "32", "--every", "2", "--chunk", "4", "--max-batch", "4",
                      "--max-sources", "3", "--out", str(out)]) == 0
    back = tool.read_rows(out)
    with engine(pkg, off, frac, 64, 32, 4) as eng:
        want = eng.find_blocks(wire[: 11 * B], 32, 32, every=2, radius=2, max_sources=3, min_ratio=0.25)
    assert len(back) == int(want.count.sum()) >= 6
    k = 0
    for j, (entries, n) in enumerate(zip(want.sources, want.count)):
        for rank in range(n):
            assert (back[k]["block"], back[k]["rank"], back[k]["pixel"]) == (2 * j, rank, entries[rank]["pixel"])
            assert back[k]["power"] == entries[rank]["power"] and back[k]["row"] == entries[rank]["row"]
            assert back[k]["theta"] == entries[rank]["theta"] and back[k]["phi"] == entries[rank]["phi"]
            k += 1
