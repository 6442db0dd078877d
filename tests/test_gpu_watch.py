"""Watching runs of blocks (include/awpu_hip_watch.h) on the device: the display images of every Nth block equal, byte for byte,
what the per-block live loop (awpu_hip_live_block) shows for those blocks in the exact mode, and in every mode the composition
awpu_hip_process -> awpu_hip_heatmap_u8 -> the oracle's restated cv::resize -> colour table -> mirror; every block reaches the
ring, shown or not.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import util
from test_gpu_blocks import chunked_process, engine, recording, snapshots

pytestmark = pytest.mark.gpu

B = 256 * 1032
CASES = [(0, 1), (0, 3), (2, 3), (5, 7), (36, 4), (40, 3)]


def colour_table(seed=3):
    import torch

    table = np.random.default_rng(seed).integers(0, 256, size=(256, 3), dtype=np.uint8)
    return table, torch.from_numpy(table).cuda()


def compose(pkg, oracle, power, rows, cols, out_rows, out_cols, table, flip):
    """(image, big) of the definition: heatmap_u8 per frame, the oracle's upscale, the table, the mirror."""
    image = np.stack([pkg.heatmap_u8(p) for p in power]).reshape(-1, rows, cols)
    big = np.stack([oracle.resize_linear_u8(im, out_rows, out_cols) for im in image])
    if table is not None:
        big = table[big]
    if flip:
        big = np.ascontiguousarray(big[:, :, ::-1])
    return image, big


@pytest.fixture(scope="module")
def small(oracle):
    """The reference's array on a 16 x 16 grid, 37 blocks."""
    xyz = oracle.create_antenna()
    off, frac = oracle.compute_delay_lut(xyz, 16, 16)
    wire, samples = recording(oracle, 37, 64, seed=21)
    return off, frac, wire, samples, xyz


@pytest.fixture(scope="module")
def ref100(oracle):
    """The reference's shape: its array on a 100 x 100 grid, 37 blocks."""
    xyz = oracle.create_antenna()
    off, frac = oracle.compute_delay_lut(xyz, 100, 100)
    wire, samples = recording(oracle, 37, 64, seed=22)
    return off, frac, wire, samples, xyz


def live_loop_case(pkg, grid, max_batch, out, coloured, cases, label):
    """watch_blocks against the per-block loop of live_block over all 37 blocks, for every (first, every) of `cases`: prints the
    figures of every case, then asserts equality of power, image, big image and ring."""
    off, frac, wire, samples = grid
    res = int(round(off.shape[0] ** 0.5))
    table, d_table = colour_table() if coloured else (None, None)
    ptr = d_table.data_ptr() if coloured else 0
    with engine(pkg, off, frac, 64, res, max_batch) as loop:
        want = [loop.live_block(wire[k * B: (k + 1) * B], res, res, out[0], out[1], d_colormap_ptr=ptr) for k in range(37)]
        ring = loop.ring_snapshot()
    assert np.array_equal(ring, snapshots(samples)[-1])
    failures = []
    for first, every in cases:
        shown = list(range(first, 37, every))
        with engine(pkg, off, frac, 64, res, max_batch) as eng:
            got = eng.watch_blocks(wire, res, res, first=first, every=every, out_rows=out[0], out_cols=out[1], d_colormap_ptr=ptr,
                                   want_power=True)
            assert got.image.shape == (len(shown), res, res) and got.big.shape[:3] == (len(shown), out[0], out[1])
            assert got.next_first == (shown[-1] + every if shown else first) - 37
            assert eng.stats().frames == len(shown)
            assert np.array_equal(eng.ring_snapshot(), ring), (first, every)
        w_power = np.stack([want[k][0] for k in shown]) if shown else got.power
        w_image = np.stack([want[k][1] for k in shown]) if shown else got.image
        w_big = np.stack([want[k][2] for k in shown]) if shown else got.big
        rel = float(np.max(np.abs(got.power - w_power) / np.maximum(np.abs(w_power), 1e-30))) if shown else 0.0
        figures = (int((got.power != w_power).sum()), got.power.size, rel, int((got.image != w_image).sum()), got.image.size,
                   int((got.big != w_big).sum()), got.big.size)
        print(f"{label} out {out} coloured {coloured} first {first} every {every}: powers differing %d of %d (max rel %.3g), "
              f"image bytes %d of %d, big image bytes %d of %d" % figures)
        if figures[0] or figures[3] or figures[5]:
            failures.append((first, every) + figures)
    assert not failures, failures


@pytest.mark.parametrize("out,coloured", [((32, 32), False), ((32, 32), True), ((40, 56), False), ((40, 56), True)])
def test_exact_equals_the_live_loop(pkg, small, out, coloured):
    """Item 6 as the issue states it: exact mode, the reference's array on a 16 x 16 grid, 37 blocks, a batched handle
    (max_batch 8): image, big image and power of the shown blocks == the per-block loop of live_block over all 37 blocks, the
    ring afterwards == the loop's; (40, 3) shows nothing and still moves the ring 37 blocks on.

    On this coarse grid the quads of the table do not share, so a batch is swept by das_exact_pair_kernel while the live loop's
    single frames take das_exact_ndp_kernel: the check needs both to reduce a pixel's wave in the same order (they did not
    before this feature: 3209 of 9472 powers differed by up to 2.28e-7 relative, 1 image byte and 3 to 29 large-image bytes)."""
    off, frac, wire, samples, _ = small
    live_loop_case(pkg, (off, frac, wire, samples), 8, out, coloured, CASES, "16x16 max_batch 8")


def test_a_frame_alone_gives_its_batch_bits_on_a_coarse_grid(pkg, small):
    """What the exact mode of the block, listen and watch calls rests on, where the batch falls to das_exact_pair_kernel:
    awpu_hip_process of a batch == of its frames one by one == process_blocks == the per-block loop, bit for bit."""
    from test_gpu_blocks import per_block_loop

    off, frac, wire, samples, _ = small
    snaps = snapshots(samples)
    with engine(pkg, off, frac, 64, 16, 8) as eng, engine(pkg, off, frac, 64, 16, 8) as loop:
        batched = chunked_process(eng, snaps, 8)
        assert eng.stats().kernel_variant == pkg.binding.KERNEL_NAMES.index("exact_pair")
        alone = np.stack([eng.process(s) for s in snaps])
        assert np.array_equal(batched, alone)
        assert np.array_equal(eng.process_blocks(wire), alone)
        assert np.array_equal(per_block_loop(loop, wire, 37), alone)


@pytest.mark.parametrize("which", ["16x16 one frame per sweep", "100x100 max_batch 16"])
def test_exact_equals_the_live_loop_where_the_sweeps_agree(pkg, small, ref100, which):
    """The same check where a chunk and a frame alone are swept to the same bits: the 16 x 16 grid with max_batch 1 (every chunk
    is one frame: the live loop's own kernel), and the reference's 100 x 100 grid with max_batch 16 (chunks of 16, 16, 5 ...)."""
    grid, max_batch = (small[:4], 1) if which.startswith("16") else (ref100[:4], 16)
    live_loop_case(pkg, grid, max_batch, (120, 168), True, CASES, which)
    live_loop_case(pkg, grid, max_batch, (128, 200), False, [(0, 1), (2, 3)], which)


@pytest.mark.parametrize("mode", ["exact", "fast", "fir8"])
@pytest.mark.parametrize("max_batch", [1, 4, 32])
def test_every_mode_equals_the_composition(pkg, oracle, mode, max_batch):
    """Item 7: power == Engine.process of the shown snapshots in chunks of max_batch; image == heatmap_u8 of it; big image ==
    the oracle's resize of that, through the table, mirrored when flip.  Blocks 9 .. 16 are silent: the snapshots after blocks
    12 .. 16 are all zero and so are their images.  One large image has the compact one's size."""
    xyz = oracle.create_antenna()
    off, frac = oracle.compute_delay_lut(xyz, 32, 32)
    rng = np.random.default_rng(31)
    streams = rng.integers(-(1 << 21), 1 << 21, size=(41, 256, 256), dtype=np.int32)
    streams[9:17] = 0
    from test_gpu_blocks import make_datagrams

    wire = b"".join(make_datagrams(s, counter0=256 * b) for b, s in enumerate(streams))
    samples = np.concatenate([oracle.unpack_exposure(s, 64) for s in streams], axis=1)
    snaps = snapshots(samples)
    kw = dict(math=pkg.MATH_F32_FAST) if mode == "fast" else dict(interp=pkg.binding.INTERP_FIR8, fir=util.synthetic_fir_table()) \
        if mode == "fir8" else {}
    table, d_table = colour_table(5)
    first, every = 1, 2
    shown = list(range(first, 41, every))
    with engine(pkg, off, frac, 64, 32, max_batch, **kw) as ref:
        power = chunked_process(ref, snaps[shown], max_batch)
    for out, coloured, flip in (((32, 32), True, True), ((75, 90), True, False), ((64, 48), False, True)):
        with engine(pkg, off, frac, 64, 32, max_batch, **kw) as eng:
            got = eng.watch_blocks(wire, 32, 32, first=first, every=every, out_rows=out[0], out_cols=out[1],
                                   d_colormap_ptr=d_table.data_ptr() if coloured else 0, flip=flip, want_power=True)
            assert np.array_equal(got.power, power), (mode, max_batch)
            image, big = compose(pkg, oracle, got.power, 32, 32, out[0], out[1], table if coloured else None, flip)
            assert np.array_equal(got.image, image)
            assert np.array_equal(got.big, big), (out, coloured, flip)
            assert np.array_equal(eng.ring_snapshot(), snaps[-1])
            st = eng.stats()
            assert st.frames == len(shown) and st.launches == -(-len(shown) // max_batch)
    quiet = [j for j, k in enumerate(shown) if 12 <= k <= 16]
    assert len(quiet) == 2 and not got.power[quiet].any() and not got.image[quiet].any()
    assert got.image.any()


@pytest.mark.parametrize("res,out", [(8, (9, 13)), (8, (8, 15)), (16, (33, 37)), (16, (17, 16)), (16, (21, 1027))])
def test_odd_sizes_of_the_large_image(pkg, oracle, res, out):
    """Rows that are not whole 16-byte units, not whole dwords, narrower than one lane's 16 pixels, wider than one wave's 1024:
    grey and coloured, mirrored and not, equal to the composition; nothing is written past a frame (a canary row follows)."""
    import torch

    xyz = oracle.create_antenna()
    off, frac = oracle.compute_delay_lut(xyz, res, res)
    wire, samples = recording(oracle, 9, 64, seed=res + out[1])
    snaps = snapshots(samples)
    table, d_table = colour_table(7)
    for coloured in (False, True):
        for flip in (False, True):
            with engine(pkg, off, frac, 64, res, 4) as eng:
                got = eng.watch_blocks(wire, res, res, first=1, every=3, out_rows=out[0], out_cols=out[1],
                                       d_colormap_ptr=d_table.data_ptr() if coloured else 0, flip=flip, want_power=True)
                assert np.array_equal(got.power, chunked_process(eng, snaps[1::3], 4))
                image, big = compose(pkg, oracle, got.power, res, res, out[0], out[1], table if coloured else None, flip)
                assert np.array_equal(got.image, image) and np.array_equal(got.big, big), (coloured, flip)
    # the device form writes straight into the caller's frames: the bytes behind the last frame stay
    frame = out[0] * out[1] * 3
    d_in = torch.from_numpy(np.ascontiguousarray(samples)).cuda()
    d_big = torch.full((3 * frame + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    with engine(pkg, off, frac, 64, res, 4) as eng:
        eng.watch_samples_device(d_in.data_ptr(), samples.shape[1], 9, res, res, first=1, every=3, d_big_ptr=d_big.data_ptr(),
                                 out_rows=out[0], out_cols=out[1], d_colormap_ptr=d_table.data_ptr(), flip=True)
        eng.synchronize()
    back = d_big.cpu().numpy()
    assert np.array_equal(back[: 3 * frame].reshape(3, out[0], out[1], 3), big)
    assert np.all(back[3 * frame:] == 0xA5)


def test_split_and_interleaved_runs(pkg, ref100):
    """Item 8: one call == the recording split at random points and continued with next_first == a run whose skipped blocks go
    to process_blocks, listen_blocks and live_block instead.  A split changes how the shown frames fall into chunks (a call that
    shows one frame sweeps it alone), so this is a statement about the exact mode where a frame's bits do not depend on its
    batch: the reference's 100 x 100 grid, as in test_gpu_blocks.test_calls_continue_each_other_and_the_live_loop -- not the
    16 x 16 grid of test_exact_equals_the_live_loop, whose docstring says why."""
    off, frac, wire, samples, xyz = ref100
    table, d_table = colour_table(9)
    kw = dict(out_rows=128, out_cols=136, d_colormap_ptr=d_table.data_ptr(), flip=True, want_power=True)
    rng = np.random.default_rng(41)
    for first0, every in ((2, 3), (0, 1), (5, 7), (1, 2), (3, 5)):
        with engine(pkg, off, frac, 64, 100, 4) as one:
            whole = one.watch_blocks(wire, 100, 100, first=first0, every=every, **kw)
            ring = one.ring_snapshot()
        for _ in range(3):
            cuts = [0] + sorted(rng.choice(np.arange(1, 37), size=int(rng.integers(1, 9)), replace=False).tolist()) + [37]
            with engine(pkg, off, frac, 64, 100, 4) as eng:
                parts, first = [], first0
                for a, b in zip(cuts, cuts[1:]):
                    parts.append(eng.watch_blocks(wire[a * B: b * B], 100, 100, first=first, every=every, **kw))
                    first = parts[-1].next_first
                for name in ("power", "image", "big"):
                    assert np.array_equal(np.concatenate([getattr(p, name) for p in parts]), getattr(whole, name)), (every, cuts, name)
                assert first == whole.next_first
                assert np.array_equal(eng.ring_snapshot(), ring)
    # shown: 2, 5, ..., 35; blocks 9-10, 21-22 and 30-31 are skipped ones, given to the other calls
    with engine(pkg, off, frac, 64, 100, 4) as one:
        whole = one.watch_blocks(wire, 100, 100, first=2, every=3, **kw)
        ring = one.ring_snapshot()
    with engine(pkg, off, frac, 64, 100, 4) as eng:
        eng.set_antenna(xyz)
        a = eng.watch_blocks(wire[: 9 * B], 100, 100, first=2, every=3, **kw)
        assert a.next_first == 2 and len(a) == 3
        eng.process_blocks(wire[9 * B: 11 * B])
        b = eng.watch_blocks(wire[11 * B: 21 * B], 100, 100, first=0, every=3, **kw)
        assert b.next_first == 2 and len(b) == 4
        eng.listen_blocks(wire[21 * B: 23 * B], 0.3, 1.0, 0.03, 5e-5, 0, 1.5, want_trail=False)
        c = eng.watch_blocks(wire[23 * B: 30 * B], 100, 100, first=0, every=3, **kw)
        assert c.next_first == 2 and len(c) == 3
        for k in (30, 31):
            eng.live_block(wire[k * B: (k + 1) * B], 100, 100)
        d = eng.watch_blocks(wire[32 * B:], 100, 100, first=0, every=3, **kw)
        assert d.next_first == 1 and len(d) == 2
        for name in ("power", "image", "big"):
            assert np.array_equal(np.concatenate([getattr(p, name) for p in (a, b, c, d)]), getattr(whole, name)), name
        assert np.array_equal(eng.ring_snapshot(), ring)
        # and the live loop goes on from where the watched run ends
        p, _, _ = eng.live_block(wire[:B], 100, 100)
        one_more = snapshots(np.concatenate([samples, samples[:, :256]], axis=1))[-1]
        assert np.array_equal(eng.ring_snapshot(), one_more)


@pytest.fixture(scope="module")
def c1(pkg, oracle):
    """test_gpu_find's c1 recording (64 mics, 32 x 32, 23 blocks); that module imports this one, so it is imported here."""
    from test_gpu_find import c1_recording

    return c1_recording(pkg, oracle)


def test_kinds_in_turn_on_one_handle(pkg, c1):
    """The run kinds share the handle's display and find buffers (and the run buffers), which grow from device-only to device plus
    pinned when a host form follows a device form: one engine (max_batch 4) takes the whole recording through watch_samples_device,
    expose_samples, find_blocks, cohere_samples, locate_samples, watch_blocks and expose_samples_device in turn, and every result
    equals the same call on a fresh engine.  Both engines ran process_samples(recording) first, so every call starts from the same
    ring.  Images, counts, pixel / row / col and the powers' bits are equal, theta / phi within test_find_cpu.TOL, the ring
    afterwards equal; device outputs are guarded.  The coherence run's large image is 49 x 65: the 17 x 33 one is below the 32 x 32
    grid and is refused (upscale only), by both engines alike, before anything of the handle is touched."""
    import torch

    from test_gpu_expose import assert_sources, device_run

    off, frac, xyz, wire, samples = c1
    table, d_table = colour_table(11)
    d_in = torch.from_numpy(np.ascontiguousarray(samples)).cuda()
    find = dict(radius=2, max_sources=4, min_ratio=0.25)

    def prepared():
        eng = engine(pkg, off, frac, 64, 32, 4)
        eng.set_antenna(xyz)
        eng.process_samples(samples)
        return eng

    def watch_device(eng):
        n_frames = len(range(1, 23, 2))
        d_image = torch.full((n_frames * 1024 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        nxt = eng.watch_samples_device(d_in.data_ptr(), samples.shape[1], 23, 32, 32, first=1, every=2, d_image_ptr=d_image.data_ptr())
        eng.synchronize()
        back = d_image.cpu().numpy()
        assert np.all(back[n_frames * 1024:] == 0xA5)
        return pkg.binding.WatchResult(back[: n_frames * 1024].reshape(n_frames, 32, 32), None, None, nxt)

    def expose_device(eng):
        d_carry = torch.zeros(1024, dtype=torch.float32, device="cuda")
        got, _ = device_run(pkg, eng, d_in, samples.shape[1], 23, 2, 3, 2, pkg.binding.EXPOSE_MEAN, d_carry, d_table, (40, 56), True)
        got.carry = d_carry.cpu().numpy()
        return got

    def refused_then_cohere(eng):
        with pytest.raises(pkg.AwpuError) as ei:
            eng.cohere_samples(samples, 32, 32, first=0, every=2, out_rows=17, out_cols=33, find=find)
        assert "upscale only" in str(ei.value)
        return eng.cohere_samples(samples, 32, 32, first=0, every=2, out_rows=49, out_cols=65, want_power=True, find=find)

    calls = [
        ("watch_samples_device", watch_device),
        ("expose_samples", lambda e: e.expose_samples(samples, 32, 32, 2, first=2, every=3, out_rows=40, out_cols=56,
                                                      d_colormap_ptr=d_table.data_ptr(), want_power=True, find=find)),
        ("find_blocks", lambda e: e.find_blocks(wire, 32, 32, first=0, every=1, want_power=True, radius=2, max_sources=8, min_ratio=0.25)),
        ("cohere_samples", refused_then_cohere),
        ("locate_samples", lambda e: e.locate_samples(samples, 32, 32, [0.5, 2.0, np.inf], first=1, every=3, want_power=True,
                                                      want_range_power=True, **find)),
        ("watch_blocks", lambda e: e.watch_blocks(wire, 32, 32, first=0, every=1, out_rows=64, out_cols=64, d_colormap_ptr=d_table.data_ptr())),
        ("expose_samples_device", expose_device),
    ]
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    with prepared() as one:
        for where, call in calls:
            got = call(one)
            with prepared() as fresh:
                want = call(fresh)
                assert np.array_equal(one.ring_snapshot(), fresh.ring_snapshot()), where
            assert got.next_first == want.next_first and len(got) == len(want) > 0, where
            for name in ("image", "big", "power", "carry", "range_power"):
                a, b = getattr(got, name, None), getattr(want, name, None)
                assert (a is None) == (b is None), (where, name)
                if a is not None:
                    assert a.shape == b.shape and np.array_equal(bits(a) if a.dtype == np.float32 else a, bits(b) if b.dtype == np.float32 else b), (where, name)
            if getattr(want, "sources", None) is not None:
                assert want.count.max() >= 1, where
                assert_sources(got.sources, got.count, want, where)
            if hasattr(want, "ranges"):
                assert np.array_equal(got.ranges["index"], want.ranges["index"]) and (want.ranges["index"] >= 0).any(), where
                assert np.array_equal(bits(got.ranges["power"]), bits(want.ranges["power"])), where
                assert np.array_equal(got.ranges["distance"], want.ranges["distance"], equal_nan=True), where


def test_samples_forms(pkg, oracle, small):
    """Item 9: the host samples form == the wire form; 512 streams, which the wire cannot carry; the device form == the host form."""
    import torch

    off, frac, wire, samples, _ = small
    table, d_table = colour_table(13)
    kw = dict(first=1, every=4, out_rows=32, out_cols=48, d_colormap_ptr=d_table.data_ptr(), want_power=True)
    with engine(pkg, off, frac, 64, 16, 4) as a, engine(pkg, off, frac, 64, 16, 4) as b:
        want = a.watch_blocks(wire, 16, 16, **kw)
        got = b.watch_samples(samples, 16, 16, **kw)
        for name in ("power", "image", "big"):
            assert np.array_equal(getattr(got, name), getattr(want, name)), name
        assert got.next_first == want.next_first and np.array_equal(a.ring_snapshot(), b.ring_snapshot())
    xyz = oracle.create_tiled_antenna(4, 2)  # 512 mics: two FPGAs
    off2, frac2 = oracle.compute_delay_lut(xyz, 32, 32)
    rng = np.random.default_rng(9)
    wide = (rng.integers(-(1 << 21), 1 << 21, size=(512, 256 * 14)) / 8388608.0).astype(np.float32)
    snaps = snapshots(wide)
    for first, every in ((0, 1), (2, 3), (1, 5)):
        shown = list(range(first, 14, every))
        with engine(pkg, off2, frac2, 512, 32, 4) as a, engine(pkg, off2, frac2, 512, 32, 4) as b:
            got = a.watch_samples(wide, 32, 32, first=first, every=every, out_rows=64, out_cols=64, d_colormap_ptr=d_table.data_ptr(),
                                  flip=True, want_power=True)
            assert np.array_equal(got.power, chunked_process(a, snaps[shown], 4))
            image, big = compose(pkg, oracle, got.power, 32, 32, 64, 64, table, True)
            assert np.array_equal(got.image, image) and np.array_equal(got.big, big)
            assert np.array_equal(a.ring_snapshot(), snaps[-1])
            padded = np.zeros((512, 256 * 14 + 100), np.float32)  # pitch above 256 * n_blocks
            padded[:, : 256 * 14] = wide
            d_in = torch.from_numpy(padded).cuda()
            n = len(shown)
            d_image = torch.empty((n, 32 * 32), dtype=torch.uint8, device="cuda")
            d_big = torch.empty((n, 64, 64, 3), dtype=torch.uint8, device="cuda")
            d_power = torch.empty((n, 32 * 32), dtype=torch.float32, device="cuda")
            nxt = b.watch_samples_device(d_in.data_ptr(), padded.shape[1], 14, 32, 32, first=first, every=every,
                                         d_image_ptr=d_image.data_ptr(), d_big_ptr=d_big.data_ptr(), d_power_ptr=d_power.data_ptr(),
                                         out_rows=64, out_cols=64, d_colormap_ptr=d_table.data_ptr(), flip=True)
            b.synchronize()
            assert nxt == got.next_first
            assert np.array_equal(d_power.cpu().numpy(), got.power)
            assert np.array_equal(d_image.cpu().numpy().reshape(n, 32, 32), got.image)
            assert np.array_equal(d_big.cpu().numpy(), got.big)
            assert np.array_equal(b.ring_snapshot(), snaps[-1])
            # the large image alone: the compact one and the powers stay in the handle's own buffers
            d_big.zero_()
            b.watch_samples_device(d_in.data_ptr(), padded.shape[1], 14, 32, 32, first=first, every=every, d_big_ptr=d_big.data_ptr(),
                                   out_rows=64, out_cols=64, d_colormap_ptr=d_table.data_ptr(), flip=True)
            b.synchronize()
            again = compose(pkg, oracle, chunked_process(a, snapshots(wide, ring=snaps[-1])[shown], 4), 32, 32, 64, 64, table, True)[1]
            assert np.array_equal(d_big.cpu().numpy(), again)


@pytest.mark.parametrize("where", ["handle_stream", "other_stream"])
def test_device_run_then_host_run_are_ordered(pkg, where):
    """Item 9: a long asynchronous device-form run, then at once a host-form run on the same handle: the host run continues the
    ring the device run leaves, whichever stream the device run was enqueued on.  Both equal one call over the whole recording."""
    import torch

    S = pkg.synthetic
    spec = S.WORKLOADS["headline"]
    off, frac = S.delay_table(spec, S.geometry(spec))
    rng = np.random.default_rng(6)
    n, cut, every = 130, 121, 2
    samples = (rng.integers(-(1 << 21), 1 << 21, size=(spec.n_mics, 256 * n)) / 8388608.0).astype(np.float32)
    res = spec.res
    with engine(pkg, off, frac, spec.n_mics, res, 32) as one, engine(pkg, off, frac, spec.n_mics, res, 32) as two:
        want = one.watch_samples(samples, res, res, first=1, every=every, out_rows=2 * res, out_cols=2 * res, want_power=True)
        n_dev, nxt = pkg.binding.watch_count(cut, 1, every)
        d_in = torch.from_numpy(np.ascontiguousarray(samples[:, : 256 * cut])).cuda()
        d_image = torch.empty((n_dev, res * res), dtype=torch.uint8, device="cuda")
        d_big = torch.empty((n_dev, 2 * res, 2 * res), dtype=torch.uint8, device="cuda")
        d_power = torch.empty((n_dev, res * res), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        args = (d_in.data_ptr(), 256 * cut, cut, res, res)
        kw = dict(first=1, every=every, d_image_ptr=d_image.data_ptr(), d_big_ptr=d_big.data_ptr(), d_power_ptr=d_power.data_ptr(),
                  out_rows=2 * res, out_cols=2 * res)
        if where == "other_stream":
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                assert two.watch_samples_device(*args, stream=side.cuda_stream, **kw) == nxt
        else:
            assert two.watch_samples_device(*args, **kw) == nxt
        tail = two.watch_samples(samples[:, 256 * cut:], res, res, first=nxt, every=every, out_rows=2 * res, out_cols=2 * res,
                                 want_power=True)  # enqueued while the device run is still going
        torch.cuda.synchronize()
        assert np.array_equal(tail.power, want.power[n_dev:]) and np.array_equal(tail.big, want.big[n_dev:])
        assert np.array_equal(tail.image, want.image[n_dev:])
        assert np.array_equal(d_power.cpu().numpy(), want.power[:n_dev])
        assert np.array_equal(d_image.cpu().numpy().reshape(n_dev, res, res), want.image[:n_dev])
        assert np.array_equal(d_big.cpu().numpy(), want.big[:n_dev])
        assert np.array_equal(two.ring_snapshot(), one.ring_snapshot())


def test_stats_count_shown_frames(pkg, small):
    """Items 10 and the sweeps saved: every = 3 sweeps a third of the frames in a third of the launches of every = 1."""
    off, frac, wire, _, _ = small
    counts = {}
    for every in (1, 3):
        with engine(pkg, off, frac, 64, 16, 4) as eng:
            eng.watch_blocks(wire[: 36 * B], 16, 16, every=every)
            st = eng.stats()
            counts[every] = (st.frames, st.launches)
            eng.watch_blocks(wire[: 2 * B], 16, 16, first=5, every=every)  # shows nothing: nothing swept
            st = eng.stats()
            assert (st.frames, st.launches) == counts[every]
    assert counts == {1: (36, 9), 3: (12, 3)}


def test_refusals_leave_the_ring(pkg, small):
    """Item 10: a device group and a missing table / mic list: AWPU_ERR_STATE; a handle that holds a slab of the grid, rows x cols
    that is not the grid, hist != 1024: AWPU_ERR_INVALID; the ring as it was."""
    off, frac, wire, samples, _ = small
    ST, INV = pkg.binding.ERR_STATE, pkg.binding.ERR_INVALID

    def refused(eng, status, **kw):
        args = dict(rows=16, cols=16, every=2)
        args.update(kw)
        before = eng.ring_snapshot()
        with pytest.raises(pkg.AwpuError) as ei:
            eng.watch_blocks(wire[B: 4 * B], args.pop("rows"), args.pop("cols"), **args)
        assert ei.value.status == status
        with pytest.raises(pkg.AwpuError) as ei:
            eng.watch_samples(samples[:, 256: 1024], 16, 16, every=2)
        assert ei.value.status == status
        assert np.array_equal(eng.ring_snapshot(), before)

    with pkg.Engine(n_pixels=256, n_streams=64, max_batch=4) as eng:  # no table, then no mic list
        eng.ingest_block(wire[:B])
        refused(eng, ST)
        eng.set_delay_table(off, frac)
        refused(eng, ST)
        eng.set_active_mics(None)
        before = eng.ring_snapshot()
        for kw in (dict(rows=8, cols=16), dict(rows=16, cols=32), dict(rows=256, cols=256)):  # rows x cols is not the grid
            with pytest.raises(pkg.AwpuError) as ei:
                eng.watch_blocks(wire[B: 4 * B], kw["rows"], kw["cols"])
            assert ei.value.status == INV
        assert np.array_equal(eng.ring_snapshot(), before)
        assert len(eng.watch_blocks(wire[B: 4 * B], 16, 16, every=2)) == 2  # the handle still works
    with pkg.Engine(n_pixels=256, n_streams=64, max_batch=4, grid_columns=16, devices=[0, 0]) as eng:  # a device group
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        eng.ingest_block(wire[:B])
        refused(eng, ST)
    with pkg.Engine(n_pixels=256, n_streams=64, max_batch=4, pixel_begin=64, pixel_count=128) as eng:  # a slab of the grid
        eng.set_delay_table(off[64:192], frac[64:192])
        eng.set_active_mics(None)
        eng.ingest_block(wire[:B])
        refused(eng, INV)
    with pkg.Engine(n_pixels=256, n_streams=64, hist=2048, max_batch=4) as eng:
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        with pytest.raises(pkg.AwpuError) as ei:
            eng.watch_blocks(wire[: 2 * B], 16, 16)
        assert ei.value.status == INV


def test_reference_shape_at_video_size(pkg, oracle):
    """Item 11: 64 mics, 100 x 100 -> 1024 x 1024 x 3, 64 blocks, every third: the composition of item 7."""
    xyz = oracle.create_antenna()
    off, frac = oracle.compute_delay_lut(xyz, 100, 100)
    wire, samples = recording(oracle, 64, 64, seed=5)
    snaps = snapshots(samples)
    table, d_table = colour_table(17)
    shown = list(range(0, 64, 3))
    with engine(pkg, off, frac, 64, 100, 16) as eng:
        got = eng.watch_blocks(wire, 100, 100, every=3, out_rows=1024, out_cols=1024, d_colormap_ptr=d_table.data_ptr(), want_power=True)
        assert got.next_first == 2 and got.big.shape == (22, 1024, 1024, 3)
        assert np.array_equal(got.power, chunked_process(eng, snaps[shown], 16))
        image, big = compose(pkg, oracle, got.power, 100, 100, 1024, 1024, table, False)
        assert np.array_equal(got.image, image)
        assert np.array_equal(got.big, big)
        assert np.array_equal(eng.ring_snapshot(), snaps[-1])
        flipped = eng.watch_blocks(wire, 100, 100, every=3, out_rows=1024, out_cols=1024, d_colormap_ptr=d_table.data_ptr(), flip=True,
                                   want_image=False)
        # (the second run starts from the first one's ring: its own powers, and the mirror of their images)
        again = chunked_process(eng, snapshots(samples, ring=snaps[-1])[shown], 16)
        assert flipped.image is None and np.array_equal(flipped.big, compose(pkg, oracle, again, 100, 100, 1024, 1024, table, True)[1])
