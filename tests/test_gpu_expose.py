"""Exposure (include/awpu_hip_expose.h) on the device: awpu_hip_expose_rows_device equals the host definition bit for bit -- vector
path, scalar tail, rows that start at no 16-byte boundary, both modes, the value edges, a window longer than a launch has grid
rows to spare --; the three run forms equal their composition -- awpu_hip_process_samples of the whole recording, then
awpu_hip_expose_rows, then the display chain and awpu_hip_find_peaks of every exposed row -- bit for bit in the exact mode,
with windows that straddle the sweep pieces, the watch run's ring and the swept blocks in the stats; a split recording chained
through next_first and carry equals one call; the handle's band goes in front; refusals leave the ring, the outputs and carry
alone.

AWPU_MATH_F32_FAST and AWPU_INTERP_FIR8 (test_other_modes_expose_their_own_rows): the run's frames against expose_rows of that
mode's own process_samples rows.  Where every block of the recording is swept (every == length) the run sweeps the same batches
as process_samples and the bits are equal, which is asserted, as it is for FIR8 in the default math everywhere (its bits do not
depend on the batch); where blocks are skipped the run's batches hold other snapshots than process_samples' and FAST's bits may
depend on the batch, so there the bound is 2e-5 relative per pixel (each side within 1e-5 of the reference, and a mean of
non-negative rows keeps a relative bound).  On an MI355X: FIR8 equal in all twelve cases; FAST equal in eleven and 5.4e-7 apart
at (first, every, length) = (6, 7, 4) with max_batch 32."""
import numpy as np
import pytest

import expose_util as X
import util
import value_edges as V
from test_find_cpu import TOL
from test_gpu_blocks import engine
from test_gpu_find import c1  # noqa: F401  (64 mics, 32 x 32, 23 blocks of a plane wave in noise)
from test_gpu_watch import colour_table, compose

pytestmark = pytest.mark.gpu

B = 256 * 1032
FIND = dict(radius=2, max_sources=4, min_ratio=0.25)
RUNS = [(0, 1, 1), (2, 3, 3), (1, 3, 2), (6, 7, 4), (3, 4, 4), (0, 5, 1)]


# ------------------------------------------------------------------------------------------------ the exposure pass alone

def device_rows(pkg, eng, power, first, every, L, mode, carry):
    """expose_rows_device of power [n_blocks, n_pixels] -> (frames, carry afterwards or None); the guard floats behind the frames
    and behind the carry row are intact."""
    import torch

    n_blocks, n_pixels = power.shape
    n_frames = pkg.expose_count(n_blocks, first, every, L)[0]
    d_power = torch.from_numpy(np.ascontiguousarray(power)).cuda()
    d_frames = torch.full((n_frames * n_pixels + 16,), -3.0, dtype=torch.float32, device="cuda")
    d_carry = None
    if carry is not None:
        d_carry = torch.full((n_pixels + 16,), -3.0, dtype=torch.float32, device="cuda")
        d_carry[:n_pixels] = torch.from_numpy(carry).cuda()
    torch.cuda.synchronize()
    nxt = eng.expose_rows_device(d_power.data_ptr(), n_blocks, n_pixels, first, every, L, d_frames.data_ptr(), mode,
                                 d_carry.data_ptr() if carry is not None else 0)
    eng.synchronize()
    assert nxt == pkg.expose_count(n_blocks, first, every, L)[1]
    frames = d_frames.cpu().numpy()
    assert np.all(frames[n_frames * n_pixels:] == -3.0)
    after = None
    if carry is not None:
        after = d_carry.cpu().numpy()
        assert np.all(after[n_pixels:] == -3.0)
        after = after[:n_pixels]
    return frames[: n_frames * n_pixels].reshape(n_frames, n_pixels), after


@pytest.mark.parametrize("mode", [X.MEAN, X.PEAK])
@pytest.mark.parametrize("n_pixels", [1, 3, 4, 5, 1024, 10000, 16385])
def test_rows_device_equals_rows(pkg, n_pixels, mode):
    """Whole vectors, a tail alone, a vector and a tail, rows that start at no 16-byte boundary; random rows and the value edges."""
    import torch  # noqa: F401

    assert not V.host_flushes()
    rng = np.random.default_rng(n_pixels)
    with pkg.Engine(n_pixels=16) as eng:  # (no delay table, no mic list: the exposure pass needs neither)
        for power in (rng.random((23, n_pixels), dtype=np.float32) * np.float32(50.0), X.edge_rows(23, n_pixels, seed=n_pixels)):
            for first, every, L in RUNS + [(0, 3, 3), (1, 4, 3), (30, 2, 2), (22, 23, 23), (4, 23, 23)]:
                carry0 = rng.random(n_pixels, dtype=np.float32)
                host_carry = carry0.copy()
                want, _ = pkg.expose_rows(power, first, every, L, mode, host_carry)
                got, after = device_rows(pkg, eng, power, first, every, L, mode, carry0)
                assert X.same_bits(got, want), (n_pixels, first, every, L)
                assert X.same_bits(after, host_carry)  # the open window, or carry as it was
                _, _, c_in, c_out, _ = pkg.expose_count(23, first, every, L)
                if c_in == 0 and c_out == 0:
                    assert X.same_bits(device_rows(pkg, eng, power, first, every, L, mode, None)[0], want)


@pytest.mark.parametrize("mode", [X.MEAN, X.PEAK])
def test_rows_device_long_windows(pkg, mode):
    """every = length = 64 over 70 rows of 16 pixels: one closing window and one open one; and 2600 windows of one row, more than
    a launch has grid rows."""
    power = X.edge_rows(70, 16, seed=9)
    power[:, 4:12] = np.random.default_rng(1).random((70, 8), dtype=np.float32)
    with pkg.Engine(n_pixels=16) as eng:
        for first in (63, 0, 10):
            carry0 = np.full(16, 0.5, np.float32)
            host_carry = carry0.copy()
            want, _ = pkg.expose_rows(power, first, 64, 64, mode, host_carry)
            got, after = device_rows(pkg, eng, power, first, 64, 64, mode, carry0)
            assert len(want) == (70 - first + 63) // 64 and X.same_bits(got, want) and X.same_bits(after, host_carry)
        many = np.random.default_rng(2).random((2600 * 2, 8), dtype=np.float32)
        want, _ = pkg.expose_rows(many, 1, 2, 2, mode, None)
        got, _ = device_rows(pkg, eng, many, 1, 2, 2, mode, None)
        assert len(want) == 2600 and X.same_bits(got, want)


# ------------------------------------------------------------------------------------------------ the runs

@pytest.fixture(scope="module")
def rows_c1(pkg, c1):  # noqa: F811
    """awpu_hip_process_samples of the c1 recording in the exact mode: every block's power row [23, 1024], computed once."""
    off, frac, _, _, samples = c1
    with engine(pkg, off, frac, 64, 32, 32) as ref:
        return ref.process_samples(samples)


def assert_sources(got_sources, got_count, want, where):
    assert np.array_equal(got_count, want.count), where
    for name in ("pixel", "row", "col"):
        assert np.array_equal(got_sources[name], want.sources[name]), (where, name)
    assert np.array_equal(got_sources["power"].view(np.uint32), want.sources["power"].view(np.uint32)), where
    for name in ("theta", "phi"):
        assert float(np.abs(got_sources[name] - want.sources[name]).max(initial=0.0)) <= TOL, (where, name)


def device_run(pkg, eng, d_in, pitch, n_blocks, first, every, L, mode, d_carry, table=None, out=(0, 0), flip=False, want=("image", "big", "power", "find")):
    """expose_samples_device with guarded outputs -> (ExposeResult with host arrays, next_first)."""
    import torch

    n_frames = pkg.expose_count(n_blocks, first, every, L)[0]
    P, big_px = 1024, out[0] * out[1] * (3 if table is not None else 1)
    bufs = {
        "image": torch.full((n_frames * P + 64,), 0xA5, dtype=torch.uint8, device="cuda") if "image" in want else None,
        "big": torch.full((n_frames * big_px + 64,), 0xA5, dtype=torch.uint8, device="cuda") if "big" in want else None,
        "power": torch.full((n_frames * P + 16,), -3.0, dtype=torch.float32, device="cuda") if "power" in want else None,
        "sources": torch.full((n_frames * 160 + 64,), 0xA5, dtype=torch.uint8, device="cuda") if "find" in want else None,
        "count": torch.full((n_frames + 4,), -7, dtype=torch.int32, device="cuda") if "find" in want else None,
    }
    ptr = lambda t: 0 if t is None else t.data_ptr()
    torch.cuda.synchronize()
    nxt = eng.expose_samples_device(d_in.data_ptr(), pitch, n_blocks, 32, 32, L, first, every, mode=mode, d_carry_ptr=ptr(d_carry),
                                    d_image_ptr=ptr(bufs["image"]), d_big_ptr=ptr(bufs["big"]), d_power_ptr=ptr(bufs["power"]),
                                    d_sources_ptr=ptr(bufs["sources"]), d_count_ptr=ptr(bufs["count"]), out_rows=out[0] if "big" in want else 0,
                                    out_cols=out[1] if "big" in want else 0, d_colormap_ptr=ptr(table), flip=flip,
                                    find=FIND if "find" in want else None)
    eng.synchronize()
    host = {k: None if t is None else t.cpu().numpy() for k, t in bufs.items()}
    image = big = power = sources = count = None
    if host["image"] is not None:
        assert np.all(host["image"][n_frames * P:] == 0xA5)
        image = host["image"][: n_frames * P].reshape(n_frames, 32, 32)
    if host["big"] is not None:
        assert np.all(host["big"][n_frames * big_px:] == 0xA5)
        big = host["big"][: n_frames * big_px].reshape((n_frames, out[0], out[1], 3) if table is not None else (n_frames, out[0], out[1]))
    if host["power"] is not None:
        assert np.all(host["power"][n_frames * P:] == -3.0)
        power = host["power"][: n_frames * P].reshape(n_frames, P)
    if host["sources"] is not None:
        assert np.all(host["sources"][n_frames * 160:] == 0xA5) and np.all(host["count"][n_frames:] == -7)
        sources = host["sources"][: n_frames * 160].view(pkg.binding.SOURCE_DTYPE).reshape(n_frames, 4)
        count = host["count"][:n_frames]
    return pkg.binding.ExposeResult(image, big, power, sources, count, nxt, None), nxt


@pytest.mark.parametrize("max_batch", [1, 4, 32])
@pytest.mark.parametrize("first,every,L", RUNS)
def test_run_forms_equal_the_composition(pkg, oracle, c1, rows_c1, max_batch, first, every, L):  # noqa: F811
    """expose_blocks, expose_samples and expose_samples_device == process_samples, expose_rows, heatmap_u8, the upscale / colour /
    flip chain and find_peaks, bit for bit; the ring is the watch run's; the stats count the swept blocks; carry is written exactly
    when a window stays open."""
    import torch

    off, frac, _, wire, samples = c1
    n_frames, nxt, c_in, c_out, n_swept = pkg.expose_count(23, first, every, L)
    table, d_table = colour_table(7)
    out = (40, 56)
    rng = np.random.default_rng(first + every)
    carry0 = rng.random(1024, dtype=np.float32)
    with engine(pkg, off, frac, 64, 32, max_batch) as ref:
        watched = ref.watch_samples(samples, 32, 32, first=first, every=every, want_image=False, want_power=True)
        ring = ref.ring_snapshot()
    for mode in (X.MEAN, X.PEAK):
        want_carry = carry0.copy()
        frames, _ = pkg.expose_rows(rows_c1, first, every, L, mode, want_carry)
        assert len(frames) == n_frames and frames[-1].max() > 0
        image, big = compose(pkg, oracle, frames, 32, 32, out[0], out[1], table, True)
        found = pkg.find_peaks(frames, 32, 32, **FIND)
        assert found.count[-1] >= 1

        def check(got, eng, carry, where):
            assert got.next_first == nxt and len(got) == n_frames
            assert X.same_bits(got.power, frames), where
            assert np.array_equal(got.image, image) and np.array_equal(got.big, big), where
            assert_sources(got.sources, got.count, found, where)
            assert X.same_bits(carry, want_carry), where
            assert np.array_equal(eng.ring_snapshot(), ring) and eng.stats().frames == n_swept, where
            if L == 1 and mode == X.MEAN:
                assert X.same_bits(got.power, watched.power)

        kw = dict(first=first, every=every, mode=mode, out_rows=out[0], out_cols=out[1], d_colormap_ptr=d_table.data_ptr(), flip=True,
                  want_power=True, find=FIND)
        forms = ["blocks", "samples", "device"] if mode == X.MEAN else ["samples"]
        if "blocks" in forms:
            with engine(pkg, off, frac, 64, 32, max_batch) as eng:
                carry = carry0.copy()
                check(eng.expose_blocks(wire, 32, 32, L, carry=carry, **kw), eng, carry, "blocks")
        with engine(pkg, off, frac, 64, 32, max_batch) as eng:
            carry = carry0.copy()
            check(eng.expose_samples(samples, 32, 32, L, carry=carry, **kw), eng, carry, "samples")
        if mode == X.PEAK:  # the sources alone: no frame crosses PCIe
            with engine(pkg, off, frac, 64, 32, max_batch) as eng:
                alone = eng.expose_samples(samples, 32, 32, L, first=first, every=every, mode=mode, carry=carry0.copy(), want_image=False, find=FIND)
                assert alone.power is None and alone.image is None
                assert_sources(alone.sources, alone.count, found, "sources alone")
                assert np.array_equal(eng.ring_snapshot(), ring)
        if "device" in forms:
            d_in = torch.from_numpy(np.ascontiguousarray(samples)).cuda()
            for asked in (("image", "big", "power", "find"), ("image",), ("find",)):
                d_carry = torch.full((1024 + 16,), -3.0, dtype=torch.float32, device="cuda")
                d_carry[:1024] = torch.from_numpy(carry0).cuda()
                with engine(pkg, off, frac, 64, 32, max_batch) as eng:
                    got, _ = device_run(pkg, eng, d_in, samples.shape[1], 23, first, every, L, mode, d_carry, d_table, out, True, asked)
                    after = d_carry.cpu().numpy()
                    assert np.all(after[1024:] == -3.0) and X.same_bits(after[:1024], want_carry)
                    assert np.array_equal(eng.ring_snapshot(), ring) and eng.stats().frames == n_swept
                    if "power" in asked:
                        check(got, eng, after[:1024], "device")
                    else:
                        assert got.image is None or np.array_equal(got.image, image)
                        if got.sources is not None:
                            assert_sources(got.sources, got.count, found, "device, sources alone")


@pytest.mark.parametrize("mode", [X.MEAN, X.PEAK])
def test_split_recording_equals_one_call(pkg, c1, rows_c1, mode):  # noqa: F811
    """5 + 1 + 9 + 8 blocks chained through next_first and carry, wire and sample forms in turn and once all on the device: the
    frames, the sources, the final carry and the ring of one call.  With (6, 7, 4) the first call has no frame at all, and with
    (2, 3, 3) the one-block call begins and ends inside a window."""
    import torch

    off, frac, _, wire, samples = c1
    cuts = [0, 5, 6, 15, 23]
    for first0, every, L in ((6, 7, 4), (2, 3, 3), (1, 3, 2), (0, 1, 1)):
        want_carry = np.zeros(1024, np.float32)
        frames, nxt = pkg.expose_rows(rows_c1, first0, every, L, mode, want_carry)
        open_at_the_end = pkg.expose_count(23, first0, every, L)[3] > 0  # (else the chain's carry is what an earlier call left in it)
        found = pkg.find_peaks(frames, 32, 32, **FIND)
        with engine(pkg, off, frac, 64, 32, 4) as one:
            one.process_samples(samples)
            ring = one.ring_snapshot()
        with engine(pkg, off, frac, 64, 32, 4) as eng:
            parts, first, carry = [], first0, np.zeros(1024, np.float32)
            for k, (a, b) in enumerate(zip(cuts, cuts[1:])):
                kw = dict(first=first, every=every, mode=mode, carry=carry, want_image=False, want_power=True, find=FIND)
                parts.append(eng.expose_blocks(wire[a * B: b * B], 32, 32, L, **kw) if k % 2 == 0 else
                             eng.expose_samples(samples[:, 256 * a: 256 * b], 32, 32, L, **kw))
                first = parts[-1].next_first
            if (first0, every, L) == (6, 7, 4):
                assert len(parts[0]) == 0
            assert X.same_bits(np.concatenate([p.power for p in parts]), frames), (first0, every, L)
            assert_sources(np.concatenate([p.sources for p in parts]), np.concatenate([p.count for p in parts]), found, (first0, every, L))
            assert first == nxt and (not open_at_the_end or X.same_bits(carry, want_carry)) and np.array_equal(eng.ring_snapshot(), ring)
        with engine(pkg, off, frac, 64, 32, 4) as eng:  # the same chain on device buffers
            d_in = torch.from_numpy(np.ascontiguousarray(samples)).cuda()
            d_carry = torch.zeros((1024,), dtype=torch.float32, device="cuda")
            got, first = [], first0
            for a, b in zip(cuts, cuts[1:]):
                part, first = device_run(pkg, eng, d_in[:, 256 * a:], samples.shape[1], b - a, first, every, L, mode, d_carry, want=("power",))
                got.append(part.power)
            assert X.same_bits(np.concatenate(got), frames) and first == nxt
            assert (not open_at_the_end or X.same_bits(d_carry.cpu().numpy(), want_carry)) and np.array_equal(eng.ring_snapshot(), ring)


def test_the_band_goes_in_front(pkg, c1):  # noqa: F811
    """With awpu_hip_set_band the exposed frames are those of the banded process_samples rows."""
    off, frac, _, wire, samples = c1
    band = pkg.band_design(6400.0, 9000.0, 31)
    with engine(pkg, off, frac, 64, 32, 4) as ref:
        plain = ref.process_samples(samples)
    with engine(pkg, off, frac, 64, 32, 4) as ref:
        ref.set_band(band)
        rows = ref.process_samples(samples)
        ring = ref.ring_snapshot()
    assert not np.array_equal(rows, plain)
    for first, every, L in ((2, 3, 3), (6, 7, 4), (1, 3, 2)):
        want_carry = np.zeros(1024, np.float32)
        frames, _ = pkg.expose_rows(rows, first, every, L, X.MEAN, want_carry)
        for form in ("blocks", "samples"):
            with engine(pkg, off, frac, 64, 32, 4) as eng:
                eng.set_band(band)
                carry = np.zeros(1024, np.float32)
                kw = dict(first=first, every=every, carry=carry, want_power=True)
                got = eng.expose_blocks(wire, 32, 32, L, **kw) if form == "blocks" else eng.expose_samples(samples, 32, 32, L, **kw)
                assert X.same_bits(got.power, frames), (first, every, L, form)
                assert np.array_equal(got.image.reshape(-1, 1024), np.stack([pkg.heatmap_u8(f) for f in frames]))
                assert X.same_bits(carry, want_carry) and np.array_equal(eng.ring_snapshot(), ring)


@pytest.mark.parametrize("mode_name", ["fast", "fir8"])
def test_other_modes_expose_their_own_rows(pkg, c1, mode_name):  # noqa: F811
    """AWPU_MATH_F32_FAST and AWPU_INTERP_FIR8: the run's frames against expose_rows of that mode's own process_samples rows (see the
    module's header for which comparison holds where)."""
    off, frac, _, _, samples = c1
    kw = dict(math=pkg.MATH_F32_FAST) if mode_name == "fast" else dict(interp=pkg.binding.INTERP_FIR8, fir=util.synthetic_fir_table())
    for max_batch in (4, 32):
        with engine(pkg, off, frac, 64, 32, max_batch, **kw) as ref:
            rows = ref.process_samples(samples)
        for first, every, L in ((2, 3, 3), (1, 3, 2), (6, 7, 4)):
            frames, _ = pkg.expose_rows(rows, first, every, L, X.MEAN, np.zeros(1024, np.float32))
            with engine(pkg, off, frac, 64, 32, max_batch, **kw) as eng:
                got = eng.expose_samples(samples, 32, 32, L, first=first, every=every, want_image=False, want_power=True).power
            rel = float((np.abs(got.astype(np.float64) - frames) / np.maximum(np.abs(frames.astype(np.float64)), 1e-300)).max())
            print(f"{mode_name} max_batch {max_batch} (first, every, L) = {(first, every, L)}: bits equal {X.same_bits(got, frames)}, worst relative {rel:.3g}")
            if every == L or mode_name == "fir8":
                assert X.same_bits(got, frames), (mode_name, max_batch, first, every, L)
            else:
                assert rel <= 2e-5, (mode_name, max_batch, first, every, L, rel)


def test_refusals_leave_ring_outputs_and_carry(pkg, c1):  # noqa: F811
    """A bad length or mode, a grid that is not the handle's, a find request without its outputs: AWPU_ERR_INVALID; a missing table
    and a device group: AWPU_ERR_STATE; the ring, the outputs and carry as they were."""
    import torch

    off, frac, _, wire, samples = c1
    ST, INV = pkg.binding.ERR_STATE, pkg.binding.ERR_INVALID

    def refused(eng, status, rows=32, cols=32, L=2, every=2, mode=X.MEAN, find=FIND):
        before = eng.ring_snapshot()
        carry = np.full(1024, 7.0, np.float32)
        for call in (lambda: eng.expose_blocks(wire[B: 4 * B], rows, cols, L, first=0, every=every, mode=mode, carry=carry, find=find),
                     lambda: eng.expose_samples(samples[:, 256: 1024], rows, cols, L, first=0, every=every, mode=mode, carry=carry, find=find)):
            with pytest.raises(pkg.AwpuError) as ei:
                call()
            assert ei.value.status == status
        assert np.all(carry == 7.0)
        d_in = torch.from_numpy(np.ascontiguousarray(samples[:, 256: 1024])).cuda()
        d_carry = torch.full((1024,), 7.0, dtype=torch.float32, device="cuda")
        d_power = torch.full((2 * 1024,), -3.0, dtype=torch.float32, device="cuda")
        d_sources = torch.full((2 * 4 * 40,), 0xA5, dtype=torch.uint8, device="cuda")
        d_count = torch.full((2,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(pkg.AwpuError) as ei:
            eng.expose_samples_device(d_in.data_ptr(), 768, 3, rows, cols, L, 0, every, mode=mode, d_carry_ptr=d_carry.data_ptr(),
                                      d_power_ptr=d_power.data_ptr(), d_sources_ptr=d_sources.data_ptr(), d_count_ptr=d_count.data_ptr(), find=find)
        assert ei.value.status == status
        eng.synchronize()
        assert bool((d_sources == 0xA5).all()) and bool((d_count == -7).all()) and bool((d_power == -3.0).all()) and bool((d_carry == 7.0).all())
        assert np.array_equal(eng.ring_snapshot(), before)

    with pkg.Engine(n_pixels=1024, n_streams=64, max_batch=4) as eng:  # no table, then no mic list
        eng.ingest_block(wire[:B])
        refused(eng, ST)
        eng.set_delay_table(off, frac)
        refused(eng, ST)
        eng.set_active_mics(None)
        refused(eng, INV, rows=16, cols=32)    # rows x cols is not the grid
        refused(eng, INV, L=3)                 # length above every
        refused(eng, INV, L=0)
        refused(eng, INV, mode=2)
        refused(eng, INV, every=1025, L=2)
        refused(eng, INV, find=dict(radius=0))
        carry = np.zeros(1024, np.float32)
        assert len(eng.expose_blocks(wire[B: 4 * B], 32, 32, 2, first=0, every=2, carry=carry, find=FIND)) == 2  # the handle still works
    with pkg.Engine(n_pixels=1024, n_streams=64, max_batch=4, grid_columns=32, devices=[0, 0]) as eng:  # a device group
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        eng.ingest_block(wire[:B])
        refused(eng, ST)
    with pkg.Engine(n_pixels=1024, n_streams=64, max_batch=4, pixel_begin=256, pixel_count=512) as eng:  # a slab of the grid
        eng.set_delay_table(off[256:768], frac[256:768])
        eng.set_active_mics(None)
        eng.ingest_block(wire[:B])
        before = eng.ring_snapshot()
        carry = np.full(512, 7.0, np.float32)
        with pytest.raises(pkg.AwpuError) as ei:
            eng.expose_blocks(wire[B: 4 * B], 32, 32, 2, first=0, every=2, carry=carry)
        assert ei.value.status == INV and np.all(carry == 7.0) and np.array_equal(eng.ring_snapshot(), before)


# ------------------------------------------------------------------------------------------------ the tools

def test_the_tools_expose_across_chunks(pkg, c1, tmp_path):  # noqa: F811
    """tools/pcap_video.py --exposure and tools/pcap_sources.py --exposure on a capture of the first 11 blocks, in chunks that cut
    windows: the AVI's frames and the CSV's lines are those of one expose_blocks call over the capture."""
    import importlib.util
    import sys

    from test_blocks_cpu import udp_frame, write_pcap
    from test_find_cpu import REPO

    def load(name):
        spec = importlib.util.spec_from_file_location(name, REPO / "tools" / f"{name}.py")
        tool = importlib.util.module_from_spec(spec)
        sys.modules[name] = tool
        spec.loader.exec_module(tool)
        return tool

    video, sources = load("pcap_video"), load("pcap_sources")
    off, frac, _, wire, _ = c1
    pcap = tmp_path / "rec.pcap"
    write_pcap(pcap, [udp_frame(wire[k: k + 1032], 21844) for k in range(0, 11 * B, 1032)])
    common = [str(pcap), "--port", "21844", "--cols", "32", "--every", "3", "--chunk", "4", "--max-batch", "4"]
    table = video.jet_table()
    import torch

    d_table = torch.from_numpy(table).cuda()
    for extra, mode in (([], X.MEAN), (["--peak-hold"], X.PEAK)):
        assert video.main(common + ["--size", "50", "--flip", "--exposure", "2", *extra, "--out", str(tmp_path / "exposed")]) == 0
        frames, rate, scale = video.read_avi(tmp_path / "exposed.000.avi")
        assert (rate, scale) == video.frame_rate(3)
        with engine(pkg, off, frac, 64, 32, 4) as eng:
            want = eng.expose_blocks(wire[: 11 * B], 32, 32, 2, first=1, every=3, mode=mode, out_rows=50, out_cols=50,
                                     d_colormap_ptr=d_table.data_ptr(), flip=True, want_image=False)
        assert len(want) == 4 and np.array_equal(frames, want.big) and frames.any()
    out = tmp_path / "sources.csv"
    assert sources.main(common + ["--exposure", "3", "--max-sources", "3", "--out", str(out)]) == 0
    back = sources.read_rows(out)
    with engine(pkg, off, frac, 64, 32, 4) as eng:
        want = eng.expose_blocks(wire[: 11 * B], 32, 32, 3, first=2, every=3, want_image=False, find=dict(radius=2, max_sources=3, min_ratio=0.25))
    assert len(back) == int(want.count.sum()) >= 3
    k = 0
    for j, (entries, n) in enumerate(zip(want.sources, want.count)):
        for rank in range(n):
            assert (back[k]["block"], back[k]["rank"], back[k]["pixel"]) == (2 + 3 * j, rank, entries[rank]["pixel"])
            assert back[k]["power"] == entries[rank]["power"] and back[k]["row"] == entries[rank]["row"] and back[k]["col"] == entries[rank]["col"]
            k += 1
