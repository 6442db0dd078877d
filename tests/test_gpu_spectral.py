"""Spectral heatmaps (include/awpu_hip_spectral.h) on the device.  The result is defined by composition with calls that exist, so
everything here is bit for bit: a band's powers are what the call of the same form returns on a handle with that band set
(awpu_hip_band.h); the image and the dominant bands are binding.spectral_compose of the frame's band powers; the large image is
resize_linear_u8 of every byte plane.  Checked for the single calls in both fp32 modes and both interpolations, ragged mic lists
with gains, c2, a batch that goes up in pieces; for the runs in their three forms, split recordings, both scales and flips; a NaN
that stays in its frames; the refusals; and two plane waves that separate by colour.  Bit-equal = equal uint32 views, or bytes."""
import numpy as np
import pytest

import util
from test_gpu_band import DC, Scene, bits, c1, c2, coeffs, device_process, recording, same, status_of  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

B = 256 * 1032
BANDS = [coeffs(2, seed=24), coeffs(63, seed=21), coeffs(128, seed=22), coeffs(7, seed=23)]  # unequal taps: (2, 63, 128, 7)
RUN_BANDS = [coeffs(63, seed=30), coeffs(128, seed=31), coeffs(7, seed=32)]
FIND = dict(radius=2, max_sources=4, min_ratio=0.25)


def modes(pkg, mode, interp="lerp"):
    return dict(math=pkg.MATH_F32_EXACT if mode == "exact" else pkg.MATH_F32_FAST, interp=1 if interp == "fir8" else 0,
                fir=util.synthetic_fir_table() if interp == "fir8" else None)


def device_process_bands(eng, frames, bands):
    """process_bands_device of host frames -> powers [n_bands, batch, pixels]."""
    import torch

    d_x = torch.from_numpy(np.array(frames, np.float32)).cuda()
    d_p = torch.zeros((len(bands), len(frames), eng.pixel_count), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.process_bands_device(d_x.data_ptr(), len(frames), bands, d_p.data_ptr())
    eng.synchronize()
    return d_p.cpu().numpy()


def counted(eng):
    st = eng.stats()
    return st.frames, st.launches, st.kernel_variant


# ------------------------------------------------------------------------------------------------ 1. the single calls

@pytest.mark.parametrize("interp", ["lerp", "fir8"])
@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_single_calls_are_the_band_by_band_calls(pkg, c1, mode, interp):
    """math x interpolation, batches 1, 2, 3, 8, sets of 1 to 4 bands of 2, 63, 128 and 7 taps: process_bands(frames)[b] ==
    process on a second handle with set_band(coef[b]) == a band-less handle on band_filter(frames); process_bands_device likewise;
    frames and launches are counted as the band-by-band handle counts them in sum."""
    kw = modes(pkg, mode, interp)
    with c1.engine(8, **kw) as spec, c1.engine(8, **kw) as banded, c1.engine(8, **kw) as plain:
        for n_bands in (1, 2, 3, 4):
            bands = BANDS[:n_bands]
            for batch in (1, 2, 3, 8):
                got = spec.process_bands(c1.frames[:batch], bands)
                assert got.shape == (n_bands, batch, 1024)
                for b, c in enumerate(bands):
                    banded.set_band(c)
                    assert np.array_equal(bits(got[b]), bits(banded.process(c1.frames[:batch]))), (n_bands, batch, b)
                    assert np.array_equal(bits(got[b]), bits(plain.process(c1.filtered(c)[:batch]))), (n_bands, batch, b)
                assert np.all(np.isfinite(got)) and float(got.max(axis=(1, 2)).min()) > 0.0
                assert counted(spec) == counted(banded), (n_bands, batch)
            got = device_process_bands(spec, c1.frames[:3], bands)
            for b, c in enumerate(bands):
                banded.set_band(c)
                assert np.array_equal(bits(got[b]), bits(device_process(banded, c1.frames[:3]))), (n_bands, b)
                assert np.array_equal(bits(got[b]), bits(device_process(plain, c1.filtered(c)[:3]))), (n_bands, b)
            assert counted(spec) == counted(banded), n_bands
        assert spec.stats().last_kernel_ms > 0.0


@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_ragged_mics_and_gains_stay_behind_the_filter(pkg, c1, mode):
    rng = np.random.default_rng(7)
    index = np.sort(rng.choice(64, 51, replace=False)).astype(np.int32)
    gains = rng.uniform(0.5, 2.0, 64).astype(np.float32)
    kw = dict(modes(pkg, mode), index=index, gains=gains)
    with c1.engine(8, **kw) as spec, c1.engine(8, **kw) as banded:
        for batch in (1, 3, 8):
            got = spec.process_bands(c1.frames[:batch], BANDS)
            for b, c in enumerate(BANDS):
                banded.set_band(c)
                assert np.array_equal(bits(got[b]), bits(banded.process(c1.frames[:batch]))), (batch, b)
        got = device_process_bands(spec, c1.frames[:3], BANDS)
        for b, c in enumerate(BANDS):
            banded.set_band(c)
            assert np.array_equal(bits(got[b]), bits(device_process(banded, c1.frames[:3]))), b
        assert counted(spec) == counted(banded)


@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_c2_chunked_batch_and_wider_window(pkg, c2, mode):
    """256 mics, 64 x 64, batch 4, 128 taps among shorter ones: the chunked batch kernel behind a pre-pass of 64 workgroups a frame."""
    kw = modes(pkg, mode)
    bands = [coeffs(128, seed=2), coeffs(5, seed=24), coeffs(64, seed=25)]
    with c2.engine(4, **kw) as spec, c2.engine(4, **kw) as banded:
        got = spec.process_bands(c2.frames, bands)
        dev = device_process_bands(spec, c2.frames, bands)
        for b, c in enumerate(bands):
            banded.set_band(c)
            assert np.array_equal(bits(got[b]), bits(banded.process(c2.frames))) and float(got[b].max()) > 0.0, b
            assert spec.stats().kernel_variant == banded.stats().kernel_variant
            assert np.array_equal(bits(dev[b]), bits(device_process(banded, c2.frames))), b
        assert counted(spec) == counted(banded)


def test_a_batch_that_goes_up_in_pieces(pkg, c1):
    """64 host frames travel as two pieces on a second stream, each through one pre-pass and three sweeps."""
    frames = np.concatenate([c1.frames + np.float32(0.001 * k) for k in range(8)])
    bands = BANDS[1:]
    with c1.engine(64) as spec, c1.engine(64) as banded:
        got = spec.process_bands(frames, bands)
        assert spec.stats().last_kernel_ms > 0.0
        for b, c in enumerate(bands):
            banded.set_band(c)
            assert np.array_equal(bits(got[b]), bits(banded.process(frames))) and float(got[b].max()) > 0.0, b
        assert counted(spec) == counted(banded) and counted(spec)[:2] == (3 * 64, 3 * 2)


# ------------------------------------------------------------------------------------------------ 2. the runs

SHOWN = [dict(first=2, every=3), dict(first=0, every=1)]
_references = {}


def reference(pkg, c1, recording, mode, shown):
    """The band-by-band watch runs of the 11-block recording on fresh handles (max_batch 4: chunks of 4, 4, 3 and, where the last
    block is not shown, a frameless tail piece), and the raw run's ring: computed once per (mode, shown frames), left unchanged."""
    key = (mode, shown["first"], shown["every"])
    if key not in _references:
        _, samples = recording
        power = []
        for c in RUN_BANDS:
            with c1.engine(4, **modes(pkg, mode)) as eng:
                eng.set_band(c)
                power.append(eng.watch_samples(samples, 32, 32, want_image=False, want_power=True, **shown).power)
        with c1.engine(4, **modes(pkg, mode)) as raw:
            raw.process_samples(samples)
            ring = raw.ring_snapshot()
        power = np.stack(power)
        for a in (power, ring):
            a.setflags(write=False)
        assert float(power[:, -1].max(axis=1).min()) > 0.0
        _references[key] = (power, ring)
    return _references[key]


def check_images(pkg, got, power, channel, scale, flip):
    """image, dominant and big of a result against the rule, frame by frame."""
    Bn = pkg.binding
    assert got.image.shape == (power.shape[1], 32, 32, 3) and got.dominant.shape == (power.shape[1], 32, 32)
    for j in range(power.shape[1]):
        image, dominant = Bn.spectral_compose(power[:, j], channel, scale)
        assert np.array_equal(got.image[j].reshape(1024, 3), image), j
        assert np.array_equal(got.dominant[j].reshape(1024), dominant), j
        if got.big is not None:
            for c in range(3):
                plane = Bn.resize_linear_u8(got.image[j, :, :, c], 48, 40)
                assert np.array_equal(got.big[j, :, :, c], plane[:, ::-1] if flip else plane), (j, c)


def same_result(a, b):
    return all(same(getattr(a, name), getattr(b, name)) for name in ("image", "big", "dominant", "power")) and a.next_first == b.next_first


@pytest.mark.parametrize("shown", SHOWN, ids=["2_3", "0_1"])
@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_runs(pkg, c1, recording, mode, shown):
    import torch

    Bn = pkg.binding
    wire, samples = recording
    want_power, raw_ring = reference(pkg, c1, recording, mode, shown)
    n_frames = want_power.shape[1]
    kw = modes(pkg, mode)
    big = dict(out_rows=48, out_cols=40)
    results = {}
    for channel, scale, flip in (((2, -1, 0), Bn.SPECTRAL_SCALE_COMMON, False), ((0, 1, 2), Bn.SPECTRAL_SCALE_PER_BAND, True),
                                 ((1, 1, -1), Bn.SPECTRAL_SCALE_COMMON, True)):
        with c1.engine(4, **kw) as eng:
            got = eng.spectral_samples(samples, 32, 32, RUN_BANDS, channel, scale, flip=flip, want_power=True, **big, **shown)
            assert len(got) == n_frames and got.next_first == Bn.watch_count(11, **shown)[1]
            assert np.array_equal(bits(got.power), bits(want_power))
            check_images(pkg, got, want_power, channel, scale, flip)
            assert got.image.any() and got.big.any() and int(got.dominant.max()) <= 2
            assert np.array_equal(bits(eng.ring_snapshot()), bits(raw_ring))
            results[(channel, scale, flip)] = got
    channel, scale, flip = (2, -1, 0), Bn.SPECTRAL_SCALE_COMMON, False
    whole = results[(channel, scale, flip)]
    # the wire form
    with c1.engine(4, **kw) as eng:
        assert same_result(eng.spectral_blocks(wire, 32, 32, RUN_BANDS, channel, scale, want_power=True, **big, **shown), whole)
        assert np.array_equal(bits(eng.ring_snapshot()), bits(raw_ring))
    # any subset of the outputs
    with c1.engine(4, **kw) as eng:
        only = eng.spectral_samples(samples, 32, 32, RUN_BANDS, channel, scale, want_image=False, want_dominant=False, want_power=True, **shown)
        assert only.image is None and only.dominant is None and same(only.power, whole.power)
    with c1.engine(4, **kw) as eng:
        only = eng.spectral_samples(samples, 32, 32, RUN_BANDS, channel, scale, want_image=False, want_dominant=True, **big, **shown)
        assert only.power is None and same(only.big, whole.big) and same(only.dominant, whole.dominant)
    # 5 + 6 blocks over two calls
    with c1.engine(4, **kw) as eng:
        one = eng.spectral_samples(samples[:, : 256 * 5], 32, 32, RUN_BANDS, channel, scale, want_power=True, **big, **shown)
        two = eng.spectral_blocks(wire[5 * B:], 32, 32, RUN_BANDS, channel, scale, want_power=True, **big, first=one.next_first, every=shown["every"])
        assert len(one) + len(two) == n_frames and two.next_first == whole.next_first
        for name in ("image", "big", "dominant"):
            assert same(np.concatenate([getattr(one, name), getattr(two, name)]), getattr(whole, name)), name
        assert same(np.concatenate([one.power, two.power], axis=1), whole.power)
        assert np.array_equal(bits(eng.ring_snapshot()), bits(raw_ring))
    # the device form writes the same bytes in place; the sources of band 2 out of its device powers
    with c1.engine(4, **kw) as eng:
        d_x = torch.from_numpy(samples).cuda()
        d_p = torch.zeros((3, n_frames, 1024), dtype=torch.float32, device="cuda")
        d_i = torch.zeros((n_frames, 1024, 3), dtype=torch.uint8, device="cuda")
        d_b = torch.zeros((n_frames, 48, 40, 3), dtype=torch.uint8, device="cuda")
        d_d = torch.zeros((n_frames, 1024), dtype=torch.uint8, device="cuda")
        d_src = torch.zeros(n_frames * 4 * 40, dtype=torch.uint8, device="cuda")
        d_cnt = torch.zeros(n_frames, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        nxt = eng.spectral_samples_device(d_x.data_ptr(), samples.shape[1], 11, 32, 32, RUN_BANDS, channel, scale, d_image_ptr=d_i.data_ptr(),
                                          d_big_ptr=d_b.data_ptr(), d_dominant_ptr=d_d.data_ptr(), d_power_ptr=d_p.data_ptr(), **big, **shown)
        eng.find_peaks_device(d_p[2].data_ptr(), n_frames, 32, 32, d_src.data_ptr(), d_cnt.data_ptr(), **FIND)
        eng.synchronize()
        assert nxt == whole.next_first
        assert same(d_p.cpu().numpy(), whole.power) and same(d_i.cpu().numpy().reshape(whole.image.shape), whole.image)
        assert same(d_b.cpu().numpy(), whole.big) and same(d_d.cpu().numpy().reshape(whole.dominant.shape), whole.dominant)
        host = pkg.find_peaks(want_power[2], 32, 32, **FIND)
        found = d_src.cpu().numpy().view(Bn.SOURCE_DTYPE).reshape(n_frames, 4)
        assert np.array_equal(d_cnt.cpu().numpy(), host.count) and host.count[-1] >= 1
        assert np.array_equal(found["pixel"], host.sources["pixel"]) and np.array_equal(bits(found["power"]), bits(host.sources["power"]))
        assert np.array_equal(bits(eng.ring_snapshot()), bits(raw_ring))
        # the device form with only the large image asked for, unaligned: its compact image is the handle's own
        d_b1 = torch.zeros(n_frames * 48 * 40 * 3 + 1, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
    with c1.engine(4, **kw) as eng:
        eng.spectral_samples_device(d_x.data_ptr(), samples.shape[1], 11, 32, 32, RUN_BANDS, channel, scale, d_big_ptr=d_b1.data_ptr() + 1, **big, **shown)
        eng.synchronize()
        assert same(d_b1.cpu().numpy()[1:].reshape(whole.big.shape), whole.big) and int(d_b1[0]) == 0


def test_a_call_that_shows_nothing_ingests(pkg, c1, recording):
    """first >= n_blocks: nothing is written, the ring moves on by the call's blocks, and the run goes on from next_first."""
    import torch

    Bn = pkg.binding
    _, samples = recording
    want_power, raw_ring = reference(pkg, c1, recording, "exact", SHOWN[1])
    with c1.engine(4) as eng:
        none = eng.spectral_samples(samples[:, : 256 * 5], 32, 32, RUN_BANDS, want_power=True, out_rows=48, out_cols=40, first=5, every=1)
        assert len(none) == 0 and none.next_first == 0 and none.power.shape == (3, 0, 1024)
        rest = eng.spectral_samples(samples[:, 256 * 5:], 32, 32, RUN_BANDS, want_power=True, first=none.next_first, every=1)
        assert np.array_equal(bits(rest.power), bits(want_power[:, 5:]))
        assert np.array_equal(bits(eng.ring_snapshot()), bits(raw_ring))
    with c1.engine(4) as eng:
        d_x = torch.from_numpy(samples).cuda()
        d_out = torch.full((4096,), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        nxt = eng.spectral_samples_device(d_x.data_ptr(), samples.shape[1], 11, 32, 32, RUN_BANDS, d_image_ptr=d_out.data_ptr(),
                                          d_dominant_ptr=d_out.data_ptr(), d_power_ptr=d_out.data_ptr(), first=13, every=2)
        eng.synchronize()
        assert nxt == 2 and bool((d_out == 7).all().item())
        assert np.array_equal(bits(eng.ring_snapshot()), bits(raw_ring))


# ------------------------------------------------------------------------------------------------ 3. isolation

@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_a_nan_stays_in_its_frames(pkg, c1, recording, mode):
    """A NaN in mic 7 at sample 240 of block 5.  The snapshots after blocks 5 to 8 hold it, at history sample 256 * (8 - j) + 240
    of frame j; a frame is reached where a sweep's window [off, off + 256) of that mic, over all pixels, takes in one of the
    samples the NaN filters into -- with this table (off 228 .. 256) frames 7 and 8, in every band; every other frame is the
    clean run's, bit for bit."""
    _, samples = recording
    clean, _ = reference(pkg, c1, recording, mode, SHOWN[1])
    dirty = samples.copy()
    dirty[7, 256 * 5 + 240] = np.nan
    off7 = c1.off[:, 7].astype(np.int64)
    reached = {b: [j for j in range(5, 9) if np.any((off7 < 256 * (8 - j) + 240 + len(c)) & (off7 + 256 > 256 * (8 - j) + 240))]
               for b, c in enumerate(RUN_BANDS)}
    assert reached == {0: [7, 8], 1: [7, 8], 2: [7, 8]}
    with c1.engine(4, **modes(pkg, mode)) as eng:
        got = eng.spectral_samples(dirty, 32, 32, RUN_BANDS, (0, 1, 2), want_power=True)
    for b, c in enumerate(RUN_BANDS):
        with c1.engine(4, **modes(pkg, mode)) as banded:
            banded.set_band(c)
            want = banded.watch_samples(dirty, 32, 32, want_image=False, want_power=True).power
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got.power[b]), nan) and np.array_equal(bits(got.power[b])[~nan], bits(want)[~nan]), b
        assert sorted(set(np.argwhere(nan)[:, 0])) == [7, 8], b
        for j in range(11):
            if j not in (7, 8):
                assert np.array_equal(bits(got.power[b, j]), bits(clean[b, j])), (b, j)
    check_images(pkg, got, got.power, (0, 1, 2), pkg.binding.SPECTRAL_SCALE_COMMON, False)


# ------------------------------------------------------------------------------------------------ 4. refusals

def test_refusals_leave_the_handle_and_the_ring_alone(pkg, c1, recording):
    import torch

    Bn = pkg.binding
    wire, samples = recording
    good = RUN_BANDS
    inf = np.array([1.0, np.inf, 0.5], np.float32)
    with c1.engine(4) as eng, c1.engine(4) as twin:
        for e in (eng, twin):
            for b in range(4):
                e.ingest_block(wire[B * b: B * (b + 1)])
        ring = twin.ring_snapshot()
        before = eng.watch_samples(samples[:, 256 * 4:], 32, 32, want_power=True)  # (and the twin keeps step)
        twin.watch_samples(samples[:, 256 * 4:], 32, 32, want_power=True)
        ring = twin.ring_snapshot()
        d_x = torch.from_numpy(c1.frames[:2].copy()).cuda()
        d_s = torch.from_numpy(samples).cuda()
        d_p = torch.zeros((4, 11, 1024), dtype=torch.float32, device="cuda")
        d_c = torch.zeros(768, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        run = lambda bands, **kw: eng.spectral_samples(samples, 32, 32, bands, want_power=True, **kw)

        def with_colour_table(form):
            """A colour table in w: the Python interface has no way to say it, so the call is made on the library itself."""
            import ctypes as C

            w = Bn.Watch(0, 1, 32, 32, 0, 0, 0, C.c_void_p(d_c.data_ptr()))
            sp, _keep = Bn.spectral_of(good)
            out = np.zeros((3, 11, 1024), np.float32)
            tail = (11, C.byref(w), C.byref(sp), None, None, None, out.ctypes.data_as(C.POINTER(C.c_float)))
            if form == "samples":
                status = eng._lib.awpu_hip_spectral_samples(eng._h, samples.ctypes.data_as(C.POINTER(C.c_float)), samples.shape[1], *tail)
            else:
                status = eng._lib.awpu_hip_spectral_blocks(eng._h, wire, 1032, *tail)
            assert not out.any()
            Bn._check(status, "awpu_hip_spectral_" + form)

        refused = [
            (lambda: run([np.ones(129, np.float32)] + good), Bn.ERR_INVALID),
            (lambda: run(good[:2] + [inf]), Bn.ERR_INVALID),
            (lambda: run([]), Bn.ERR_INVALID),
            (lambda: run(BANDS + [good[0]]), Bn.ERR_INVALID),
            (lambda: run(good, channel=(0, 1, 4)), Bn.ERR_INVALID),
            (lambda: run(good, channel=(0, 1, 3)), Bn.ERR_INVALID),
            (lambda: run(good, scale=2), Bn.ERR_INVALID),
            (lambda: with_colour_table("samples"), Bn.ERR_INVALID),
            (lambda: with_colour_table("blocks"), Bn.ERR_INVALID),
            (lambda: eng.spectral_blocks(wire, 32, 32, [inf]), Bn.ERR_INVALID),
            (lambda: eng.process_bands(c1.frames[:2], [np.ones(129, np.float32)]), Bn.ERR_INVALID),
            (lambda: eng.process_bands(c1.frames[:2], [inf]), Bn.ERR_INVALID),
            (lambda: eng.process_bands(c1.frames[:2], []), Bn.ERR_INVALID),
            (lambda: eng.process_bands(c1.frames[:2], BANDS + [good[0]]), Bn.ERR_INVALID),
            (lambda: eng.process_bands(c1.frames[:5], good), Bn.ERR_INVALID),  # batch above max_batch
            (lambda: eng.process_bands_device(d_x.data_ptr(), 2, [inf], d_p.data_ptr()), Bn.ERR_INVALID),
            (lambda: eng.spectral_samples_device(d_s.data_ptr(), samples.shape[1], 11, 32, 32, good, channel=(4, 0, 0), d_power_ptr=d_p.data_ptr()), Bn.ERR_INVALID),
        ]

        def untouched(k):
            assert np.array_equal(bits(eng.ring_snapshot()), bits(ring)), k
            assert np.array_equal(bits(eng.process(c1.frames[:2])), bits(twin.process(c1.frames[:2]))), k
            assert np.array_equal(bits(eng.process_ring()), bits(twin.process_ring())), k

        for k, (call, status) in enumerate(refused):
            assert status_of(pkg, call) == status, k
            untouched(k)
        # a handle with a band of its own: the two would compose ambiguously
        for e in (eng, twin):
            e.set_band(good[0])
        for k, call in enumerate((lambda: run(good), lambda: eng.spectral_blocks(wire, 32, 32, good), lambda: eng.process_bands(c1.frames[:2], good),
                                  lambda: eng.process_bands_device(d_x.data_ptr(), 2, good, d_p.data_ptr()),
                                  lambda: eng.spectral_samples_device(d_s.data_ptr(), samples.shape[1], 11, 32, 32, good, d_power_ptr=d_p.data_ptr()))):
            assert status_of(pkg, call) == Bn.ERR_STATE, k
            untouched(("band", k))
        for e in (eng, twin):
            e.set_band(None)
        # a call in flight
        for e in (eng, twin):
            e.process_async(c1.frames[:2])
        for k, call in enumerate((lambda: run(good), lambda: eng.process_bands(c1.frames[:2], good),
                                  lambda: eng.process_bands_device(d_x.data_ptr(), 2, good, d_p.data_ptr()))):
            assert status_of(pkg, call) == Bn.ERR_STATE, k
        assert np.array_equal(bits(eng.wait()), bits(twin.wait()))
        untouched("async")
        eng.synchronize()
        assert not d_p.any().item()  # nothing was enqueued
        # afterwards: a valid spectral call, then a valid plain one with the plain call's bits
        got = eng.spectral_samples(samples[:, 256 * 4:], 32, 32, good, want_power=True)
        assert float(got.power.max()) > 0.0 and got.image.any()
        again = eng.watch_samples(samples[:, 256 * 4:], 32, 32, want_power=True)
        twin.watch_samples(samples[:, 256 * 4:], 32, 32, want_power=True)
        same_again = twin.watch_samples(samples[:, 256 * 4:], 32, 32, want_power=True)
        assert same(again.power, same_again.power) and same(again.image, same_again.image)
        assert np.array_equal(bits(again.power[3:]), bits(before.power[3:]))  # (from the fourth frame on a snapshot is the call's own blocks)
    with pkg.Engine(n_pixels=100 * 100, n_streams=64, max_batch=4, grid_columns=100, devices=[0, 0]) as group:
        assert status_of(pkg, lambda: group.process_bands(c1.frames[:2], good)) == Bn.ERR_STATE
        assert status_of(pkg, lambda: group.spectral_samples(samples, 100, 100, good)) == Bn.ERR_STATE
    # a handle without a table
    with pkg.Engine(n_pixels=1024, n_streams=64, max_batch=4, grid_columns=32) as bare:
        assert status_of(pkg, lambda: bare.process_bands(c1.frames[:2], good)) == Bn.ERR_STATE
        assert status_of(pkg, lambda: bare.spectral_samples(samples, 32, 32, good)) == Bn.ERR_STATE


def test_a_table_that_leaves_too_little_history(pkg):
    """The hand-made table of tests/test_gpu_band.py whose smallest off is 10: one band of 12 taps among shorter ones is refused
    with AWPU_ERR_RANGE by every form, before anything is enqueued; 11 taps read the snapshot from its first sample on."""
    Bn = pkg.binding
    rng = np.random.default_rng(9)
    off = rng.integers(10, 120, (64, 64)).astype(np.int32)
    off[5, 9] = 10
    frac = rng.uniform(0.0, 0.999, (64, 64)).astype(np.float32)
    frames = util.hash_frames(64, 1024, seed=10, batch=2) + DC
    long, short = [coeffs(3, seed=9), coeffs(12, seed=9), coeffs(5, seed=9)], [coeffs(3, seed=9), coeffs(11, seed=9), coeffs(5, seed=9)]

    def make():
        eng = pkg.Engine(n_pixels=64, n_streams=64, max_batch=2, grid_columns=8)
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        return eng

    with make() as eng, make() as banded:
        for call in (lambda: eng.process_bands(frames, long), lambda: eng.spectral_samples(np.zeros((64, 512), np.float32), 8, 8, long)):
            assert status_of(pkg, call) == Bn.ERR_RANGE
        with pytest.raises(pkg.AwpuError):
            eng.ring_snapshot()  # nothing was enqueued: not even the ring exists
        got = eng.process_bands(frames, short)
        for b, c in enumerate(short):
            banded.set_band(c)
            assert np.array_equal(bits(got[b]), bits(banded.process(frames))), b


# ------------------------------------------------------------------------------------------------ 5. physics

def test_two_sources_separate_by_colour(pkg, c1):
    """Two plane waves on c1 in noise of 1e-3, of amplitude 0.05 each: 3 kHz from (20, 35) degrees and 8 kHz from (35, 200) degrees;
    the reference's three bands (1950-3541, 3541-6375, 6375-9000 Hz) at 63 taps.  Amplitudes of equal order, so that the low
    source's sidelobe in band 0 stays below the high source's peak in band 2 at that pixel.  The host composition -- the oracle's
    fp32 sweep of band_filter(frame) per band, then spectral_compose -- shows on the CPU with these amplitudes: dominant 0 at the
    low source's pixel (628) and 2 at the high one's (391); band 0 / band 2 there 254 and 1 / 8490; with SCALE_PER_BAND the
    brightest byte-0 pixel is 628 and the brightest byte-2 pixel 391 (one pixel of level 255 each)."""
    S, Bn = pkg.synthetic, pkg.binding
    low, high = (np.deg2rad(20.0), np.deg2rad(35.0)), (np.deg2rad(35.0), np.deg2rad(200.0))
    t = np.arange(1024, dtype=np.float64)
    frame = S.NOISE * np.random.default_rng(12).uniform(-1.0, 1.0, (64, 1024))
    for (theta, phi), hz in ((low, 3e3), (high, 8e3)):
        tau = pkg.steering_delays(c1.xyz, theta, phi).astype(np.float64)
        frame += 0.05 * np.sin(2.0 * np.pi * hz * (t[None, :] + tau[:, None]) / S.SAMPLE_RATE)  # the phase model of synthetic.make_frames
    frame = frame.astype(np.float32)
    pixel = lambda d: S.source_pixel(c1.spec, *d)[0] * 32 + S.source_pixel(c1.spec, *d)[1]
    p_low, p_high = pixel(low), pixel(high)
    assert p_low != p_high
    bands = [Bn.band_design(lo, hi, 63) for lo, hi in ((1950, 3541), (3541, 6375), (6375, 9000))]
    # the host composition: a band-less engine on the filtered frame, then the rule
    with c1.engine(4) as plain:
        host_power = np.stack([plain.process(Bn.band_filter(frame, c)) for c in bands])
    host_image, host_dominant = Bn.spectral_compose(host_power, (0, 1, 2), Bn.SPECTRAL_SCALE_PER_BAND)
    assert host_dominant[p_low] == 0 and host_dominant[p_high] == 2
    # the run: a recording whose last block ends the frame, on a fresh handle
    with c1.engine(4) as eng:
        got = eng.spectral_samples(frame, 32, 32, bands, (0, 1, 2), Bn.SPECTRAL_SCALE_PER_BAND, first=3, want_power=True)
    assert len(got) == 1
    power, image, dominant = got.power[:, 0], got.image[0].reshape(1024, 3), got.dominant[0].reshape(1024)
    print(f"band 0 / band 2 power: {power[0, p_low] / power[2, p_low]:.3g} at the 3 kHz pixel {p_low}, {power[0, p_high] / power[2, p_high]:.3g} at the "
          f"8 kHz pixel {p_high}; band 0's sidelobe there / band 2's peak {power[0, p_high] / power[2].max():.3g}; "
          f"brightest byte 0 at {int(image[:, 0].argmax())}, byte 2 at {int(image[:, 2].argmax())}")
    assert np.array_equal(bits(power), bits(host_power)) and np.array_equal(image, host_image) and np.array_equal(dominant, host_dominant)
    assert dominant[p_low] == 0 and dominant[p_high] == 2
    assert power[0, p_high] < power[2, p_high]
    assert int(image[:, 0].argmax()) == p_low and int((image[:, 0] == 255).sum()) == 1
    assert int(image[:, 2].argmax()) == p_high and int((image[:, 2] == 255).sum()) == 1


# ------------------------------------------------------------------------------------------------ 6. sizes that are no multiple of four

def test_an_odd_grid_and_a_large_image_of_odd_width(pkg, recording):
    """33 x 33 pixels (1089: the last lane of the display step holds one pixel, and every frame but the first starts at an odd
    address) and a large image of 50 x 43 (a row's last unit of four pixels is moved left to end with the row; rows are not whole
    dwords), both flips and both scales, against the same rules."""
    Bn = pkg.binding
    _, samples = recording
    off, frac = pkg.build_delay_table(pkg.create_antenna(), 33, 33)
    assert int(off.min()) >= 62
    bands = [Bn.band_design(lo, hi, 63) for lo, hi in ((1950, 3541), (3541, 6375), (6375, 9000))]

    def make():
        eng = pkg.Engine(n_pixels=33 * 33, n_streams=64, max_batch=4, grid_columns=33)
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        return eng

    power = []
    for c in bands:
        with make() as eng:
            eng.set_band(c)
            power.append(eng.watch_samples(samples, 33, 33, want_image=False, want_power=True, first=1, every=2).power)
    power = np.stack(power)
    for channel, scale, flip in (((0, 1, 2), Bn.SPECTRAL_SCALE_COMMON, True), ((2, -1, 1), Bn.SPECTRAL_SCALE_PER_BAND, False)):
        with make() as eng:
            got = eng.spectral_samples(samples, 33, 33, bands, channel, scale, first=1, every=2, out_rows=50, out_cols=43, flip=flip, want_power=True)
        assert len(got) == 5 and np.array_equal(bits(got.power), bits(power))
        for j in range(5):
            image, dominant = Bn.spectral_compose(power[:, j], channel, scale)
            assert np.array_equal(got.image[j].reshape(1089, 3), image) and np.array_equal(got.dominant[j].reshape(1089), dominant), j
            for c in range(3):
                plane = Bn.resize_linear_u8(got.image[j, :, :, c], 50, 43)
                assert np.array_equal(got.big[j, :, :, c], plane[:, ::-1] if flip else plane), (j, c)
        assert got.image.any() and got.big.any()


# ------------------------------------------------------------------------------------------------ 7. the video tool

@pytest.mark.parametrize("band_scale", ["common", "per-band"])
def test_the_video_tool_writes_the_bands_as_colours(pkg, recording, tmp_path, band_scale):
    """tools/pcap_video.py --bands on a capture of the 11-block recording: the frames of the AVI it writes are spectral_blocks' large
    images, the lowest band in the red byte of a B G R pixel, for both --band-scale choices."""
    import importlib.util
    from pathlib import Path

    from test_blocks_cpu import udp_frame, write_pcap

    Bn = pkg.binding
    spec = importlib.util.spec_from_file_location("pcap_video", Path(__file__).resolve().parent.parent / "tools" / "pcap_video.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    wire, _ = recording
    write_pcap(tmp_path / "rec.pcap", [udp_frame(wire[k: k + 1032], 21844) for k in range(0, 11 * B, 1032)])
    text = "6375:9000,1950:3541:31,3541:6375"
    assert tool.main([str(tmp_path / "rec.pcap"), "--port", "21844", "--cols", "32", "--every", "2", "--chunk", "4", "--max-batch", "4", "--size", "50",
                      "--flip", "--bands", text, "--band-scale", band_scale, "--out", str(tmp_path / "colours")]) == 0
    frames, rate, scale = tool.read_avi(tmp_path / "colours.000.avi")
    assert (rate, scale) == tool.frame_rate(2)
    bands, channel = tool.bands_of_text(Bn, text)
    assert channel == (2, 1, 0)
    off, frac = pkg.build_delay_table(pkg.create_tiled_antenna(1, 1), 32, 32, 180.0)
    with pkg.Engine(n_pixels=1024, n_streams=64, max_batch=4, grid_columns=32) as eng:
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        want = eng.spectral_blocks(wire, 32, 32, bands, channel, Bn.SPECTRAL_SCALE_COMMON if band_scale == "common" else Bn.SPECTRAL_SCALE_PER_BAND,
                                   every=2, out_rows=50, out_cols=50, flip=True, want_power=True)
    assert len(want) == 6 and np.array_equal(frames, want.big) and frames.any()
    # red is the lowest band: under the common scale a pixel's red byte (2) and blue byte (0) stand as its powers in bands 0 and 2 do
    if band_scale == "common":
        level = want.image.reshape(6, 1024, 3).astype(np.int32)
        lower_wins = want.power[0] >= want.power[2]
        assert np.all(level[..., 2][lower_wins] >= level[..., 0][lower_wins]) and np.all(level[..., 0][~lower_wins] >= level[..., 2][~lower_wins])
        assert np.any(level[..., 2] != level[..., 0])
