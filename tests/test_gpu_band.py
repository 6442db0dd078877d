"""Band-limited heatmaps (include/awpu_hip_band.h) on the device.  What a call returns with a band is defined by composition:
bit for bit what the same call on a band-less handle of the same configuration returns on input that awpu_hip_band_filter has
filtered on the host.  Checked here for the single calls in both fp32 modes and both interpolations, for ragged mic lists with
gains, at c2, for the exported sums, the asynchronous and one-frame calls, the ring, the runs of blocks (heatmaps, images,
sources; audio and trail stay raw), replaced and cleared bands, a NaN that stays in its frame, the refusals, and two plane waves
of which the band picks the weak high one.  Bit-equal = equal as uint32 views."""
import math

import numpy as np
import pytest

import util
from test_gpu_blocks import engine, make_datagrams

pytestmark = pytest.mark.gpu

B = 256 * 1032
DC = np.float32(0.01)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def coeffs(taps, seed=0):
    """Seeded coefficients of both signs, of a size that keeps the filtered frames near the frames' own."""
    c = (np.random.default_rng(1000 * seed + taps).standard_normal(taps) / math.sqrt(taps)).astype(np.float32)
    assert taps == 1 or (np.any(c > 0) and np.any(c < 0))
    return c


class Scene:
    def __init__(self, pkg, name, batch, seed):
        S = pkg.synthetic
        self.spec = S.WORKLOADS[name]
        self.xyz = S.geometry(self.spec)
        self.off, self.frac = S.delay_table(self.spec, self.xyz)
        self.frames = S.make_frames(self.xyz, batch, seed=seed) + DC
        self.lo = int(self.off.min())
        self._filtered = {}
        self.pkg = pkg

    def filtered(self, c):
        """binding.band_filter(frames) for these coefficients, computed once and left unchanged."""
        key = c.tobytes()
        if key not in self._filtered:
            self._filtered[key] = self.pkg.binding.band_filter(self.frames, c)
            self._filtered[key].setflags(write=False)
        return self._filtered[key]

    def engine(self, max_batch, **kw):
        return engine(self.pkg, self.off, self.frac, self.spec.n_mics, self.spec.res, max_batch, **kw)


@pytest.fixture(scope="module")
def c1(pkg):
    scene = Scene(pkg, "c1", 8, seed=41)
    assert scene.lo >= 127, scene.lo  # 128 taps fit this geometry's history
    return scene


@pytest.fixture(scope="module")
def c2(pkg):
    scene = Scene(pkg, "c2", 4, seed=42)
    assert scene.lo >= 127, scene.lo
    return scene


def device_process(eng, frames, sums=False):
    """process_device (or process_device_sums) of host frames -> powers (, sums)."""
    import torch

    d_x = torch.from_numpy(np.array(frames, np.float32)).cuda()  # (a copy: the shared references are read-only)
    d_p = torch.zeros((len(frames), eng.pixel_count), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    if not sums:
        eng.process_device(d_x.data_ptr(), len(frames), d_p.data_ptr())
        eng.synchronize()
        return d_p.cpu().numpy()
    d_s = torch.zeros((len(frames), eng.pixel_count, 256), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.process_device_sums(d_x.data_ptr(), len(frames), d_p.data_ptr(), d_s.data_ptr())
    eng.synchronize()
    return d_p.cpu().numpy(), d_s.cpu().numpy()


@pytest.fixture(scope="module")
def recording(pkg, oracle, c1):
    """11 blocks of c1's plane wave in noise plus the DC offset, quantised to the wire's 24 bits (as tests/test_gpu_find.py builds
    its recording): (wire, the samples the wire unpacks to [64, 2816])."""
    wave = pkg.synthetic.make_frames(c1.xyz, 1, seed=43, hist=256 * 11)[0] + DC
    ints = np.rint(wave.astype(np.float64) * 8388608.0).astype(np.int32)
    wire, blocks = [], []
    for b in range(11):
        stream = np.zeros((256, 256), np.int32)
        stream[:, :64] = ints[:, 256 * b: 256 * (b + 1)].T
        wire.append(make_datagrams(stream, counter0=256 * b))
        blocks.append(oracle.unpack_exposure(stream, 64))
    return b"".join(wire), np.ascontiguousarray(np.concatenate(blocks, axis=1), np.float32)


# ------------------------------------------------------------------------------------------------ 1. identity

@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_one_tap_of_one_changes_nothing(pkg, c1, recording, mode):
    """taps 1, c = {1.0}: process (batch 1, 2, 5), process_device and process_ring return the bits of the same handle without a band."""
    wire, _ = recording
    math_mode = pkg.MATH_F32_EXACT if mode == "exact" else pkg.MATH_F32_FAST
    with c1.engine(8, math=math_mode) as eng:
        for b in range(4):
            eng.ingest_block(wire[B * b: B * (b + 1)])
        call = lambda: [eng.process(c1.frames[:1]), eng.process(c1.frames[:2]), eng.process(c1.frames[:5]), device_process(eng, c1.frames[:5]),
                        eng.process_ring(), eng.process(c1.frames[0])]
        plain = call()
        eng.set_band(np.ones(1, np.float32))
        banded = call()
    for k, (got, want) in enumerate(zip(banded, plain)):
        assert np.array_equal(bits(got), bits(want)), k
        assert np.all(np.isfinite(got)) and float(np.max(got)) > 0.0


# ------------------------------------------------------------------------------------------------ 2. the definition

@pytest.mark.parametrize("interp", ["lerp", "fir8"])
@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_band_is_the_sweep_of_filtered_frames(pkg, c1, mode, interp):
    """math x interpolation, batches 1, 2, 3, 8, taps 2, 63, 128: powers with the band == powers of a band-less engine on
    binding.band_filter(frames)."""
    kw = dict(math=pkg.MATH_F32_EXACT if mode == "exact" else pkg.MATH_F32_FAST, interp=1 if interp == "fir8" else 0,
              fir=util.synthetic_fir_table() if interp == "fir8" else None)
    with c1.engine(8, **kw) as banded, c1.engine(8, **kw) as plain:
        for taps in (2, 63, 128):
            c = coeffs(taps)
            banded.set_band(c)
            for batch in (1, 2, 3, 8):
                got, want = banded.process(c1.frames[:batch]), plain.process(c1.filtered(c)[:batch])
                assert np.array_equal(bits(got), bits(want)), (taps, batch)
                assert np.all(np.isfinite(got)) and float(np.max(got)) > 0.0
        # device frames take another path to the same definition
        assert np.array_equal(bits(device_process(banded, c1.frames[:3])), bits(device_process(plain, c1.filtered(c)[:3])))
        st_b, st_p = banded.stats(), plain.stats()
        assert (st_b.frames, st_b.launches, st_b.kernel_variant) == (st_p.frames, st_p.launches, st_p.kernel_variant)  # counted like the plain calls


def test_a_batch_that_goes_up_in_pieces(pkg, c1):
    """64 host frames travel as two pieces on a second stream, each through the pre-pass: the pieces' sweeps, and the timed span."""
    frames = np.concatenate([c1.frames + np.float32(0.001 * k) for k in range(8)])
    c = coeffs(7)
    with c1.engine(64) as banded, c1.engine(64) as plain:
        banded.set_band(c)
        got, want = banded.process(frames), plain.process(pkg.binding.band_filter(frames, c))
        assert np.array_equal(bits(got), bits(want)) and float(got.max()) > 0.0
        st_b, st_p = banded.stats(), plain.stats()
        assert (st_b.frames, st_b.launches) == (st_p.frames, st_p.launches) == (64, 2) and st_b.last_kernel_ms > 0.0


@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_ragged_mics_and_gains_stay_behind_the_filter(pkg, c1, mode):
    rng = np.random.default_rng(7)
    index = np.sort(rng.choice(64, 51, replace=False)).astype(np.int32)
    gains = rng.uniform(0.5, 2.0, 64).astype(np.float32)
    kw = dict(math=pkg.MATH_F32_EXACT if mode == "exact" else pkg.MATH_F32_FAST, index=index, gains=gains)
    c = coeffs(63)
    with c1.engine(8, **kw) as banded, c1.engine(8, **kw) as plain:
        banded.set_band(c)
        for batch in (1, 3, 8):
            assert np.array_equal(bits(banded.process(c1.frames[:batch])), bits(plain.process(c1.filtered(c)[:batch]))), batch
        assert np.array_equal(bits(device_process(banded, c1.frames[:3])), bits(device_process(plain, c1.filtered(c)[:3])))


@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_c2_chunked_batch_and_wider_window(pkg, c2, mode):
    """256 mics, 64 x 64, batch 4: the chunked batch kernel, four streams' worth of workgroups, a wider window."""
    kw = dict(math=pkg.MATH_F32_EXACT if mode == "exact" else pkg.MATH_F32_FAST)
    c = coeffs(128, seed=2)
    with c2.engine(4, **kw) as banded, c2.engine(4, **kw) as plain:
        banded.set_band(c)
        got, want = banded.process(c2.frames), plain.process(c2.filtered(c))
        assert np.array_equal(bits(got), bits(want)) and float(np.max(got)) > 0.0
        assert banded.stats().kernel_variant == plain.stats().kernel_variant
        assert np.array_equal(bits(device_process(banded, c2.frames)), bits(device_process(plain, c2.filtered(c))))
        assert np.array_equal(bits(banded.process(c2.frames[:1])), bits(plain.process(c2.filtered(c)[:1])))


@pytest.mark.parametrize("interp", ["lerp", "fir8"])
def test_exported_sums_follow_the_band(pkg, c1, interp):
    kw = dict(interp=1 if interp == "fir8" else 0, fir=util.synthetic_fir_table() if interp == "fir8" else None)
    c = coeffs(63)
    with c1.engine(4, **kw) as banded, c1.engine(4, **kw) as plain:
        banded.set_band(c)
        got_p, got_s = device_process(banded, c1.frames[:3], sums=True)
        want_p, want_s = device_process(plain, c1.filtered(c)[:3], sums=True)
    assert np.array_equal(bits(got_p), bits(want_p)) and np.array_equal(bits(got_s), bits(want_s))
    assert float(np.abs(got_s).max()) > 0.0


# ------------------------------------------------------------------------------------------------ 3. async, and the one-frame call

def test_async_equals_process(pkg, c1):
    c = coeffs(63)
    with c1.engine(8) as eng:
        eng.set_band(c)
        want = eng.process(c1.frames[:5])
        eng.process_async(c1.frames[:5])
        with pytest.raises(pkg.AwpuError) as e:  # (the band is not replaced under a call in flight)
            eng.set_band(None)
        assert e.value.status == pkg.binding.ERR_STATE
        got = eng.wait()
        assert np.array_equal(bits(got), bits(want))
    with c1.engine(8) as plain:
        assert np.array_equal(bits(got), bits(plain.process(c1.filtered(c)[:5])))


def test_one_frame_host_call_at_the_reference_shape(pkg, oracle):
    """64 mics, 100 x 100, one frame per call: the host call == process_device of the same frame, both with the band."""
    xyz = oracle.create_antenna()
    off, frac = oracle.compute_delay_lut(xyz, 100, 100)
    frame = pkg.synthetic.make_frames(pkg.create_antenna(), 1, seed=44) + DC
    c = coeffs(63)
    with engine(pkg, off, frac, 64, 100, 1) as eng, engine(pkg, off, frac, 64, 100, 1) as plain:
        eng.set_band(c)
        got = eng.process(frame[0])
        assert np.array_equal(bits(got), bits(device_process(eng, frame)[0]))
        assert np.array_equal(bits(got), bits(plain.process(pkg.binding.band_filter(frame, c)[0])))
        assert np.array_equal(bits(eng.process(frame[0])), bits(got))  # and again: nothing of the first call lingers


# ------------------------------------------------------------------------------------------------ 4. the runs

@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_runs_of_blocks(pkg, c1, recording, mode):
    """11 blocks, max_batch 4, fresh handles (a zero ring filters to a zero ring): the run with a band == the band-less run over
    the filtered recording, for every block, however the recording is split; the ring keeps the raw samples."""
    wire, samples = recording
    c = coeffs(128, seed=3)
    filtered = pkg.binding.band_filter(samples, c)
    kw = dict(math=pkg.MATH_F32_EXACT if mode == "exact" else pkg.MATH_F32_FAST)
    with c1.engine(4, **kw) as plain:
        want = plain.process_samples(filtered)
    with c1.engine(4, **kw) as raw:
        raw.process_samples(samples)
        raw_ring = raw.ring_snapshot()
    assert float(want[-1].max()) > 0.0
    with c1.engine(4, **kw) as eng:
        eng.set_band(c)
        got = eng.process_samples(samples)
        assert np.array_equal(bits(got), bits(want))
        assert np.array_equal(bits(eng.ring_snapshot()), bits(raw_ring))
        # the ring, swept under the same band: the last block's row
        assert np.array_equal(bits(eng.process_ring()), bits(eng.process(eng.ring_snapshot())))
        assert mode == "fast" or np.array_equal(bits(eng.process_ring()), bits(want[-1]))
    with c1.engine(4, **kw) as eng:
        eng.set_band(c)
        split = np.concatenate([eng.process_samples(samples[:, : 256 * 5]), eng.process_samples(samples[:, 256 * 5:])])
        assert np.array_equal(bits(split), bits(want))
    with c1.engine(4, **kw) as eng:
        eng.set_band(c)
        assert np.array_equal(bits(eng.process_blocks(wire)), bits(want))
    with c1.engine(4, **kw) as eng:
        eng.set_band(c)
        for b in range(6):
            eng.ingest_block(wire[B * b: B * (b + 1)])
            assert np.array_equal(bits(eng.process_ring()), bits(eng.process(eng.ring_snapshot()))), b
        assert mode == "fast" or np.array_equal(bits(eng.process_ring()), bits(want[5]))


def test_watch_find_and_listen_runs(pkg, c1, recording):
    import torch

    _, samples = recording
    c = coeffs(63, seed=4)
    filtered = pkg.binding.band_filter(samples, c)
    shown = dict(first=2, every=3)
    with c1.engine(4) as plain:
        want = plain.watch_samples(filtered, 32, 32, out_rows=48, out_cols=40, want_power=True, **shown)
    assert len(want) == 3 and want.image.any() and want.big.any()
    find = dict(radius=2, max_sources=4, min_ratio=0.25)
    with c1.engine(4) as eng:
        eng.set_band(c)
        got = eng.watch_samples(samples, 32, 32, out_rows=48, out_cols=40, want_power=True, **shown)
        assert np.array_equal(got.image, want.image) and np.array_equal(got.big, want.big) and np.array_equal(bits(got.power), bits(want.power))
        assert got.next_first == want.next_first
    with c1.engine(4) as eng:
        eng.set_band(c)
        found = eng.find_samples(samples, 32, 32, want_power=True, **shown, **find)
        host = pkg.find_peaks(want.power, 32, 32, **find)
        assert np.array_equal(bits(found.power), bits(want.power))
        assert np.array_equal(found.count, host.count) and found.count[-1] >= 1
        for name in ("pixel", "row", "col"):
            assert np.array_equal(found.sources[name], host.sources[name]), name
        assert np.array_equal(bits(found.sources["power"]), bits(host.sources["power"]))
    # the device form: the same powers and sources, in place
    with c1.engine(4) as eng:
        eng.set_band(c)
        d_x = torch.from_numpy(samples).cuda()
        d_p = torch.zeros((3, 1024), dtype=torch.float32, device="cuda")
        d_src = torch.zeros(3 * 4 * 40, dtype=torch.uint8, device="cuda")
        d_cnt = torch.zeros(3, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        eng.find_samples_device(d_x.data_ptr(), samples.shape[1], 11, 32, 32, d_src.data_ptr(), d_cnt.data_ptr(), d_power_ptr=d_p.data_ptr(), **shown, **find)
        eng.synchronize()
        assert np.array_equal(bits(d_p.cpu().numpy()), bits(want.power)) and np.array_equal(d_cnt.cpu().numpy(), host.count)
        assert np.array_equal(d_src.cpu().numpy().view(pkg.binding.SOURCE_DTYPE)["pixel"].reshape(3, 4), host.sources["pixel"])
    # listening: audio and trail hear the raw recording, the heatmaps of the same pass the band
    who = (np.array([0.3, 0.6, 0.35]), np.array([0.5, 3.4, 0.6]), 0.05, 0.1, np.array([0, 0, 2], np.int32))
    with c1.engine(4) as plain:
        band_power = plain.process_samples(filtered)
    with c1.engine(4) as eng, c1.engine(4) as raw:
        for e in (eng, raw):
            e.set_antenna(c1.xyz)
        eng.set_band(c)
        got = eng.listen_samples(samples, *who, math.pi / 2, want_power=True)
        heard = raw.listen_samples(samples, *who, math.pi / 2, want_power=True)
        assert same(got.audio, heard.audio) and same(got.trail, heard.trail) and same(got.listeners, heard.listeners)
        assert float(np.abs(got.audio[:2]).max()) > 0.0
        assert np.array_equal(bits(got.power), bits(band_power)) and not np.array_equal(bits(got.power), bits(heard.power))
        assert np.array_equal(bits(eng.ring_snapshot()), bits(raw.ring_snapshot()))


# ------------------------------------------------------------------------------------------------ 5. replace and clear

def test_replace_and_clear(pkg, c1):
    with c1.engine(8) as eng, c1.engine(8) as plain:
        never = plain.process(c1.frames[:3])
        for taps in (128, 3, 63):
            c = coeffs(taps, seed=5)
            eng.set_band(c)
            assert np.array_equal(bits(eng.process(c1.frames[:3])), bits(plain.process(c1.filtered(c)[:3]))), taps
            assert np.array_equal(bits(eng.process(c1.frames[0])), bits(plain.process(c1.filtered(c)[0]))), taps
        eng.set_band(None)
        assert np.array_equal(bits(eng.process(c1.frames[:3])), bits(never))
        assert np.array_equal(bits(eng.process(c1.frames[0])), bits(never[0]))
        assert np.array_equal(bits(device_process(eng, c1.frames[:3])), bits(device_process(plain, c1.frames[:3])))


# ------------------------------------------------------------------------------------------------ 6. isolation

@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_a_nan_stays_in_its_frame(pkg, c1, mode):
    c = coeffs(63, seed=6)
    dirty = c1.frames[:3].copy()
    dirty[1, 7, c1.lo + 100] = np.nan
    kw = dict(math=pkg.MATH_F32_EXACT if mode == "exact" else pkg.MATH_F32_FAST)
    with c1.engine(4, **kw) as eng, c1.engine(4, **kw) as plain:
        eng.set_band(c)
        clean = eng.process(c1.frames[:3])
        got = eng.process(dirty)
        want = plain.process(pkg.binding.band_filter(dirty, c))
        got_dev = device_process(eng, dirty)
    for k in (0, 2):
        assert np.array_equal(bits(got[k]), bits(clean[k])), k
        assert np.array_equal(bits(got_dev[k]), bits(clean[k])), k
    for g in (got[1], got_dev[1]):
        nan = np.isnan(want[1])
        assert nan.any() and np.array_equal(np.isnan(g), nan)
        assert np.array_equal(bits(g)[~nan], bits(want[1])[~nan])
    # ... and the filter itself: the NaN reaches the 63 outputs behind it in its own row, and nothing else
    y = pkg.binding.band_filter(dirty, c)
    where = np.argwhere(np.isnan(y))
    assert len(where) == 63 and np.all(where[:, 0] == 1) and np.all(where[:, 1] == 7) and where[:, 2].min() == c1.lo + 100 and where[:, 2].max() == c1.lo + 162


# ------------------------------------------------------------------------------------------------ 7. refusals

def status_of(pkg, call):
    with pytest.raises(pkg.AwpuError) as e:
        call()
    return e.value.status


def test_refusals_leave_the_handle_and_the_ring_alone(pkg, c1, recording):
    import torch

    Bn = pkg.binding
    wire, _ = recording
    c = coeffs(63, seed=8)
    with c1.engine(4) as eng, c1.engine(4) as twin:
        for e in (eng, twin):
            e.set_band(c)
            for b in range(4):
                e.ingest_block(wire[B * b: B * (b + 1)])
        ring = twin.ring_snapshot()
        d_x = torch.from_numpy(c1.frames[:2].copy()).cuda()
        d_k = torch.zeros(2 * 64 * 1024 * 4, dtype=torch.float32, device="cuda")
        d_p = torch.zeros((2, 1024), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        refused = [
            (lambda: eng.set_band(np.ones(129, np.float32)), Bn.ERR_INVALID),
            (lambda: eng.set_band(np.array([1.0, np.inf, 0.5], np.float32)), Bn.ERR_INVALID),
            (lambda: eng.set_band(np.array([np.nan], np.float32)), Bn.ERR_INVALID),
            (lambda: eng.set_band(np.zeros(0, np.float32)), Bn.ERR_INVALID),
            (lambda: eng.live_block(wire[:B], 32, 32), Bn.ERR_STATE),
            (lambda: eng.packed_bytes(2), Bn.ERR_STATE),
            (lambda: eng.pack_frames(d_x.data_ptr(), 2, d_k.data_ptr()), Bn.ERR_STATE),
            (lambda: eng.process_packed(d_k.data_ptr(), 2, d_p.data_ptr()), Bn.ERR_STATE),
        ]
        for k, (call, status) in enumerate(refused):
            assert status_of(pkg, call) == status, k
            assert np.array_equal(bits(eng.ring_snapshot()), bits(ring)), k
            assert np.array_equal(bits(eng.process(c1.frames[:2])), bits(twin.process(c1.frames[:2]))), k
            assert np.array_equal(bits(eng.process_ring()), bits(twin.process_ring())), k
        eng.synchronize()
        assert not d_k.any().item() and not d_p.any().item()  # nothing was enqueued
        # without the band the same calls go through again
        eng.set_band(None)
        power, _, _ = eng.live_block(wire[4 * B: 5 * B], 32, 32)
        twin.set_band(None)
        twin.ingest_block(wire[4 * B: 5 * B])
        assert np.array_equal(bits(power), bits(twin.process_ring()))
    with pkg.Engine(n_pixels=100 * 100, n_streams=64, max_batch=4, grid_columns=100, devices=[0, 0]) as group:
        assert status_of(pkg, lambda: group.set_band(c)) == Bn.ERR_STATE
        assert status_of(pkg, lambda: group.set_band(None)) == Bn.ERR_STATE


def test_a_table_that_leaves_too_little_history(pkg):
    """A hand-made table whose smallest off is 10: 12 taps are refused with AWPU_ERR_RANGE -- by set_band when the table comes
    first, by the call that would sweep when the band comes first --, 11 taps read the snapshot from its first sample on."""
    Bn = pkg.binding
    rng = np.random.default_rng(9)
    off = rng.integers(10, 120, (64, 64)).astype(np.int32)
    off[5, 9] = 10
    frac = rng.uniform(0.0, 0.999, (64, 64)).astype(np.float32)
    frames = util.hash_frames(64, 1024, seed=10, batch=2) + DC
    c12, c11 = coeffs(12, seed=9), coeffs(11, seed=9)

    def make():
        eng = pkg.Engine(n_pixels=64, n_streams=64, max_batch=2, grid_columns=8)
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        return eng

    with make() as eng, make() as plain:
        before = eng.process(frames)
        assert status_of(pkg, lambda: eng.set_band(c12)) == Bn.ERR_RANGE  # the table came first
        assert np.array_equal(bits(eng.process(frames)), bits(before))    # ... and the handle has no band
        eng.set_band(c11)
        assert np.array_equal(bits(eng.process(frames)), bits(plain.process(Bn.band_filter(frames, c11))))
        assert np.array_equal(bits(eng.process(frames[0])), bits(plain.process(Bn.band_filter(frames, c11)[0])))
        assert np.array_equal(bits(device_process(eng, frames)), bits(device_process(plain, Bn.band_filter(frames, c11))))
    with pkg.Engine(n_pixels=64, n_streams=64, max_batch=2, grid_columns=8) as eng, make() as plain:
        eng.set_band(c12)  # the band comes first: nothing to hold it against
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        for call in (lambda: eng.process(frames), lambda: eng.process(frames[0]), lambda: device_process(eng, frames),
                     lambda: eng.process_samples(np.zeros((64, 512), np.float32))):
            assert status_of(pkg, call) == Bn.ERR_RANGE
        with pytest.raises(pkg.AwpuError):
            eng.ring_snapshot()  # nothing was enqueued: not even the ring exists
        eng.set_band(c11)
        assert np.array_equal(bits(eng.process(frames)), bits(plain.process(Bn.band_filter(frames, c11))))


# ------------------------------------------------------------------------------------------------ 8. physics

def test_the_band_picks_the_weak_high_source(pkg, c1):
    """Two plane waves on c1 in noise of 1e-3: 3 kHz of amplitude 0.2 from (20, 35) degrees and 8 kHz of amplitude 0.01 from (35, 200)
    degrees.  Without a band the strongest source is the 3 kHz one's pixel; with band_design(6375, 9000, 63) the 8 kHz one's."""
    S = pkg.synthetic
    low, high = (np.deg2rad(20.0), np.deg2rad(35.0)), (np.deg2rad(35.0), np.deg2rad(200.0))
    t = np.arange(1024, dtype=np.float64)
    frame = S.NOISE * np.random.default_rng(12).uniform(-1.0, 1.0, (64, 1024))
    for (theta, phi), hz, amp in ((low, 3e3, 0.2), (high, 8e3, 0.01)):
        tau = pkg.steering_delays(c1.xyz, theta, phi).astype(np.float64)
        frame += amp * np.sin(2.0 * np.pi * hz * (t[None, :] + tau[:, None]) / S.SAMPLE_RATE)  # the phase model of synthetic.make_frames
    frame = frame.astype(np.float32)
    pixel = lambda d: S.source_pixel(c1.spec, *d)[0] * 32 + S.source_pixel(c1.spec, *d)[1]
    assert pixel(low) != pixel(high)
    with c1.engine(1) as eng:
        wide = eng.process(frame)
        eng.set_band(pkg.binding.band_design(6375, 9000, 63))
        narrow = eng.process(frame)
    find = dict(radius=2, max_sources=4)
    wide_src, narrow_src = pkg.find_peaks(wide, 32, 32, **find), pkg.find_peaks(narrow, 32, 32, **find)
    print(f"low / high pixel power: {wide[pixel(low)] / wide[pixel(high)]:.3g} without the band, {narrow[pixel(low)] / narrow[pixel(high)]:.3g} with it; "
          f"strongest pixels {wide_src.pixel[0, 0]} (3 kHz at {pixel(low)}), {narrow_src.pixel[0, 0]} (8 kHz at {pixel(high)})")
    assert wide_src.pixel[0, 0] == pixel(low)
    assert narrow_src.pixel[0, 0] == pixel(high)
