"""Runs of consecutive blocks (include/awpu_hip_blocks.h) on the device: one heatmap per block, bit-equal to the per-block live
loop (ingest_block + process_ring) in the exact mode and to awpu_hip_process of the same snapshots in every mode, with the
ingest ring left where the loop leaves it.  The host model of the snapshots is the rolling ring of
test_gpu_parity.test_wire_ingest_and_ring_sweep, built with the oracle's restated unpack."""
import ctypes as C

import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu


def make_datagrams(stream_block, counter0=0, n_arrays=1):
    """256 wire datagrams (src/fpga/receiver.h:24-30: u16 frequency, u8 n_arrays, u8 version, u32 counter,
    i32 stream[256], packed) from stream_block[256 samples][256 channels] int32."""
    msg = np.zeros(256, dtype=np.dtype([("frequency", "<u2"), ("n_arrays", "u1"), ("version", "u1"),
                                        ("counter", "<u4"), ("stream", "<i4", (256,))]))
    assert msg.dtype.itemsize == 1032
    msg["frequency"] = 48828
    msg["n_arrays"] = n_arrays
    msg["version"] = 2
    msg["counter"] = counter0 + np.arange(256)
    msg["stream"] = stream_block
    return msg.tobytes()


def recording(oracle, n_blocks, n_streams, seed):
    """(wire bytes of n_blocks blocks, unpacked samples [n_streams, 256 * n_blocks]) of random 24-bit samples (zero mean)."""
    rng = np.random.default_rng(seed)
    wire, blocks = [], []
    for b in range(n_blocks):
        stream = rng.integers(-(1 << 21), 1 << 21, size=(256, 256), dtype=np.int32)
        wire.append(make_datagrams(stream, counter0=256 * b))
        blocks.append(oracle.unpack_exposure(stream, n_streams))
    return b"".join(wire), np.concatenate(blocks, axis=1)


def snapshots(samples, ring=None):
    """The rolling ring after every block: [n_blocks, n_streams, 1024], starting from `ring` (zeros)."""
    n, total = samples.shape
    hist = np.concatenate([np.zeros((n, 1024), np.float32) if ring is None else ring, samples], axis=1)
    return np.stack([hist[:, 256 * (k + 1): 256 * (k + 1) + 1024] for k in range(total // 256)])


def chunked_process(eng, snaps, chunk):
    return np.concatenate([eng.process(snaps[k: k + chunk]) for k in range(0, len(snaps), chunk)])


def per_block_loop(eng, wire, n_blocks):
    out = []
    for b in range(n_blocks):
        eng.ingest_block(wire[256 * 1032 * b: 256 * 1032 * (b + 1)])
        out.append(eng.process_ring())
    return np.stack(out)


def engine(pkg, off, frac, n_streams, res, max_batch, math=None, interp=0, fir=None, index=None, gains=None):
    """`index`: the active mics (None = all, in id order); `gains`: per-mic gains (None = off)."""
    eng = pkg.Engine(n_pixels=res * res, n_streams=n_streams, max_batch=max_batch, grid_columns=res, math=math, interp=interp)
    eng.set_delay_table(off, frac)
    eng.set_active_mics(index)
    if gains is not None:
        eng.set_mic_gains(gains)
    if fir is not None:
        eng.set_fir_table(fir)
    return eng


@pytest.fixture(scope="module")
def ref_shape(oracle):
    xyz = oracle.create_antenna()
    off, frac = oracle.compute_delay_lut(xyz, 100, 100)
    wire, samples = recording(oracle, 38, 64, seed=5)
    return off, frac, wire, samples


@pytest.fixture(scope="module")
def headline(pkg, oracle):
    S = pkg.synthetic
    spec = S.WORKLOADS["headline"]
    off, frac = S.delay_table(spec, S.geometry(spec))
    wire, samples = recording(oracle, 130, spec.n_mics, seed=6)
    return off, frac, wire, samples, spec


def test_reference_shape_exact(pkg, oracle, ref_shape):
    """64 mics, 100 x 100, 16 frames per launch, 37 blocks (chunks 16 + 16 + 5): the per-block loop's bits, its ring, the
    batched process()'s bits, and the oracle."""
    off, frac, wire, samples = ref_shape
    n = 37
    snaps = snapshots(samples[:, : 256 * n])
    with engine(pkg, off, frac, 64, 100, 16) as eng, engine(pkg, off, frac, 64, 100, 16) as loop:
        got = eng.process_blocks(wire[: 256 * 1032 * n])
        st = eng.stats()
        assert st.frames == n and st.launches == 3
        want = per_block_loop(loop, wire, n)
        assert np.array_equal(got, want)
        assert np.array_equal(eng.ring_snapshot(), loop.ring_snapshot())
        assert np.array_equal(eng.ring_snapshot(), snaps[-1])
        assert np.array_equal(got, chunked_process(eng, snaps, 16))
        for k in (0, 17, 36):
            assert util.power_rel_err_unfloored(got[k], oracle.das_f32(snaps[k], off, frac)) <= util.POWER_RTOL, k


def test_calls_continue_each_other_and_the_live_loop(pkg, ref_shape):
    """13 + 24 blocks in two calls = one call of 37; then one live block = row 37 of a 38-block call."""
    off, frac, wire, _ = ref_shape
    B = 256 * 1032
    with engine(pkg, off, frac, 64, 100, 16) as one, engine(pkg, off, frac, 64, 100, 16) as two:
        whole = one.process_blocks(wire[: 38 * B])
        split = np.concatenate([two.process_blocks(wire[: 13 * B]), two.process_blocks(wire[13 * B: 37 * B])])
        assert np.array_equal(split, whole[:37])
        two.ingest_block(wire[37 * B: 38 * B])
        assert np.array_equal(two.process_ring(), whole[37])
        assert np.array_equal(two.ring_snapshot(), one.ring_snapshot())
        # and a live display step after a run continues it too
        p, _, _ = two.live_block(wire[:B], 100, 100)
        one.ingest_block(wire[:B])
        assert np.array_equal(p, one.process_ring())


def test_headline_exact(pkg, oracle, headline):
    """256 streams on the wire, 128 x 128, 128 frames per launch, 130 blocks (chunks 128 + 2)."""
    off, frac, wire, samples, spec = headline
    snaps = snapshots(samples)
    with engine(pkg, off, frac, spec.n_mics, spec.res, 128) as eng:
        got = eng.process_blocks(wire)
        assert np.array_equal(got, chunked_process(eng, snaps, 128))
        for k in (5, 129):
            assert util.power_rel_err_unfloored(got[k], oracle.das_f32(snaps[k], off, frac)) <= util.POWER_RTOL, k
    with engine(pkg, off, frac, spec.n_mics, spec.res, 128) as eng:
        got = eng.process_blocks(wire[: 128 * 256 * 1032])
        assert eng.stats().kernel_variant == 14  # AWPU_KERNEL_EXACT_ND: the batch sweep of awpu_hip_process
        assert np.array_equal(got, chunked_process(eng, snaps[:128], 128))


@pytest.mark.parametrize("shape", ["reference", "headline"])
def test_fast_mode(pkg, oracle, ref_shape, headline, shape):
    """FAST: process()'s bits on the same chunking; block call and per-block loop each within 1e-5 of the oracle (zero-mean input)."""
    if shape == "reference":
        off, frac, wire, samples = ref_shape
        n_streams, res, mb, n = 64, 100, 16, 37
    else:
        off, frac, wire, samples, spec = headline
        n_streams, res, mb, n = spec.n_mics, spec.res, 128, 130
    snaps = snapshots(samples[:, : 256 * n])
    fast = pkg.MATH_F32_FAST
    with engine(pkg, off, frac, n_streams, res, mb, math=fast) as eng, engine(pkg, off, frac, n_streams, res, mb, math=fast) as loop:
        got = eng.process_blocks(wire[: 256 * 1032 * n])
        assert np.array_equal(got, chunked_process(eng, snaps, mb))
        live = per_block_loop(loop, wire, n)
        for k in (0, n // 2, n - 1):
            want = oracle.das_f32(snaps[k], off, frac)
            assert util.power_rel_err_unfloored(got[k], want) <= util.POWER_RTOL, k
            assert util.power_rel_err_unfloored(live[k], want) <= util.POWER_RTOL, k


def test_samples_forms(pkg, oracle, ref_shape):
    """process_samples (host) and process_samples_device equal process_blocks; and with 512 streams, which the wire cannot carry."""
    import torch

    off, frac, wire, samples = ref_shape
    n = 21
    with engine(pkg, off, frac, 64, 100, 8) as a, engine(pkg, off, frac, 64, 100, 8) as b, engine(pkg, off, frac, 64, 100, 8) as c:
        want = a.process_blocks(wire[: 256 * 1032 * n])
        assert np.array_equal(b.process_samples(samples[:, : 256 * n]), want)
        wide = np.zeros((64, 256 * n + 100), np.float32)  # pitch above 256 * n_blocks
        wide[:, : 256 * n] = samples[:, : 256 * n]
        d_in = torch.from_numpy(wide).cuda()
        d_out = torch.empty((n, 100 * 100), dtype=torch.float32, device="cuda")
        c.process_samples_device(d_in.data_ptr(), wide.shape[1], n, d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(d_out.cpu().numpy(), want)
        assert np.array_equal(c.ring_snapshot(), a.ring_snapshot())
    xyz = oracle.create_tiled_antenna(4, 2)  # 512 mics: two FPGAs
    off2, frac2 = oracle.compute_delay_lut(xyz, 32, 32)
    rng = np.random.default_rng(9)
    big = (rng.integers(-(1 << 21), 1 << 21, size=(512, 256 * 11)) / 8388608.0).astype(np.float32)
    snaps = snapshots(big)
    with engine(pkg, off2, frac2, 512, 32, 4) as a, engine(pkg, off2, frac2, 512, 32, 4) as b:
        got = a.process_samples(big)
        assert np.array_equal(got, chunked_process(a, snaps, 4))
        d_in = torch.from_numpy(big).cuda()
        d_out = torch.empty((11, 32 * 32), dtype=torch.float32, device="cuda")
        b.process_samples_device(d_in.data_ptr(), big.shape[1], 11, d_out.data_ptr())
        b.synchronize()
        assert np.array_equal(d_out.cpu().numpy(), got)
        assert np.array_equal(b.ring_snapshot(), snaps[-1])
        assert util.power_rel_err_unfloored(got[10], oracle.das_f32(snaps[10], off2, frac2)) <= util.POWER_RTOL


def test_fir8_exact_equals_the_loop(pkg, ref_shape):
    off, frac, wire, _ = ref_shape
    n, fir = 21, util.synthetic_fir_table()
    kw = dict(interp=pkg.binding.INTERP_FIR8, fir=fir)
    with engine(pkg, off, frac, 64, 100, 8, **kw) as eng, engine(pkg, off, frac, 64, 100, 8, **kw) as loop:
        assert np.array_equal(eng.process_blocks(wire[: 256 * 1032 * n]), per_block_loop(loop, wire, n))


def test_refusals_leave_the_ring(pkg, ref_shape):
    off, frac, wire, samples = ref_shape
    B = 256 * 1032
    lib = pkg.binding.load()
    power = np.empty((4, 100 * 100), np.float32)
    # no table / no mic list: AWPU_ERR_STATE, the ring untouched
    with pkg.Engine(n_pixels=100 * 100, n_streams=64, max_batch=4) as eng:
        eng.ingest_block(wire[:B])
        before = eng.ring_snapshot()
        with pytest.raises(pkg.AwpuError) as ei:
            eng.process_blocks(wire[B: 3 * B])
        assert ei.value.status == pkg.binding.ERR_STATE
        eng.set_delay_table(off, frac)
        with pytest.raises(pkg.AwpuError) as ei:
            eng.process_samples(samples[:, :512])
        assert ei.value.status == pkg.binding.ERR_STATE
        assert np.array_equal(eng.ring_snapshot(), before)
        # a stride below one datagram, n_blocks 0, a short pitch: AWPU_ERR_INVALID
        buf = np.frombuffer(wire[: 2 * B], np.uint8)
        assert lib.awpu_hip_process_blocks(eng._h, buf.ctypes.data_as(C.c_void_p), 1031, 2, power.ctypes.data_as(C.POINTER(C.c_float))) \
            == pkg.binding.ERR_INVALID
        assert lib.awpu_hip_process_blocks(eng._h, buf.ctypes.data_as(C.c_void_p), 1032, 0, power.ctypes.data_as(C.POINTER(C.c_float))) \
            == pkg.binding.ERR_INVALID
        s = np.ascontiguousarray(samples[:, :512])
        assert lib.awpu_hip_process_samples(eng._h, s.ctypes.data_as(C.POINTER(C.c_float)), 512, 3,
                                            power.ctypes.data_as(C.POINTER(C.c_float))) == pkg.binding.ERR_INVALID
        assert np.array_equal(eng.ring_snapshot(), before)
    # hist != 1024: AWPU_ERR_INVALID
    with pkg.Engine(n_pixels=100 * 100, n_streams=64, hist=2048, max_batch=4) as eng:
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        with pytest.raises(pkg.AwpuError) as ei:
            eng.process_blocks(wire[: 2 * B])
        assert ei.value.status == pkg.binding.ERR_INVALID
    # a device group (one device listed twice): AWPU_ERR_STATE, its ring untouched
    with pkg.Engine(n_pixels=100 * 100, n_streams=64, max_batch=4, grid_columns=100, devices=[0, 0]) as eng:
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        eng.ingest_block(wire[:B])
        before = eng.ring_snapshot()
        with pytest.raises(pkg.AwpuError) as ei:
            eng.process_blocks(wire[B: 3 * B])
        assert ei.value.status == pkg.binding.ERR_STATE
        assert np.array_equal(eng.ring_snapshot(), before)


@pytest.mark.parametrize("where", ["handle_stream", "other_stream"])
def test_device_run_then_host_run_are_ordered(pkg, headline, where):
    """A long asynchronous device-form run, then at once a host-form run on the same handle: the host run continues the ring
    the device run leaves (its upload side waits for the handle's stream), whether the device run was enqueued on the handle's
    stream or on another one.  Both equal one call over the whole recording."""
    import torch

    off, frac, wire, samples, spec = headline
    n, first = 130, 122
    with engine(pkg, off, frac, spec.n_mics, spec.res, 128) as one, engine(pkg, off, frac, spec.n_mics, spec.res, 128) as two:
        want = one.process_samples(samples[:, : 256 * n])
        d_in = torch.from_numpy(np.ascontiguousarray(samples[:, : 256 * first])).cuda()
        d_out = torch.empty((first, spec.n_pixels), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        if where == "other_stream":
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                two.process_samples_device(d_in.data_ptr(), 256 * first, first, d_out.data_ptr(), side.cuda_stream)
        else:
            two.process_samples_device(d_in.data_ptr(), 256 * first, first, d_out.data_ptr())
        tail = two.process_blocks(wire[256 * 1032 * first: 256 * 1032 * n])  # enqueued while the device run is still going
        torch.cuda.synchronize()
        assert np.array_equal(tail, want[first:])
        assert np.array_equal(d_out.cpu().numpy(), want[:first])
        assert np.array_equal(two.ring_snapshot(), one.ring_snapshot())


def test_datagram_stride_and_one_frame_tail(pkg, ref_shape):
    """Datagrams 1040 bytes apart (a receive buffer with room per datagram) give the tight wire's heatmaps; a run whose last
    chunk is one frame (8 + 8 + 1) equals the per-block loop and process() with the same chunking."""
    off, frac, wire, samples = ref_shape
    n = 17
    tight = np.frombuffer(wire[: 256 * 1032 * n], np.uint8).reshape(256 * n, 1032)
    loose = np.full((256 * n, 1040), 0xA5, np.uint8)
    loose[:, :1032] = tight
    snaps = snapshots(samples[:, : 256 * n])
    with engine(pkg, off, frac, 64, 100, 8) as a, engine(pkg, off, frac, 64, 100, 8) as b, engine(pkg, off, frac, 64, 100, 8) as loop:
        got = a.process_blocks(tight.tobytes())
        assert np.array_equal(b.process_blocks(loose.tobytes(), stride=1040), got)
        assert np.array_equal(got, per_block_loop(loop, wire, n))
        assert np.array_equal(got, chunked_process(a, snaps, 8))
        assert np.array_equal(b.ring_snapshot(), snaps[-1])
