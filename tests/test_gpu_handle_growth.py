"""One live handle through calls of growing, then shrinking, size: every buffer of the handle that grows on demand is replaced
while its earlier contents were in use, and every call must still give the bits of a handle created for that call alone.  (The
rest of the suite mostly gives every size its own handle, so a grow path that frees the wrong thing, or forgets a reset, passes
there.)  The reference is the fresh handle's answer, which the parity tests tie to the oracle."""
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import test_tracker_cpu as R

pytestmark = pytest.mark.gpu

LIMIT = math.pi / 2


def _wire(n_blocks=4):
    rng = np.random.default_rng(9)
    out = []
    for _ in range(n_blocks):
        msg = np.zeros(256, dtype=np.dtype([("frequency", "<u2"), ("n_arrays", "u1"), ("version", "u1"), ("counter", "<u4"), ("stream", "<i4", (256,))]))
        msg["n_arrays"] = 4
        msg["stream"] = rng.integers(-(1 << 21), 1 << 21, size=(256, 256), dtype=np.int32)
        out.append(msg.tobytes())
    return out


@pytest.mark.parametrize("math_mode", ["exact", "fast"])
@pytest.mark.parametrize("res", [16, 100])
def test_single_device_handle_grows_and_shrinks(pkg, res, math_mode):
    """64 mics, max_batch 8.  First a narrow delay table and one frame, then the real one: the window, and with it the pinned
    one-frame buffers and d_frames, grows.  calibrate_host grows d_frames again (whole rows).  Then process at batch
    1 -> 3 -> 8 -> 1 (d_frames and d_power twice over, the packed frames and the item list of the frame-pair shapes), the same
    through process_device, process_ring after four ingested blocks (the ring and its staging, allocated late), and runs of
    2, then 8 blocks (the runs' buffers)."""
    import torch

    S = pkg.synthetic
    spec = S.WorkloadSpec("one array", 1, 1, res)
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    frames = S.make_frames(xyz, 8, seed=77)
    d_X = torch.from_numpy(frames).cuda()
    wire = _wire()

    off_narrow = np.clip(off, off.min(), off.min() + 8).astype(off.dtype)

    def engine(o=off):
        eng = pkg.Engine(n_pixels=spec.n_pixels, n_streams=spec.n_mics, max_batch=8, grid_columns=res,
                         math=pkg.MATH_F32_FAST if math_mode == "fast" else pkg.MATH_F32_EXACT)
        eng.set_delay_table(o, frac)
        eng.set_active_mics(None)
        return eng

    def on_device(eng, batch):
        d_P = torch.zeros((batch, spec.n_pixels), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        eng.process_device(d_X.data_ptr(), batch, d_P.data_ptr())
        eng.synchronize()
        return d_P.cpu().numpy()

    def from_ring(eng):
        for block in wire:
            eng.ingest_block(block)
        return eng.process_ring()

    fresh = {}  # (entry, batch) -> what a handle that has served nothing else answers

    def want(entry, batch, call):
        if (entry, batch) not in fresh:
            with engine() as one:
                fresh[entry, batch] = call(one)
        return fresh[entry, batch]

    def blocks(eng, before, run):  # a run of blocks behind `before` blocks ingested one by one
        for block in before:
            eng.ingest_block(block)
        return eng.process_blocks(b"".join(run))

    with engine(off_narrow) as live:
        with engine(off_narrow) as one:
            assert np.array_equal(live.process(frames[:1]), one.process(frames[:1])), "narrow table"
        live.set_delay_table(off, frac)
        assert np.array_equal(live.process(frames[:1]), want("host", 1, lambda e: e.process(frames[:1]))), "wide table"
        with engine() as one:
            for got, ref in zip(live.calibrate_host(frames[1]), one.calibrate_host(frames[1])):
                assert np.array_equal(got, ref), "calibrate_host"
        for batch in (1, 3, 8, 1):
            assert np.array_equal(live.process(frames[:batch]), want("host", batch, lambda e: e.process(frames[:batch]))), ("host", batch)
        for batch in (1, 3, 8, 1):
            assert np.array_equal(on_device(live, batch), want("device", batch, lambda e: on_device(e, batch))), ("device", batch)
        assert np.array_equal(from_ring(live), want("ring", 1, from_ring))
        assert np.array_equal(live.process(frames[:3]), fresh["host", 3])  # (and the ring took nothing from the host path)
        more = _wire(10)
        with engine() as one:
            assert np.array_equal(blocks(live, [], more[:2]), blocks(one, wire, more[:2])), "run of 2 blocks"
        with engine() as one:
            assert np.array_equal(blocks(live, [], more[2:]), blocks(one, wire + more[:2], more[2:])), "run of 8 blocks"


def test_beams_and_tracker_grow_and_shrink(pkg):
    """beams with 1 -> 40 -> 3 directions (the entry table and the output buffer, whose layout follows its allocation), track
    with 1 -> 12 -> 2 particles (the particle buffer, with and without beams; the first call on 30 active mics, so that the
    tracker's mic list grows too), and listening to 2 blocks with one listener, then to 6 with five (the listeners' state and
    the runs' buffers) on one handle."""
    import torch

    xyz = pkg.create_antenna()
    frame = pkg.synthetic.make_frames(xyz, 1, seed=1234)[0]
    d_frame = torch.from_numpy(frame).cuda()
    rng = np.random.default_rng(5)
    theta, phi = rng.uniform(0.0, LIMIT - 0.3, 40), rng.uniform(0.0, 2 * math.pi, 40)
    off, frac = pkg.steer_table(xyz, theta, phi)
    reference = R.reference_power(frame)

    def engine(mics=None):
        eng = pkg.Engine(n_pixels=16, n_streams=xyz.shape[1])
        eng.set_antenna(xyz)
        eng.set_active_mics(mics)
        return eng

    def beams(eng, n):
        return eng.beams(off[:n], frac[:n], d_frame.data_ptr())

    def track(eng, n):
        got = eng.track(theta[:n], phi[:n], R.TRACKER_SPREAD, R.PARTICLE_RATE, 2, LIMIT, reference, d_frame.data_ptr(), want_beams=n != 12)
        return got.particles.tobytes(), got.reference, got.beams

    with engine() as live:
        for n in (1, 40, 3):
            with engine() as one:
                want = beams(one, n)
            got = beams(live, n)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), n
        for n in (1, 12, 2):
            mics = np.arange(30, dtype=np.int32) if n == 1 else None
            live.set_active_mics(mics)
            with engine(mics) as one:
                want = track(one, n)
            got = track(live, n)
            assert got[0] == want[0] and got[1] == want[1], n
            assert (got[2] is None and want[2] is None) or np.array_equal(got[2], want[2]), n
        wire = _wire(12)
        done = 4  # a primer: on a zeroed ring the reference power is 0 and a tracker's direction becomes NaN
        for block in wire[:done]:
            live.ingest_block(block)
        for n_blocks, n in ((2, 1), (6, 5)):
            def listen(eng):
                return eng.listen_blocks(b"".join(wire[done:done + n_blocks]), theta[:n], phi[:n], R.TRACKER_SPREAD, R.PARTICLE_RATE / 10, 1, LIMIT)
            with engine() as one:
                for block in wire[:done]:
                    one.ingest_block(block)
                want = listen(one)
            got = listen(live)
            assert np.isfinite(want.audio).all() and np.isfinite(want.listeners["theta"]).all(), (n_blocks, n)  # (no comparison of NaNs)
            assert np.array_equal(got.audio, want.audio) and got.listeners.tobytes() == want.listeners.tobytes(), (n_blocks, n)
            assert got.trail.tobytes() == want.trail.tobytes(), (n_blocks, n)
            done += n_blocks


GROWTH_GROUP_CHILD = r"""
import importlib, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import util
pkg = importlib.import_module("beamforming-lk_amd")
B = pkg.binding
S = pkg.synthetic
spec = S.WORKLOADS["ref_default"]
xyz = S.geometry(spec)
off, frac = S.delay_table(spec, xyz)
off_narrow = np.clip(off, off.min(), off.min() + 8).astype(off.dtype)
frames = S.make_frames(xyz, 4, seed=41)
d_X = torch.from_numpy(frames).cuda()
def engine(devices, o=off):
    eng = pkg.Engine(n_pixels=spec.n_pixels, n_streams=spec.n_mics, max_batch=4, grid_columns=spec.res, devices=devices)
    eng.set_delay_table(o, frac); eng.set_active_mics(None)
    return eng
def call(eng, batch, times):
    d_P = torch.zeros((times, batch, spec.n_pixels), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    for k in range(times):  # back to back: both buffers of every pair get reused; every call has its own output
        eng.process_device(d_X.data_ptr(), batch, d_P[k].data_ptr(), st.cuda_stream)
    st.synchronize(); eng.synchronize()
    return d_P.cpu().numpy(), eng.stats()
def same(got, want, exchange, what):  # every call of `got` against the fresh handle's one
    for k, power in enumerate(got):
        if exchange == B.EXCHANGE_PACKED_PAIRS:  # the same quads of the same packed samples through the same kernel
            assert np.array_equal(power, want[0]), (what, k)
        else:                                    # windows: a part may run another shape than the whole grid (rounding)
            assert util.power_rel_err(power, want[0]) < 5e-6, (what, k)
fresh = {}
for batch in (1, 4):
    with engine(None) as one:
        fresh[batch] = call(one, batch, 1)
with engine([0, 0]) as live:
    for batch in (1, 4, 1, 4):  # windows, packed pairs (the packed and receive buffers appear, the staging grows), and again
        power, stats = call(live, batch, 3)
        kind = B.EXCHANGE_WINDOWS if batch == 1 else B.EXCHANGE_PACKED_PAIRS
        assert stats.group_exchange == kind, (batch, stats.group_exchange)
        same(power, fresh[batch][0], kind, batch)
    live.set_delay_table(off_narrow, frac)  # a narrower table: the union window is taken anew
    power, stats = call(live, 4, 1)
    with engine(None, off_narrow) as one:
        want, want_stats = call(one, 4, 1)
    assert stats.window == want_stats.window and stats.window < fresh[4][1].window, (stats.window, want_stats.window)
    same(power, want, stats.group_exchange, "narrow table")
    live.set_delay_table(off, frac)  # and the wide one back: the packed rows are longer, every pair of buffers is replaced
    power, stats = call(live, 4, 3)
    assert stats.group_exchange == B.EXCHANGE_PACKED_PAIRS
    same(power, fresh[4][0], stats.group_exchange, "wide table back")
print("GROWTH GROUP OK")
"""


@pytest.mark.parametrize("force_copy", ["0", "1", "2"])
def test_device_group_handle_grows_and_shrinks(force_copy):
    """devices=[0, 0], 64 mics, 100 x 100, default math, max_batch 4: process_device three times back to back at batch
    1 -> 4 -> 1 -> 4 on one group handle (raw windows, then packed frame pairs, and back: the change of payload keeps the staging
    buffers), against a fresh single-device handle; then a narrower delay table.  force_copy as in test_device_group_equals_one_device:
    in place / the peer-copy path / through pinned host memory (read once per process, hence the child)."""
    env = dict(os.environ, AWPU_GROUP_FORCE_COPY=force_copy)
    out = subprocess.run([sys.executable, "-c", GROWTH_GROUP_CHILD, str(Path(__file__).resolve().parent.parent)],
                         env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "GROWTH GROUP OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
