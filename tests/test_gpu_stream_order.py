"""What include/awpu_hip.h promises about `stream` ("Streams", (a) to (d)), with work pending on the stream: the rest of the suite
settles the device around every device-form call, so a missing wait on the way into or out of one of the library's own streams
cannot fail there.

1. Every entry point that takes `stream`, between a producer and a consumer on that stream and no host synchronisation (the
   harness: stream_order.py), against the same call on a settled handle, bit for bit.
2. Two calls on ONE handle on two streams, back to back, the first still running when the second has been enqueued ((c): calls on
   a handle take effect in call order whatever their streams): both must give the settled handle's bits.  Without the order the
   second call's pack pass rewrites d_pack -- and zeroes the item queues of das_exact_nd_kernel -- under the first call's sweep;
   a banded first call loses d_band, a run of blocks d_blk_frames and the ring, a group the parts' d_power under the tile copies.
3. The device group, in a child process per AWPU_GROUP_FORCE_COPY (read once per process)."""
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import stream_order as H
import test_tracker_cpu as R

pytestmark = pytest.mark.gpu

LIMIT = math.pi / 2
N_BLOCKS = 5   # runs: pieces of 4 + 1 blocks at max_batch 4, so the i & 1 buffers are used again
BIG = (50, 43)  # the large image of a display step
DIST = [0.5, 2.0, math.inf]


@pytest.fixture(scope="module")
def busy():
    return H.Busy()


class Scene:
    """One 8x8 array on a res x res grid: tables, frames and samples of two seeds (the true data and the decoy)."""

    def __init__(self, pkg, res):
        S = pkg.synthetic
        self.pkg, self.res, self.P = pkg, res, res * res
        self.spec = S.WorkloadSpec("one array", 1, 1, res)
        self.xyz = S.geometry(self.spec)
        self.off, self.frac = S.delay_table(self.spec, self.xyz)
        self.frames = (S.make_frames(self.xyz, 4, seed=11), S.make_frames(self.xyz, 4, seed=12, theta=0.5, phi=2.0))
        n = 256 * N_BLOCKS
        self.samples = tuple(np.ascontiguousarray(S.make_frames(self.xyz, 1, seed=s, theta=t, hist=n)[0]) for s, t in ((21, 0.3), (22, 0.7)))

    def engine(self, math_mode="exact", band=None, antenna=False, table=True, max_batch=4, **kw):
        pkg = self.pkg

        def make():
            eng = pkg.Engine(n_pixels=self.P, n_streams=64, max_batch=max_batch, grid_columns=self.res,
                             math=pkg.MATH_F32_FAST if math_mode == "fast" else pkg.MATH_F32_EXACT, **kw)
            if antenna:
                eng.set_antenna(self.xyz)
            eng.set_active_mics(None)
            if table:
                eng.set_delay_table(self.off, self.frac)
            if band is not None:
                eng.set_band(band)
            return eng

        return make


@pytest.fixture(scope="module")
def scenes(pkg):
    made = {}

    def scene(res):
        if res not in made:
            made[res] = Scene(pkg, res)
        return made[res]

    return scene


def check(case, busy):
    want = H.reference(case)
    got = H.run(case, busy)
    H.assert_same(got, want)
    return got


def variant(eng):
    return eng.stats().kernel_variant


# ------------------------------------------------------------------------------------------------------------------- the sweep

@pytest.mark.parametrize("batch", [1, 4])
@pytest.mark.parametrize("math_mode", ["exact", "fast"])
@pytest.mark.parametrize("res", [16, 100])
def test_process_device(scenes, busy, res, math_mode, batch):
    sc = scenes(res)
    case = H.Case(sc.engine(math_mode), {"frames": tuple(f[:batch] for f in sc.frames)}, {"power": ((batch, sc.P), np.float32)},
                  lambda e, i, o, s: e.process_device(i["frames"], batch, o["power"], s), variant=variant)
    got = check(case, busy)
    assert np.isfinite(got["power"]).all() and (got["power"] > 0).any()


def test_process_device_sums(scenes, busy):
    sc = scenes(16)
    case = H.Case(sc.engine("exact"), {"frames": sc.frames}, {"power": ((4, sc.P), np.float32), "sums": ((4, sc.P, 256), np.float32)},
                  lambda e, i, o, s: e.process_device_sums(i["frames"], 4, o["power"], o["sums"], s), variant=variant)
    check(case, busy)


@pytest.mark.parametrize("math_mode", ["exact", "fast"])
def test_pack_frames_then_process_packed(scenes, busy, math_mode):
    """The two halves of the sweep back to back on the stream, nothing between them: the packed buffer is the caller's."""
    sc = scenes(100)
    with sc.engine(math_mode)() as e:
        n = e.packed_bytes(4)

    def call(e, i, o, s):
        e.pack_frames(i["frames"], 4, o["packed"], s)
        e.process_packed(o["packed"], 4, o["power"], s)

    case = H.Case(sc.engine(math_mode), {"frames": sc.frames}, {"packed": ((n // 4,), np.float32), "power": ((4, sc.P), np.float32)}, call,
                  variant=variant)
    check(case, busy)


@pytest.mark.parametrize("math_mode", ["exact", "fast"])
def test_process_bands_device(pkg, scenes, busy, math_mode):
    sc = scenes(16)
    bands = [pkg.band_design(1000.0, 4000.0, 31), pkg.band_design(6400.0, 9000.0, 31)]
    case = H.Case(sc.engine(math_mode), {"frames": sc.frames}, {"power": ((2, 4, sc.P), np.float32)},
                  lambda e, i, o, s: e.process_bands_device(i["frames"], 4, bands, o["power"], s), variant=variant)
    check(case, busy)


@pytest.mark.parametrize("math_mode", ["exact", "fast"])
def test_process_device_with_a_band(pkg, scenes, busy, math_mode):
    sc = scenes(16)
    case = H.Case(sc.engine(math_mode, band=pkg.band_design(6375.0, 9000.0, 63)), {"frames": sc.frames}, {"power": ((4, sc.P), np.float32)},
                  lambda e, i, o, s: e.process_device(i["frames"], 4, o["power"], s), variant=variant)
    check(case, busy)


# ------------------------------------------------------------------------------------------------------- display, find, calibrate

def powers(n, P, seed):
    return np.abs(np.random.default_rng(seed).standard_normal((n, P))).astype(np.float32) + np.float32(1e-3)


@pytest.mark.parametrize("peak_given", [False, True])
def test_heatmap_u8_device(scenes, busy, peak_given):
    sc = scenes(16)
    ins = {"power": (powers(4, sc.P, 1), powers(4, sc.P, 2))}
    outs = {"pix": ((4, sc.P), np.uint8)}
    if peak_given:
        ins["peak"] = (np.array([3.0, 2.5, 4.0, 1.0], np.float32), np.array([9.0, 8.0, 7.0, 6.0], np.float32))
    else:
        outs["peak"] = ((4,), np.float32)
    case = H.Case(sc.engine(), ins, outs,
                  lambda e, i, o, s: e.heatmap_device(i["power"], sc.P, 4, (i if peak_given else o)["peak"], o["pix"], peak_given, s))
    check(case, busy)


def test_upscale_u8_device(scenes, busy):
    sc = scenes(16)
    rng = np.random.default_rng(3)
    pix = tuple(rng.integers(0, 256, (4, 16, 16), dtype=np.uint8) for _ in range(2))
    case = H.Case(sc.engine(), {"pix": pix}, {"big": ((4,) + BIG, np.uint8)},
                  lambda e, i, o, s: e.upscale_device(i["pix"], 16, 16, 4, o["big"], BIG[0], BIG[1], stream=s))
    check(case, busy)


def test_find_peaks_device(scenes, busy):
    sc = scenes(16)
    case = H.Case(sc.engine(), {"power": (powers(4, sc.P, 4), powers(4, sc.P, 5))}, {"sources": ((4, 4, 40), np.uint8), "count": ((4,), np.int32)},
                  lambda e, i, o, s: e.find_peaks_device(i["power"], 4, 16, 16, o["sources"], o["count"], stream=s))
    got = check(case, busy)
    assert (got["count"] >= 1).all()


def test_expose_rows_device_with_a_carry(pkg, scenes, busy):
    """Windows of 3 blocks closing at blocks 0 and 3 of 5: the first began two blocks before the call (the carry is read), the
    next one has begun at block 4 (the carry is written)."""
    sc = scenes(16)
    n_frames, _, carry_in, carry_out, _ = pkg.binding.expose_count(N_BLOCKS, 0, 3, 3)
    assert n_frames == 2 and carry_in > 0 and carry_out > 0
    ins = {"power": (powers(N_BLOCKS, sc.P, 6), powers(N_BLOCKS, sc.P, 7)), "carry": (powers(1, sc.P, 8)[0], powers(1, sc.P, 9)[0])}
    case = H.Case(sc.engine(), ins, {"frames": ((n_frames, sc.P), np.float32)},
                  lambda e, i, o, s: e.expose_rows_device(i["power"], N_BLOCKS, sc.P, 0, 3, 3, o["frames"], d_carry_ptr=i["carry"], stream=s),
                  inout=("carry",))
    check(case, busy)


def test_calibrate_device(scenes, busy):
    """Synchronous (it returns the usable mics): the producer must still be running immediately before the call."""
    sc = scenes(16)
    true, decoy = sc.frames[0][0].copy(), sc.frames[1][0].copy()
    true[5] *= 40.0   # a mic far off the median, and a dead one: the decoy's answer is another list
    true[17] = 0.0
    case = H.Case(sc.engine(), {"frame": (true, decoy)}, {},
                  lambda e, i, o, s: e.calibrate_device(i["frame"], 0, 1e-5, s), synchronous=True)
    got = check(case, busy)
    assert 5 not in got["host"][0] and 17 not in got["host"][0]


# ------------------------------------------------------------------------------------------------------ runs of blocks, device form

def run_case(sc, engine, outs, call, **kw):
    n = 256 * N_BLOCKS
    return H.Case(engine, {"samples": sc.samples}, outs, lambda e, i, o, s: call(e, i["samples"], n, o, s), variant=variant, **kw)


@pytest.mark.parametrize("math_mode", ["exact", "fast"])
@pytest.mark.parametrize("res", [16, 100])
def test_process_samples_device(scenes, busy, res, math_mode):
    sc = scenes(res)
    case = run_case(sc, sc.engine(math_mode), {"power": ((N_BLOCKS, sc.P), np.float32)},
                    lambda e, x, n, o, s: e.process_samples_device(x, n, N_BLOCKS, o["power"], s))
    check(case, busy)


def test_watch_samples_device(scenes, busy):
    sc = scenes(16)
    outs = {"image": ((N_BLOCKS, sc.P), np.uint8), "big": ((N_BLOCKS,) + BIG, np.uint8), "power": ((N_BLOCKS, sc.P), np.float32)}
    case = run_case(sc, sc.engine(), outs,
                    lambda e, x, n, o, s: e.watch_samples_device(x, n, N_BLOCKS, 16, 16, d_image_ptr=o["image"], d_big_ptr=o["big"],
                                                                 d_power_ptr=o["power"], out_rows=BIG[0], out_cols=BIG[1], stream=s))
    check(case, busy)


def test_find_samples_device(scenes, busy):
    sc = scenes(16)
    outs = {"sources": ((N_BLOCKS, 4, 40), np.uint8), "count": ((N_BLOCKS,), np.int32), "power": ((N_BLOCKS, sc.P), np.float32)}
    case = run_case(sc, sc.engine(), outs,
                    lambda e, x, n, o, s: e.find_samples_device(x, n, N_BLOCKS, 16, 16, o["sources"], o["count"], d_power_ptr=o["power"], stream=s))
    got = check(case, busy)
    assert (got["count"] >= 1).all()


def test_locate_samples_device(scenes, busy):
    sc = scenes(16)
    outs = {"sources": ((N_BLOCKS, 4, 40), np.uint8), "count": ((N_BLOCKS,), np.int32), "ranges": ((N_BLOCKS, 4, 16), np.uint8),
            "range_power": ((N_BLOCKS, 4, len(DIST)), np.float32)}
    case = run_case(sc, sc.engine(antenna=True), outs,
                    lambda e, x, n, o, s: e.locate_samples_device(x, n, N_BLOCKS, 16, 16, DIST, o["sources"], o["count"], o["ranges"],
                                                                  d_range_power_ptr=o["range_power"], stream=s))
    check(case, busy)


def test_expose_samples_device_with_a_carry(pkg, scenes, busy):
    sc = scenes(16)
    n_frames, _, carry_in, carry_out, _ = pkg.binding.expose_count(N_BLOCKS, 0, 3, 3)
    assert n_frames == 2 and carry_in > 0 and carry_out > 0
    n = 256 * N_BLOCKS
    outs = {"image": ((n_frames, sc.P), np.uint8), "big": ((n_frames,) + BIG, np.uint8), "power": ((n_frames, sc.P), np.float32)}
    case = H.Case(sc.engine(), {"samples": sc.samples, "carry": (powers(1, sc.P, 8)[0], powers(1, sc.P, 9)[0])}, outs,
                  lambda e, i, o, s: e.expose_samples_device(i["samples"], n, N_BLOCKS, 16, 16, 3, 0, 3, d_carry_ptr=i["carry"], d_image_ptr=o["image"],
                                                             d_big_ptr=o["big"], d_power_ptr=o["power"], out_rows=BIG[0], out_cols=BIG[1], stream=s),
                  inout=("carry",), variant=variant)
    check(case, busy)


def test_spectral_samples_device(pkg, scenes, busy):
    sc = scenes(16)
    bands = [pkg.band_design(1000.0, 4000.0, 31), pkg.band_design(6400.0, 9000.0, 31)]
    outs = {"image": ((N_BLOCKS, sc.P, 3), np.uint8), "big": ((N_BLOCKS,) + BIG + (3,), np.uint8), "dominant": ((N_BLOCKS, sc.P), np.uint8),
            "power": ((2, N_BLOCKS, sc.P), np.float32)}
    case = run_case(sc, sc.engine(), outs,
                    lambda e, x, n, o, s: e.spectral_samples_device(x, n, N_BLOCKS, 16, 16, bands, d_image_ptr=o["image"], d_big_ptr=o["big"],
                                                                    d_dominant_ptr=o["dominant"], d_power_ptr=o["power"], out_rows=BIG[0],
                                                                    out_cols=BIG[1], stream=s))
    check(case, busy)


@pytest.mark.parametrize("heatmaps", [False, True])
def test_listen_samples_device(pkg, scenes, busy, heatmaps):
    """Three listeners (one steered, two tracking).  The call waits for its stream, because the listeners come back to the host:
    the producer must still be running immediately before it."""
    sc = scenes(16)
    n_l = 3
    rng = np.random.default_rng(29)
    theta, phi = rng.uniform(0.05, 1.2, n_l), rng.uniform(0.0, 2 * math.pi, n_l)
    spread = np.array([R.TRACKER_SPREAD, R.SEEKER_SPREAD, R.TRACKER_SPREAD])
    steps = np.array([0, 1, 2], np.int32)
    reference = R.reference_power(sc.frames[0][0])
    outs = {"audio": ((n_l, 256 * N_BLOCKS), np.float32), "trail": ((N_BLOCKS, n_l, 80), np.uint8)}
    if heatmaps:
        outs["power"] = ((N_BLOCKS, sc.P), np.float32)
    case = run_case(sc, sc.engine(antenna=True, table=heatmaps), outs,
                    lambda e, x, n, o, s: e.listen_samples_device(x, n, N_BLOCKS, theta, phi, spread, R.PARTICLE_RATE / 10, steps, LIMIT, o["audio"],
                                                                  256 * N_BLOCKS, reference, d_trail_ptr=o["trail"],
                                                                  d_power_ptr=o["power"] if heatmaps else 0, stream=s),
                    synchronous=True)
    got = check(case, busy)
    assert np.isfinite(got["audio"]).all() and np.isfinite(got["host"]["theta"]).all()


# ----------------------------------------------------------------------------------------------- call order across streams: (c)

class Pairs:
    """c2 (256 mics, 64 x 64), max_batch 32: frames A, and B = A reversed along the batch plus another seed; a recording for the
    runs.  Every answer a settled handle of its own gives is computed once per (math mode, call).  32 frames keep the first call of
    a pair running until the second has been enqueued; a group, whose fan-out is a dozen copies and event calls, needs 128."""

    def __init__(self, pkg, batch=32):
        S = pkg.synthetic
        self.pkg = pkg
        self.BATCH = batch
        self.spec = S.WORKLOADS["c2"]
        self.P = self.spec.n_pixels
        self.xyz = S.geometry(self.spec)
        self.off, self.frac = S.delay_table(self.spec, self.xyz)
        a = S.make_frames(self.xyz, self.BATCH, seed=51)
        self.frames = {"A": a, "B": np.ascontiguousarray(a[::-1] + S.make_frames(self.xyz, self.BATCH, seed=52, theta=0.6, phi=4.0))}
        n = 256 * self.BATCH
        self.samples = {k: np.ascontiguousarray(S.make_frames(self.xyz, 1, seed=s, theta=t, hist=n)[0]) for k, s, t in (("A", 61, 0.3), ("B", 62, 0.8))}
        self.bands = [pkg.band_design(1000.0, 4000.0, 31), pkg.band_design(6400.0, 9000.0, 31)]
        self.fresh = {}

    def engine(self, math_mode, devices=None):
        pkg = self.pkg
        eng = pkg.Engine(n_pixels=self.P, n_streams=self.spec.n_mics, max_batch=self.BATCH, grid_columns=self.spec.res, devices=devices,
                         math=pkg.MATH_F32_FAST if math_mode == "fast" else pkg.MATH_F32_EXACT)
        eng.set_active_mics(None)
        eng.set_delay_table(self.off, self.frac)
        return eng

    # the calls: (engine, device tensors of one data set, stream) -> the tensor the answer is in, or the host's answer
    def shape_of(self, kind):
        return (2, self.BATCH, self.P) if kind == "bands" else (self.BATCH, self.P)

    def enqueue(self, kind, eng, d, out, stream):
        B = self.BATCH
        if kind == "device":
            eng.process_device(d["frames"].data_ptr(), B, out.data_ptr(), stream)
        elif kind == "bands":
            eng.process_bands_device(d["frames"].data_ptr(), B, self.bands, out.data_ptr(), stream)
        elif kind == "packed":
            eng.process_packed(d["packed"].data_ptr(), B, out.data_ptr(), stream)
        elif kind == "samples":
            eng.process_samples_device(d["samples"].data_ptr(), 256 * B, B, out.data_ptr(), stream)
        else:
            raise AssertionError(kind)


@pytest.fixture(scope="module")
def pairs(pkg):
    return Pairs(pkg)


def device_data(pr, math_mode, which):
    """Frames, samples and (packed by a handle of its own, settled) the packed pairs of data set `which`, on the device."""
    import torch

    d = {"frames": torch.from_numpy(pr.frames[which]).cuda(), "samples": torch.from_numpy(pr.samples[which]).cuda()}
    with pr.engine(math_mode) as e:
        d["packed"] = torch.zeros(e.packed_bytes(pr.BATCH) // 4, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        e.pack_frames(d["frames"].data_ptr(), pr.BATCH, d["packed"].data_ptr())
        e.synchronize()
    torch.cuda.synchronize()
    return d


def settled(pr, math_mode, sequence, devices=None):
    """What a handle of its own answers to `sequence` = ((kind, data set), ...) with the device settled around every call (a run of
    blocks leaves its ring to the next one, so the sequence is the unit).  kind "host": process() of the frames."""
    import torch

    key = (math_mode, sequence, None if devices is None else tuple(devices))
    if key not in pr.fresh:
        answers = []
        with pr.engine(math_mode, devices) as eng:
            for kind, which in sequence:
                if kind == "host":
                    answers.append(eng.process(pr.frames[which]))
                    continue
                d = device_data(pr, math_mode, which)
                out = torch.zeros(pr.shape_of(kind), dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                pr.enqueue(kind, eng, d, out, 0)
                eng.synchronize()
                torch.cuda.synchronize()
                answers.append(out.cpu().numpy())
        pr.fresh[key] = answers
    return pr.fresh[key]


PAIRS = [("device", "device"), ("device", "host"), ("device", "packed"), ("device", "samples"), ("samples", "device"), ("bands", "device")]


def two_calls(pr, math_mode, first, second, devices=None, must_overlap=True):
    """`first` on data set A on stream S1, then at once `second` on data set B on stream S2 (or through the host form), on one
    handle that has served both calls twice before on the same streams (settled, other data: no buffer is grown between the two,
    and the runtime has set up what a stream's first copies through pinned memory cost -- a staged group's calls block the host
    for milliseconds until then).  The first call must still be running when the second has been enqueued.  must_overlap=False
    is for the one path where that is not in the library's hands (test_device_group): the answer is printed, the bits are checked."""
    import torch

    sequence = ((first, "B"), (second, "A")) * 2 + ((first, "A"), (second, "B"))  # (the warm-up, then the pair)
    want = settled(pr, math_mode, sequence, devices)[4:]
    dA, dB = device_data(pr, math_mode, "A"), device_data(pr, math_mode, "B")
    out1 = torch.full(pr.shape_of(first), -3.0, dtype=torch.float32, device="cuda")
    out2 = torch.full(pr.shape_of(second), -3.0, dtype=torch.float32, device="cuda") if second != "host" else None
    scratch = torch.zeros((2,) + pr.shape_of("bands"), dtype=torch.float32, device="cuda")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    behind_first = torch.cuda.Event()
    with pr.engine(math_mode, devices) as eng:
        torch.cuda.synchronize()
        for _ in range(2):
            pr.enqueue(first, eng, dB, scratch[0], s1.cuda_stream)
            torch.cuda.synchronize()
            if second == "host":
                eng.process(pr.frames["A"])
            else:
                pr.enqueue(second, eng, dA, scratch[1], s2.cuda_stream)
            torch.cuda.synchronize()  # (the last one: the last host synchronisation before the comparison's)
        pr.enqueue(first, eng, dA, out1, s1.cuda_stream)
        behind_first.record(s1)
        if second == "host":
            got2 = eng.process(pr.frames["B"])  # (synchronous: no precondition to assert behind it)
        else:
            pr.enqueue(second, eng, dB, out2, s2.cuda_stream)
            overlapped = not behind_first.query()
            print("the first call was still running when the second had been enqueued:", overlapped)
            assert overlapped or not must_overlap, "precondition: the first call was over when the second had been enqueued"
            s2.synchronize()
            got2 = out2.cpu().numpy()
        s1.synchronize()
        got1 = out1.cpu().numpy()
        print("variant:", eng.stats().kernel_variant)
    assert H.bits(got1) == H.bits(want[0]), f"the first call ({first}) lost its scratch to the second ({second})"
    assert H.bits(got2) == H.bits(want[1]), f"the second call ({second}) ran on the first one's ({first}) scratch"


@pytest.mark.parametrize("math_mode", ["exact", "fast"])
@pytest.mark.parametrize("first,second", PAIRS, ids=["-".join(p) for p in PAIRS])
def test_two_calls_on_two_streams(pairs, first, second, math_mode):
    two_calls(pairs, math_mode, first, second)


# ------------------------------------------------------------------------------------------------------------ the device group

GROUP_CHILD = r"""
import importlib, os, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import stream_order as H
import test_gpu_stream_order as T
pkg = importlib.import_module("beamforming-lk_amd")
B = pkg.binding
busy = H.Busy()
sc = T.Scene(pkg, 100)
for batch, kind in ((1, B.EXCHANGE_WINDOWS), (4, B.EXCHANGE_PACKED_PAIRS)):
    seen = []
    def call(e, i, o, s):
        for k in range(3):  # back to back: both buffers of every pair get used again
            e.process_device(i["frames"], batch, o["power%d" % k], s)
        seen.append(e.stats().group_exchange)
    case = H.Case(sc.engine("exact", devices=[0, 0]), {"frames": tuple(f[:batch] for f in sc.frames)},
                  {"power%d" % k: ((batch, sc.P), np.float32) for k in range(3)}, call)
    want = H.reference(case)
    got = H.run(case, busy)
    assert seen and all(x == kind for x in seen), (batch, seen)
    H.assert_same(got, want)
    assert H.bits(got["power0"]) == H.bits(got["power1"]) == H.bits(got["power2"])
pr = T.Pairs(pkg, batch=128)
T.two_calls(pr, "exact", "device", "device", devices=[0, 0], must_overlap=os.environ["AWPU_GROUP_FORCE_COPY"] != "2")
print("STREAM ORDER GROUP OK")
"""


@pytest.mark.parametrize("force_copy", ["0", "1", "2"])
def test_device_group(force_copy):
    """devices=[0, 0], 64 mics, 100 x 100: process_device three times back to back between the producer and the consumer, at batch 1
    (windows) and batch 4 (packed pairs); then the pair of calls on two streams on a group of c2, 128 frames.  force_copy: in place /
    the peer-copy path / through pinned host memory.  Through pinned memory the pair's precondition is printed, not asserted: there
    the HIP runtime itself blocks the host inside the second call's copies until the first call's are over, in most runs but not in
    all (measured: 7 to 15 ms inside the call against 0.1 ms), so the two calls cannot be made to overlap from here; their bits
    are checked all the same, and the producer / consumer half above holds its precondition on that path too."""
    env = dict(os.environ, AWPU_GROUP_FORCE_COPY=force_copy)
    out = subprocess.run([sys.executable, "-c", GROUP_CHILD, str(Path(__file__).resolve().parent.parent)],
                         env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "STREAM ORDER GROUP OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
