"""The coherence sweep (include/awpu_hip_cohere.h) on the device.

1. Export: out[] and e[] of every pixel equal the host rule (awpu_hip_cohere_host) bit for bit, and out[] equals
   awpu_hip_process_device_sums in the exact mode, on c1 (two LDS chunks), a ragged list, one mic, four arrays, a table of three
   pixels and a hand-made table whose entries sit at both ends of the history; batches of 1 and 3, gains on and off, every math
   mode's handle; guard floats around every output stay intact.
2. Maps against the host rule, relative, no floor, every pixel: power within 1e-5 (the project's bound), coherence within 2e-5 (two
   254-term positive sums, each within that bound), weighted within 3e-5.  Worst values measured on MI355X over every shape of
   item 1: power 1.12e-06, coherence 1.43e-06, weighted 2.34e-06.  One mic gives exactly 1.0f; a frame swept alone gives the bits it gives inside a batch; the host form
   (windows uploaded: the compact layout) gives the device form's bits (whole frames).
3. Value edges: finite frames scaled by 2^-40 and 2^55 give sums and energies bit for bit; a NaN and an inf stay in their frames.
4. The band in front: the band-less call on band_filter'ed input, bit for bit.
5. Runs: the three forms equal the composition -- Engine.cohere of the shown snapshots, then heatmap_u8, the upscale, find_peaks --
   with the watch run's ring and stats, split or whole; the physics of tests/test_cohere_cpu.py holds on the device rows; refusals
   leave the ring and the outputs alone.
6. Stream order: cohere_device and cohere_samples_device behind pending work on their stream (tests/stream_order.py)."""
from pathlib import Path

import numpy as np
import pytest

import cohere_util as CU
import stream_order as H
import util
import value_edges as V
from test_gpu_blocks import engine, snapshots
from test_gpu_find import FIND, assert_equal_to_host, c1 as find_c1  # noqa: F401  (c1's 23-block recording)
from test_gpu_stream_order import BIG, N_BLOCKS, busy, check, run_case, scenes, variant  # noqa: F401
from test_gpu_watch import colour_table, compose

pytestmark = pytest.mark.gpu

GOLDEN = str(Path(__file__).resolve().parent / "golden")
GUARD = 64  # floats in front of and behind every device output
CANARY = -3.0
NAMES = ("power", "coherence", "weighted", "sums", "energy")
BOUND = {"power": 1e-5, "coherence": 2e-5, "weighted": 3e-5}
worst = {name: 0.0 for name in BOUND}


class Shape:
    """A table, a mic list, frames [3, n_streams, 1024] and the host rule's answer on them (computed once, left unchanged)."""

    def __init__(self, pkg, name, off, frac, n_streams, index=None, grid_columns=0, seed=0):
        self.pkg, self.name, self.off, self.frac, self.n_streams, self.grid_columns = pkg, name, off, frac, n_streams, grid_columns
        self.index = None if index is None else np.asarray(index, np.int32)
        self.active = np.arange(n_streams, dtype=np.int32) if index is None else self.index
        self.P = off.shape[0]
        self.frames = util.hash_frames(n_streams, 1024, seed=7001 + seed, batch=3)
        self.gains = (0.5 + np.random.default_rng(50 + seed).random(n_streams)).astype(np.float32)
        self._rule = {}

    def rule(self, gains: bool):
        if gains not in self._rule:
            got = self.pkg.cohere_host(self.frames, self.off, self.frac, index=self.active, gain=self.gains[self.active] if gains else None,
                                       want_sums=True)
            for a in got:
                a.setflags(write=False)
            self._rule[gains] = dict(zip(NAMES, got))
        return self._rule[gains]

    def engine(self, max_batch=3, math=None, gains=False, band=None):
        eng = self.pkg.Engine(n_pixels=self.P, n_streams=self.n_streams, max_batch=max_batch, grid_columns=self.grid_columns, math=math)
        eng.set_delay_table(self.off, self.frac)
        eng.set_active_mics(self.index)
        if gains:
            eng.set_mic_gains(self.gains)
        if band is not None:
            eng.set_band(band)
        return eng


@pytest.fixture(scope="module")
def shapes(pkg):
    S = pkg.synthetic
    c1 = S.WORKLOADS["c1"]
    xyz = S.geometry(c1)
    off, frac = S.delay_table(c1, xyz)
    four = S.WorkloadSpec("four arrays, 16 x 16", 4, 1, 16)
    off4, frac4 = S.delay_table(four)
    # entries at both ends of the history: window = 1024, 16 mics to an LDS chunk; the first row of every chunk (mics 0, 16, 32, 48)
    # has off_rel = 0 for some pixels and reads the window's last sample (off + 256 = 1023) for others; 9 pixels: a last workgroup
    # with one wave at work, its last three pixels off the grid
    rng = np.random.default_rng(9)
    off_e = rng.integers(0, 768, size=(9, 64)).astype(np.int32)
    off_e[:, ::16] = np.where(np.arange(9)[:, None] % 2 == 0, 0, 767)
    off_e[:, 15::16] = np.where(np.arange(9)[:, None] % 2 == 0, 767, 0)
    off_e[4] = 767
    off_e[5] = 0
    frac_e = rng.random((9, 64)).astype(np.float32)
    frac_e[:, ::7] = 0.0
    frac_e[:, 3::7] = 1.0
    made = [Shape(pkg, "c1", off, frac, 64, grid_columns=32, seed=1),
            Shape(pkg, "ragged51", off, frac, 64, index=np.load(GOLDEN + "/sweep_c1_ragged.npz")["index"], grid_columns=32, seed=2),
            Shape(pkg, "onemic", off, frac, 64, index=[37], grid_columns=32, seed=3),
            Shape(pkg, "four_arrays", off4, frac4, 256, grid_columns=16, seed=4),
            Shape(pkg, "three_pixels", off[[0, 517, 1023]], frac[[0, 517, 1023]], 64, seed=5),
            Shape(pkg, "edges", off_e, frac_e, 64, seed=6)]
    return {s.name: s for s in made}


def device_sweep(eng, frames, want=NAMES, stream=0):
    """cohere_device_sums of host frames -> {name: array}; every output sits between guard floats, which must survive."""
    import torch

    frames = np.ascontiguousarray(frames, np.float32)
    batch, P = len(frames), eng.pixel_count
    d_x = torch.from_numpy(np.array(frames)).cuda()
    size = {name: batch * P * (256 if name in ("sums", "energy") else 1) for name in want}
    raw = {name: torch.full((n + 2 * GUARD,), CANARY, dtype=torch.float32, device="cuda") for name, n in size.items()}
    ptr = {f"d_{name}_ptr": raw[name].data_ptr() + 4 * GUARD for name in want}
    torch.cuda.synchronize()
    eng.cohere_device_sums(d_x.data_ptr(), batch, stream=stream, **ptr)
    eng.synchronize()
    out = {}
    for name in want:
        host = raw[name].cpu().numpy()
        assert (host[:GUARD] == CANARY).all() and (host[-GUARD:] == CANARY).all(), f"{name}: guard overwritten"
        out[name] = host[GUARD:-GUARD].reshape((batch, P, 256) if name in ("sums", "energy") else (batch, P))
    return out


def exact_sums(eng, frames):
    import torch

    d_x = torch.from_numpy(np.array(frames, np.float32)).cuda()
    d_p = torch.zeros((len(frames), eng.pixel_count), dtype=torch.float32, device="cuda")
    d_s = torch.zeros((len(frames), eng.pixel_count, 256), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.process_device_sums(d_x.data_ptr(), len(frames), d_p.data_ptr(), d_s.data_ptr())
    eng.synchronize()
    return d_s.cpu().numpy()


def check_maps(got, want, where):
    for name, bound in BOUND.items():
        err = CU.rel_err(got[name], want[name])
        worst[name] = max(worst[name], err)
        print(f"{where}: {name} max rel err {err:.3g} (worst so far {worst[name]:.3g})")
        assert err <= bound, (where, name, err)


# ------------------------------------------------------------------------------------------------ 1, 2. export and maps

@pytest.mark.parametrize("gains", [False, True], ids=["plain", "gains"])
@pytest.mark.parametrize("name", ["c1", "ragged51", "onemic", "four_arrays", "three_pixels", "edges"])
def test_export_and_maps_equal_the_host_rule(pkg, shapes, name, gains):
    sh = shapes[name]
    want = sh.rule(gains)
    with sh.engine(gains=gains) as eng:
        for batch in (1, 3):
            got = device_sweep(eng, sh.frames[:batch])
            assert eng.stats().kernel_variant == pkg.binding.KERNEL_NAMES.index("cohere")
            assert CU.same_bits(got["sums"], want["sums"][:batch]), (name, batch, "sums")
            assert CU.same_bits(got["energy"], want["energy"][:batch]), (name, batch, "energy")
            assert not got["energy"][:, :, 0].any() and not got["energy"][:, :, 255].any()
            check_maps(got, {k: v[:batch] for k, v in want.items()}, (name, gains, batch))
            assert (got["coherence"] >= 0).all() and (got["coherence"] <= 1).all()
            assert CU.same_bits(got["weighted"], got["power"] * got["coherence"])
        whole = got
        # each output alone, and the maps through cohere_device, give the same bits
        for alone in NAMES:
            assert CU.same_bits(device_sweep(eng, sh.frames, want=(alone,))[alone], whole[alone]), alone
        # a frame swept alone gives the bits it gives inside a batch
        for b in range(3):
            one = device_sweep(eng, sh.frames[b: b + 1], want=("power", "coherence", "weighted"))
            for k, v in one.items():
                assert CU.same_bits(v[0], whole[k][b]), (k, b)
        # the host form uploads the windows alone where they can be cut out (the compact layout): the same bits
        maps = eng.cohere(sh.frames)
        for k in ("power", "coherence", "weighted"):
            assert CU.same_bits(maps[k], whole[k]), k
        assert CU.same_bits(eng.cohere(sh.frames[1], want=("coherence",))["coherence"], whole["coherence"][1])
        # the exact mode's own export: the same out[], on every shape
        assert CU.same_bits(exact_sums(eng, sh.frames), whole["sums"])
    if name == "onemic":
        assert CU.same_bits(whole["coherence"], np.ones_like(whole["coherence"]))
        assert CU.same_bits(whole["weighted"], whole["power"])


@pytest.mark.parametrize("name", ["c1", "edges"])
def test_every_math_mode_sweeps_the_same_rule(pkg, shapes, name):
    """The rule does not depend on cfg.math: AWPU_MATH_F32_FAST (whose handle has no LutEntry table of its own) and
    AWPU_MATH_BF16_ACC give the exact handle's bits."""
    sh = shapes[name]
    want = sh.rule(True)
    for math in (pkg.MATH_F32_FAST, pkg.MATH_BF16_ACC):
        with sh.engine(math=math, gains=True) as eng:
            got = device_sweep(eng, sh.frames)
            assert CU.same_bits(got["sums"], want["sums"]) and CU.same_bits(got["energy"], want["energy"])
            check_maps(got, want, (name, math))
            eng.set_active_mics(sh.active[::2])  # the tables are rebuilt: the sweep's own table with them
            half = device_sweep(eng, sh.frames[:1], want=("sums",))["sums"]
            ref = pkg.cohere_host(sh.frames[:1], sh.off, sh.frac, index=sh.active[::2], gain=sh.gains[sh.active[::2]], want_sums=True)[3]
            assert CU.same_bits(half, ref)


def test_a_slab_handle_sweeps_its_own_pixels(pkg, shapes):
    sh = shapes["c1"]
    want = sh.rule(False)
    with pkg.Engine(n_pixels=1024, n_streams=64, max_batch=3, pixel_begin=320, pixel_count=200) as eng:
        eng.set_delay_table(sh.off[320:520], sh.frac[320:520])
        eng.set_active_mics(None)
        got = device_sweep(eng, sh.frames)
        assert CU.same_bits(got["sums"], want["sums"][:, 320:520]) and CU.same_bits(got["energy"], want["energy"][:, 320:520])
        check_maps(got, {k: v[:, 320:520] for k, v in want.items()}, "slab")
        assert CU.same_bits(eng.cohere(sh.frames)["weighted"], got["weighted"])


def test_handle_forms_refuse(pkg, shapes):
    """FIR8 and a device group: AWPU_ERR_STATE; no table, no mics: AWPU_ERR_STATE; no frames, no output, a batch over max_batch:
    AWPU_ERR_INVALID; the outputs are left alone."""
    import torch

    sh = shapes["c1"]
    B = pkg.binding
    d_x = torch.from_numpy(sh.frames).cuda()
    d_o = torch.full((3 * 1024,), CANARY, dtype=torch.float32, device="cuda")
    host = np.full((3, 1024), CANARY, np.float32)

    def refused(eng, status, batch=1, frames=True, out=True):
        calls = (lambda: eng.cohere_device(d_x.data_ptr() if frames else 0, batch, d_o.data_ptr() if out else 0),
                 lambda: eng.cohere_device_sums(d_x.data_ptr() if frames else 0, batch, d_sums_ptr=0, d_weighted_ptr=d_o.data_ptr() if out else 0),
                 lambda: eng._lib.awpu_hip_cohere(eng._h, B._f32(sh.frames) if frames else None, batch, B._f32(host) if out else None, None, None))
        for call in calls:
            try:
                rc = call()
            except pkg.AwpuError as e:
                rc = e.status
            assert rc == status, (rc, status)

    with pkg.Engine(n_pixels=1024, n_streams=64, max_batch=2, interp=1) as eng:
        eng.set_delay_table(sh.off, sh.frac)
        eng.set_active_mics(None)
        eng.set_fir_table(util.synthetic_fir_table())
        refused(eng, B.ERR_STATE)
    with pkg.Engine(n_pixels=1024, n_streams=64, max_batch=2, grid_columns=32, devices=[0, 0]) as eng:
        eng.set_delay_table(sh.off, sh.frac)
        eng.set_active_mics(None)
        refused(eng, B.ERR_STATE)
    with pkg.Engine(n_pixels=1024, n_streams=64, max_batch=2) as eng:
        refused(eng, B.ERR_STATE)
        eng.set_delay_table(sh.off, sh.frac)
        refused(eng, B.ERR_STATE)
        eng.set_active_mics(None)
        refused(eng, B.ERR_INVALID, batch=3)
        refused(eng, B.ERR_INVALID, batch=0)
        refused(eng, B.ERR_INVALID, frames=False)
        refused(eng, B.ERR_INVALID, out=False)
        assert eng.stats().frames == 0
        assert CU.rel_err(eng.cohere(sh.frames[:2])["power"], sh.rule(False)["power"][:2]) <= BOUND["power"]  # the handle still works
    torch.cuda.synchronize()
    assert (d_o.cpu().numpy() == CANARY).all() and (host == CANARY).all()


# ------------------------------------------------------------------------------------------------ 3. value edges

@pytest.mark.parametrize("k", [-40, 55])
def test_scaled_frames_give_the_rules_bits(pkg, shapes, k):
    sh = shapes["ragged51"]
    frames = V.scale_pow2(sh.frames[:2], k)
    want = dict(zip(NAMES, pkg.cohere_host(frames, sh.off, sh.frac, index=sh.active, want_sums=True)))
    assert np.isfinite(want["energy"]).all() and want["energy"].any()
    with sh.engine() as eng:
        got = device_sweep(eng, frames)
    assert CU.same_bits(got["sums"], want["sums"]) and CU.same_bits(got["energy"], want["energy"])
    # the scaling is exact: the sums are 2^k and the energies 2^2k times the unscaled ones, and the coherence does not move
    assert CU.same_bits(got["sums"], V.scale_pow2(sh.rule(False)["sums"][:2], k))
    check_maps(got, want, ("scaled", k))
    assert CU.rel_err(got["coherence"], sh.rule(False)["coherence"][:2]) <= 2 * BOUND["coherence"]


def test_a_nan_and_an_inf_stay_in_their_frames(pkg, shapes):
    sh = shapes["c1"]
    clean = np.concatenate([sh.frames, sh.frames[:1] * np.float32(0.5)])
    at = int(np.median(sh.off[:, 9])) + 256  # the last sample that half of the pixels read of mic 9
    bad = clean.copy()
    bad[1, 9, at] = np.nan
    bad[2, 9, at] = np.inf
    want = dict(zip(NAMES, pkg.cohere_host(bad, sh.off, sh.frac, want_sums=True)))
    with sh.engine(max_batch=4) as eng:
        ok = device_sweep(eng, clean)
        got = device_sweep(eng, bad)
    for name in NAMES:
        for b in (0, 3):
            assert CU.same_bits(got[name][b], ok[name][b]), (name, b)
    for name in ("sums", "energy"):
        assert V.same_nonfinite(got[name], want[name]), name
    reached = ~np.isfinite(want["sums"][1]).all(axis=1)
    assert reached.any() and not reached.all()
    for b in (1, 2):
        for name in ("power", "coherence", "weighted"):
            g, w = got[name][b], want[name][b]
            assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(np.isinf(g), np.isinf(w)), (name, b)
            assert np.array_equal(g == 0, w == 0), (name, b)
            fin = np.isfinite(w)
            assert CU.rel_err(g[fin], w[fin]) <= BOUND[name], (name, b)
        assert not got["coherence"][b][reached].any()  # den is NaN there: the rule says 0
        assert np.isnan(got["power"][b][reached]).all()


# ------------------------------------------------------------------------------------------------ 4. the band

def test_the_band_in_front_is_the_sweep_of_filtered_frames(pkg, shapes):
    sh = shapes["ragged51"]
    assert int(sh.off.min()) >= 62
    c = pkg.binding.band_design(6375, 9000, 63)
    filtered = pkg.binding.band_filter(sh.frames, c)
    with sh.engine(gains=True) as plain, sh.engine(gains=True, band=c) as banded:
        want = device_sweep(plain, filtered)
        got = device_sweep(banded, sh.frames)
        for name in NAMES:
            assert CU.same_bits(got[name], want[name]), name
        assert not CU.same_bits(got["sums"], device_sweep(plain, sh.frames, want=("sums",))["sums"])
        host_got, host_want = banded.cohere(sh.frames), plain.cohere(filtered)
        for name in ("power", "coherence", "weighted"):
            assert CU.same_bits(host_got[name], host_want[name]) and CU.same_bits(host_got[name], want[name]), name


# ------------------------------------------------------------------------------------------------ 5. the runs

def composition(pkg, off, frac, samples, first, every, show, ring=None):
    """Rows of the shown snapshots by Engine.cohere on a handle of its own."""
    snaps = snapshots(samples, ring)[first::every]
    with engine(pkg, off, frac, 64, 32, 32) as eng:
        return eng.cohere(snaps, want=("coherence" if show else "weighted",))["coherence" if show else "weighted"]


@pytest.mark.parametrize("max_batch", [1, 4, 32])
@pytest.mark.parametrize("first,every", [(0, 1), (2, 3), (5, 7)])
def test_run_forms_equal_the_composition(pkg, oracle, find_c1, max_batch, first, every):  # noqa: F811
    import torch

    off, frac, _, wire, samples = find_c1
    n_frames = len(range(first, 23, every))
    table, d_table = colour_table()
    with engine(pkg, off, frac, 64, 32, max_batch) as ref:
        watched = ref.watch_samples(samples, 32, 32, first=first, every=every, want_image=False, want_power=True)
        ring, frames_swept, launches = ref.ring_snapshot(), ref.stats().frames, ref.stats().launches
    d_in = torch.from_numpy(np.ascontiguousarray(samples)).cuda()
    for show in (pkg.binding.COHERE_WEIGHTED, pkg.binding.COHERE_FACTOR):
        rows = composition(pkg, off, frac, samples, first, every, show)
        assert rows.shape == (n_frames, 1024) and not CU.same_bits(rows, watched.power)
        image, big = compose(pkg, oracle, rows, 32, 32, 50, 43, table, True)
        want = pkg.find_peaks(rows, 32, 32, **FIND)

        def check_run(got, eng):
            assert got.next_first == watched.next_first and len(got) == n_frames
            assert CU.same_bits(got.power, rows)
            assert np.array_equal(got.image, image) and np.array_equal(got.big, big)
            assert_equal_to_host(got.sources, got.count, want, (max_batch, first, every, show))
            assert np.array_equal(eng.ring_snapshot(), ring)
            assert (eng.stats().frames, eng.stats().launches) == (frames_swept, launches)

        kw = dict(first=first, every=every, show=show, out_rows=50, out_cols=43, d_colormap_ptr=d_table.data_ptr(), flip=True, want_power=True,
                  find=FIND)
        with engine(pkg, off, frac, 64, 32, max_batch) as eng:
            check_run(eng.cohere_blocks(wire, 32, 32, **kw), eng)
        with engine(pkg, off, frac, 64, 32, max_batch) as eng:
            check_run(eng.cohere_samples(samples, 32, 32, **kw), eng)
        with engine(pkg, off, frac, 64, 32, max_batch) as eng:  # the sources alone
            alone = eng.cohere_samples(samples, 32, 32, first=first, every=every, show=show, want_image=False, find=FIND)
            assert alone.power is None and alone.image is None and alone.big is None
            assert_equal_to_host(alone.sources, alone.count, want, "alone")
        with engine(pkg, off, frac, 64, 32, max_batch) as eng:  # the device form, every output between guards
            outs = {"image": (n_frames * 1024, torch.uint8), "big": (n_frames * 50 * 43 * 3, torch.uint8), "power": (n_frames * 1024, torch.float32),
                    "sources": (n_frames * 4 * 40, torch.uint8), "count": (n_frames, torch.int32)}
            fill = {torch.uint8: 0xA5, torch.float32: CANARY, torch.int32: -7}
            raw = {k: torch.full((n + 128,), fill[t], dtype=t, device="cuda") for k, (n, t) in outs.items()}
            ptr = {k: v.data_ptr() + 64 * v.element_size() for k, v in raw.items()}
            torch.cuda.synchronize()
            nxt = eng.cohere_samples_device(d_in.data_ptr(), samples.shape[1], 23, 32, 32, first=first, every=every, show=show,
                                            d_image_ptr=ptr["image"], d_big_ptr=ptr["big"], d_power_ptr=ptr["power"], d_sources_ptr=ptr["sources"],
                                            d_count_ptr=ptr["count"], out_rows=50, out_cols=43, d_colormap_ptr=d_table.data_ptr(), flip=True, find=FIND)
            eng.synchronize()
            assert nxt == watched.next_first
            host = {k: v.cpu().numpy() for k, v in raw.items()}
            for k, v in host.items():
                assert (v[:64] == fill[outs[k][1]]).all() and (v[-64:] == fill[outs[k][1]]).all(), k
            assert CU.same_bits(host["power"][64:-64].reshape(n_frames, 1024), rows)
            assert np.array_equal(host["image"][64:-64].reshape(n_frames, 32, 32), image)
            assert np.array_equal(host["big"][64:-64].reshape(big.shape), big)
            assert_equal_to_host(host["sources"][64:-64].view(pkg.binding.SOURCE_DTYPE).reshape(n_frames, 4), host["count"][64:-64], want, "device")
            assert np.array_equal(eng.ring_snapshot(), ring)


def test_a_split_recording_equals_one_call(pkg, find_c1):  # noqa: F811
    off, frac, _, wire, samples = find_c1
    BYTES = 256 * 1032
    kw = dict(every=3, want_image=True, want_power=True, find=FIND)
    with engine(pkg, off, frac, 64, 32, 4) as eng:
        whole = eng.cohere_samples(samples, 32, 32, first=2, **kw)
        ring = eng.ring_snapshot()
    with engine(pkg, off, frac, 64, 32, 4) as eng:
        a = eng.cohere_samples(samples[:, : 256 * 10], 32, 32, first=2, **kw)
        b = eng.cohere_blocks(wire[10 * BYTES: 11 * BYTES], 32, 32, first=a.next_first, **kw)  # a call that may show nothing
        c = eng.cohere_blocks(wire[11 * BYTES:], 32, 32, first=b.next_first, **kw)
        assert c.next_first == whole.next_first and len(a) + len(b) + len(c) == len(whole)
        for name in ("power", "image", "count"):
            joined = np.concatenate([getattr(r, name) for r in (a, b, c)])
            assert joined.tobytes() == getattr(whole, name).tobytes(), name
        assert np.concatenate([r.sources for r in (a, b, c)]).tobytes() == whole.sources.tobytes()
        assert np.array_equal(eng.ring_snapshot(), ring)
        # mixing with the other run calls: a watch run continues from the same ring
        rows = composition(pkg, off, frac, samples[:, : 256 * 4], 0, 1, 0, ring=ring)
        again = eng.cohere_samples(samples[:, : 256 * 4], 32, 32, want_image=False, want_power=True)
        assert CU.same_bits(again.power, rows)


def test_the_physics_holds_on_the_device_rows(pkg):
    """The figures of tests/test_cohere_cpu.py, on the rows the device gives for c1's synthetic frame."""
    S = pkg.synthetic
    spec = S.WORKLOADS["c1"]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    frame = S.make_frames(xyz, 1)[0]
    r, c = S.source_pixel(spec)
    source = r * spec.res + c
    with engine(pkg, off, frac, 64, 32, 1) as eng:
        maps = eng.cohere(frame)
        noise = (1e-3 * (np.random.RandomState(5).rand(64, 1024) * 2 - 1)).astype(np.float32)
        quiet = eng.cohere(noise)["coherence"]
    coh = maps["coherence"]
    on_power = pkg.find_peaks(maps["power"], 32, 32, radius=2, max_sources=32, min_ratio=0.01)
    on_weighted = pkg.find_peaks(maps["weighted"], 32, 32, radius=2, max_sources=32, min_ratio=0.01)
    p, w = CU.median_over_max_db(maps["power"]), CU.median_over_max_db(maps["weighted"])
    print(f"coherence at the source {coh[source]:.4f}; peaks {int(on_power.count[0])} and {int(on_weighted.count[0])}; median over maximum "
          f"{p:.1f} dB and {w:.1f} dB; median coherence of noise {np.median(quiet):.4f}")
    assert coh[source] >= 0.9 and int(coh.argmax()) == source
    assert int(on_power.count[0]) > 1
    assert int(on_weighted.count[0]) == 1 and int(on_weighted.sources[0, 0]["pixel"]) == source
    assert w <= p - 20.0
    assert 0.5 / 64 <= np.median(quiet) <= 2.0 / 64


def test_run_refusals_leave_the_ring_and_the_outputs(pkg, find_c1):  # noqa: F811
    """Every refusal of the three run forms -- those that need a real handle (no table, no mic list, FIR8, a device group, a slab,
    a grid that is not the handle's) and those of the request (show, the find request) --: the status, the ring as it was, and
    every output as the caller left it: image, big_image, power, sources and count are the caller's own buffers, filled with a
    canary, for the host forms through the C entry points and for the device form in device memory."""
    import ctypes as C

    import torch

    off, frac, _, wire, samples = find_c1
    B = pkg.binding
    BYTES = 256 * 1032
    ST, INV = B.ERR_STATE, B.ERR_INVALID
    N, OUT = 2, (50, 43)  # blocks 1 .. 3 of the recording, every second one: two frames; the upscaled image's rows and columns
    sizes = {"image": (N * 1024, np.uint8), "big": (N * OUT[0] * OUT[1], np.uint8), "power": (N * 1024, np.float32),
             "sources": (N * 4 * 40, np.uint8), "count": (N, np.int32)}
    fill = {"image": 0xA5, "big": 0xA5, "power": CANARY, "sources": 0xA5, "count": -7}
    part = np.ascontiguousarray(samples[:, 256: 1024])
    d_in = torch.from_numpy(part).cuda()
    blocks = np.frombuffer(wire[BYTES: 4 * BYTES], dtype=np.uint8)

    def refused(eng, status, rows=32, cols=32, show=B.COHERE_WEIGHTED, find=FIND):
        before = eng.ring_snapshot()
        lib, h = eng._lib, eng._h
        # the binding's own calls: the status
        for call in (lambda: eng.cohere_blocks(wire[BYTES: 4 * BYTES], rows, cols, every=2, show=show, find=find),
                     lambda: eng.cohere_samples(part, rows, cols, every=2, show=show, find=find)):
            with pytest.raises(pkg.AwpuError) as ei:
                call()
            assert ei.value.status == status
        # the host forms through the C entry points, the caller's buffers filled with a canary
        w = B.Watch(0, 2, rows, cols, OUT[0], OUT[1], 0, None)
        co = B.Cohere(show)
        f = B.Find(rows, cols, find.get("radius", 2), find.get("max_sources", 4), find.get("min_power", 0.0), find.get("min_ratio", 0.0),
                   find.get("fov_deg", 180.0))
        for form in ("blocks", "samples"):
            host = {k: np.full(n, fill[k], t) for k, (n, t) in sizes.items()}
            tail = (3, C.byref(w), C.byref(co), C.byref(f), host["image"].ctypes.data_as(B._u8p), host["big"].ctypes.data_as(B._u8p),
                    host["power"].ctypes.data_as(B._f32p), C.c_void_p(host["sources"].ctypes.data), C.c_void_p(host["count"].ctypes.data))
            if form == "blocks":
                rc = lib.awpu_hip_cohere_blocks(h, blocks.ctypes.data_as(C.c_void_p), 1032, *tail)
            else:
                rc = lib.awpu_hip_cohere_samples(h, part.ctypes.data_as(B._f32p), part.shape[1], *tail)
            assert rc == status, (form, rc, status)
            for k, v in host.items():
                assert (v == np.asarray(fill[k], v.dtype)).all(), (form, k)
        # the device form, every output in device memory
        dev = {k: torch.full((n,), fill[k], dtype=torch.from_numpy(np.empty(0, t)).dtype, device="cuda") for k, (n, t) in sizes.items()}
        torch.cuda.synchronize()
        with pytest.raises(pkg.AwpuError) as ei:
            eng.cohere_samples_device(d_in.data_ptr(), part.shape[1], 3, rows, cols, every=2, show=show, d_image_ptr=dev["image"].data_ptr(),
                                      d_big_ptr=dev["big"].data_ptr(), d_power_ptr=dev["power"].data_ptr(),
                                      d_sources_ptr=dev["sources"].data_ptr(), d_count_ptr=dev["count"].data_ptr(), out_rows=OUT[0],
                                      out_cols=OUT[1], find=find)
        assert ei.value.status == status
        eng.synchronize()
        torch.cuda.synchronize()
        for k, v in dev.items():
            assert bool((v == fill[k]).all()), ("device", k)
        assert np.array_equal(eng.ring_snapshot(), before)

    with pkg.Engine(n_pixels=1024, n_streams=64, max_batch=4) as eng:  # no table, then no mic list
        eng.ingest_block(wire[:BYTES])
        refused(eng, ST)
        eng.set_delay_table(off, frac)
        refused(eng, ST)
        eng.set_active_mics(None)
        refused(eng, INV, rows=16, cols=32)   # rows x cols is not the grid
        refused(eng, INV, show=2)
        refused(eng, INV, find=dict(radius=0))
        assert eng.stats().frames == 0
        assert len(eng.cohere_blocks(wire[BYTES: 4 * BYTES], 32, 32, every=2)) == 2  # the handle still works
    with pkg.Engine(n_pixels=1024, n_streams=64, max_batch=4, interp=1) as eng:  # FIR8
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        eng.set_fir_table(util.synthetic_fir_table())
        eng.ingest_block(wire[:BYTES])
        refused(eng, ST)
    with pkg.Engine(n_pixels=1024, n_streams=64, max_batch=4, grid_columns=32, devices=[0, 0]) as eng:  # a device group
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        eng.ingest_block(wire[:BYTES])
        refused(eng, ST)
    with pkg.Engine(n_pixels=1024, n_streams=64, max_batch=4, pixel_begin=64, pixel_count=128) as eng:  # a slab of the grid
        eng.set_delay_table(off[64:192], frac[64:192])
        eng.set_active_mics(None)
        eng.ingest_block(wire[:BYTES])
        refused(eng, INV)


# ------------------------------------------------------------------------------------------------ 6. stream order

@pytest.mark.parametrize("math_mode", ["exact", "fast"])
def test_cohere_device_behind_pending_work(scenes, busy, math_mode):  # noqa: F811
    sc = scenes(16)
    outs = {"power": ((4, sc.P), np.float32), "coherence": ((4, sc.P), np.float32), "weighted": ((4, sc.P), np.float32)}
    case = H.Case(sc.engine(math_mode), {"frames": sc.frames}, outs,
                  lambda e, i, o, s: e.cohere_device(i["frames"], 4, o["power"], o["coherence"], o["weighted"], s), variant=variant)
    got = check(case, busy)
    assert np.isfinite(got["weighted"]).all() and (got["coherence"] > 0).any()


def test_cohere_device_with_a_band_behind_pending_work(pkg, scenes, busy):  # noqa: F811
    sc = scenes(16)
    outs = {"weighted": ((4, sc.P), np.float32), "sums": ((4, sc.P, 256), np.float32)}
    case = H.Case(sc.engine(band=pkg.binding.band_design(6375, 9000, 31)), {"frames": sc.frames}, outs,
                  lambda e, i, o, s: e.cohere_device_sums(i["frames"], 4, d_sums_ptr=o["sums"], d_weighted_ptr=o["weighted"], stream=s), variant=variant)
    check(case, busy)


def test_cohere_samples_device_behind_pending_work(scenes, busy):  # noqa: F811
    sc = scenes(16)
    outs = {"image": ((N_BLOCKS, sc.P), np.uint8), "big": ((N_BLOCKS,) + BIG, np.uint8), "power": ((N_BLOCKS, sc.P), np.float32),
            "sources": ((N_BLOCKS, 4, 40), np.uint8), "count": ((N_BLOCKS,), np.int32)}
    case = run_case(sc, sc.engine(), outs,
                    lambda e, x, n, o, s: e.cohere_samples_device(x, n, N_BLOCKS, 16, 16, d_image_ptr=o["image"], d_big_ptr=o["big"],
                                                                  d_power_ptr=o["power"], d_sources_ptr=o["sources"], d_count_ptr=o["count"],
                                                                  out_rows=BIG[0], out_cols=BIG[1], stream=s, find={}))
    got = check(case, busy)
    assert (got["count"] >= 1).all()
