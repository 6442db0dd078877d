"""The tone sweep (include/awpu_hip_tones.h) on the device.

1. Export: bins, spectrum and pitch of every pixel equal the host rule (awpu_hip_tones_host) bit for bit, on the shapes of
   tests/test_gpu_cohere.py -- c1 (two LDS chunks: the sweep reserves no scratch, so das_exact_kernel's chunk rule holds), a ragged
   list, one mic, four arrays, a table of three pixels and the hand-made table whose entries sit at both ends of the history --,
   batches of 1 and 3, gains on and off, both windows, every math mode's handle; guard floats around every output stay intact.
2. Groups: groups of one bin equal the rule bit for bit; wider groups, added in the device's own order, are within 2e-5 (relative,
   no floor, every pixel) of the rule's: two orders of a sum of at most 129 non-negative terms, 2 * 128 * 2^-24.  Worst measured on
   MI355X over every shape of item 1: 5.32e-07.  A frame swept alone gives the bits it gives inside a batch; the host form gives the
   device form's bits; a slab handle's planes are the full handle's rows.
3. Value edges: silence, -0.0 and DC give zero bins and pitch edge[0]; frames scaled by 2^-40 and 2^55 scale the spectrum exactly;
   a NaN stays in its frame and in the pixels that read it.
4. The band in front: the band-less call on band_filter'ed input, bit for bit.
5. Runs: the three forms equal the composition -- Engine.tones of the shown snapshots, then heatmap_u8, the upscale, find_peaks --
   for one group and for the pitch row, whole and split over calls; refusals leave the ring and the outputs alone; the tools'
   --tone and --pitch on a capture give that call's frames and lines.
6. Stream order: tones_device and tones_samples_device behind pending work on their stream (tests/stream_order.py)."""
import numpy as np
import pytest

import stream_order as H
import tones_util as TU
import util
import value_edges as V
from test_gpu_blocks import engine, snapshots
from test_gpu_cohere import CANARY, GUARD, shapes  # noqa: F401  (the shapes' tables, frames and gains)
from test_gpu_find import FIND, assert_equal_to_host, c1 as find_c1  # noqa: F401  (c1's 23-block recording)
from test_gpu_stream_order import BIG, N_BLOCKS, busy, check, run_case, scenes, variant  # noqa: F401
from test_gpu_watch import colour_table, compose

pytestmark = pytest.mark.gpu

ALL = ("tone", "pitch", "bins", "spectrum")
UNEVEN = [3, 4, 40, 41, 127]  # edge[0] > 0, edge[n] < 129; groups 0 and 2 hold one bin
GROUP_BOUND = 2e-5            # 2 * 128 * 2^-24 = 1.53e-5, rounded up
worst = {"group": 0.0}
_rules = {}


def rule(sh, gains, edges, window):
    """The host rule's answer on a shape's three frames (computed once per setting, left unchanged)."""
    key = (sh.name, gains, tuple(edges), window)
    if key not in _rules:
        got = sh.pkg.tones_host(sh.frames, sh.off, sh.frac, list(edges), window, index=sh.active, gain=sh.gains[sh.active] if gains else None, want=ALL)
        for a in got.values():
            a.setflags(write=False)
        _rules[key] = got
    return _rules[key]


def device_sweep(eng, frames, edges, window, want=ALL, stream=0):
    """tones_device_bins of host frames -> {name: array}; every output sits between guards, which must survive."""
    import torch

    frames = np.ascontiguousarray(frames, np.float32)
    batch, P, G = len(frames), eng.pixel_count, len(edges) - 1
    d_x = torch.from_numpy(np.array(frames)).cuda()
    shape = {"tone": (batch, G, P), "pitch": (batch, P), "bins": (batch, P, 129), "spectrum": (batch, P, 129, 2)}
    raw = {}
    for name in want:
        if name == "pitch":
            raw[name] = torch.full((batch * P + 2 * GUARD,), -7, dtype=torch.int32, device="cuda")
        else:
            raw[name] = torch.full((int(np.prod(shape[name])) + 2 * GUARD,), CANARY, dtype=torch.float32, device="cuda")
    ptr = {f"d_{name}_ptr": raw[name].data_ptr() + 4 * GUARD for name in want}
    torch.cuda.synchronize()
    eng.tones_device_bins(d_x.data_ptr(), batch, list(edges), window, stream=stream, **ptr)
    eng.synchronize()
    out = {}
    for name in want:
        host = raw[name].cpu().numpy()
        canary = -7 if name == "pitch" else CANARY
        assert (host[:GUARD] == canary).all() and (host[-GUARD:] == canary).all(), f"{name}: guard overwritten"
        out[name] = host[GUARD:-GUARD].reshape(shape[name])
    return out


def check_against_rule(got, want, edges, where):
    """bins, spectrum, pitch and the groups of one bin: bits; wider groups: GROUP_BOUND."""
    for name in ("bins", "spectrum"):
        if name in got:
            assert TU.same_bits(got[name], want[name]), (where, name)
    if "pitch" in got:
        assert np.array_equal(got["pitch"], want["pitch"]), (where, "pitch")
    if "tone" in got:
        for g in range(len(edges) - 1):
            if edges[g + 1] - edges[g] == 1:
                assert TU.same_bits(got["tone"][:, g], want["tone"][:, g]), (where, "group of one bin", g)
            else:
                err = TU.rel_err(got["tone"][:, g], want["tone"][:, g])
                worst["group"] = max(worst["group"], err)
                print(f"{where}: group {g} max rel err {err:.3g} (worst so far {worst['group']:.3g})")
                assert err <= GROUP_BOUND, (where, g, err)


# ------------------------------------------------------------------------------------------------ 1, 2. export, groups, composition

def test_c1_takes_more_than_one_lds_chunk(shapes):  # noqa: F811
    """The sweep reserves no LDS scratch (the transform's exchanges are cross-lane moves): a chunk is das_exact_kernel's,
    64 KB / (window * 4 bytes) mics, and c1's 64 mics do not fit one."""
    sh = shapes["c1"]
    with sh.engine() as eng:
        eng.tones(sh.frames[0], [0, 129])  # (the tables are laid out by the first call)
        window = eng.stats().window
    assert window >= 257 and (64 * 1024) // (4 * window) < 64, window


@pytest.mark.parametrize("gains", [False, True], ids=["plain", "gains"])
@pytest.mark.parametrize("name", ["c1", "ragged51", "onemic", "four_arrays", "three_pixels", "edges"])
def test_export_and_groups_equal_the_host_rule(pkg, shapes, name, gains):  # noqa: F811
    sh = shapes[name]
    edges, window = (UNEVEN, 1) if gains else ([0, 129], 0)
    want = rule(sh, gains, edges, window)
    with sh.engine(gains=gains) as eng:
        for batch in (1, 3):
            got = device_sweep(eng, sh.frames[:batch], edges, window)
            assert eng.stats().kernel_variant == 19 == pkg.binding.KERNEL_NAMES.index("tones")
            check_against_rule(got, {k: v[:batch] for k, v in want.items()}, edges, (name, gains, batch))
        whole = got
        # each output alone, and the maps through tones_device, give the same bits
        for alone in ALL:
            assert whole[alone].tobytes() == device_sweep(eng, sh.frames, edges, window, want=(alone,))[alone].tobytes(), alone
        # a frame swept alone gives the bits it gives inside a batch
        for b in range(3):
            one = device_sweep(eng, sh.frames[b: b + 1], edges, window, want=("tone", "pitch"))
            for k, v in one.items():
                assert v[0].tobytes() == whole[k][b].tobytes(), (k, b)
        # the host form uploads the windows alone where they can be cut out (the compact layout): the same bits
        maps = eng.tones(sh.frames, edges, window)
        assert maps["tone"].tobytes() == whole["tone"].tobytes() and maps["pitch"].tobytes() == whole["pitch"].tobytes()
        assert eng.tones(sh.frames[1], edges, window, want=("pitch",))["pitch"].tobytes() == whole["pitch"][1].tobytes()


def test_129_groups_are_the_bins(pkg, shapes):  # noqa: F811
    sh = shapes["ragged51"]
    edges = list(range(130))
    want = rule(sh, False, edges, 1)
    with sh.engine() as eng:
        got = device_sweep(eng, sh.frames, edges, 1)
    check_against_rule(got, want, edges, "129 groups")
    assert TU.same_bits(got["tone"], np.swapaxes(got["bins"], 1, 2))


@pytest.mark.parametrize("name", ["c1", "edges"])
def test_every_math_mode_sweeps_the_same_rule(pkg, shapes, name):  # noqa: F811
    """The rule does not depend on cfg.math: AWPU_MATH_F32_FAST (whose handle has no LutEntry table of its own) and
    AWPU_MATH_BF16_ACC give the rule's bits as the exact handle does."""
    sh = shapes[name]
    want = rule(sh, True, UNEVEN, 1)
    for math in (pkg.MATH_F32_EXACT, pkg.MATH_F32_FAST, pkg.MATH_BF16_ACC):
        with sh.engine(math=math, gains=True) as eng:
            got = device_sweep(eng, sh.frames, UNEVEN, 1)
            check_against_rule(got, want, UNEVEN, (name, math))
            eng.set_active_mics(sh.active[::2])  # the tables are rebuilt: the sweep's own table with them
            half = device_sweep(eng, sh.frames[:1], UNEVEN, 1, want=("bins",))["bins"]
            ref = pkg.tones_host(sh.frames[:1], sh.off, sh.frac, UNEVEN, 1, index=sh.active[::2], gain=sh.gains[sh.active[::2]], want=("bins",))["bins"]
            assert TU.same_bits(half, ref)


def test_a_slab_handle_sweeps_its_own_pixels(pkg, shapes):  # noqa: F811
    """The middle 8 rows of c1."""
    sh = shapes["c1"]
    lo, hi = 12 * 32, 20 * 32
    want = rule(sh, False, UNEVEN, 1)
    with sh.engine() as full, pkg.Engine(n_pixels=1024, n_streams=64, max_batch=3, pixel_begin=lo, pixel_count=hi - lo) as eng:
        eng.set_delay_table(sh.off[lo:hi], sh.frac[lo:hi])
        eng.set_active_mics(None)
        got = device_sweep(eng, sh.frames, UNEVEN, 1)
        rows = device_sweep(full, sh.frames, UNEVEN, 1)
        assert got["tone"].tobytes() == np.ascontiguousarray(rows["tone"][:, :, lo:hi]).tobytes()
        for name in ("pitch", "bins", "spectrum"):
            assert got[name].tobytes() == np.ascontiguousarray(rows[name][:, lo:hi]).tobytes(), name
        check_against_rule(got, {"tone": want["tone"][:, :, lo:hi], "pitch": want["pitch"][:, lo:hi], "bins": want["bins"][:, lo:hi],
                                 "spectrum": want["spectrum"][:, lo:hi]}, UNEVEN, "slab")
        assert eng.tones(sh.frames, UNEVEN, 1)["tone"].tobytes() == got["tone"].tobytes()


def test_handle_forms_refuse(pkg, shapes):  # noqa: F811
    """FIR8 and a device group: AWPU_ERR_STATE; no table, no mics: AWPU_ERR_STATE; no frames, no output, a bad request, a batch over
    max_batch: AWPU_ERR_INVALID; the outputs are left alone."""
    import ctypes as C

    import torch

    sh = shapes["c1"]
    B = pkg.binding
    d_x = torch.from_numpy(sh.frames).cuda()
    d_o = torch.full((3 * 4 * 1024,), CANARY, dtype=torch.float32, device="cuda")
    host = np.full((3, 4, 1024), CANARY, np.float32)
    good = B.tones_of(UNEVEN, 1)

    def refused(eng, status, batch=1, frames=True, out=True, t=good):
        calls = (lambda: eng.tones_device(d_x.data_ptr() if frames else 0, batch, t, d_tone_ptr=d_o.data_ptr() if out else 0),
                 lambda: eng.tones_device_bins(d_x.data_ptr() if frames else 0, batch, t, d_bins_ptr=0, d_tone_ptr=d_o.data_ptr() if out else 0),
                 lambda: eng._lib.awpu_hip_tones(eng._h, B._f32(sh.frames) if frames else None, batch, C.byref(t), B._f32(host) if out else None, None))
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
        for bad in (B.tones_of(UNEVEN, 2), B.tones_of([5, 5]), B.tones_of([0, 130])):
            refused(eng, B.ERR_INVALID, t=bad)
        assert eng.stats().frames == 0
        got = eng.tones(sh.frames[:2], UNEVEN, 1)  # the handle still works
        assert np.array_equal(got["pitch"], rule(sh, False, UNEVEN, 1)["pitch"][:2])
    torch.cuda.synchronize()
    assert (d_o.cpu().numpy() == CANARY).all() and (host == CANARY).all()


# ------------------------------------------------------------------------------------------------ 3. value edges

def test_silence_and_dc_have_no_tones(pkg, shapes):  # noqa: F811
    sh = shapes["c1"]
    frames = np.stack([np.zeros((64, 1024), np.float32), np.full((64, 1024), -0.0, np.float32), np.full((64, 1024), 0.25, np.float32)])
    with sh.engine() as eng:
        got = device_sweep(eng, frames, UNEVEN, 1)
    assert TU.same_bits(got["bins"], np.zeros_like(got["bins"])) and TU.same_bits(got["tone"], np.zeros_like(got["tone"]))
    assert (got["pitch"] == UNEVEN[0]).all()


@pytest.mark.parametrize("k", [-40, 55])
def test_scaled_frames_scale_the_spectrum_exactly(pkg, shapes, k):  # noqa: F811
    sh = shapes["ragged51"]
    frames = V.scale_pow2(sh.frames[:2], k)
    want = pkg.tones_host(frames, sh.off, sh.frac, UNEVEN, 1, index=sh.active, want=ALL)
    assert np.isfinite(want["spectrum"]).all() and want["spectrum"].any()
    with sh.engine() as eng:
        got = device_sweep(eng, frames, UNEVEN, 1)
    assert TU.same_bits(got["spectrum"], want["spectrum"])
    assert TU.same_bits(got["spectrum"], V.scale_pow2(rule(sh, False, UNEVEN, 1)["spectrum"][:2], k))
    if np.isfinite(want["bins"]).all():  # (2^55 squared leaves fp32: the rule as written gives inf on both sides, NaN nowhere)
        check_against_rule(got, want, UNEVEN, ("scaled", k))
    else:
        assert np.array_equal(np.isinf(got["bins"]), np.isinf(want["bins"])) and not np.isnan(got["bins"]).any()
        fin = np.isfinite(want["bins"])
        assert TU.same_bits(got["bins"][fin], want["bins"][fin])


def test_a_nan_stays_in_its_frame_and_its_pixels(pkg, shapes):  # noqa: F811
    sh = shapes["c1"]
    at = int(np.median(sh.off[:, 9])) + 256  # the last sample that half of the pixels read of mic 9
    bad = sh.frames.copy()
    bad[1, 9, at] = np.nan
    reads = (sh.off[:, 9] <= at) & (at <= sh.off[:, 9] + 256)
    assert reads.any() and not reads.all()
    with sh.engine() as eng:
        ok = device_sweep(eng, sh.frames, UNEVEN, 1)
        got = device_sweep(eng, bad, UNEVEN, 1)
    for name in ALL:
        for b in (0, 2):
            assert got[name][b].tobytes() == ok[name][b].tobytes(), (name, b)
    assert TU.same_bits(got["bins"][1][~reads], ok["bins"][1][~reads]) and np.array_equal(got["pitch"][1][~reads], ok["pitch"][1][~reads])
    assert TU.same_bits(got["tone"][1][:, ~reads], ok["tone"][1][:, ~reads])
    want = pkg.tones_host(bad[1], sh.off, sh.frac, UNEVEN, 1, want=("bins",))["bins"]
    assert np.array_equal(np.isnan(got["bins"][1]), np.isnan(want)) and np.isnan(got["bins"][1][reads]).all()


# ------------------------------------------------------------------------------------------------ 4. the band

def test_the_band_in_front_is_the_sweep_of_filtered_frames(pkg, shapes):  # noqa: F811
    sh = shapes["ragged51"]
    assert int(sh.off.min()) >= 62
    c = pkg.binding.band_design(6375, 9000, 63)
    filtered = pkg.binding.band_filter(sh.frames, c)
    with sh.engine(gains=True) as plain, sh.engine(gains=True, band=c) as banded:
        want = device_sweep(plain, filtered, UNEVEN, 1)
        got = device_sweep(banded, sh.frames, UNEVEN, 1)
        for name in ALL:
            assert got[name].tobytes() == want[name].tobytes(), name
        assert not TU.same_bits(got["bins"], device_sweep(plain, sh.frames, UNEVEN, 1, want=("bins",))["bins"])
        host_got, host_want = banded.tones(sh.frames, UNEVEN, 1), plain.tones(filtered, UNEVEN, 1)
        for name in ("tone", "pitch"):
            assert host_got[name].tobytes() == host_want[name].tobytes() == want[name].tobytes(), name


# ------------------------------------------------------------------------------------------------ 5. the runs

RUN_EDGES = [30, 44, 51, 60]  # group 1 holds the recording's 9 kHz (bin 47)


def composition(pkg, off, frac, samples, first, every, show, ring=None):
    """Rows of the shown snapshots by Engine.tones on a handle of its own."""
    snaps = snapshots(samples, ring)[first::every]
    with engine(pkg, off, frac, 64, 32, 32) as eng:
        if show == pkg.binding.TONES_SHOW_PITCH:
            return eng.tones(snaps, RUN_EDGES, 1, want=("pitch",))["pitch"].astype(np.float32)
        return np.ascontiguousarray(eng.tones(snaps, RUN_EDGES, 1, want=("tone",))["tone"][:, show])


@pytest.mark.parametrize("max_batch", [4, 32])
@pytest.mark.parametrize("first,every", [(0, 1), (2, 3)])
def test_run_forms_equal_the_composition(pkg, oracle, find_c1, max_batch, first, every):  # noqa: F811
    import torch

    off, frac, _, wire, samples = find_c1
    n_frames = len(range(first, 23, every))
    table, d_table = colour_table()
    with engine(pkg, off, frac, 64, 32, max_batch) as ref:
        watched = ref.watch_samples(samples, 32, 32, first=first, every=every, want_image=False, want_power=True)
        ring, frames_swept, launches = ref.ring_snapshot(), ref.stats().frames, ref.stats().launches
    d_in = torch.from_numpy(np.ascontiguousarray(samples)).cuda()
    for show in (1, pkg.binding.TONES_SHOW_PITCH):
        rows = composition(pkg, off, frac, samples, first, every, show)
        assert rows.shape == (n_frames, 1024) and not TU.same_bits(rows, watched.power)
        image, big = compose(pkg, oracle, rows, 32, 32, 50, 43, table, True)
        want = pkg.find_peaks(rows, 32, 32, **FIND)

        def check_run(got, eng):
            assert got.next_first == watched.next_first and len(got) == n_frames
            assert TU.same_bits(got.power, rows)
            assert np.array_equal(got.image, image) and np.array_equal(got.big, big)
            assert_equal_to_host(got.sources, got.count, want, (max_batch, first, every, show))
            assert np.array_equal(eng.ring_snapshot(), ring)
            assert (eng.stats().frames, eng.stats().launches) == (frames_swept, launches)

        kw = dict(show=show, first=first, every=every, out_rows=50, out_cols=43, d_colormap_ptr=d_table.data_ptr(), flip=True, want_power=True,
                  find=FIND)
        with engine(pkg, off, frac, 64, 32, max_batch) as eng:
            check_run(eng.tones_blocks(wire, 32, 32, RUN_EDGES, 1, **kw), eng)
        with engine(pkg, off, frac, 64, 32, max_batch) as eng:
            check_run(eng.tones_samples(samples, 32, 32, RUN_EDGES, 1, **kw), eng)
        with engine(pkg, off, frac, 64, 32, max_batch) as eng:  # the device form, every output between guards
            outs = {"image": (n_frames * 1024, torch.uint8), "big": (n_frames * 50 * 43 * 3, torch.uint8), "power": (n_frames * 1024, torch.float32),
                    "sources": (n_frames * 4 * 40, torch.uint8), "count": (n_frames, torch.int32)}
            fill = {torch.uint8: 0xA5, torch.float32: CANARY, torch.int32: -7}
            raw = {k: torch.full((n + 128,), fill[t], dtype=t, device="cuda") for k, (n, t) in outs.items()}
            ptr = {k: v.data_ptr() + 64 * v.element_size() for k, v in raw.items()}
            torch.cuda.synchronize()
            nxt = eng.tones_samples_device(d_in.data_ptr(), samples.shape[1], 23, 32, 32, RUN_EDGES, 1, show=show, first=first, every=every,
                                           d_image_ptr=ptr["image"], d_big_ptr=ptr["big"], d_power_ptr=ptr["power"], d_sources_ptr=ptr["sources"],
                                           d_count_ptr=ptr["count"], out_rows=50, out_cols=43, d_colormap_ptr=d_table.data_ptr(), flip=True, find=FIND)
            eng.synchronize()
            assert nxt == watched.next_first
            host = {k: v.cpu().numpy() for k, v in raw.items()}
            for k, v in host.items():
                assert (v[:64] == fill[outs[k][1]]).all() and (v[-64:] == fill[outs[k][1]]).all(), k
            assert TU.same_bits(host["power"][64:-64].reshape(n_frames, 1024), rows)
            assert np.array_equal(host["image"][64:-64].reshape(n_frames, 32, 32), image)
            assert np.array_equal(host["big"][64:-64].reshape(big.shape), big)
            assert_equal_to_host(host["sources"][64:-64].view(pkg.binding.SOURCE_DTYPE).reshape(n_frames, 4), host["count"][64:-64], want, "device")
            assert np.array_equal(eng.ring_snapshot(), ring)


@pytest.mark.parametrize("show", [1, -1], ids=["group", "pitch"])
def test_a_split_recording_equals_one_call(pkg, find_c1, show):  # noqa: F811
    off, frac, _, wire, samples = find_c1
    BYTES = 256 * 1032
    kw = dict(show=show, every=3, want_image=True, want_power=True, find=FIND)
    with engine(pkg, off, frac, 64, 32, 4) as eng:
        whole = eng.tones_samples(samples, 32, 32, RUN_EDGES, 1, first=2, **kw)
        ring = eng.ring_snapshot()
    with engine(pkg, off, frac, 64, 32, 4) as eng:
        a = eng.tones_samples(samples[:, : 256 * 10], 32, 32, RUN_EDGES, 1, first=2, **kw)
        b = eng.tones_blocks(wire[10 * BYTES:], 32, 32, RUN_EDGES, 1, first=a.next_first, **kw)
        assert b.next_first == whole.next_first and len(a) + len(b) == len(whole)
        for name in ("power", "image", "count"):
            joined = np.concatenate([getattr(r, name) for r in (a, b)])
            assert joined.tobytes() == getattr(whole, name).tobytes(), name
        assert np.concatenate([r.sources for r in (a, b)]).tobytes() == whole.sources.tobytes()
        assert np.array_equal(eng.ring_snapshot(), ring)
        # mixing with the other run calls: the next run continues from the same ring
        rows = composition(pkg, off, frac, samples[:, : 256 * 4], 0, 1, show, ring=ring)
        again = eng.tones_samples(samples[:, : 256 * 4], 32, 32, RUN_EDGES, 1, show=show, want_image=False, want_power=True)
        assert TU.same_bits(again.power, rows)


def test_the_pitch_row_finds_the_recordings_tone(pkg, find_c1):  # noqa: F811
    """The recording is synthetic.make_frames' 9 kHz wave: bin 47 at the source's pixel of every block."""
    off, frac, _, wire, samples = find_c1
    S = pkg.synthetic
    r, c = S.source_pixel(S.WORKLOADS["c1"])
    with engine(pkg, off, frac, 64, 32, 8) as eng:
        got = eng.tones_samples(samples, 32, 32, [0, 129], show=-1, first=4, every=5, want_image=False, want_power=True)
    assert (got.power[:, r * 32 + c] == 47.0).all()


def test_run_refusals_leave_the_ring_and_the_outputs(pkg, find_c1):  # noqa: F811
    """The refusals of the three run forms that need a real handle (no table, no mic list, FIR8, a device group, a slab, a grid
    that is not the handle's) and those of the request (t, show, the find request): the status, the ring as it was, and every
    output as the caller left it."""
    import ctypes as C

    import torch

    off, frac, _, wire, samples = find_c1
    B = pkg.binding
    BYTES = 256 * 1032
    ST, INV = B.ERR_STATE, B.ERR_INVALID
    N, OUT = 2, (50, 43)
    sizes = {"image": (N * 1024, np.uint8), "big": (N * OUT[0] * OUT[1], np.uint8), "power": (N * 1024, np.float32),
             "sources": (N * 4 * 40, np.uint8), "count": (N, np.int32)}
    fill = {"image": 0xA5, "big": 0xA5, "power": CANARY, "sources": 0xA5, "count": -7}
    part = np.ascontiguousarray(samples[:, 256: 1024])
    d_in = torch.from_numpy(part).cuda()
    blocks = np.frombuffer(wire[BYTES: 4 * BYTES], dtype=np.uint8)
    good = B.tones_of(RUN_EDGES, 1)

    def refused(eng, status, rows=32, cols=32, t=good, show=1, find=FIND):
        before = eng.ring_snapshot()
        lib, h = eng._lib, eng._h
        w = B.Watch(0, 2, rows, cols, OUT[0], OUT[1], 0, None)
        f = B.Find(rows, cols, find.get("radius", 2), find.get("max_sources", 4), find.get("min_power", 0.0), find.get("min_ratio", 0.0),
                   find.get("fov_deg", 180.0))
        for form in ("blocks", "samples"):
            host = {k: np.full(n, fill[k], ty) for k, (n, ty) in sizes.items()}
            tail = (3, C.byref(w), C.byref(t), show, C.byref(f), host["image"].ctypes.data_as(B._u8p), host["big"].ctypes.data_as(B._u8p),
                    host["power"].ctypes.data_as(B._f32p), C.c_void_p(host["sources"].ctypes.data), C.c_void_p(host["count"].ctypes.data))
            if form == "blocks":
                rc = lib.awpu_hip_tones_blocks(h, blocks.ctypes.data_as(C.c_void_p), 1032, *tail)
            else:
                rc = lib.awpu_hip_tones_samples(h, part.ctypes.data_as(B._f32p), part.shape[1], *tail)
            assert rc == status, (form, rc, status)
            for k, v in host.items():
                assert (v == np.asarray(fill[k], v.dtype)).all(), (form, k)
        dev = {k: torch.full((n,), fill[k], dtype=torch.from_numpy(np.empty(0, ty)).dtype, device="cuda") for k, (n, ty) in sizes.items()}
        torch.cuda.synchronize()
        with pytest.raises(pkg.AwpuError) as ei:
            eng.tones_samples_device(d_in.data_ptr(), part.shape[1], 3, rows, cols, t, show=show, every=2, d_image_ptr=dev["image"].data_ptr(),
                                     d_big_ptr=dev["big"].data_ptr(), d_power_ptr=dev["power"].data_ptr(), d_sources_ptr=dev["sources"].data_ptr(),
                                     d_count_ptr=dev["count"].data_ptr(), out_rows=OUT[0], out_cols=OUT[1], find=find)
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
        refused(eng, INV, show=3)
        refused(eng, INV, show=-2)
        refused(eng, INV, t=B.tones_of(RUN_EDGES, 2))
        refused(eng, INV, t=B.tones_of([30, 30, 40]))
        refused(eng, INV, find=dict(radius=0))
        assert eng.stats().frames == 0
        assert len(eng.tones_blocks(wire[BYTES: 4 * BYTES], 32, 32, RUN_EDGES, 1, every=2)) == 2  # the handle still works
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


def test_the_tools_show_and_search_a_tone(pkg, find_c1, tmp_path):  # noqa: F811
    """tools/pcap_video.py --tone / --pitch and tools/pcap_sources.py --tone on a capture of the first 11 blocks, in chunks: the
    AVI's frames and the CSV's lines are those of one tones_blocks call over the capture."""
    import importlib.util
    import sys

    import torch

    from test_blocks_cpu import udp_frame, write_pcap
    from test_find_cpu import REPO

    def load(name):
        spec = importlib.util.spec_from_file_location(name, REPO / "tools" / f"{name}.py")
        tool = importlib.util.module_from_spec(spec)
        sys.modules[name] = tool
        spec.loader.exec_module(tool)
        return tool

    video, sources = load("pcap_video"), load("pcap_sources")
    off, frac, _, wire, _ = find_c1
    BYTES = 256 * 1032
    pcap = tmp_path / "rec.pcap"
    write_pcap(pcap, [udp_frame(wire[k: k + 1032], 21844) for k in range(0, 11 * BYTES, 1032)])
    common = [str(pcap), "--port", "21844", "--cols", "32", "--every", "3", "--chunk", "4", "--max-batch", "4"]
    d_table = torch.from_numpy(video.jet_table()).cuda()
    groups = pkg.binding.tones_from_text("8000:10000:hann")
    assert list(pkg.binding.tones_edges(groups)) == [42, 53] and groups.window == 1
    for flag, show in (("--tone", 0), ("--pitch", pkg.binding.TONES_SHOW_PITCH)):
        assert video.main(common + ["--size", "50", "--flip", flag, "8000:10000:hann", "--out", str(tmp_path / "toned")]) == 0
        frames, rate, scale = video.read_avi(tmp_path / "toned.000.avi")
        assert (rate, scale) == video.frame_rate(3)
        with engine(pkg, off, frac, 64, 32, 4) as eng:
            want = eng.tones_blocks(wire[: 11 * BYTES], 32, 32, groups, show=show, every=3, out_rows=50, out_cols=50,
                                    d_colormap_ptr=d_table.data_ptr(), flip=True, want_image=False)
        assert len(want) == 4 and np.array_equal(frames, want.big) and frames.any()
    out = tmp_path / "sources.csv"
    assert sources.main(common + ["--tone", "8000:10000", "--max-sources", "3", "--out", str(out)]) == 0
    back = sources.read_rows(out)
    with engine(pkg, off, frac, 64, 32, 4) as eng:
        want = eng.tones_blocks(wire[: 11 * BYTES], 32, 32, [42, 53], every=3, want_image=False, find=dict(radius=2, max_sources=3, min_ratio=0.25))
    assert len(back) == int(want.count.sum()) >= 4
    k = 0
    for j, (entries, n) in enumerate(zip(want.sources, want.count)):
        for rank in range(n):
            assert (back[k]["block"], back[k]["rank"], back[k]["pixel"]) == (3 * j, rank, entries[rank]["pixel"])
            assert back[k]["power"] == entries[rank]["power"] and back[k]["row"] == entries[rank]["row"] and back[k]["col"] == entries[rank]["col"]
            k += 1


# ------------------------------------------------------------------------------------------------ 6. stream order

@pytest.mark.parametrize("math_mode", ["exact", "fast"])
def test_tones_device_behind_pending_work(scenes, busy, math_mode):  # noqa: F811
    sc = scenes(16)
    outs = {"tone": ((4, 4, sc.P), np.float32), "pitch": ((4, sc.P), np.int32)}
    case = H.Case(sc.engine(math_mode), {"frames": sc.frames}, outs,
                  lambda e, i, o, s: e.tones_device(i["frames"], 4, UNEVEN, 1, d_tone_ptr=o["tone"], d_pitch_ptr=o["pitch"], stream=s), variant=variant)
    got = check(case, busy)
    assert np.isfinite(got["tone"]).all() and (got["tone"] > 0).any() and (got["pitch"] >= 3).all() and (got["pitch"] < 127).all()


def test_tones_samples_device_behind_pending_work(scenes, busy):  # noqa: F811
    sc = scenes(16)
    outs = {"image": ((N_BLOCKS, sc.P), np.uint8), "big": ((N_BLOCKS,) + BIG, np.uint8), "power": ((N_BLOCKS, sc.P), np.float32),
            "sources": ((N_BLOCKS, 4, 40), np.uint8), "count": ((N_BLOCKS,), np.int32)}
    case = run_case(sc, sc.engine(), outs,
                    lambda e, x, n, o, s: e.tones_samples_device(x, n, N_BLOCKS, 16, 16, UNEVEN, 1, show=1, d_image_ptr=o["image"], d_big_ptr=o["big"],
                                                                 d_power_ptr=o["power"], d_sources_ptr=o["sources"], d_count_ptr=o["count"],
                                                                 out_rows=BIG[0], out_cols=BIG[1], stream=s, find={}))
    got = check(case, busy)
    assert (got["count"] >= 1).all()
