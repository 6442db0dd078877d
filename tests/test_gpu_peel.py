"""Peeling sources (include/awpu_hip_peel.h) on the device.

1. The step: residual frames and beams of awpu_hip_peel_step_device equal the host rule (awpu_hip_peel_step_host) bit for bit, on the
   small shape of tests/test_peel_cpu.py (8 streams, 5 active, gains with a 0 and a negative value, pixels at both ends of the
   reach, a frame without a pixel) and on the 8 x 8 array's table with 61 of 64 mics; guard floats around the beams stay intact.
2. The loop on the two-source scene, a second seed and a silent frame: awpu_hip_peel_device equals, bit for bit, the composition
   a caller drives by hand (process_device, the pick, peel_step_device); against awpu_hip_peel_host on an exact-math handle the
   picks are identical, the residual frames bit-identical, `residual` within 1e-5 relative per pixel (the project's sweep
   tolerance), `removed` and `clean` within 1e-5 (before + after) absolute (the subtraction of two such powers), `map` within
   the sum of the two; the physics of tests/test_peel_cpu.py holds on the device's output.  The host form gives the same bits.
3. A fast-math handle: the composition identity.
4. Value edges: a NaN sample stays in its frame; stop_ratio; one step; gain 0.5.
5. Stream order: peel_device behind pending work on its stream (tests/stream_order.py).
6. Runs: peel_samples_device on a 5-block recording with every 2, each show value, equals the composition of the snapshots,
   Engine.peel, the display chain and find_peaks bit for bit; split across two calls; _blocks and _samples against it.
7. Every refusal of the header, the three run forms included; the handle serves a plain sweep with its usual bits afterwards."""
import numpy as np
import pytest

import cohere_util as CU
import peel_util as PU
import stream_order as H
# (stream_order.py holds the harness; the fixtures that feed it -- the busywork sized once per module, the scenes, check() -- live in
# test_gpu_stream_order.py, and the recordings and display compositions of the run tests in the run test modules.  They are imported
# from there, as tests/test_gpu_cohere.py does: existing test files and conftest.py are not to be changed, so they cannot be moved.)
from test_gpu_blocks import engine as run_engine, snapshots
from test_gpu_find import FIND, assert_equal_to_host, c1 as find_c1  # noqa: F401  (c1's 23-block recording)
from test_gpu_stream_order import busy, check, scenes, variant  # noqa: F401
from test_gpu_watch import colour_table, compose
from test_peel_cpu import SCENE_SEED, SECOND_SEED, check_physics, check_preconditions, small_shape, true_weak_db

pytestmark = pytest.mark.gpu

GUARD = 64  # floats in front of and behind a guarded device output
CANARY = -3.0
STEPS = 4


def engine(pkg, off, frac, n_streams, max_batch, index=None, gains=None, math=None, **kw):
    eng = pkg.Engine(n_pixels=off.shape[0], n_streams=n_streams, max_batch=max_batch, math=math, **kw)
    eng.set_delay_table(off, frac)
    eng.set_active_mics(index)
    if gains is not None:
        eng.set_mic_gains(gains)
    return eng


def step_on_device(eng, frames, pixel, gamma, length):
    """peel_step_device of host frames -> (frames after it, beams); the beams sit between guard floats."""
    import torch

    d_x = torch.from_numpy(np.array(frames, np.float32)).cuda()
    d_pix = torch.from_numpy(np.asarray(pixel, np.int32)).cuda()
    raw = torch.full((len(frames) * length + 2 * GUARD,), CANARY, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.peel_step_device(d_x.data_ptr(), len(frames), d_pix.data_ptr(), gamma, raw.data_ptr() + 4 * GUARD)
    eng.synchronize()
    host = raw.cpu().numpy()
    assert (host[:GUARD] == CANARY).all() and (host[-GUARD:] == CANARY).all(), "beams: guard overwritten"
    return d_x.cpu().numpy(), host[GUARD:-GUARD].reshape(len(frames), length)


def loop_on_device(eng, frames, steps=STEPS, gain=1.0, stop_ratio=0.0, stream=0):
    """peel_device of host frames -> dict(steps, clean, residual, map, frames); the input frames must come back untouched."""
    import torch

    frames = np.ascontiguousarray(frames, np.float32)
    batch, P = len(frames), eng.pixel_count
    d_x = torch.from_numpy(np.array(frames)).cuda()
    d_steps = torch.full((batch * steps * 3 + 2 * GUARD,), -7, dtype=torch.int32, device="cuda")
    maps = {name: torch.full((batch * P + 2 * GUARD,), CANARY, dtype=torch.float32, device="cuda") for name in ("clean", "residual", "map")}
    d_left = torch.full((frames.size + 2 * GUARD,), CANARY, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.peel_device(d_x.data_ptr(), batch, steps, gain, stop_ratio, d_steps.data_ptr() + 4 * GUARD, *[maps[n].data_ptr() + 4 * GUARD for n in maps],
                    d_left.data_ptr() + 4 * GUARD, stream)
    eng.synchronize()
    assert CU.same_bits(d_x.cpu().numpy(), frames), "the input frames were written"
    out = {}
    for name, t in list(maps.items()) + [("frames", d_left)]:
        host = t.cpu().numpy()
        assert (host[:GUARD] == CANARY).all() and (host[-GUARD:] == CANARY).all(), f"{name}: guard overwritten"
        out[name] = host[GUARD:-GUARD].reshape(frames.shape if name == "frames" else (batch, P))
    host = d_steps.cpu().numpy()
    assert (host[:GUARD] == -7).all() and (host[-GUARD:] == -7).all(), "steps: guard overwritten"
    out["steps"] = host[GUARD:-GUARD].copy().view(eng_step_dtype(eng)).reshape(batch, steps)
    return out


def eng_step_dtype(eng):
    import importlib

    return importlib.import_module(type(eng).__module__).PEEL_STEP_DTYPE


def loop_by_hand(eng, frames, steps=STEPS, gain=1.0, stop_ratio=0.0):
    """The loop a caller drives through the public calls: process_device, the pick on the host, peel_step_device."""
    import torch

    batch, P = len(frames), eng.pixel_count
    d_x = torch.from_numpy(np.array(frames, np.float32)).cuda()
    d_p = torch.zeros((batch, P), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def sweep():
        eng.process_device(d_x.data_ptr(), batch, d_p.data_ptr())
        eng.synchronize()
        return d_p.cpu().numpy()

    rec = np.zeros((batch, steps), eng_step_dtype(eng))
    rec["pixel"] = -1
    done, first = [False] * batch, [np.float32(0)] * batch
    rows = sweep()
    for k in range(steps):
        pixel = np.full(batch, -1, np.int32)
        for b in range(batch):
            p = -1 if done[b] else PU.pick(rows[b])
            if p >= 0:
                if k == 0:
                    first[b] = rows[b][p]
                if rows[b][p] < PU.floor_ratio(stop_ratio, first[b]):
                    p = -1
            done[b] = p < 0
            if p >= 0:
                pixel[b] = p
                rec[b, k]["pixel"], rec[b, k]["before"] = p, rows[b][p]
        d_pix = torch.from_numpy(pixel).cuda()
        eng.peel_step_device(d_x.data_ptr(), batch, d_pix.data_ptr(), gain)
        rows = sweep()
        for b in range(batch):
            if pixel[b] >= 0:
                d = np.float32(rec[b, k]["before"] - rows[b][pixel[b]])
                rec[b, k]["removed"] = d if d > 0 else np.float32(0)
    clean = np.zeros((batch, P), np.float32)
    for b in range(batch):
        for s in rec[b]:
            if s["pixel"] >= 0:
                clean[b, s["pixel"]] = clean[b, s["pixel"]] + s["removed"]
    return dict(steps=rec, clean=clean, residual=rows, map=clean + rows, frames=d_x.cpu().numpy())


def assert_same_loop(got, want, where=""):
    assert got["steps"].tobytes() == want["steps"].tobytes(), (where, got["steps"], want["steps"])
    for name in ("clean", "residual", "map", "frames"):
        assert CU.same_bits(got[name], want[name]), (where, name)


# ------------------------------------------------------------------------------------------------ 1. the step

@pytest.mark.parametrize("gamma", [1.0, 0.5])
@pytest.mark.parametrize("with_gain", [False, True], ids=["plain", "gains"])
def test_step_equals_the_host_rule_on_the_small_shape(pkg, gamma, with_gain):
    s = small_shape()
    by_stream = np.ones(8, np.float32)
    by_stream[s["index"]] = s["gain"]
    want_frames, want_beams = pkg.peel_step_host(s["frames"], s["off"], s["frac"], s["pixel"], gamma, index=s["index"], gain=s["gain"] if with_gain else None)
    with engine(pkg, s["off"], s["frac"], 8, 3, index=s["index"], gains=by_stream if with_gain else None) as eng:
        got_frames, got_beams = step_on_device(eng, s["frames"], s["pixel"], gamma, want_beams.shape[1])
        assert CU.same_bits(got_frames, want_frames) and CU.same_bits(got_beams, want_beams)
        # a second step on the residual, the pixels swapped: the kernel's reads see the first step's writes
        again = s["pixel"][[1, 0, 2]]
        want2, _ = pkg.peel_step_host(want_frames, s["off"], s["frac"], again, gamma, index=s["index"], gain=s["gain"] if with_gain else None)
        got2, _ = step_on_device(eng, got_frames, again, gamma, want_beams.shape[1])
        assert CU.same_bits(got2, want2)


@pytest.mark.parametrize("math_mode", ["exact", "fast"])
def test_step_equals_the_host_rule_with_61_of_64_mics(pkg, math_mode):
    off, frac = PU.scene_table(pkg)
    index = np.random.default_rng(4).permutation(np.delete(np.arange(64), [5, 17, 40])).astype(np.int32)
    frames = np.stack([PU.scene_frame(off, frac, SCENE_SEED), PU.scene_frame(off, frac, SECOND_SEED)])
    pixel = np.array([0, 24 * 24 - 1], np.int32)  # two corners of the grid: the table's extreme delays
    want_frames, want_beams = pkg.peel_step_host(frames, off, frac, pixel, 1.0, index=index)
    with engine(pkg, off, frac, 64, 2, index=index, math=pkg.MATH_F32_FAST if math_mode == "fast" else None, grid_columns=24) as eng:
        got_frames, got_beams = step_on_device(eng, frames, pixel, 1.0, want_beams.shape[1])
    assert CU.same_bits(got_frames, want_frames) and CU.same_bits(got_beams, want_beams)
    assert not CU.same_bits(got_frames[:, index], frames[:, index]) and CU.same_bits(got_frames[:, [5, 17, 40]], frames[:, [5, 17, 40]])


# ------------------------------------------------------------------------------------------------ 2, 3. the loop

@pytest.fixture(scope="module")
def scene(pkg):
    """The table, the batch (the scene, a second seed, silence) and the host rule's answer on it (computed once, left unchanged)."""
    off, frac = PU.scene_table(pkg)
    frames = np.stack([PU.scene_frame(off, frac, SCENE_SEED), PU.scene_frame(off, frac, SECOND_SEED), np.zeros((64, 1024), np.float32)])
    host = pkg.peel_host(frames, off, frac, STEPS)
    for a in (frames, host.steps, host.clean, host.residual, host.map, host.frames):
        a.setflags(write=False)
    return dict(off=off, frac=frac, frames=frames, host=host, strong=PU.STRONG[0] * PU.RES + PU.STRONG[1], weak=PU.WEAK[0] * PU.RES + PU.WEAK[1])


@pytest.fixture(scope="module")
def exact_loop(pkg, scene):
    with engine(pkg, scene["off"], scene["frac"], 64, 3, grid_columns=24) as eng:
        got = loop_on_device(eng, scene["frames"])
        by_hand = loop_by_hand(eng, scene["frames"])
        host_form = eng.peel(scene["frames"], STEPS, want_frames=True)
    return got, by_hand, host_form


def test_loop_equals_the_composition_by_hand(exact_loop):
    got, by_hand, host_form = exact_loop
    assert_same_loop(got, by_hand)
    assert_same_loop(got, dict(steps=host_form.steps, clean=host_form.clean, residual=host_form.residual, map=host_form.map, frames=host_form.frames),
                     "host form")


def test_loop_against_the_host_rule(scene, exact_loop):
    got, host = exact_loop[0], scene["host"]
    assert np.array_equal(got["steps"]["pixel"], host.steps["pixel"]), (got["steps"]["pixel"], host.steps["pixel"])
    assert CU.same_bits(got["frames"], host.frames)
    err = CU.rel_err(got["residual"], host.residual)
    print("residual: max rel err", err)
    assert err <= 1e-5
    for b in range(3):
        bound = np.zeros(got["clean"].shape[1])
        for g, w in zip(got["steps"][b], host.steps[b]):
            if w["pixel"] < 0:
                continue
            after = np.float64(w["before"]) - np.float64(w["removed"])
            step_bound = 1e-5 * (np.float64(w["before"]) + after)
            print(f"frame {b}: pixel {w['pixel']} before {w['before']:.6g} removed {w['removed']:.6g} device - host {float(g['removed']) - float(w['removed']):.3g} bound {step_bound:.3g}")
            assert abs(np.float64(g["before"]) - np.float64(w["before"])) <= 1e-5 * np.float64(w["before"])
            assert abs(np.float64(g["removed"]) - np.float64(w["removed"])) <= step_bound
            bound[w["pixel"]] += step_bound
        d_clean = np.abs(got["clean"][b].astype(np.float64) - host.clean[b])
        assert (d_clean <= bound).all(), (b, d_clean.max())
        d_map = np.abs(got["map"][b].astype(np.float64) - host.map[b])
        assert (d_map <= bound + 1e-5 * host.residual[b].astype(np.float64)).all(), (b, d_map.max())


def test_a_silent_frame_has_no_step_and_zero_maps(exact_loop):
    got = exact_loop[0]
    assert (got["steps"][2]["pixel"] == -1).all() and not got["steps"][2]["before"].any() and not got["steps"][2]["removed"].any()
    for name in ("clean", "residual", "map", "frames"):
        assert not got[name][2].any(), name


def test_the_device_loop_finds_the_weak_source(pkg, scene, exact_loop):
    got = exact_loop[0]
    by_hand = PU.loop(scene["frames"][0], lambda f: pkg.cohere_host(f, scene["off"], scene["frac"])[0],
                      lambda f, p: pkg.peel_step_host(f[None], scene["off"], scene["frac"], [p])[0][0], STEPS)
    check_preconditions(pkg, dict(by_hand=by_hand, strong=scene["strong"], weak=scene["weak"]))
    true_db = true_weak_db(pkg, scene["off"], scene["frac"], SCENE_SEED, scene["strong"], scene["weak"])
    check_physics(got["steps"][0], got["clean"][0], scene["strong"], scene["weak"], true_db)


def test_loop_on_a_fast_math_handle_equals_the_composition(pkg, scene):
    with engine(pkg, scene["off"], scene["frac"], 64, 3, math=pkg.MATH_F32_FAST, grid_columns=24) as eng:
        got = loop_on_device(eng, scene["frames"])
        assert_same_loop(got, loop_by_hand(eng, scene["frames"]))
    assert [int(p) for p in got["steps"][0]["pixel"][:2]] == [scene["strong"], scene["weak"]]


def test_null_outputs_and_the_handles_own_residual(pkg, scene, exact_loop):
    """Every output may be null; without d_residual_frames the residual lives in the handle and the maps are the same."""
    import torch

    d_x = torch.from_numpy(np.array(scene["frames"])).cuda()
    d_map = torch.zeros((3, 576), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with engine(pkg, scene["off"], scene["frac"], 64, 3, grid_columns=24) as eng:
        eng.peel_device(d_x.data_ptr(), 3, STEPS, d_map_ptr=d_map.data_ptr())
        eng.synchronize()
        assert CU.same_bits(d_map.cpu().numpy(), exact_loop[0]["map"]) and CU.same_bits(d_x.cpu().numpy(), scene["frames"])
        eng.peel_device(d_x.data_ptr(), 3, STEPS)
        eng.synchronize()


# ------------------------------------------------------------------------------------------------ 4. value edges

def test_a_nan_sample_stays_in_its_frame(pkg, scene):
    frames = np.array(scene["frames"][[0, 1, 1]])
    frames[1, 9, 300] = np.nan
    with engine(pkg, scene["off"], scene["frac"], 64, 3, grid_columns=24) as eng:
        got = loop_on_device(eng, frames)
        for b in (0, 2):
            solo = loop_on_device(eng, frames[b:b + 1])
            assert got["steps"][b].tobytes() == solo["steps"][0].tobytes()
            for name in ("clean", "residual", "map", "frames"):
                assert CU.same_bits(got[name][b], solo[name][0]), (b, name)
    assert (got["steps"][1]["pixel"] == -1).all() and np.isnan(got["residual"][1]).all() and not got["clean"][1].any()
    assert CU.same_bits(got["frames"][1], frames[1])  # no finite pick: done at once, never modified


def test_stop_ratio_steps_1_and_gain_half(pkg, scene, exact_loop):
    whole = exact_loop[0]
    with engine(pkg, scene["off"], scene["frac"], 64, 3, grid_columns=24) as eng:
        stopped = loop_on_device(eng, scene["frames"], stop_ratio=0.5)  # the second pick is 15 dB under the first
        one = loop_on_device(eng, scene["frames"], steps=1)
        half = loop_on_device(eng, scene["frames"], steps=8, gain=0.5)
        half_by_hand = loop_by_hand(eng, scene["frames"], steps=8, gain=0.5)
    for b in (0, 1):
        assert [int(p) for p in stopped["steps"][b]["pixel"]] == [scene["strong"], -1, -1, -1]
        assert stopped["steps"][b][0].tobytes() == whole["steps"][b][0].tobytes() == one["steps"][b][0].tobytes()
        assert CU.same_bits(stopped["frames"][b], one["frames"][b]) and CU.same_bits(stopped["residual"][b], one["residual"][b])
        assert CU.same_bits(stopped["map"][b], one["map"][b])
    assert one["steps"].shape == (3, 1)
    assert_same_loop(half, half_by_hand, "gain 0.5")
    # with gain 0.5 the same two pixels carry everything above -25 dB after 8 steps (seen in the float32 prototype; here on the device)
    clean = half["clean"][0].astype(np.float64)
    above = np.flatnonzero(clean > clean.max() * 10.0 ** -2.5)
    print("gain 0.5: pixels above -25 dB", above, [PU.db(clean[p], clean.max()) for p in above])
    assert sorted(above) == sorted([scene["strong"], scene["weak"]])


# ------------------------------------------------------------------------------------------------ 5. stream order

@pytest.mark.parametrize("math_mode", ["exact", "fast"])
def test_peel_device_behind_pending_work(scenes, busy, math_mode):  # noqa: F811
    sc = scenes(16)
    outs = {"steps": ((4, 3, 3), np.int32), "clean": ((4, sc.P), np.float32), "residual": ((4, sc.P), np.float32), "map": ((4, sc.P), np.float32),
            "left": ((4, 64, 1024), np.float32)}
    case = H.Case(sc.engine(math_mode), {"frames": sc.frames}, outs,
                  lambda e, i, o, s: e.peel_device(i["frames"], 4, 3, 1.0, 0.0, o["steps"], o["clean"], o["residual"], o["map"], o["left"], s), variant=variant)
    got = check(case, busy)
    assert (got["steps"][:, :, 0] >= 0).all() and np.isfinite(got["map"]).all() and (got["clean"] > 0).any()


def test_peel_step_device_behind_pending_work(scenes, busy):  # noqa: F811
    sc = scenes(16)
    length = sc.pkg.peel_beam_length(64, 1024, sc.off, sc.frac)
    pixel = (np.array([0, 255, -1, 100], np.int32), np.array([7, -1, 3, 200], np.int32))
    case = H.Case(sc.engine(), {"frames": sc.frames, "pixel": pixel}, {"beams": ((4, length), np.float32)},
                  lambda e, i, o, s: e.peel_step_device(i["frames"], 4, i["pixel"], 0.5, o["beams"], s), inout=("frames",))
    got = check(case, busy)
    assert not got["beams"][2].any() and got["beams"][0].any()


# ------------------------------------------------------------------------------------------------ 6. refusals

def test_refusals_leave_the_handle_usable(pkg, scene):
    import torch

    B = pkg.binding
    off, frac = scene["off"], scene["frac"]
    frames = np.array(scene["frames"][:2])
    d_x = torch.from_numpy(frames.copy()).cuda()
    d_pix = torch.zeros(2, dtype=torch.int32, device="cuda")
    d_out = torch.full((2, 576), CANARY, dtype=torch.float32, device="cuda")
    d_p = torch.zeros((2, 576), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def refused(eng, status, usable=True):
        """All three forms answer `status`, write nothing, and the handle sweeps as before."""
        before = None
        if usable:
            eng.process_device(d_x.data_ptr(), 2, d_p.data_ptr())
            eng.synchronize()
            before = d_p.cpu().numpy()
        calls = (lambda: eng.peel_device(d_x.data_ptr(), 2, STEPS, d_map_ptr=d_out.data_ptr(), d_clean_ptr=d_out.data_ptr()),
                 lambda: eng.peel_step_device(d_x.data_ptr(), 2, d_pix.data_ptr(), 1.0),
                 lambda: eng.peel(frames, STEPS))
        for call in calls:
            with pytest.raises(B.AwpuError) as err:
                call()
            assert err.value.status == status, err.value
        torch.cuda.synchronize()
        assert CU.same_bits(d_x.cpu().numpy(), frames) and (d_out.cpu().numpy() == CANARY).all()
        if usable:
            eng.process_device(d_x.data_ptr(), 2, d_p.data_ptr())
            eng.synchronize()
            assert CU.same_bits(d_p.cpu().numpy(), before)

    with engine(pkg, off, frac, 64, 2, interp=B.INTERP_FIR8) as eng:
        refused(eng, B.ERR_STATE, usable=False)  # (no FIR table set: nothing to sweep with)
    with pkg.Engine(n_pixels=576, n_streams=64, max_batch=2, pixel_begin=288, pixel_count=288) as eng:  # a slab handle
        eng.set_delay_table(off[288:], frac[288:])
        eng.set_active_mics(None)
        refused(eng, B.ERR_STATE)
    with engine(pkg, off, frac, 64, 2) as eng:  # a band on the handle
        eng.set_band(B.band_design(6375, 9000, 31))
        refused(eng, B.ERR_STATE)
        eng.set_band(None)
        got = loop_on_device(eng, frames)
        assert got["steps"][0]["pixel"][0] == scene["strong"]
    with engine(pkg, off, frac, 64, 2, index=np.array([0, 1, 2, 1], np.int32)) as eng:  # a stream twice
        refused(eng, B.ERR_STATE)
    low = off - np.int32(off.min() - 20)  # min off 20 with E = 28: the step would read in front of the history
    with engine(pkg, low, frac, 64, 2) as eng:
        refused(eng, B.ERR_RANGE)
    with engine(pkg, off, frac, 64, 2) as eng:
        for bad in (dict(steps=0), dict(steps=33), dict(gain=0.0), dict(gain=1.5), dict(stop_ratio=1.0), dict(stop_ratio=-0.5)):
            kw = dict(steps=STEPS, gain=1.0, stop_ratio=0.0)
            kw.update(bad)
            with pytest.raises(B.AwpuError) as err:
                eng.peel_device(d_x.data_ptr(), 2, d_map_ptr=d_out.data_ptr(), **kw)
            assert err.value.status == B.ERR_INVALID, bad
            with pytest.raises(B.AwpuError) as err:
                eng.peel(frames, **kw)
            assert err.value.status == B.ERR_INVALID, bad
        for gamma in (0.0, 1.5):
            with pytest.raises(B.AwpuError) as err:
                eng.peel_step_device(d_x.data_ptr(), 2, d_pix.data_ptr(), gamma)
            assert err.value.status == B.ERR_INVALID
        for call in (lambda: eng.peel_device(0, 2, STEPS), lambda: eng.peel_step_device(0, 2, d_pix.data_ptr()), lambda: eng.peel_step_device(d_x.data_ptr(), 2, 0),
                     lambda: eng.peel_device(d_x.data_ptr(), 3, STEPS), lambda: eng.peel_device(d_x.data_ptr(), 0, STEPS)):
            with pytest.raises(B.AwpuError) as err:
                call()
            assert err.value.status == B.ERR_INVALID
        refused_nothing = d_out.cpu().numpy()
        assert (refused_nothing == CANARY).all() and CU.same_bits(d_x.cpu().numpy(), frames)
        got = loop_on_device(eng, frames)  # ... and the handle peels
        assert got["steps"][0]["pixel"][0] == scene["strong"]


def test_a_device_group_takes_no_peel(pkg, scene):
    import torch

    B = pkg.binding
    with pkg.Engine(n_pixels=576, n_streams=64, max_batch=2, grid_columns=24, devices=[0, 0]) as eng:
        eng.set_delay_table(scene["off"], scene["frac"])
        eng.set_active_mics(None)
        d_x = torch.from_numpy(np.array(scene["frames"][:2])).cuda()
        torch.cuda.synchronize()
        for call in (lambda: eng.peel_device(d_x.data_ptr(), 2, STEPS), lambda: eng.peel(scene["frames"][:2], STEPS)):
            with pytest.raises(B.AwpuError) as err:
                call()
            assert err.value.status == B.ERR_STATE


# ------------------------------------------------------------------------------------------------ 6. the runs

N_RUN, EVERY, BYTES = 5, 2, 256 * 1032


def run_outputs(n_frames, steps=STEPS):
    """Device outputs of a run, every one between guards of 64 elements: (raw tensors, pointers, fills)."""
    import torch

    outs = {"image": (n_frames * 1024, torch.uint8), "big": (n_frames * 50 * 43 * 3, torch.uint8), "power": (n_frames * 1024, torch.float32),
            "steps": (n_frames * steps * 3, torch.int32), "sources": (n_frames * 4 * 40, torch.uint8), "count": (n_frames, torch.int32)}
    fill = {"image": 0xA5, "big": 0xA5, "power": CANARY, "steps": -7, "sources": 0xA5, "count": -7}
    raw = {k: torch.full((n + 128,), fill[k], dtype=dt, device="cuda") for k, (n, dt) in outs.items()}
    ptr = {k: v.data_ptr() + 64 * v.element_size() for k, v in raw.items()}
    return raw, ptr, fill


def guarded(raw, fill):
    host = {k: v.cpu().numpy() for k, v in raw.items()}
    for k, v in host.items():
        assert (v[:64] == fill[k]).all() and (v[-64:] == fill[k]).all(), f"{k}: guard overwritten"
    return {k: v[64:-64] for k, v in host.items()}


@pytest.mark.parametrize("max_batch", [1, 4])
def test_run_forms_equal_the_composition(pkg, oracle, find_c1, max_batch):  # noqa: F811
    import torch

    B = pkg.binding
    off, frac, _, wire, samples = find_c1
    wire, samples = wire[:N_RUN * BYTES], np.ascontiguousarray(samples[:, :256 * N_RUN])
    first = 0
    n_frames = len(range(first, N_RUN, EVERY))
    table, d_table = colour_table()
    with run_engine(pkg, off, frac, 64, 32, max_batch) as ref:
        watched = ref.watch_samples(samples, 32, 32, first=first, every=EVERY, want_image=False, want_power=True)
        ring = ref.ring_snapshot()
    snaps = snapshots(samples, None)[first::EVERY]
    with run_engine(pkg, off, frac, 64, 32, 32) as own:
        peeled = own.peel(snaps, STEPS)
    # (block 0's snapshot holds nothing inside the table's window yet: a silent frame, no step; the others take every step)
    assert (peeled.steps["pixel"][0] == -1).all() and (peeled.steps["pixel"][1:] >= 0).all() and not CU.same_bits(peeled.map, watched.power)
    d_in = torch.from_numpy(samples).cuda()
    for show, rows in ((B.PEEL_MAP, peeled.map), (B.PEEL_CLEAN, peeled.clean), (B.PEEL_RESIDUAL, peeled.residual)):
        image, big = compose(pkg, oracle, rows, 32, 32, 50, 43, table, True)
        want = pkg.find_peaks(rows, 32, 32, **FIND)

        def check_run(got, eng):
            assert got.next_first == watched.next_first and len(got) == n_frames
            assert CU.same_bits(got.power, rows) and got.steps.tobytes() == peeled.steps.tobytes()
            assert np.array_equal(got.image, image) and np.array_equal(got.big, big)
            assert_equal_to_host(got.sources, got.count, want, (max_batch, show))
            assert np.array_equal(eng.ring_snapshot(), ring)
            assert eng.stats().frames == n_frames * (STEPS + 1)  # every sweep of the loop is counted

        kw = dict(first=first, every=EVERY, show=show, out_rows=50, out_cols=43, d_colormap_ptr=d_table.data_ptr(), flip=True, want_power=True, find=FIND)
        with run_engine(pkg, off, frac, 64, 32, max_batch) as eng:
            check_run(eng.peel_blocks(wire, 32, 32, STEPS, **kw), eng)
        with run_engine(pkg, off, frac, 64, 32, max_batch) as eng:
            check_run(eng.peel_samples(samples, 32, 32, STEPS, **kw), eng)
        with run_engine(pkg, off, frac, 64, 32, max_batch) as eng:  # the device form, every output between guards
            raw, ptr, fill = run_outputs(n_frames)
            torch.cuda.synchronize()
            nxt = eng.peel_samples_device(d_in.data_ptr(), samples.shape[1], N_RUN, 32, 32, STEPS, first=first, every=EVERY, show=show,
                                          d_image_ptr=ptr["image"], d_big_ptr=ptr["big"], d_power_ptr=ptr["power"], d_steps_ptr=ptr["steps"],
                                          d_sources_ptr=ptr["sources"], d_count_ptr=ptr["count"], out_rows=50, out_cols=43,
                                          d_colormap_ptr=d_table.data_ptr(), flip=True, find=FIND)
            eng.synchronize()
            assert nxt == watched.next_first
            host = guarded(raw, fill)
            assert CU.same_bits(host["power"].reshape(n_frames, 1024), rows)
            assert host["steps"].tobytes() == peeled.steps.tobytes()
            assert np.array_equal(host["image"].reshape(n_frames, 32, 32), image) and np.array_equal(host["big"].reshape(big.shape), big)
            assert_equal_to_host(host["sources"].copy().view(B.SOURCE_DTYPE).reshape(n_frames, 4), host["count"], want, "device")
            assert np.array_equal(eng.ring_snapshot(), ring)
    with run_engine(pkg, off, frac, 64, 32, max_batch) as eng:  # the steps alone
        alone = eng.peel_samples(samples, 32, 32, STEPS, every=EVERY, want_image=False)
        assert alone.power is None and alone.image is None and alone.sources is None and alone.steps.tobytes() == peeled.steps.tobytes()


def test_a_split_recording_equals_one_call(pkg, find_c1):  # noqa: F811
    import torch

    off, frac, _, wire, samples = find_c1
    samples = np.ascontiguousarray(samples[:, :256 * N_RUN])
    kw = dict(every=EVERY, want_image=True, want_power=True, find=FIND)
    with run_engine(pkg, off, frac, 64, 32, 4) as eng:
        whole = eng.peel_samples(samples, 32, 32, STEPS, first=0, **kw)
        ring = eng.ring_snapshot()
    with run_engine(pkg, off, frac, 64, 32, 4) as eng:
        a = eng.peel_samples(samples[:, :256 * 2], 32, 32, STEPS, first=0, **kw)
        b = eng.peel_blocks(wire[2 * BYTES:N_RUN * BYTES], 32, 32, STEPS, first=a.next_first, **kw)
        assert b.next_first == whole.next_first and len(a) + len(b) == len(whole) == 3
        for name in ("power", "image", "count", "steps", "sources"):
            assert np.concatenate([getattr(r, name) for r in (a, b)]).tobytes() == getattr(whole, name).tobytes(), name
        assert np.array_equal(eng.ring_snapshot(), ring)
    with run_engine(pkg, off, frac, 64, 32, 4) as eng:  # the device form split the same way
        d_in = torch.from_numpy(samples).cuda()
        raw, ptr, fill = run_outputs(3)
        torch.cuda.synchronize()
        nxt = eng.peel_samples_device(d_in.data_ptr(), samples.shape[1], 2, 32, 32, STEPS, every=EVERY, d_power_ptr=ptr["power"], d_steps_ptr=ptr["steps"])
        assert nxt == a.next_first
        nxt = eng.peel_samples_device(d_in.data_ptr() + 4 * 256 * 2, samples.shape[1], 3, 32, 32, STEPS, first=nxt, every=EVERY,
                                      d_power_ptr=ptr["power"] + 4 * 1024, d_steps_ptr=ptr["steps"] + 12 * STEPS)
        eng.synchronize()
        host = guarded({k: raw[k] for k in ("power", "steps")}, fill)
        assert nxt == whole.next_first and CU.same_bits(host["power"].reshape(3, 1024), whole.power) and host["steps"].tobytes() == whole.steps.tobytes()
        assert np.array_equal(eng.ring_snapshot(), ring)


def test_run_refusals_in_all_three_forms(pkg, find_c1):  # noqa: F811
    """What the handle forms refuse, the run forms refuse: nothing written, the ring as it was, and the handle watches as before."""
    import torch

    B = pkg.binding
    off, frac, _, wire, samples = find_c1
    wire, samples = wire[:N_RUN * BYTES], np.ascontiguousarray(samples[:, :256 * N_RUN])
    d_in = torch.from_numpy(samples).cuda()
    raw, ptr, fill = run_outputs(3)
    torch.cuda.synchronize()

    def refused(eng, status, usable=True, **bad):
        ring = eng.ring_snapshot() if usable else None
        kw = dict(steps=STEPS, every=EVERY, find=FIND)
        kw.update(bad)
        steps = kw.pop("steps")
        forms = (lambda: eng.peel_blocks(wire, 32, 32, steps, want_power=True, **kw), lambda: eng.peel_samples(samples, 32, 32, steps, want_power=True, **kw),
                 lambda: eng.peel_samples_device(d_in.data_ptr(), samples.shape[1], N_RUN, 32, 32, steps, d_image_ptr=ptr["image"], d_power_ptr=ptr["power"],
                                                 d_steps_ptr=ptr["steps"], d_sources_ptr=ptr["sources"], d_count_ptr=ptr["count"], **kw))
        for form in forms:
            with pytest.raises(B.AwpuError) as err:
                form()
            assert err.value.status == status, err.value
        torch.cuda.synchronize()
        guarded(raw, fill)
        for k, v in raw.items():
            assert (v.cpu().numpy() == fill[k]).all(), k
        if usable:
            assert np.array_equal(eng.ring_snapshot(), ring)

    with pkg.Engine(n_pixels=1024, n_streams=64, max_batch=4, interp=B.INTERP_FIR8) as eng:
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        refused(eng, B.ERR_STATE, usable=False)
    with pkg.Engine(n_pixels=1024, n_streams=64, max_batch=4, grid_columns=32, devices=[0, 0]) as eng:
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        refused(eng, B.ERR_STATE, usable=False)
    with pkg.Engine(n_pixels=1024, n_streams=64, max_batch=4, pixel_begin=512, pixel_count=512) as eng:  # a slab handle
        eng.set_delay_table(off[512:], frac[512:])
        eng.set_active_mics(None)
        refused(eng, B.ERR_STATE, usable=False)
    with run_engine(pkg, off, frac, 64, 32, 4) as eng:
        eng.watch_samples(samples[:, :512], 32, 32, want_image=False, want_power=True)  # (a ring to be left alone)
        eng.set_band(B.band_design(6375, 9000, 31))
        refused(eng, B.ERR_STATE)
        eng.set_band(None)
        eng.set_active_mics(np.array([0, 1, 2, 1], np.int32))
        refused(eng, B.ERR_STATE)
        eng.set_active_mics(None)
        eng.set_delay_table(off - np.int32(off.min() - 20), frac)  # the step would read in front of the history
        refused(eng, B.ERR_RANGE)
        eng.set_delay_table(off, frac)
        for bad in (dict(steps=0), dict(steps=33), dict(gain=0.0), dict(gain=1.5), dict(stop_ratio=1.0), dict(show=3), dict(show=-1)):
            refused(eng, B.ERR_INVALID, **bad)
        with run_engine(pkg, off, frac, 64, 32, 4) as ref:
            ref.watch_samples(samples[:, :512], 32, 32, want_image=False, want_power=True)
            want = ref.peel_samples(samples, 32, 32, STEPS, every=EVERY, want_power=True)
        got = eng.peel_samples(samples, 32, 32, STEPS, every=EVERY, want_power=True)  # ... and the handle peels a run
        assert CU.same_bits(got.power, want.power) and got.steps.tobytes() == want.steps.tobytes()
