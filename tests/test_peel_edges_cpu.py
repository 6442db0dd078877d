"""The peel edge shapes (tests/peel_edges.py) on a box without a GPU: what tests/test_gpu_peel_edges.py compares the kernels
with is itself pinned here.

1. At every shape awpu_hip_peel_step_host equals the numpy restatement (peel_util.step) bit for bit, frames and beams, and the
   beam is 258 + 2 E long; the exact fit reads history samples 0 and hist - 1, and a table one sample either way is refused.
2. Ties: three pixels with the bits of the strongest power; the loop takes the lowest index.
3. Value tiers 2^k (tests/value_edges.py): the step and the loop against the restatement with subnormal beams (k = -120) and
   subnormal powers (k = -64); exact scaling at k = 55 and 120; every power +inf (k = 120) and some (k = 57).
4. The picks of the host loop on small_shape() are far enough apart for a device loop to be compared with them."""
import numpy as np
import pytest

import cohere_util as CU
import peel_edges as PE
import peel_util as PU
import value_edges as V
from test_peel_cpu import SCENE_SEED, small_shape

STEPS = 4
SCENE_PICKS = [PE.STRONG, PE.WEAK, PE.STRONG, 225]


# ------------------------------------------------------------------------------------------------ 1. the shapes

@pytest.mark.parametrize("with_gain", [False, True], ids=["plain", "gains"])
@pytest.mark.parametrize("name", list(PE.SHAPES))
def test_step_host_equals_the_restatement_at_every_shape(pkg, name, with_gain):
    s = PE.SHAPES[name]()
    E = PE.reach_of(s)
    n_streams, hist = s["frames"].shape[1:]
    gain = s["gain"] if with_gain else None
    assert pkg.peel_beam_length(n_streams, hist, s["off"], s["frac"], s["index"]) == 258 + 2 * E
    assert E == (int(name[1:]) if name[0] == "E" else 30 if name == "U256" else 40) and len(s["index"]) == (int(name[1:]) if name[0] == "U" else 8)
    for gamma in (1.0, 0.5):
        left, beams = pkg.peel_step_host(s["frames"], s["off"], s["frac"], s["pixel"], gamma, index=s["index"], gain=gain)
        assert beams.shape == (len(s["frames"]), 258 + 2 * E)
        for b, p in enumerate(s["pixel"]):
            want_frame, want_beam = PU.step(s["frames"][b], s["off"], s["frac"], int(p), gamma, s["index"], gain)
            assert CU.same_bits(left[b], want_frame) and CU.same_bits(beams[b], want_beam), (b, gamma)
            if p < 0:
                assert CU.same_bits(left[b], s["frames"][b]) and not beams[b].any()
            else:
                assert not CU.same_bits(left[b], s["frames"][b])


def test_the_shapes_are_what_they_claim():
    for name, make in PE.SHAPES.items():
        s = make()
        P, n_streams = s["off"].shape
        assert s["pixel"][0] == 0 and s["pixel"][-1] == P - 1 and (s["pixel"] == -1).any(), name
        assert len(set(s["index"].tolist())) == len(s["index"]) and s["index"].max() < n_streams
        assert (s["frac"][0] == 0).any() and (s["frac"][0] == 1).any() and ((s["frac"][0] > 0) & (s["frac"][0] < 1)).any()
        assert list(s["gain"][:5]) == list(np.array(PE.GAINS, np.float32)[:len(s["gain"])])
    assert sorted(len(PE.mic_shape(U)["index"]) for U in PE.MIC_COUNTS) == sorted(PE.MIC_COUNTS)
    assert (PE.beam_shape(0)["off"] == PE.beam_shape(0)["off"][0, 0]).all()  # every offset equal
    big = PE.mic_shape(17, n_frames=70)
    assert big["frames"].shape == (70, 40, 1024) and set(big["pixel"].tolist()) == {-1, 0, 1, 2, 3, 4}


def test_the_exact_fit_reads_both_ends_of_the_history(pkg):
    """From the table: the first frame's pixel reads sample 0 at stream 0, the last frame's sample hist - 1 at the last stream; one
    sample either way is refused."""
    s = PE.beam_shape(255)
    off, index, hist = s["off"], s["index"], s["frames"].shape[2]
    lo, length = PU.reach(off, index)
    assert list(index) == list(range(8)) and off.min() == 256 and off.max() == 511 and (lo, length) == (-256, 768)
    first, last = int(s["pixel"][0]), int(s["pixel"][-1])
    assert off[first, 0] + lo == 0                        # the lowest sample read: X[o + lo]
    assert off[last, 7] + lo + length == hist - 1 == 1023  # the highest: X[o + hi + 1]
    B = pkg.binding
    for shift in (1, -1):
        with pytest.raises(B.AwpuError) as err:
            pkg.peel_step_host(s["frames"], off + np.int32(shift), s["frac"], s["pixel"], index=index)
        assert err.value.status == B.ERR_RANGE
        with pytest.raises(B.AwpuError) as err:
            pkg.peel_host(s["frames"], off + np.int32(shift), s["frac"], 2, index=index)
        assert err.value.status == B.ERR_RANGE
    # ... and the step does write both ends: they differ from the input afterwards
    left, _ = pkg.peel_step_host(s["frames"], off, s["frac"], s["pixel"], index=index)
    assert left[0, 0, 1] != s["frames"][0, 0, 1] and left[-1, 7, 1022] != s["frames"][-1, 7, 1022]
    assert left[0, 0, 0] == s["frames"][0, 0, 0] and left[-1, 7, 1023] == s["frames"][-1, 7, 1023]  # read, never written (i + 1 = lo + 1 .. hi)


# ------------------------------------------------------------------------------------------------ the scene

@pytest.fixture(scope="module")
def scene(pkg):
    off, frac = PU.scene_table(pkg)
    frame = PU.scene_frame(off, frac, SCENE_SEED)
    for a in (off, frac, frame):
        a.setflags(write=False)
    return dict(off=off, frac=frac, frame=frame)


def by_hand(pkg, frame, off, frac, steps=STEPS):
    """The host loop driven through the host sweep and the host step: every row the loop picks from."""
    return PU.loop(frame, lambda f: pkg.cohere_host(f, off, frac)[0], lambda f, p: pkg.peel_step_host(f[None], off, frac, [p])[0][0], steps)


# ------------------------------------------------------------------------------------------------ 2. ties

def test_a_tie_goes_to_the_lower_index(pkg, scene):
    plain = pkg.peel_host(scene["frame"][None], scene["off"], scene["frac"], STEPS)
    assert [int(p) for p in plain.steps[0]["pixel"]] == SCENE_PICKS
    off, frac = PE.tied_table(scene["off"], scene["frac"])
    first = pkg.cohere_host(scene["frame"], off, frac)[0]
    assert len({int(b) for b in CU.bits(first[[5, PE.STRONG, 570]])}) == 1 and PU.pick(first) == 5
    got = pkg.peel_host(scene["frame"][None], off, frac, STEPS)
    assert [int(p) for p in got.steps[0]["pixel"]] == [5, PE.WEAK, 5, 225]
    # the tied pixels are the same direction: the steps' powers and the residual frames are those of the untouched table
    assert CU.same_bits(got.steps[0]["before"], plain.steps[0]["before"]) and CU.same_bits(got.steps[0]["removed"], plain.steps[0]["removed"])
    assert CU.same_bits(got.frames, plain.frames)
    # the lowest index in another place: rows 301 and 3
    off, frac = PE.tied_table(scene["off"], scene["frac"], at=(301, 3))
    got = pkg.peel_host(scene["frame"][None], off, frac, STEPS)
    assert got.steps[0]["pixel"][0] == 3


# ------------------------------------------------------------------------------------------------ 3. value tiers

def step_both(pkg, s, frames, with_gain, gamma=1.0):
    """(frames, beams) of the host rule, checked against the restatement."""
    gain = s["gain"] if with_gain else None
    left, beams = pkg.peel_step_host(frames, s["off"], s["frac"], s["pixel"], gamma, index=s["index"], gain=gain)
    for b, p in enumerate(s["pixel"]):
        want_frame, want_beam = PU.step(frames[b], s["off"], s["frac"], int(p), gamma, s["index"], gain)
        assert V.same_bits(left[b], want_frame) and V.same_bits(beams[b], want_beam), b
    return left, beams


@pytest.mark.parametrize("with_gain", [False, True], ids=["plain", "gains"])
@pytest.mark.parametrize("k", [-120, -64, 55, 120])
def test_step_tiers_against_the_restatement(pkg, k, with_gain):
    """(With the gains of tests/peel_edges.py the seventeenth mic's is 0: both cases, as on the device.)"""
    assert not V.host_flushes()
    s = PE.mic_shape(17)
    frames = V.scale_pow2(s["frames"], k)
    left, beams = step_both(pkg, s, frames, with_gain, 0.5)
    if k == -120:  # the samples are partly subnormal, the beams too: an implementation that flushed them would differ
        assert V.subnormal(frames).any() and V.subnormal(beams).any() and (np.abs(beams) >= V.TINY).any()
    if k > 0:  # exactly 2^k times the unscaled result, and finite
        left0, beams0 = step_both(pkg, s, s["frames"], with_gain, 0.5)
        assert V.same_bits(left, V.scale_pow2(left0, k)) and V.same_bits(beams, V.scale_pow2(beams0, k))
        assert np.isfinite(left).all() and np.isfinite(beams).all()


@pytest.mark.parametrize("with_gain", [False, True], ids=["plain", "gains"])
def test_step_on_negative_zeros(pkg, with_gain):
    assert not V.host_flushes()
    s = PE.mic_shape(17)
    frames = s["frames"].copy()
    frames[0] = -0.0
    frames[2, s["index"][1]] = -0.0
    step_both(pkg, s, frames, with_gain)


@pytest.mark.parametrize("k", [-120, -64, 55, 120])
def test_loop_tiers_against_the_restatement(pkg, k):
    """The loop on small_shape() scaled: the host rule equals the numpy restatement, sweep and step, bit for bit."""
    assert not V.host_flushes()
    s = small_shape()
    frames = V.scale_pow2(s["frames"], k)
    got = pkg.peel_host(frames, s["off"], s["frac"], 3, index=s["index"], gain=s["gain"])
    for b in range(3):
        want = PU.loop(frames[b], lambda f: CU.rule(f, s["off"], s["frac"], s["index"], s["gain"])[0],
                       lambda f, p: PU.step(f, s["off"], s["frac"], p, 1.0, s["index"], s["gain"])[0], 3)
        assert PU.steps_equal(got.steps[b], want["steps"]), (b, got.steps[b], want["steps"])
        for name in ("clean", "residual", "map"):
            assert V.same_bits(getattr(got, name)[b], want[name]), (b, name)
        assert V.same_bits(got.frames[b], want["frame"]), b
    if k == 120:  # every power +inf: nothing to pick, the frames untouched
        assert (got.steps["pixel"] == -1).all() and np.isposinf(got.residual).all() and not got.clean.any() and V.same_bits(got.frames, frames)
    elif k == -120:  # every power 0
        assert (got.steps["pixel"] == -1).all() and not got.residual.any() and V.same_bits(got.frames, frames)
    else:
        assert (got.steps["pixel"] >= 0).all()
    if k == -64:
        assert V.subnormal(got.steps["before"]).all() and V.subnormal(got.residual).all()


def test_scene_with_subnormal_powers(pkg, scene):
    """k = -64: the picks of the unscaled scene; every power the loop handles is subnormal and none 0."""
    assert not V.host_flushes()
    frame = V.scale_pow2(scene["frame"], -64)
    got = pkg.peel_host(frame[None], scene["off"], scene["frac"], STEPS)
    assert [int(p) for p in got.steps[0]["pixel"]] == SCENE_PICKS
    for name in ("before", "removed"):
        assert V.subnormal(got.steps[0][name]).all(), (name, got.steps[0][name])
    assert V.subnormal(got.residual).all() and V.subnormal(got.map).all()


@pytest.mark.parametrize("k", [55, 120])
def test_scene_step_scales_exactly(pkg, scene, k):
    assert not V.host_flushes()
    pixel = [PE.STRONG]
    left0, beams0 = pkg.peel_step_host(scene["frame"][None], scene["off"], scene["frac"], pixel)
    left, beams = pkg.peel_step_host(V.scale_pow2(scene["frame"], k)[None], scene["off"], scene["frac"], pixel)
    assert V.same_bits(left, V.scale_pow2(left0, k)) and V.same_bits(beams, V.scale_pow2(beams0, k))
    assert np.isfinite(left).all() and np.isfinite(beams).all()


def test_scene_with_every_power_infinite(pkg, scene):
    """k = 120: no finite pick, no step, the frames untouched."""
    frame = V.scale_pow2(scene["frame"], 120)
    assert np.isfinite(frame).all()
    got = pkg.peel_host(frame[None], scene["off"], scene["frac"], STEPS)
    assert (got.steps["pixel"] == -1).all() and not got.steps["before"].any() and not got.steps["removed"].any()
    assert np.isposinf(got.residual).all() and np.isposinf(got.map).all() and not got.clean.any() and V.same_bits(got.frames[0], frame)


def test_scene_with_some_powers_infinite(pkg, scene):
    """k = 57: the first row holds +inf and finite pixels; no step picks a pixel whose power is +inf in the row it is picked from
    (measured: 5 pixels of the first row are +inf; the picks are 275, 325, 226, 137)."""
    frame = V.scale_pow2(scene["frame"], 57)
    want = by_hand(pkg, frame, scene["off"], scene["frac"])
    first = want["rows"][0]
    print("+inf pixels of the first row", np.flatnonzero(np.isposinf(first)), "picks", [s[0] for s in want["steps"]])
    assert np.isposinf(first).any() and np.isfinite(first).any() and not np.isnan(first).any()
    picks = [s[0] for s in want["steps"]]
    assert all(p >= 0 for p in picks)
    for k, p in enumerate(picks):
        row = want["rows"][k]
        assert np.isfinite(row[p]) and row[p] == np.where(np.isfinite(row), row, 0).max(), (k, p)
    assert np.isposinf(first[PE.STRONG]) and PE.STRONG not in picks[:1]
    got = pkg.peel_host(frame[None], scene["off"], scene["frac"], STEPS)
    assert PU.steps_equal(got.steps[0], want["steps"]) and V.same_bits(got.frames[0], want["frame"])


# ------------------------------------------------------------------------------------------------ 4. the picks on small_shape()

@pytest.mark.parametrize("gamma", [1.0, 0.5])
def test_the_picks_on_the_small_shape_are_well_apart(pkg, gamma):
    """test_gpu_peel_edges.py compares the device loop's picks on small_shape() with the host rule's: at every pick the best and
    the second-best power differ by more than 1e-4 relative (measured: 6e-3 at the least)."""
    s = small_shape()
    worst = np.inf
    for b in (0, 1):
        want = PU.loop(s["frames"][b], lambda f: pkg.cohere_host(f, s["off"], s["frac"], index=s["index"], gain=s["gain"])[0],
                       lambda f, p: pkg.peel_step_host(f[None], s["off"], s["frac"], [p], gamma, index=s["index"], gain=s["gain"])[0][0], 3)
        assert all(st[0] >= 0 for st in want["steps"])
        for row in want["rows"][:-1]:
            top = np.sort(row.astype(np.float64))[-2:]
            gap = (top[1] - top[0]) / top[1]
            worst = min(worst, gap)
            assert gap > 1e-4, (b, top)
    print("gain", gamma, "smallest gap between the best two powers", worst)
