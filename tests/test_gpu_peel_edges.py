"""Peeling on the device at the edges of its kernels (csrc/peel_kernels.hip): the shapes of tests/peel_edges.py, whose host-rule
answers tests/test_peel_edges_cpu.py pins against the numpy restatement.

1. The step at every mic count and beam length, plain and with gains: residual frames and beams equal awpu_hip_peel_step_host bit
   for bit, then a second step on the result; a batch of 70 frames; 256 mics pass, 257 are refused.
2. The exact fit in a moat of NaN: a read outside the frames would reach a beam, a write outside would change the moat; one
   sample either way is refused.  Pixels off the table skip their frames.  The beam holds the sweep's sums.
3. The loop: on small_shape() (a ragged list, gains with a 0) against the composition by hand and the host rule; tables of 1, 511,
   512, 513 and 4161 pixels; ties; 32 steps.
4. Value tiers 2^k in the step and the loop; bad samples in the step.
5. One handle through a change of table and of mic list and back: every result is a fresh handle's.

Everything is bit for bit but the loop against the host rule, which takes the 1e-5 rules of tests/test_gpu_peel.py."""
import numpy as np
import pytest

import cohere_util as CU
import peel_edges as PE
import peel_util as PU
import test_gpu_peel as TP  # (its loop-against-the-host-rule check is called as it stands: the project's 1e-5 rules, stated once)
import value_edges as V
from test_gpu_peel import CANARY, GUARD, assert_same_loop, engine, loop_by_hand, loop_on_device, step_on_device
from test_peel_cpu import SCENE_SEED, SECOND_SEED, small_shape

pytestmark = pytest.mark.gpu

STEPS = 4
INT32_MAX, INT32_MIN = np.iinfo(np.int32).max, np.iinfo(np.int32).min


def shape_engine(pkg, s, with_gain=False, max_batch=None, math_mode="exact", off=None):
    return engine(pkg, s["off"] if off is None else off, s["frac"], s["off"].shape[1], max_batch or len(s["frames"]), index=s["index"],
                  gains=PE.by_stream(s) if with_gain else None, math=pkg.MATH_F32_FAST if math_mode == "fast" else None)


def zero_bits(a) -> bool:
    return not CU.bits(a).any()


def check_step(pkg, eng, s, with_gain, frames, pixel, gamma=1.0, on_device=step_on_device, same=CU.same_bits):
    """One step on the device against the host rule: (frames after it, beams).  A frame without a pixel keeps its bits and gets a
    zero beam row."""
    gain = s["gain"] if with_gain else None
    want_frames, want_beams = pkg.peel_step_host(frames, s["off"], s["frac"], np.where(np.asarray(pixel) < 0, -1, pixel), gamma, index=s["index"], gain=gain)
    got_frames, got_beams = on_device(eng, frames, pixel, gamma, want_beams.shape[1])
    assert same(got_frames, want_frames), "frames"
    assert same(got_beams, want_beams), "beams"
    for b, p in enumerate(pixel):
        if p < 0:
            assert CU.same_bits(got_frames[b], frames[b]) and zero_bits(got_beams[b]), b
    return got_frames, got_beams


# ------------------------------------------------------------------------------------------------ 1. the step at every shape

@pytest.mark.parametrize("with_gain", [False, True], ids=["plain", "gains"])
@pytest.mark.parametrize("name", list(PE.SHAPES))
def test_step_equals_the_host_rule_at_every_shape(pkg, name, with_gain):
    s = PE.SHAPES[name]()
    with shape_engine(pkg, s, with_gain) as eng:
        left, _ = check_step(pkg, eng, s, with_gain, s["frames"], s["pixel"])
        assert not CU.same_bits(left[0], s["frames"][0]) and not CU.same_bits(left[-1], s["frames"][-1])
        # a second step on the residual, every frame with its neighbour's pixel: the kernel's reads see the first step's writes
        check_step(pkg, eng, s, with_gain, left, PE.rotated(s["pixel"]), 0.5)


@pytest.mark.parametrize("with_gain", [False, True], ids=["plain", "gains"])
@pytest.mark.parametrize("math_mode", ["exact", "fast"])
def test_step_on_a_batch_of_70_frames(pkg, math_mode, with_gain):
    """(With the gains of tests/peel_edges.py the seventeenth mic's is 0: it is the plain case that sees the beam pass's tail.)"""
    s = PE.mic_shape(17, n_frames=70)
    with shape_engine(pkg, s, with_gain, math_mode=math_mode) as eng:
        left, _ = check_step(pkg, eng, s, with_gain, s["frames"], s["pixel"])
        check_step(pkg, eng, s, with_gain, left, PE.rotated(s["pixel"]))


def assert_refused(pkg, eng, frames, status, beam_floats):
    """peel_device, peel_step_device and peel answer `status`, write nothing, and the handle sweeps the same bits before and after."""
    import torch

    B = pkg.binding
    batch, P = len(frames), eng.pixel_count
    d_x = torch.from_numpy(np.array(frames)).cuda()
    d_pix = torch.zeros(batch, dtype=torch.int32, device="cuda")
    d_out = torch.full((batch, max(P, 3 * STEPS)), CANARY, dtype=torch.float32, device="cuda")
    d_beams = torch.full((batch * beam_floats,), CANARY, dtype=torch.float32, device="cuda")
    d_p = torch.zeros((batch, P), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def sweep():
        eng.process_device(d_x.data_ptr(), batch, d_p.data_ptr())
        eng.synchronize()
        return d_p.cpu().numpy()

    before = sweep()
    calls = (lambda: eng.peel_device(d_x.data_ptr(), batch, STEPS, d_steps_ptr=d_out.data_ptr(), d_map_ptr=d_out.data_ptr(), d_clean_ptr=d_out.data_ptr(),
                                     d_residual_ptr=d_out.data_ptr()),
             lambda: eng.peel_step_device(d_x.data_ptr(), batch, d_pix.data_ptr(), 1.0, d_beams.data_ptr()),
             lambda: eng.peel(frames, STEPS))
    for call in calls:
        with pytest.raises(B.AwpuError) as err:
            call()
        assert err.value.status == status, err.value
    torch.cuda.synchronize()
    assert CU.same_bits(d_x.cpu().numpy(), frames) and (d_out.cpu().numpy() == CANARY).all() and (d_beams.cpu().numpy() == CANARY).all()
    assert CU.same_bits(sweep(), before)


def test_257_mics_are_refused(pkg):
    """AWPU_PEEL_MAX_MICS is 256 (the U256 shape above passes): one more is AWPU_ERR_STATE from every handle form."""
    s = PE.synthetic(300, 257, 30, 2, seed=7257)
    assert len(s["index"]) == pkg.binding.PEEL_MAX_MICS + 1
    with shape_engine(pkg, s) as eng:
        assert_refused(pkg, eng, s["frames"], pkg.binding.ERR_STATE, 258 + 2 * 30)


# ------------------------------------------------------------------------------------------------ 2. the range rule, pixels, sums

NAN_BITS = 0x7FC00000


def step_in_a_moat(eng, frames, pixel, gamma, length):
    """step_on_device with the frames inside a larger device buffer of NaN, GUARD floats either side, which must stay NaN."""
    import torch

    frames = np.ascontiguousarray(frames, np.float32)
    moat = np.full(frames.size + 2 * GUARD, np.uint32(NAN_BITS), np.uint32).view(np.float32)
    moat[GUARD:-GUARD] = frames.ravel()
    raw_x = torch.from_numpy(moat).cuda()
    d_pix = torch.from_numpy(np.asarray(pixel, np.int32)).cuda()
    raw = torch.full((len(frames) * length + 2 * GUARD,), CANARY, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.peel_step_device(raw_x.data_ptr() + 4 * GUARD, len(frames), d_pix.data_ptr(), gamma, raw.data_ptr() + 4 * GUARD)
    eng.synchronize()
    host, x = raw.cpu().numpy(), raw_x.cpu().numpy()
    assert (host[:GUARD] == CANARY).all() and (host[-GUARD:] == CANARY).all(), "beams: guard overwritten"
    assert (CU.bits(x[:GUARD]) == NAN_BITS).all() and (CU.bits(x[-GUARD:]) == NAN_BITS).all(), "the moat around the frames was written"
    return x[GUARD:-GUARD].reshape(frames.shape), host[GUARD:-GUARD].reshape(len(frames), length)


@pytest.mark.parametrize("with_gain", [False, True], ids=["plain", "gains"])
@pytest.mark.parametrize("E", [255, 128])
def test_step_in_a_moat_of_nan(pkg, E, with_gain):
    """E = 255: the table fits the history exactly -- the first frame's step reads sample 0 of stream 0, the last frame's sample
    1023 of stream 7 (tests/test_peel_edges_cpu.py), one float from the moat."""
    s = PE.beam_shape(E)
    with shape_engine(pkg, s, with_gain) as eng:
        left, beams = check_step(pkg, eng, s, with_gain, s["frames"], s["pixel"], on_device=step_in_a_moat)
        assert np.isfinite(left).all() and np.isfinite(beams).all()
        check_step(pkg, eng, s, with_gain, left, PE.rotated(s["pixel"]), on_device=step_in_a_moat)


@pytest.mark.parametrize("shift", [1, -1])
def test_the_exact_fit_shifted_by_one_is_refused(pkg, shift):
    s = PE.beam_shape(255)
    with shape_engine(pkg, s, off=s["off"] + np.int32(shift)) as eng:
        assert_refused(pkg, eng, s["frames"], pkg.binding.ERR_RANGE, 258 + 2 * 255)
    with shape_engine(pkg, s) as eng:  # (the handle that is refused differs from one that is not by the table alone)
        check_step(pkg, eng, s, False, s["frames"], s["pixel"])


def test_pixels_off_the_table_skip_their_frames(pkg):
    """d_pixel is not checked on the host (include/awpu_hip_peel.h): the kernel tests the pixel before it forms any address."""
    s = PE.mic_shape(17, n_frames=5)
    P = s["off"].shape[0]
    pixel = np.array([P, INT32_MAX, 2, -2, INT32_MIN], np.int32)
    with shape_engine(pkg, s) as eng:
        left, beams = check_step(pkg, eng, s, False, s["frames"], np.where((pixel >= 0) & (pixel < P), pixel, -1))  # (-1: as the header has it)
        got_left, got_beams = step_on_device(eng, s["frames"], pixel, 1.0, beams.shape[1])
    assert CU.same_bits(got_left, left) and CU.same_bits(got_beams, beams)
    for b in (0, 1, 3, 4):
        assert CU.same_bits(got_left[b], s["frames"][b]) and zero_bits(got_beams[b]), b
    assert not CU.same_bits(got_left[2], s["frames"][2]) and got_beams[2].any()


def test_the_beam_holds_the_sweeps_sums_on_the_device(pkg):
    """tests/test_peel_cpu.py::test_the_beam_holds_the_sweeps_sums with both sides from the device."""
    import torch

    s = small_shape()
    lo, length = PU.reach(s["off"], s["index"])
    with shape_engine(pkg, s, True) as eng:
        d_x = torch.from_numpy(np.array(s["frames"])).cuda()
        d_p = torch.zeros((3, 42), dtype=torch.float32, device="cuda")
        d_sums = torch.zeros((3, 42, 256), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        eng.process_device_sums(d_x.data_ptr(), 3, d_p.data_ptr(), d_sums.data_ptr())
        eng.synchronize()
        sums = d_sums.cpu().numpy()
        _, beams = step_on_device(eng, s["frames"], s["pixel"], 1.0, length)
    assert sums.any()
    for b in (0, 1):
        assert CU.same_bits(beams[b, -lo:-lo + 256], sums[b, s["pixel"][b]] * (np.float32(1.0) / np.float32(5))), b


# ------------------------------------------------------------------------------------------------ 3. the loop

@pytest.mark.parametrize("gain", [1.0, 0.5])
def test_loop_on_the_small_shape(pkg, gain):
    """5 of 8 mics in a shuffled list, gains with a 0 and a negative value: set_u's gain[index[s]] in the device loop.  The picks'
    preconditions: tests/test_peel_edges_cpu.py::test_the_picks_on_the_small_shape_are_well_apart."""
    s = small_shape()
    frames = s["frames"].copy()
    frames[2] = 0.0
    host = pkg.peel_host(frames, s["off"], s["frac"], 3, gain, 0.0, index=s["index"], gain=s["gain"])
    with shape_engine(pkg, s, True) as eng:
        got = loop_on_device(eng, frames, steps=3, gain=gain)
        assert_same_loop(got, loop_by_hand(eng, frames, steps=3, gain=gain))
    assert (got["steps"]["pixel"][:2] >= 0).all() and (got["steps"]["pixel"][2] == -1).all()
    TP.test_loop_against_the_host_rule(dict(host=host), (got,))  # identical picks, residual frames bit for bit, the 1e-5 rules; prints the errors
    assert CU.same_bits(got["frames"][:, 1], frames[:, 1]) and not CU.same_bits(got["frames"][:2, 6], frames[:2, 6])  # stream 1: gain 0; stream 6: 1.5
    with shape_engine(pkg, s, True, math_mode="fast") as eng:
        assert_same_loop(loop_on_device(eng, frames, steps=3, gain=gain), loop_by_hand(eng, frames, steps=3, gain=gain), "fast")


@pytest.fixture(scope="module")
def scene(pkg):
    """The scene's table and batch (the scene, a second seed, silence), left unchanged."""
    off, frac = PU.scene_table(pkg)
    frames = np.stack([PU.scene_frame(off, frac, SCENE_SEED), PU.scene_frame(off, frac, SECOND_SEED), np.zeros((64, 1024), np.float32)])
    for a in (off, frac, frames):
        a.setflags(write=False)
    return dict(off=off, frac=frac, frames=frames)


def scene_engine(pkg, off, frac, max_batch=3, math_mode="exact"):
    return engine(pkg, off, frac, 64, max_batch, math=pkg.MATH_F32_FAST if math_mode == "fast" else None)


@pytest.mark.parametrize("n_pixels", [1, 511, 512, 513, 4161])
def test_pick_at_table_sizes(pkg, scene, n_pixels):
    """The pick's strided maximum: one pixel; one trip of the 512 threads less one, exactly, and one more; 4161 pixels -- the scene
    table's rows repeated, so that threads make nine trips (the loop is unrolled by eight) and every power is there seven times
    over: the pick is the first of them."""
    rows = np.arange(n_pixels) % 576
    off, frac = scene["off"][rows], scene["frac"][rows]
    with scene_engine(pkg, off, frac, 2) as eng:
        got = loop_on_device(eng, scene["frames"][:2], steps=2)
        assert_same_loop(got, loop_by_hand(eng, scene["frames"][:2], steps=2))
    assert (got["steps"]["pixel"] >= 0).all() and (got["steps"]["pixel"] < min(n_pixels, 576)).all(), got["steps"]["pixel"]
    if n_pixels >= 576:
        assert (got["steps"]["pixel"][:, 0] == PE.STRONG).all()


@pytest.mark.parametrize("at,first", [((5, 570), 5), ((301, 3), 3)])
def test_a_tie_goes_to_the_lower_index(pkg, scene, at, first):
    """Three pixels with the strong pixel's table row: equal power bits, so the order's second key decides (power bits, then the
    lower index).  (5, 570): the lowest index in the first trip of the maximum, the highest in the second; (301, 3): the lowest in
    another wave than the pixel that holds the maximum without a tie."""
    import torch

    off, frac = PE.tied_table(scene["off"], scene["frac"], at)
    tied = sorted(at + (PE.STRONG,))
    with scene_engine(pkg, off, frac) as eng:
        d_x = torch.from_numpy(np.array(scene["frames"])).cuda()
        d_p = torch.zeros((3, 576), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        eng.process_device(d_x.data_ptr(), 3, d_p.data_ptr())
        eng.synchronize()
        row = d_p.cpu().numpy()
        for b in (0, 1):  # the device's own first row: were these bits not equal, the sweep would depend on where a pixel lies
            assert len({int(v) for v in CU.bits(row[b, tied])}) == 1 and row[b].argmax() == first, (b, row[b, tied])
        got = loop_on_device(eng, scene["frames"])
        assert_same_loop(got, loop_by_hand(eng, scene["frames"]))
    host = pkg.peel_host(scene["frames"], off, frac, STEPS)
    for b in (0, 1):
        assert [int(p) for p in got["steps"][b]["pixel"]] == [first, PE.WEAK, first, int(host.steps[b]["pixel"][3])], got["steps"][b]
    assert np.array_equal(got["steps"]["pixel"], host.steps["pixel"])


def test_32_steps(pkg, scene):
    with scene_engine(pkg, scene["off"], scene["frac"]) as eng:
        got = loop_on_device(eng, scene["frames"], steps=32, gain=0.1)
        assert_same_loop(got, loop_by_hand(eng, scene["frames"], steps=32, gain=0.1))
    assert got["steps"].shape == (3, 32) and (got["steps"]["pixel"][:2] >= 0).all() and (got["steps"]["before"][:2] > 0).all()
    assert (got["steps"]["pixel"][2] == -1).all() and zero_bits(got["steps"]["before"][2]) and zero_bits(got["steps"]["removed"][2])
    assert got["steps"][0]["pixel"][0] == PE.STRONG and PE.WEAK in got["steps"][0]["pixel"]


# ------------------------------------------------------------------------------------------------ 4. value tiers

@pytest.fixture(scope="module", params=[False, True], ids=["plain", "gains"])
def tier_shape(pkg, request):
    """The U = 17 shape, plain (the seventeenth mic is the beam pass's tail) and with gains (u = gamma / g; that mic's gain is 0),
    its handle, and the device's own step of the unscaled frames."""
    s = PE.mic_shape(17)
    with shape_engine(pkg, s, request.param) as eng:
        yield s, eng, request.param, check_step(pkg, eng, s, request.param, s["frames"], s["pixel"], 0.5)


@pytest.mark.parametrize("k", [-120, -64, 55, 120])
def test_step_at_a_value_tier(pkg, tier_shape, k):
    assert not V.host_flushes()
    s, eng, with_gain, (left0, beams0) = tier_shape
    frames = V.scale_pow2(s["frames"], k)
    left, beams = check_step(pkg, eng, s, with_gain, frames, s["pixel"], 0.5)
    if k == -120:  # partly subnormal samples, partly subnormal beams: a kernel that flushed either would differ from the host rule
        assert V.subnormal(frames).any() and V.subnormal(beams).any() and V.subnormal(left).any() and (np.abs(beams) >= V.TINY).any()
    if k > 0:  # exactly 2^k times the device's own unscaled result, and finite
        assert V.same_bits(left, V.scale_pow2(left0, k)) and V.same_bits(beams, V.scale_pow2(beams0, k))
        assert np.isfinite(left).all() and np.isfinite(beams).all()


def test_step_on_negative_zeros(pkg, tier_shape):
    s, eng, with_gain, _ = tier_shape
    frames = s["frames"].copy()
    frames[0] = -0.0
    frames[2, s["index"][1]] = -0.0
    left, beams = check_step(pkg, eng, s, with_gain, frames, s["pixel"])
    assert not left[0].any() and not beams[0].any()


def test_step_with_bad_samples(pkg, tier_shape):
    """+inf, NaN and a 3e38 / -3e38 pair (its difference overflows) at the lowest sample that pixel 0 reads of a mic and pixel P - 1
    does not: the first frame's step meets them, the last frame's does not."""
    s, eng, with_gain, _ = tier_shape
    off, index = s["off"], s["index"]
    lo, length = PU.reach(off, index)
    first, last = int(s["pixel"][0]), int(s["pixel"][-1])
    mics = [int(m) for m in index if off[last, m] >= off[first, m] + 2][:3]
    assert len(mics) == 3
    frames = s["frames"].copy()
    for m, what in zip(mics, ("inf", "nan", "overflow")):
        t = off[first, m] + lo  # X[o + lo]: the first sample the step reads
        frames[:, m, t:t + len(V.BAD[what])] = V.BAD[what]
        assert t + len(V.BAD[what]) - 1 < off[last, m] + lo
    left, beams = check_step(pkg, eng, s, with_gain, frames, s["pixel"], same=V.same_nonfinite)
    assert not np.isfinite(beams[0]).all() and not np.isfinite(left[0, index]).all(axis=1).any()  # every active mic of frame 0 got some of it
    clean_left, clean_beams = check_step(pkg, eng, s, with_gain, s["frames"], s["pixel"])
    bad = ~np.isfinite(frames[-1]) | (np.abs(frames[-1]) > 2)
    assert bad.sum() == 4 and np.isfinite(beams[-1]).all()
    assert CU.same_bits(beams[-1], clean_beams[-1]) and CU.same_bits(left[-1][~bad], clean_left[-1][~bad]) and CU.same_bits(left[-1][bad], frames[-1][bad])
    assert CU.same_bits(left[1], frames[1])  # (the frame without a pixel)


@pytest.fixture(scope="module")
def scene_handle(pkg, scene):
    """An exact-math handle on the scene table, and the solo runs of the batch's second and third frame."""
    with scene_engine(pkg, scene["off"], scene["frac"]) as eng:
        yield eng, [loop_on_device(eng, scene["frames"][b:b + 1]) for b in (1, 2)]


def first_row(eng, frame):
    import torch

    d_x = torch.from_numpy(np.array(frame[None])).cuda()
    d_p = torch.zeros((1, eng.pixel_count), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.process_device(d_x.data_ptr(), 1, d_p.data_ptr())
    eng.synchronize()
    return d_p.cpu().numpy()[0]


@pytest.mark.parametrize("k", [-64, 120, 57])
def test_loop_at_a_value_tier(pkg, scene, scene_handle, k):
    assert not V.host_flushes()
    eng, solo = scene_handle
    if k == 57:  # some powers +inf: which ones depends on the order of the sum of squares, so on the device's own row
        for k in (57, 58, 56, 59):
            row = first_row(eng, V.scale_pow2(scene["frames"][0], k))
            if np.isposinf(row).any() and np.isfinite(row).any():
                break
        print("k", k, "+inf pixels of the device's first row", np.flatnonzero(np.isposinf(row)))
        assert np.isposinf(row).any() and np.isfinite(row).any() and not np.isnan(row).any()
    frames = np.array(scene["frames"])
    frames[0] = V.scale_pow2(frames[0], k)
    got = loop_on_device(eng, frames)
    assert_same_loop(got, loop_by_hand(eng, frames))
    for b, alone in ((1, solo[0]), (2, solo[1])):  # the other frames of the batch: the bits of their solo runs
        assert got["steps"][b].tobytes() == alone["steps"][0].tobytes(), b
        for name in ("clean", "residual", "map", "frames"):
            assert CU.same_bits(got[name][b], alone[name][0]), (b, name)
    st = got["steps"][0]
    print("k", k, "steps", st)
    if k == -64:
        host = pkg.peel_host(frames[:1], scene["off"], scene["frac"], STEPS)
        assert np.array_equal(st["pixel"], host.steps[0]["pixel"]) and list(st["pixel"][:3]) == [PE.STRONG, PE.WEAK, PE.STRONG]
        assert V.subnormal(st["before"]).all() and V.subnormal(st["removed"]).all() and V.subnormal(got["residual"][0]).all()
        assert CU.same_bits(got["frames"][0], host.frames[0])
    elif k == 120:
        assert (st["pixel"] == -1).all() and zero_bits(st["before"]) and zero_bits(st["removed"])
        assert CU.same_bits(got["frames"][0], frames[0]) and np.isposinf(got["residual"][0]).all() and zero_bits(got["clean"][0])
    else:
        assert (st["pixel"] >= 0).all() and np.isfinite(st["before"]).all() and (st["before"] > 0).all()
        assert not np.isposinf(row[st["pixel"][0]]) and st["before"][0] == row[np.isfinite(row)].max()


# ------------------------------------------------------------------------------------------------ 5. handle state

def two_reach_shape():
    """An E = 128 table of the scene's size (576 pixels, 64 streams) whose first 32 streams span 60 samples only: the list of those
    has another reach (len 378) than the whole (len 514)."""
    s = PE.synthetic(64, 64, 128, 576, seed=9128, shuffled=False)
    base = int(s["off"].min())
    s["off"][:, :32] = np.clip(s["off"][:, :32], base + 30, base + 90)
    short = np.arange(31, -1, -1, dtype=np.int32)
    assert PU.reach(s["off"], s["index"])[1] == 514 and PU.reach(s["off"], short)[1] == 378
    return s, short


@pytest.mark.parametrize("math_mode", ["exact", "fast"])
def test_one_handle_through_tables_and_lists(pkg, scene, math_mode):
    """The reach is cached per table generation (peel_gen), a fast-math handle's step table (d_cohere_lut) per prepare(): peel,
    change the table, peel, change the list, peel, and back -- every result is that of a handle that has seen nothing else."""
    s, short = two_reach_shape()
    batch = scene["frames"][:2]

    def stage(eng, frames, pixel, length):
        return step_on_device(eng, frames, pixel, 0.5, length), loop_on_device(eng, frames, steps=2)

    def same_stage(got, want, where):
        assert CU.same_bits(got[0][0], want[0][0]) and CU.same_bits(got[0][1], want[0][1]), where
        assert_same_loop(got[1], want[1], where)

    scene_pixel = np.array([PE.STRONG, -1], np.int32)
    scene_len = PU.reach(scene["off"], np.arange(64))[1]
    want = {}
    with scene_engine(pkg, scene["off"], scene["frac"], 3, math_mode) as fresh:
        want["scene"] = stage(fresh, batch, scene_pixel, scene_len)
    with scene_engine(pkg, s["off"], s["frac"], 3, math_mode) as fresh:
        want["table"] = stage(fresh, s["frames"], s["pixel"], 514)
    with engine(pkg, s["off"], s["frac"], 64, 3, index=short, math=pkg.MATH_F32_FAST if math_mode == "fast" else None) as fresh:
        want["list"] = stage(fresh, s["frames"], s["pixel"], 378)
    assert not CU.same_bits(want["table"][0][0], want["list"][0][0])
    with scene_engine(pkg, scene["off"], scene["frac"], 3, math_mode) as eng:
        same_stage(stage(eng, batch, scene_pixel, scene_len), want["scene"], "the scene")
        eng.set_delay_table(s["off"], s["frac"])
        same_stage(stage(eng, s["frames"], s["pixel"], 514), want["table"], "another table")
        eng.set_active_mics(short)
        same_stage(stage(eng, s["frames"], s["pixel"], 378), want["list"], "a shorter list")
        eng.set_active_mics(None)
        eng.set_delay_table(scene["off"], scene["frac"])
        same_stage(stage(eng, batch, scene_pixel, scene_len), want["scene"], "the scene again")
