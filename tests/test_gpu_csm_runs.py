"""Step 6a of include/awpu_hip_csm.h on the device, the loaded inverse with a written arithmetic (1 to 3), and the cross-spectral
runs on top of it (include/awpu_hip_csm_watch.h; 4 to 10, listed where they begin).

1. csm_invert_device equals csm_invert_rule_host bit for bit, the solved words included: the mic lists one, two, ragged 5 of 8, 64
   and 65 of 128 with 1 and 8 bins (the factor kernel's triangle in LDS, 16 x 16 and 32 x 32 threads), 95 and 96 of 96 (the last
   size in LDS and the first in the scratch), 257 of 320 with 2 bins; matrices from csm_accumulate_host of seeded noise with more
   blocks than mics, one with fewer blocks than mics and loading > 0, and an unsolved bin among solved ones; guards intact.
2. The synchronous csm_invert: the same bits; an unsolved bin gives AWPU_ERR_RANGE with the output untouched; more than 512 active
   mics give AWPU_ERR_RANGE; the state refusals of the cross-spectral calls.
3. Stream order: csm_invert_device behind pending work on its stream (tests/stream_order.py).
The inverse at 511 and 512 mics, its bound, and runs on lists of 545 and 512 mics with the runs' range refusals (11):
test_gpu_csm_large.py, with this file's lists, helpers and rig."""
import ctypes as C

import numpy as np
import pytest

import csm_util as CU
import stream_order as H
from test_gpu_stream_order import busy, check, scenes  # noqa: F401

pytestmark = pytest.mark.gpu

GUARD = 64
CANARY = np.float32(-3.0)
LOADING = 1e-2
EIGHT = [0, 3, 16, 47, 100, 101, 127, 128]
# name -> (n_streams, active list)
MICS = {"one_mic": (8, [3]),
        "two_mics": (8, [5, 2]),
        "ragged5": (8, [6, 1, 3, 0, 7]),
        "sixty_four": (64, list(range(64))),
        "sixty_five_of_128": (128, list(range(0, 128, 2)) + [127]),
        "ninety_five_of_96": (96, [i for i in range(96) if i != 40]),
        "ninety_six": (96, list(range(96))),
        "two_fifty_seven_of_320": (320, [i for i in range(320) if i % 5 != 4] + [319]),
        # test_gpu_csm_large.py's: the bound of the inverse, and one below it on a ragged list
        "five_eleven_of_512": (512, [i for i in range(512) if i != 300]),
        "five_twelve": (512, list(range(512)))}


def engine_of(pkg, name, **kw):
    """A handle with the list's streams, a two-pixel table (the inverse reads none of it) and the active list."""
    S, index = MICS[name]
    rng = np.random.default_rng(len(index))
    eng = pkg.Engine(n_pixels=2, n_streams=S, **kw)
    eng.set_delay_table(rng.integers(0, 700, (2, S)).astype(np.int32), rng.random((2, S)).astype(np.float32))
    eng.set_active_mics(np.asarray(index, np.int32))
    return eng


_matrices = {}


def matrix_of(pkg, name, bins, n_blocks):
    """C of seeded noise on the list's mics (computed once per setting, left unchanged), and its block count."""
    key = (name, tuple(bins), n_blocks)
    if key not in _matrices:
        S, index = MICS[name]
        x = np.random.default_rng(S + n_blocks).standard_normal((S, 256 * n_blocks)).astype(np.float32)
        Cm, n = pkg.csm_accumulate_host(x, bins, 1, index=np.asarray(index, np.int32))
        assert n == n_blocks
        Cm.setflags(write=False)
        _matrices[key] = Cm
    return _matrices[key]


def guarded(n, dtype, fill):
    import torch

    return torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")


def inner(raw, shape, fill, what):
    host = raw.cpu().numpy()
    assert (host[:GUARD] == fill).all() and (host[-GUARD:] == fill).all(), f"{what}: guard overwritten"
    return host[GUARD:-GUARD].reshape(shape)


def device_invert(eng, Cm, n, bins, loading, want_solved=True, stream=0):
    import torch

    K, U = Cm.shape[0], Cm.shape[1]
    d_C = torch.from_numpy(np.array(Cm, np.float32)).cuda()
    d_G = guarded(K * U * U * 2, torch.float32, float(CANARY))
    d_s = guarded(K, torch.int32, -7)
    torch.cuda.synchronize()
    eng.csm_invert_device(d_C.data_ptr(), n, bins, d_G.data_ptr() + 4 * GUARD, loading, d_s.data_ptr() + 4 * GUARD if want_solved else 0, stream)
    eng.synchronize()
    solved = inner(d_s, (K,), -7, "solved")
    assert want_solved or (solved == -7).all()
    return inner(d_G, (K, U, U, 2), CANARY, "inverse"), solved


# ------------------------------------------------------------------------------------------------ 1. the rule's bits

def check_bits(pkg, eng, Cm, n, bins, loading, expect):
    want, ok = pkg.csm_invert_rule_host(Cm, n, bins, loading=loading)
    assert ok.tolist() == expect
    got, solved = device_invert(eng, Cm, n, bins, loading)
    assert solved.tolist() == expect
    assert CU.same_bits(got, want)
    assert CU.same_bits(device_invert(eng, Cm, n, bins, loading, want_solved=False)[0], want)  # without the solved words: the same bits
    return want


@pytest.mark.parametrize("name", ["one_mic", "two_mics", "ragged5", "sixty_four", "sixty_five_of_128", "ninety_five_of_96", "ninety_six"])
def test_device_inverse_equals_the_host_rule(pkg, name):
    U = len(MICS[name][1])
    with engine_of(pkg, name) as eng:
        for bins in ([16], EIGHT):
            if U > 65 and len(bins) > 1:
                continue  # (the two sizes around the LDS bound: one bin)
            Cm = matrix_of(pkg, name, bins, U + 3)
            check_bits(pkg, eng, Cm, U + 3, bins, LOADING, [1] * len(bins))
            if U > 1:  # without loading too: more blocks than mics make C itself positive definite
                check_bits(pkg, eng, Cm, U + 3, bins, 0.0, [1] * len(bins))


def test_device_inverse_where_the_working_set_has_left_the_lds(pkg):
    name, bins = "two_fifty_seven_of_320", [3, 47]
    with engine_of(pkg, name) as eng:
        check_bits(pkg, eng, matrix_of(pkg, name, bins, 260), 260, bins, LOADING, [1, 1])


def test_fewer_blocks_than_mics_with_loading(pkg):
    """C is singular (rank 5 of 64): the loading alone makes A positive definite."""
    name, bins = "sixty_four", [3, 16, 128]
    with engine_of(pkg, name) as eng:
        Cm = matrix_of(pkg, name, bins, 5)
        want = check_bits(pkg, eng, Cm, 5, bins, 0.05, [1, 1, 1])
        assert np.isfinite(want).all()


@pytest.mark.parametrize("name", ["ragged5", "sixty_five_of_128", "ninety_six"])
def test_an_unsolved_bin_among_solved_ones(pkg, name):
    """A NaN entry, a negative diagonal entry, and all zeros without loading, each in one bin of three: that bin +0 with solved 0,
    the others the rule's bits -- from the factor kernel's early end, in LDS and in the scratch."""
    U = len(MICS[name][1])
    bins = [3, 16, 128]
    base = matrix_of(pkg, name, bins, U + 3)
    with engine_of(pkg, name) as eng:
        for what, bin_ in (("nan", 1), ("negative", 0), ("zeros", 2), ("nan_first", 2)):
            Cm = base.copy()
            if what == "nan":
                Cm[bin_, U - 1, U // 2, 1] = np.nan
            elif what == "nan_first":
                Cm[bin_, 0, 0, 0] = np.nan
            elif what == "negative":
                Cm[bin_, U // 2, U // 2, 0] = -1e9
            else:
                Cm[bin_] = 0.0
            expect = [0 if k == bin_ else 1 for k in range(3)]
            want = check_bits(pkg, eng, Cm, U + 3, bins, 0.0 if what == "zeros" else LOADING, expect)
            assert not want[bin_].any() and not np.signbit(want[bin_]).any()


# ------------------------------------------------------------------------------------------------ 2. the synchronous form

def test_synchronous_inverse(pkg, scenes):  # noqa: F811
    import torch

    B = pkg.binding
    name, bins = "sixty_five_of_128", [3, 16, 128]
    U = 65
    Cm = matrix_of(pkg, name, bins, U + 3)
    with engine_of(pkg, name) as eng:
        assert CU.same_bits(eng.csm_invert(Cm, U + 3, bins, LOADING), pkg.csm_invert_rule_host(Cm, U + 3, bins, LOADING)[0])
        bad = Cm.copy()
        bad[1, 7, 7, 0] = np.nan
        out = np.full(Cm.shape, CANARY, np.float32)
        c = B.csm_of(bins, 0, CU.CAPON, LOADING)
        assert eng._lib.awpu_hip_csm_invert(eng._h, B._f32(bad), U + 3, C.byref(c), B._f32(out)) == B.ERR_RANGE
        assert (out == CANARY).all()
        with pytest.raises(pkg.AwpuError) as ei:
            eng.csm_invert(bad, U + 3, bins, LOADING)
        assert ei.value.status == B.ERR_RANGE
        # bad requests: AWPU_ERR_INVALID, nothing written
        d = torch.full((3 * U * U * 2,), float(CANARY), dtype=torch.float32, device="cuda")

        def status(call):
            try:
                call()
                return B.OK
            except pkg.AwpuError as e:
                return e.status

        for call in (lambda: eng.csm_invert(Cm, 0, bins), lambda: eng.csm_invert(Cm, U + 3, [16, 3, 128]), lambda: eng.csm_invert(Cm, U + 3, bins, -1.0),
                     lambda: eng.csm_invert_device(0, 5, bins, d.data_ptr()), lambda: eng.csm_invert_device(d.data_ptr(), 5, bins, 0),
                     lambda: eng.csm_invert_device(d.data_ptr(), 0, bins, d.data_ptr()), lambda: eng.csm_invert_device(d.data_ptr(), 5, bins, d.data_ptr(), float("nan"))):
            assert status(call) == B.ERR_INVALID
        assert eng._lib.awpu_hip_csm_invert(eng._h, None, 5, C.byref(c), B._f32(out)) == B.ERR_INVALID
        assert eng._lib.awpu_hip_csm_invert(eng._h, B._f32(Cm), 5, C.byref(c), None) == B.ERR_INVALID
        assert eng._lib.awpu_hip_csm_invert(None, B._f32(Cm), 5, C.byref(c), B._f32(out)) == B.ERR_INVALID
        torch.cuda.synchronize()
        assert (d.cpu().numpy() == CANARY).all() and (out == CANARY).all()

    # more active mics than the bound
    S = B.CSM_INVERT_MAX_MICS + 1
    with pkg.Engine(n_pixels=2, n_streams=S) as eng:
        eng.set_delay_table(np.zeros((2, S), np.int32), np.zeros((2, S), np.float32))
        eng.set_active_mics(None)
        big = np.zeros((1, S, S, 2), np.float32)
        big[0, np.arange(S), np.arange(S), 0] = 1.0
        out = np.full(big.shape, CANARY, np.float32)
        c = B.csm_of([3], 0, CU.CAPON, LOADING)
        assert eng._lib.awpu_hip_csm_invert(eng._h, B._f32(big), 1, C.byref(c), B._f32(out)) == B.ERR_RANGE and (out == CANARY).all()
        d = torch.full((big.size,), float(CANARY), dtype=torch.float32, device="cuda")
        with pytest.raises(pkg.AwpuError) as ei:
            eng.csm_invert_device(d.data_ptr(), 1, [3], d.data_ptr())
        assert ei.value.status == B.ERR_RANGE
        torch.cuda.synchronize()
        assert (d.cpu().numpy() == CANARY).all()

    # the state refusals of the cross-spectral calls
    sc = scenes(16)
    Cs = np.zeros((1, 64, 64, 2), np.float32)
    d = torch.full((Cs.size,), float(CANARY), dtype=torch.float32, device="cuda")

    def refused(eng):
        seen = []
        for call in (lambda: eng.csm_invert(Cs, 1, [3]), lambda: eng.csm_invert_device(d.data_ptr(), 1, [3], d.data_ptr())):
            try:
                call()
                seen.append(B.OK)
            except pkg.AwpuError as e:
                seen.append(e.status)
        return seen

    with sc.engine()() as eng:
        eng.set_band(pkg.band_design(1000.0, 4000.0, 31))
        assert refused(eng) == [B.ERR_STATE] * 2
        eng.set_band(None)
        eng.process_async(sc.frames[0][:1])
        assert refused(eng) == [B.ERR_STATE] * 2
        eng.wait()
    with pkg.Engine(n_pixels=sc.P, n_streams=64, interp=B.INTERP_FIR8) as eng:
        eng.set_delay_table(sc.off, sc.frac)
        eng.set_active_mics(None)
        assert refused(eng) == [B.ERR_STATE] * 2
    with pkg.Engine(n_pixels=sc.P, n_streams=64, grid_columns=16, devices=[0, 0]) as eng:  # a device group
        eng.set_delay_table(sc.off, sc.frac)
        eng.set_active_mics(None)
        assert refused(eng) == [B.ERR_STATE] * 2
    with pkg.Engine(n_pixels=sc.P, n_streams=64) as eng:  # no table, no mics
        assert refused(eng) == [B.ERR_STATE] * 2
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == CANARY).all()


# ------------------------------------------------------------------------------------------------ 3. stream order

def test_csm_invert_device_behind_pending_work(pkg, scenes, busy):  # noqa: F811
    sc = scenes(16)
    bins = [3, 47, 128]
    matrices = tuple(pkg.csm_accumulate_host(x, bins, 1)[0] for x in sc.samples)  # (fewer blocks than mics: the loading makes A definite)
    n = sc.samples[0].shape[1] // 256
    case = H.Case(sc.engine(), {"matrix": matrices}, {"inverse": ((3, 64, 64, 2), np.float32), "solved": ((3,), np.int32)},
                  lambda e, i, o, s: e.csm_invert_device(i["matrix"], n, bins, o["inverse"], LOADING, o["solved"], s))
    got = check(case, busy)
    want, ok = pkg.csm_invert_rule_host(matrices[0], n, bins, LOADING)
    assert got["solved"].tolist() == ok.tolist() == [1, 1, 1] and CU.same_bits(got["inverse"], want)


# ================================================================================================ the runs (awpu_hip_csm_watch.h)
# 4. Each run equals, bit for bit per shown frame, csm_accumulate_host over the window from zeros -> (Capon) csm_invert_rule_host ->
#    csm_map_host -> the sum -> heatmap_u8 / find_peaks: all three kinds, 5 of 8 mics (ragged, with gains) and 64, length 1, 3, 7
#    and n_blocks + 1, every below and above length with first > 0, max_batch 2 (three pieces, a window across each boundary), a
#    bin shown and the sum shown, planes and solved included; 300 blocks (more than one chunk of 256 new blocks).
# 5. One recording in one call equals two and three calls through carry / carried, each cut inside a window.
# 6. The three forms agree, and the ring after each is the ring after watch_blocks on the same datagrams.
# 7. Value edges: an all-zero recording under Capon; one NaN sample.  8. Stream order.  9. The scene as one frame.  10. Refusals.
# 11. (test_gpu_csm_large.py) Conventional and diagonal-removed runs at 545 of 640 mics and Capon's at 512, on a 3 x 7 grid; more
#     mics than the map or the inverse takes: AWPU_ERR_RANGE.

from test_gpu_blocks import recording  # noqa: E402

RES = 16
RUN_BLOCKS = 11
RUN_BINS = [3, 16, 47]
RUN_FIND = dict(radius=2, max_sources=4, min_ratio=0.1)
KINDS = (CU.CONVENTIONAL, CU.DIAGONAL_REMOVED, CU.CAPON)


class Rig:
    """A hand-made table on a grid of `rows` x `res` pixels (RES x RES unless given), an active list (with gains where ragged) and a
    recording as datagrams and samples; above 256 streams, more than the wire carries, as samples alone."""

    def __init__(self, pkg, oracle, n_streams, index, gains, seed, n_blocks=RUN_BLOCKS, res=RES, rows=None):
        rng = np.random.default_rng(seed)
        self.rows = res if rows is None else rows
        self.pkg, self.S, self.res, self.P, self.n_blocks = pkg, n_streams, res, self.rows * res, n_blocks
        self.index = np.asarray(index, np.int32)
        self.off = rng.integers(0, 1024 - 256, (self.P, n_streams)).astype(np.int32)
        self.frac = rng.random((self.P, n_streams)).astype(np.float32)
        self.gains = (0.5 + rng.random(n_streams)).astype(np.float32) if gains else None
        if n_streams <= 256:
            self.wire, self.samples = recording(oracle, n_blocks, n_streams, seed)
        else:
            self.wire, self.samples = None, rng.standard_normal((n_streams, 256 * n_blocks)).astype(np.float32)
        self.samples = np.ascontiguousarray(self.samples, np.float32)
        self._frames = {}

    def engine(self, max_batch=2, **kw):
        eng = self.pkg.Engine(n_pixels=self.P, n_streams=self.S, max_batch=max_batch, grid_columns=self.res, **kw)
        eng.set_delay_table(self.off, self.frac)
        eng.set_active_mics(self.index)
        if self.gains is not None:
            eng.set_mic_gains(self.gains)
        return eng

    def frame(self, t, length, kind, loading, samples=None, bins=RUN_BINS, window=1):
        """The composition for the frame that shows block t: (planes [n_bins, P], solved [n_bins]); cached for the rig's own samples."""
        key = (t, length, kind, loading, tuple(bins), window)
        if samples is None and key in self._frames:
            return self._frames[key]
        pkg, x = self.pkg, self.samples if samples is None else samples
        lo = max(t - length + 1, 0)
        gl = None if self.gains is None else self.gains[self.index]
        with np.errstate(all="ignore"):
            Cm, n = pkg.csm_accumulate_host(np.ascontiguousarray(x[:, 256 * lo: 256 * (t + 1)]), bins, window, index=self.index, gain=gl)
            assert n == t - lo + 1
            solved = np.ones(len(bins), np.int32)
            if kind == CU.CAPON:
                Cm, solved = pkg.csm_invert_rule_host(Cm, n, bins, loading=loading)
            planes = pkg.csm_map_host(Cm, n, self.off, self.frac, bins, window, kind, index=self.index)["map"]
        if samples is None:
            self._frames[key] = (planes, solved)
        return planes, solved

    def composition(self, first, every, length, kind, loading, show, samples=None, n_blocks=None, **kw):
        shown = range(first, self.n_blocks if n_blocks is None else n_blocks, every)
        frames = [self.frame(t, length, kind, loading, samples, **kw) for t in shown]
        planes = np.stack([p for p, _ in frames])
        rows = planes[:, show] if show >= 0 else shown_sum(planes)
        return dict(planes=planes, solved=np.stack([s for _, s in frames]), power=np.ascontiguousarray(rows))


def shown_sum(planes):
    """[n_frames, n_bins, P] -> the planes added in ascending bin order with plain float32 additions, from +0."""
    with np.errstate(all="ignore"):
        total = np.zeros(planes[:, 0].shape, np.float32)
        for k in range(planes.shape[1]):
            total = (total + planes[:, k]).astype(np.float32)
    return total


@pytest.fixture(scope="module")
def rigs(pkg, oracle):
    return {"ragged5": Rig(pkg, oracle, 8, [6, 1, 3, 0, 7], True, 31), "sixty_four": Rig(pkg, oracle, 64, list(range(64)), False, 32)}


def same_where_not_nan(got, want, where):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, where
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (where, "NaN positions")
    assert np.array_equal(CU.bits(got)[~nan], CU.bits(want)[~nan]), where


def check_run(pkg, rig, got, want, where, exact=True):
    n_frames = len(want["power"])
    assert got.power.shape == (n_frames, rig.P) and got.planes.shape == want["planes"].shape, where
    same = CU.same_bits if exact else (lambda a, b: same_where_not_nan(a, b, where) is None)
    assert same(got.planes, want["planes"]), (where, "planes")
    assert np.array_equal(got.solved, want["solved"]), (where, "solved")
    assert same(got.power, want["power"]), (where, "power")
    if n_frames and not np.isnan(want["power"]).any():
        image = np.stack([pkg.heatmap_u8(p) for p in want["power"]]).reshape(-1, rig.rows, rig.res)
        assert np.array_equal(got.image, image), (where, "image")
        found = pkg.find_peaks(want["power"], rig.rows, rig.res, **RUN_FIND)
        assert np.array_equal(got.count, found.count), (where, "count")
        assert np.array_equal(got.sources["pixel"], found.sources["pixel"]), (where, "sources")
        assert CU.same_bits(got.sources["power"], found.sources["power"]), (where, "source powers")


RUN_KW = dict(want_power=True, want_planes=True, want_solved=True, find=RUN_FIND)


@pytest.mark.parametrize("kind", KINDS, ids=["conventional", "diagonal_removed", "capon"])
@pytest.mark.parametrize("name", ["ragged5", "sixty_four"])
def test_runs_equal_the_composition(pkg, rigs, name, kind):
    rig = rigs[name]
    with rig.engine(max_batch=2) as eng:
        for length in (1, 3, 7, RUN_BLOCKS + 1):
            for first, every in ((1, 2), (2, 5)):
                for show in (1, pkg.binding.CSM_SHOW_SUM):
                    where = (name, kind, length, first, every, show)
                    want = rig.composition(first, every, length, kind, 0.05, show)
                    got = eng.csm_watch_samples(rig.samples, RES, RES, RUN_BINS, 1, kind, 0.05, length, show, first, every, **RUN_KW)
                    check_run(pkg, rig, got, want, where)
                    assert got.carried == min(RUN_BLOCKS, length - 1) and got.next_first == pkg.binding.watch_count(RUN_BLOCKS, first, every)[1]
                    assert (got.solved == 1).all()
        assert len(range(1, RUN_BLOCKS, 2)) == 5  # (max_batch 2: three pieces, and with length >= 3 a window across each boundary)


def test_more_blocks_than_a_chunk(pkg, oracle):
    """300 blocks: the second chunk of new blocks starts at block 256; frames at 99, 199, 299 (Capon, length 7) and at every 64th
    block with length 70 (windows that span the chunk boundary)."""
    rig = Rig(pkg, oracle, 8, [5, 2], False, 33, n_blocks=300, res=4)
    with rig.engine(max_batch=2) as eng:
        for first, every, length in ((99, 100, 7), (63, 64, 70)):
            want = rig.composition(first, every, length, CU.CAPON, 0.05, -1, bins=[16], window=0)
            got = eng.csm_watch_samples(rig.samples, 4, 4, [16], 0, CU.CAPON, 0.05, length, -1, first, every, **RUN_KW)
            check_run(pkg, rig, got, want, (first, every, length))


@pytest.mark.parametrize("kind", [CU.DIAGONAL_REMOVED, CU.CAPON], ids=["diagonal_removed", "capon"])
def test_a_split_recording_gives_one_calls_bits(pkg, rigs, kind):
    rig = rigs["ragged5"]
    length, first, every, show = 7, 1, 2, -1
    kw = dict(RUN_KW, want_image=True)
    with rig.engine() as eng:
        whole = eng.csm_watch_samples(rig.samples, RES, RES, RUN_BINS, 1, kind, 0.05, length, show, first, every, **kw)
    check_run(pkg, rig, whole, rig.composition(first, every, length, kind, 0.05, show), "whole")
    for cuts in ((4,), (2, 6)):  # every cut lies inside the windows of the frames behind it
        with rig.engine() as eng:
            parts, carry, carried, nxt, lo = [], None, 0, first, 0
            for hi in cuts + (RUN_BLOCKS,):
                x = np.ascontiguousarray(rig.samples[:, 256 * lo: 256 * hi])
                r = eng.csm_watch_samples(x, RES, RES, RUN_BINS, 1, kind, 0.05, length, show, nxt, every, carry=carry, carried=carried, **kw)
                parts.append(r)
                carry, carried, nxt, lo = r.carry, r.carried, r.next_first, hi
        assert nxt == whole.next_first and carried == whole.carried
        assert CU.same_bits(carry[length - 1 - carried:], whole.carry[length - 1 - carried:])
        for field in ("power", "planes", "solved", "image", "count", "sources"):
            joined = np.concatenate([getattr(r, field) for r in parts])
            assert joined.tobytes() == getattr(whole, field).tobytes(), (cuts, field)


def test_the_three_forms_agree_and_leave_the_watch_runs_ring(pkg, rigs):
    import torch

    rig = rigs["sixty_four"]
    length, first, every, show, kind = 3, 1, 2, 1, CU.CAPON
    n_frames = len(range(first, RUN_BLOCKS, every))
    want = rig.composition(first, every, length, kind, 0.05, show)
    with rig.engine() as ref:
        ref.watch_blocks(rig.wire, RES, RES, first=first, every=every)
        ring = ref.ring_snapshot()
    args = (RES, RES, RUN_BINS, 1, kind, 0.05, length, show, first, every)
    with rig.engine() as eng:
        check_run(pkg, rig, eng.csm_watch_blocks(rig.wire, *args, **RUN_KW), want, "blocks")
        assert np.array_equal(eng.ring_snapshot(), ring)
    with rig.engine() as eng:
        check_run(pkg, rig, eng.csm_watch_samples(rig.samples, *args, **RUN_KW), want, "samples")
        assert np.array_equal(eng.ring_snapshot(), ring)
    with rig.engine() as eng:  # the device form, every output between guards
        K, P, U = len(RUN_BINS), rig.P, 64
        outs = {"image": (n_frames * P, torch.uint8), "power": (n_frames * P, torch.float32), "sources": (n_frames * 4 * 40, torch.uint8),
                "count": (n_frames, torch.int32), "planes": (n_frames * K * P, torch.float32), "solved": (n_frames * K, torch.int32),
                "carry": ((length - 1) * K * U * 2, torch.float32)}
        fill = {torch.uint8: 0xA5, torch.float32: float(CANARY), torch.int32: -7}
        raw = {k: torch.full((n + 128,), fill[t], dtype=t, device="cuda") for k, (n, t) in outs.items()}
        ptr = {k: v.data_ptr() + 64 * v.element_size() for k, v in raw.items()}
        d_x = torch.from_numpy(rig.samples).cuda()
        torch.cuda.synchronize()
        nxt, carried = eng.csm_watch_samples_device(d_x.data_ptr(), rig.samples.shape[1], RUN_BLOCKS, *args, d_carry_ptr=ptr["carry"], carried=0,
                                                    d_image_ptr=ptr["image"], d_power_ptr=ptr["power"], d_sources_ptr=ptr["sources"],
                                                    d_count_ptr=ptr["count"], d_planes_ptr=ptr["planes"], d_solved_ptr=ptr["solved"], find=RUN_FIND)
        eng.synchronize()
        host = {k: v.cpu().numpy() for k, v in raw.items()}
        for k, v in host.items():
            assert (v[:64] == fill[outs[k][1]]).all() and (v[-64:] == fill[outs[k][1]]).all(), k
        B = pkg.binding
        got = B.CsmWatchResult(host["image"][64:-64].reshape(n_frames, RES, RES), None, host["power"][64:-64].reshape(n_frames, P),
                               host["sources"][64:-64].view(B.SOURCE_DTYPE).reshape(n_frames, 4), host["count"][64:-64],
                               host["planes"][64:-64].reshape(n_frames, K, P), host["solved"][64:-64].reshape(n_frames, K), nxt,
                               host["carry"][64:-64].reshape(length - 1, K, U, 2), carried)
        check_run(pkg, rig, got, want, "device")
        assert carried == length - 1 and nxt == B.watch_count(RUN_BLOCKS, first, every)[1]
        assert np.array_equal(eng.ring_snapshot(), ring)
        spectra = pkg.csm_spectra_host(rig.samples, RUN_BINS, 1)
        assert CU.same_bits(got.carry, spectra[RUN_BLOCKS - (length - 1):])


def test_value_edges(pkg, rigs):
    rig = rigs["ragged5"]
    length, first, every, show = 3, 0, 1, -1
    with rig.engine() as eng:
        # an all-zero recording under Capon: nothing solved, +0 planes, no NaN
        zeros = np.zeros_like(rig.samples)
        got = eng.csm_watch_samples(zeros, RES, RES, RUN_BINS, 1, CU.CAPON, 0.05, length, show, first, every, **RUN_KW)
        assert (got.solved == 0).all() and not got.planes.any() and not np.signbit(got.planes).any() and not got.power.any()
        assert not np.isnan(got.planes).any() and not got.image.any()
        assert np.array_equal(got.count, pkg.find_peaks(got.power, RES, RES, **RUN_FIND).count)
        # one NaN sample in block 5: exactly the frames whose windows hold that block change, as the composition says
        clean = eng.csm_watch_samples(rig.samples, RES, RES, RUN_BINS, 1, CU.CAPON, 0.05, length, show, first, every, **RUN_KW)
        x = rig.samples.copy()
        x[rig.index[2], 256 * 5 + 17] = np.nan
        got = eng.csm_watch_samples(x, RES, RES, RUN_BINS, 1, CU.CAPON, 0.05, length, show, first, every, **RUN_KW)
        want = rig.composition(first, every, length, CU.CAPON, 0.05, show, samples=x)
        check_run(pkg, rig, got, want, "nan", exact=False)
        holds = np.array([t - length + 1 <= 5 <= t for t in range(RUN_BLOCKS)])
        assert holds.sum() == length
        assert CU.same_bits(got.planes[~holds], clean.planes[~holds]) and np.array_equal(got.solved[~holds], clean.solved[~holds])
        assert (got.solved[holds] == 0).all() and not got.planes[holds].any()  # (a NaN in every bin of the block: no bin of those frames is solved)
        conventional = eng.csm_watch_samples(x, RES, RES, RUN_BINS, 1, CU.CONVENTIONAL, 0.0, length, show, first, every, **RUN_KW)
        want = rig.composition(first, every, length, CU.CONVENTIONAL, 0.0, show, samples=x)
        check_run(pkg, rig, conventional, want, "nan, conventional", exact=False)
        assert np.isnan(conventional.power[holds]).any(axis=1).all() and not np.isnan(conventional.power[~holds]).any()


def test_csm_watch_samples_device_behind_pending_work(pkg, scenes, busy):  # noqa: F811
    sc = scenes(16)
    bins, length = [3, 47, 128], 3
    n_blocks = sc.samples[0].shape[1] // 256
    rng = np.random.default_rng(9)
    carries = tuple((rng.standard_normal((length - 1, 3, 64, 2)) * s).astype(np.float32) for s in (1.0, 2.0))
    outs = {"image": ((n_blocks, sc.P), np.uint8), "power": ((n_blocks, sc.P), np.float32), "sources": ((n_blocks, 4, 40), np.uint8),
            "count": ((n_blocks,), np.int32), "planes": ((n_blocks, 3, sc.P), np.float32), "solved": ((n_blocks, 3), np.int32)}
    case = H.Case(sc.engine(max_batch=2), {"samples": sc.samples, "carry": carries}, outs,
                  lambda e, i, o, s: e.csm_watch_samples_device(i["samples"], 256 * n_blocks, n_blocks, 16, 16, bins, 1, CU.CAPON, 0.05, length, -1, 0, 1,
                                                                d_carry_ptr=i["carry"], carried=length - 1, d_image_ptr=o["image"],
                                                                d_power_ptr=o["power"], d_sources_ptr=o["sources"], d_count_ptr=o["count"],
                                                                d_planes_ptr=o["planes"], d_solved_ptr=o["solved"], stream=s, find=RUN_FIND),
                  inout=("carry",))
    got = check(case, busy)
    assert got["host"] == (0, length - 1) and (got["solved"] == 1).all() and np.isfinite(got["power"]).all() and got["power"].max() > 0
    assert CU.same_bits(got["carry"], pkg.csm_spectra_host(sc.samples[0], bins, 1)[n_blocks - (length - 1):])


def test_the_scene_as_one_frame(pkg):
    """csm_util's scene (tests/test_csm_cpu.py states it) as one frame of a run: length 256, first 255, every 256.  Capon's run
    finds the two sources at their pixels, the conventional run one."""
    S = pkg.synthetic
    spec = S.WORKLOADS["c1"]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    x, _ = CU.scene_samples(pkg, spec, xyz)
    with pkg.Engine(n_pixels=spec.n_pixels, n_streams=64, grid_columns=32) as eng:
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        kw = dict(length=256, first=255, every=256, want_image=False, find=CU.SCENE_FIND)
        capon = eng.csm_watch_samples(x, 32, 32, [CU.SCENE_BIN], 1, CU.CAPON, CU.SCENE_LOADING, **kw)
        conventional = eng.csm_watch_samples(x, 32, 32, [CU.SCENE_BIN], 1, CU.CONVENTIONAL, **kw)
    assert capon.count.tolist() == [2] and conventional.count.tolist() == [1]
    pixels = [int(p) for p in capon.sources["pixel"][0, :2]]
    for true in CU.scene_pixels(spec):
        assert any(abs(p // 32 - true // 32) <= 1 and abs(p % 32 - true % 32) <= 1 for p in pixels), (true, pixels)


def test_runs_refuse(pkg, rigs, scenes):  # noqa: F811
    B = pkg.binding
    rig = rigs["ragged5"]

    def status(eng, bins=RUN_BINS, kind=CU.CAPON, length=3, show=-1, first=0, every=1, carry=None, carried=0, samples=None, **kw):
        try:
            eng.csm_watch_samples(rig.samples if samples is None else samples, RES, RES, bins, 1, kind, 0.05, length, show, first, every, carry=carry,
                                  carried=carried, **kw)
            return B.OK
        except pkg.AwpuError as e:
            return e.status

    with rig.engine() as eng:
        assert status(eng, length=1) == B.OK
        before = eng.ring_snapshot()
        assert status(eng, length=0) == B.ERR_INVALID and status(eng, length=1025) == B.ERR_INVALID
        assert status(eng, show=3) == B.ERR_INVALID and status(eng, show=-2) == B.ERR_INVALID
        assert status(eng, carried=3) == B.ERR_INVALID and status(eng, carried=-1) == B.ERR_INVALID
        assert status(eng, bins=[47, 3]) == B.ERR_INVALID and status(eng, kind=3) == B.ERR_INVALID
        assert status(eng, every=0) == B.ERR_INVALID and status(eng, first=-1) == B.ERR_INVALID
        assert status(eng, want_image=False) == B.ERR_INVALID  # no output asked for
        w, c = B.Watch(0, 1, RES, RES, 0, 0, 0, None), B.csm_of(RUN_BINS, 1, CU.CAPON, 0.05)
        held, power = C.c_int32(0), np.zeros((RUN_BLOCKS, rig.P), np.float32)
        assert eng._lib.awpu_hip_csm_watch_samples(eng._h, B._f32(rig.samples), rig.samples.shape[1], RUN_BLOCKS, C.byref(w), C.byref(c), 3, -1, None, None,
                                                   C.cast(C.byref(held), B._i32p), None, None, B._f32(power), None, None, None, None) == B.ERR_INVALID
        assert np.array_equal(eng.ring_snapshot(), before)  # a refused run leaves the ring as it was
    with rig.engine(interp=B.INTERP_FIR8) as eng:
        assert status(eng) == B.ERR_STATE
    with pkg.Engine(n_pixels=rig.P, n_streams=rig.S, grid_columns=RES, pixel_begin=0, pixel_count=128) as eng:  # a slab handle: no display step
        eng.set_delay_table(rig.off[:128], rig.frac[:128])
        eng.set_active_mics(rig.index)
        assert status(eng) == B.ERR_INVALID
    sc = scenes(16)

    def scene_status(eng):
        try:
            eng.csm_watch_samples(sc.samples[0], 16, 16, RUN_BINS, 1)
            return B.OK
        except pkg.AwpuError as e:
            return e.status

    with sc.engine()() as eng:
        eng.set_band(pkg.band_design(1000.0, 4000.0, 31))
        assert scene_status(eng) == B.ERR_STATE
        eng.set_band(None)
        assert scene_status(eng) == B.OK
    with pkg.Engine(n_pixels=sc.P, n_streams=64, grid_columns=16, devices=[0, 0]) as eng:  # a device group
        eng.set_delay_table(sc.off, sc.frac)
        eng.set_active_mics(None)
        assert scene_status(eng) == B.ERR_STATE
