"""The cross-spectral calls at every launch shape between 257 mics and the bounds their headers state: 2048 active mics for the map
and CLEAN-SC, 512 for the loaded inverse.  The device against the host rule, bit for bit, every device output between guard floats;
what that rule is worth at these sizes is test_csm_large_cpu.py's question.

1. The map's ladder (csm_map_pixels_per_wave): 544 of 544 mics (the last size at 32 pixels a workgroup, its LDS exactly 144 KiB,
   40 pixels: a tail of 8), 545 of 640 (ragged, with gains: the first size at 16 pixels, 21 pixels: a tail of 5), 1120 (the last
   at 16, exactly 144 KiB), 1121 (the first at 8 pixels, 11 pixels: a tail of 3) and 2048 (the bound; the accumulate kernel's grid
   is 128 x 128 tiles).  Two blocks, pitch 256 * 2 + 40, bin [47], Hann; 545 also [3, 47, 128].  Spectra, C, q and the three kinds
   of plane, q and map alone and together, the host forms.  Above 545 mics Capon's kind is given C itself.
2. The inverse at its bound: 512 of 512 mics, one bin, 515 blocks, loading 1e-2 and 0, with and without the solved words, and the
   synchronous form; 511 of 512, bins [3, 47], 5 blocks (rank-deficient, loading 0.05) with bin 47 unsolved by a negative
   diagonal entry.
3. CLEAN-SC at 545 of 640 (three passes of the component kernel's 256 rows) and 2048 (eight, s and v filling their LDS): the
   loop, the host form, and the step form on a matrix with a garbage upper triangle.
4. Runs on large lists, against the hand composition: csm_watch_samples_device over 3 blocks, length 2, a 3 x 7 grid --
   conventional and diagonal-removed at 545 of 640 mics, Capon at 512 --, and csm_clean_samples_device at 545, 2 steps.
5. The range refusals: 2049 active mics in csm_map, csm_map_device, csm_clean, csm_clean_device and csm_clean_step_device;
   csm_watch_samples at 2049 (conventional) and at 513 (Capon); csm_clean_samples at 2049.  Nothing is written, the ring stays,
   the next call on a smaller handle is unaffected.  csm_samples has no bound: at 2049 mics it gives csm_accumulate_host's bits."""
import ctypes as C

import numpy as np
import pytest

import csm_large as L
import csm_util as CU
import test_gpu_csm as M
import test_gpu_csm_clean as K
import test_gpu_csm_clean_runs as KR
import test_gpu_csm_runs as R

pytestmark = pytest.mark.gpu

CANARY = M.CANARY


# ------------------------------------------------------------------------------------------------ 1. the map's ladder

@pytest.mark.parametrize("name", list(L.LISTS))
def test_the_maps_ladder_equals_the_host_rule(pkg, name):
    """Every size at which csm_map_pixels_per_wave changes its answer, and the bound.  With fewer pixels than lanes a workgroup's
    lanes ppw..63 go along with its last pixel and write nothing; every pixel count here leaves a tail workgroup.  Above 545 mics
    the Capon kind is not given an inverse (csm_invert_host takes minutes at 2048 mics) but C itself: the map reads whatever matrix
    it is given, and C is positive semi-definite, so its x = s^H C s > 0 takes step 5's division and not its zero."""
    sh = L.shape(pkg, name)
    ppw = L.LISTS[name][5]
    assert sh.U == len(L.LISTS[name][1]) and ppw == L.pixels_per_workgroup(sh.U)
    assert L.map_lds_bytes(sh.U, ppw) <= L.LDS_BYTES < L.map_lds_bytes(sh.U, 2 * ppw) and sh.P % ppw and sh.P > ppw
    if name in ("544", "1120"):
        assert L.map_lds_bytes(sh.U, ppw) == L.LDS_BYTES == 147456
    settings = [(L.BINS, L.WINDOW, L.N_BLOCKS)] + ([([3, 47, 128], 1, L.N_BLOCKS)] if name == "545_of_640" else [])
    for bins, window, n_blocks in settings:
        want = sh.rule(bins, window, n_blocks)
        assert sh.samples_of(n_blocks).shape[1] == 256 * 2 + 40 and set(M.KINDS) <= set(want)
        if not sh.invert:
            assert want["G"] is want["C"] and (want[CU.CAPON]["q"] > 0).all() and (want[CU.CAPON]["map"] > 0).all()
    M.check_against_host_rule(sh, settings)


# ------------------------------------------------------------------------------------------------ 2. the inverse at its bound

_bound = {}


def matrix_at_the_bound(pkg):
    """C of 515 blocks of seeded noise on 512 mics, bin 16, Hann: more blocks than mics, so C itself is positive definite.  The
    recording is 270 MB as floats, so it is made and added 103 blocks at a time (a split recording gives one call's bits)."""
    if "C" not in _bound:
        rng = np.random.default_rng(515)
        Cm, n = None, 0
        for _ in range(5):
            Cm, n = pkg.csm_accumulate_host(rng.standard_normal((512, 256 * 103), dtype=np.float32), [16], 1, matrix=Cm, block_count=n)
        assert n == 515
        Cm.setflags(write=False)
        _bound["C"] = Cm
    return _bound["C"]


def test_the_inverse_at_512_mics(pkg):
    """csm_invert_solve_kernel runs 512 threads, exactly its launch bound; the factor kernel walks a 4 MiB triangle in the scratch;
    the Gram grid is 32 x 32 tiles and the finish grid 2048 workgroups."""
    Cm = matrix_at_the_bound(pkg)
    assert pkg.binding.CSM_INVERT_MAX_MICS == 512 == Cm.shape[1]
    with R.engine_of(pkg, "five_twelve") as eng:
        for loading in (R.LOADING, 0.0):
            want = R.check_bits(pkg, eng, Cm, 515, [16], loading, [1])
            assert np.isfinite(want).all() and want.any()
            assert CU.same_bits(eng.csm_invert(Cm, 515, [16], loading), want), ("the synchronous form", loading)


def test_the_inverse_at_511_of_512_with_an_unsolved_bin(pkg):
    """Fewer blocks than mics: C has rank 5 and the loading alone makes A positive definite.  A negative diagonal entry in bin 47
    leaves that bin +0 with solved 0; bin 3 keeps the rule's bits (check_bits compares both bins)."""
    name, bins = "five_eleven_of_512", [3, 47]
    U = len(R.MICS[name][1])
    assert U == 511
    Cm = R.matrix_of(pkg, name, bins, 5).copy()
    Cm[1, U // 2, U // 2, 0] = -1e9
    with R.engine_of(pkg, name) as eng:
        want = R.check_bits(pkg, eng, Cm, 5, bins, 0.05, [1, 0])
    assert not want[1].any() and not np.signbit(want[1]).any()
    assert np.isfinite(want[0]).all() and (np.diagonal(want[0, :, :, 0]) > 0).all()


# ------------------------------------------------------------------------------------------------ 3. CLEAN-SC

@pytest.mark.parametrize("name", ["545_of_640", "2048"])
def test_clean_sc_above_two_passes_of_rows(pkg, name):
    """The component kernel takes 256 rows a pass: three passes at 545 mics, the third of 33 rows; eight at 2048, with s and vl
    filling their 32 KiB.  The helper asserts that the host rule's first pick is >= 0 in every bin (the seeds of csm_large.py
    are chosen so)."""
    sh = L.shape(pkg, name)
    assert (sh.U + 255) // 256 == {"545_of_640": 3, "2048": 8}[name]
    K.check_against_host_rule(pkg, sh, [(L.BINS, L.WINDOW, L.N_BLOCKS, 3, 0.5)], alone=False)


# ------------------------------------------------------------------------------------------------ 4. runs

RUN_BLOCKS, RUN_LENGTH, ROWS, COLS = 3, 2, 3, 7
FILL = {"uint8": 0xA5, "float32": float(CANARY), "int32": -7}


@pytest.fixture(scope="module")
def big_rigs(pkg, oracle):
    return {"545_of_640": R.Rig(pkg, oracle, 640, L.RAGGED_545, True, 51, n_blocks=RUN_BLOCKS, res=COLS, rows=ROWS),
            "512": R.Rig(pkg, oracle, 512, list(range(512)), False, 52, n_blocks=RUN_BLOCKS, res=COLS, rows=ROWS)}


def run_on_the_device(rig, eng, n_frames, K_, call, extra):
    """A device-form run of the rig's recording, every output between guards: call(d_samples_ptr, pitch, pointers) -> (next_first,
    carried); `extra` names the run's own output beside the shown ones -> ({name: array}, next_first, carried)."""
    import torch

    P, U = rig.P, len(rig.index)
    outs = {"image": (n_frames * P, torch.uint8), "power": (n_frames * P, torch.float32), "sources": (n_frames * 4 * 40, torch.uint8),
            "count": (n_frames, torch.int32), "planes": (n_frames * K_ * P, torch.float32), "carry": ((RUN_LENGTH - 1) * K_ * U * 2, torch.float32), **extra}
    fill = {t: FILL[str(t).split(".")[1]] for _, t in outs.values()}
    raw = {k: torch.full((n + 128,), fill[t], dtype=t, device="cuda") for k, (n, t) in outs.items()}
    ptr = {k: v.data_ptr() + 64 * v.element_size() for k, v in raw.items()}
    d_x = torch.from_numpy(rig.samples).cuda()
    torch.cuda.synchronize()
    nxt, carried = call(d_x.data_ptr(), rig.samples.shape[1], ptr)
    eng.synchronize()
    host = {k: v.cpu().numpy() for k, v in raw.items()}
    for k, v in host.items():
        assert (v[:64] == fill[outs[k][1]]).all() and (v[-64:] == fill[outs[k][1]]).all(), (k, "guard overwritten")
    return {k: v[64:-64] for k, v in host.items()}, nxt, carried


def gains_of(rig):
    return None if rig.gains is None else rig.gains[rig.index]


@pytest.mark.parametrize("name,kind,bins,first", [("545_of_640", CU.CONVENTIONAL, R.RUN_BINS, 0), ("545_of_640", CU.DIAGONAL_REMOVED, R.RUN_BINS, 0),
                                                  ("512", CU.CAPON, [47], 1)], ids=["conventional_545", "diagonal_removed_545", "capon_512"])
def test_watch_runs_on_large_lists_equal_the_composition(pkg, big_rigs, name, kind, bins, first):
    """Three blocks, windows of two, max_batch 2; the 545-mic runs show every block (a first window of one block, two pieces), the
    Capon run at the inverse's bound the two full windows, of one bin (its composition inverts 512 mics once a frame)."""
    import torch

    B = pkg.binding
    rig = big_rigs[name]
    every, show, loading = 1, B.CSM_SHOW_SUM, 0.05
    n_frames, K_, P, U = len(range(first, RUN_BLOCKS, every)), len(bins), rig.P, len(rig.index)
    want = rig.composition(first, every, RUN_LENGTH, kind, loading, show, bins=bins)
    with rig.engine(max_batch=2) as eng:
        host, nxt, carried = run_on_the_device(
            rig, eng, n_frames, K_,
            lambda d_x, pitch, ptr: eng.csm_watch_samples_device(d_x, pitch, RUN_BLOCKS, ROWS, COLS, bins, 1, kind, loading, RUN_LENGTH, show, first, every,
                                                                 d_carry_ptr=ptr["carry"], carried=0, d_image_ptr=ptr["image"], d_power_ptr=ptr["power"],
                                                                 d_sources_ptr=ptr["sources"], d_count_ptr=ptr["count"], d_planes_ptr=ptr["planes"],
                                                                 d_solved_ptr=ptr["solved"], find=R.RUN_FIND),
            {"solved": (n_frames * K_, torch.int32)})
    got = B.CsmWatchResult(host["image"].reshape(n_frames, ROWS, COLS), None, host["power"].reshape(n_frames, P),
                           host["sources"].view(B.SOURCE_DTYPE).reshape(n_frames, 4), host["count"], host["planes"].reshape(n_frames, K_, P),
                           host["solved"].reshape(n_frames, K_), nxt, host["carry"].reshape(RUN_LENGTH - 1, K_, U, 2), carried)
    R.check_run(pkg, rig, got, want, (name, kind))
    assert (got.solved == 1).all() and carried == RUN_LENGTH - 1 and nxt == B.watch_count(RUN_BLOCKS, first, every)[1]
    spectra = pkg.csm_spectra_host(rig.samples, bins, 1, index=rig.index, gain=gains_of(rig))
    assert CU.same_bits(got.carry, spectra[RUN_BLOCKS - (RUN_LENGTH - 1):])


def test_a_clean_sc_run_on_a_large_list_equals_the_composition(pkg, big_rigs):
    """csm_clean_samples_device at 545 of 640 mics: every frame is csm_accumulate_host over its window -> csm_clean_host -> the clean
    rows -> their sum, two steps a frame."""
    import torch

    B = pkg.binding
    rig = big_rigs["545_of_640"]
    bins, steps, gain, stop, what, first, every, show = [16, 47], 2, 0.75, 0.05, B.CSM_CLEAN_CLEAN, 0, 1, B.CSM_SHOW_SUM
    n_frames, K_, P, U = RUN_BLOCKS, len(bins), rig.P, len(rig.index)
    frames = []
    for t in range(first, RUN_BLOCKS, every):
        lo = max(t - RUN_LENGTH + 1, 0)
        Cm, n = pkg.csm_accumulate_host(np.ascontiguousarray(rig.samples[:, 256 * lo: 256 * (t + 1)]), bins, 1, index=rig.index, gain=gains_of(rig))
        assert n == t - lo + 1
        frames.append(pkg.csm_clean_host(Cm, n, rig.off, rig.frac, bins, steps, gain, stop, 1, index=rig.index))
    planes = np.stack([fr[KR.ROWS[what]] for fr in frames])
    want = dict(planes=planes, steps=np.stack([fr["steps"] for fr in frames]), power=np.ascontiguousarray(R.shown_sum(planes)))
    assert (want["steps"]["pixel"][:, :, 0] >= 0).all()
    with rig.engine(max_batch=2) as eng:
        host, nxt, carried = run_on_the_device(
            rig, eng, n_frames, K_,
            lambda d_x, pitch, ptr: eng.csm_clean_samples_device(d_x, pitch, RUN_BLOCKS, ROWS, COLS, bins, steps, gain, stop, what, 1, RUN_LENGTH, show, first,
                                                                 every, d_carry_ptr=ptr["carry"], carried=0, d_image_ptr=ptr["image"], d_power_ptr=ptr["power"],
                                                                 d_sources_ptr=ptr["sources"], d_count_ptr=ptr["count"], d_planes_ptr=ptr["planes"],
                                                                 d_steps_ptr=ptr["steps"], find=KR.FIND),
            {"steps": (n_frames * K_ * steps * 3, torch.float32)})
    got = B.CsmCleanRunResult(host["image"].reshape(n_frames, ROWS, COLS), None, host["power"].reshape(n_frames, P),
                              host["sources"].view(B.SOURCE_DTYPE).reshape(n_frames, 4), host["count"], host["planes"].reshape(n_frames, K_, P),
                              np.ascontiguousarray(host["steps"]).view(B.CSM_CLEAN_STEP_DTYPE).reshape(n_frames, K_, steps), nxt,
                              host["carry"].reshape(RUN_LENGTH - 1, K_, U, 2), carried)
    KR.check_run(pkg, got, want, "545 of 640", res=COLS, rows=ROWS)
    assert carried == RUN_LENGTH - 1 and nxt == B.watch_count(RUN_BLOCKS, first, every)[1]
    spectra = pkg.csm_spectra_host(rig.samples, bins, 1, index=rig.index, gain=gains_of(rig))
    assert CU.same_bits(got.carry, spectra[RUN_BLOCKS - (RUN_LENGTH - 1):])


# ------------------------------------------------------------------------------------------------ 5. refusals

TOO_MANY = 2049


def engine_with_too_many(pkg, **kw):
    """A handle of 2049 streams, all active, and a two-pixel table on a 1 x 2 grid."""
    rng = np.random.default_rng(TOO_MANY)
    eng = pkg.Engine(n_pixels=2, n_streams=TOO_MANY, grid_columns=2, **kw)
    eng.set_delay_table(rng.integers(0, 700, (2, TOO_MANY)).astype(np.int32), rng.random((2, TOO_MANY)).astype(np.float32))
    eng.set_active_mics(None)
    return eng


def test_more_than_2048_mics_are_refused_and_nothing_is_written(pkg):
    """csm_map, csm_map_device, csm_clean, csm_clean_device and csm_clean_step_device at 2049 active mics: AWPU_ERR_RANGE, the
    outputs and the matrix on the host and on the device left at the canary; a smaller handle's next call gives the rule's bits."""
    import torch

    B = pkg.binding
    bins, U = [47], TOO_MANY
    d_C = torch.full((U * U * 2,), float(CANARY), dtype=torch.float32, device="cuda")
    d_o = torch.full((U * U * 2,), float(CANARY), dtype=torch.float32, device="cuda")
    d_p = torch.zeros(1, dtype=torch.int32, device="cuda")
    host_C = np.full((1, U, U, 2), CANARY, np.float32)
    host_o = np.full((1, U, U, 2), CANARY, np.float32)
    cl = B.CsmClean(3, 0.5, 0.0)
    with engine_with_too_many(pkg) as eng:
        lib, h = eng._lib, eng._h
        assert eng._usable == U == 2049
        for kind in M.KINDS:
            c = B.csm_of(bins, 1, kind)
            assert lib.awpu_hip_csm_map(h, B._f32(host_C), 2, C.byref(c), B._f32(host_o), B._f32(host_o)) == B.ERR_RANGE, kind
            assert b"2048" in lib.awpu_hip_last_error()
            assert lib.awpu_hip_csm_map_device(h, C.c_void_p(d_C.data_ptr()), 2, C.byref(c), C.c_void_p(d_o.data_ptr()), C.c_void_p(d_o.data_ptr()),
                                               None) == B.ERR_RANGE, kind
        c = B.csm_of(bins, 1, CU.CONVENTIONAL)
        assert lib.awpu_hip_csm_clean(h, B._f32(host_C), 2, C.byref(c), C.byref(cl), None, B._f32(host_o), B._f32(host_o), B._f32(host_o),
                                      B._f32(host_o)) == B.ERR_RANGE
        assert lib.awpu_hip_csm_clean_device(h, C.c_void_p(d_C.data_ptr()), 2, C.byref(c), C.byref(cl), None, C.c_void_p(d_o.data_ptr()), None, None,
                                             C.c_void_p(d_o.data_ptr()), None) == B.ERR_RANGE
        assert lib.awpu_hip_csm_clean_step_device(h, C.c_void_p(d_C.data_ptr()), C.c_void_p(d_p.data_ptr()), C.byref(c), 0.5, C.c_void_p(d_o.data_ptr()),
                                                  C.c_void_p(d_o.data_ptr()), None) == B.ERR_RANGE
        torch.cuda.synchronize()
        assert (d_C.cpu().numpy() == CANARY).all() and (d_o.cpu().numpy() == CANARY).all() and (host_C == CANARY).all() and (host_o == CANARY).all()
    # the next valid call, on a smaller handle
    sh = M.Shape(pkg, "after_a_refusal", 8, 8, [6, 1, 3, 0, 7], 3, True, 53, blocks=2)
    want = sh.rule([47], 1, 2)
    with sh.engine() as eng:
        got = M.device_map(eng, want["C"], 2, [47], 1, CU.CONVENTIONAL)
        assert CU.same_bits(got["map"], want[CU.CONVENTIONAL]["map"]) and CU.same_bits(got["q"], want[CU.CONVENTIONAL]["q"])
        same = K.device_clean(eng, B, want["C"], 2, [47], 1, 2, 0.5)
        K.same_outputs(same, K.host_clean(pkg, sh, want["C"], 2, [47], 1, 2, 0.5), "after a refusal")


def test_csm_samples_has_no_bound(pkg):
    """include/awpu_hip_csm.h gives awpu_hip_csm_samples no mic bound, where the map has one: at 2049 mics it succeeds, with
    csm_accumulate_host's bits (a 129 x 129 tile grid)."""
    x = (np.random.default_rng(54).standard_normal((TOO_MANY, 256 * 2 + 40)) * 0.1).astype(np.float32)
    want, n = pkg.csm_accumulate_host(x, [47], 1, n_blocks=2)
    with engine_with_too_many(pkg) as eng:
        got, count = eng.csm_samples(x, [47], 1, n_blocks=2)
        Cm, dcount, _ = M.device_samples(eng, x, 2, [47], 1, want_spectra=False)
    assert count == dcount == n == 2 and CU.same_bits(got, want) and CU.same_bits(Cm, want)


def test_runs_refuse_more_mics_than_their_steps_take(pkg):
    """csm_watch_samples at 2049 mics (conventional) and at 513 (Capon: more than the inverse takes), csm_clean_samples at 2049:
    AWPU_ERR_RANGE; the outputs, the carry and its count, and the ring are left alone."""
    B = pkg.binding
    n_blocks, bins, length = 3, [47], 2
    x = (np.random.default_rng(55).standard_normal((TOO_MANY, 256 * n_blocks)) * 0.1).astype(np.float32)
    power = np.full((n_blocks, 2), CANARY, np.float32)
    planes = np.full((n_blocks, 1, 2), CANARY, np.float32)
    solved = np.full((n_blocks, 1), -7, np.int32)
    steps = np.full((n_blocks, 1, 2, 3), CANARY, np.float32)
    image = np.full((n_blocks, 1, 2), 0xA5, np.uint8)
    w, cl = B.Watch(0, 1, 1, 2, 0, 0, 0, None), B.CsmClean(2, 0.5, 0.0)

    def watch(eng, kind, usable):
        carry, held = np.full((length - 1, 1, usable, 2), CANARY, np.float32), C.c_int32(0)
        c = B.csm_of(bins, 1, kind, 0.05)
        rc = eng._lib.awpu_hip_csm_watch_samples(eng._h, B._f32(x), x.shape[1], n_blocks, C.byref(w), C.byref(c), length, -1, None, B._f32(carry),
                                                 C.cast(C.byref(held), B._i32p), image.ctypes.data_as(B._u8p), None, B._f32(power), None, None, B._f32(planes),
                                                 solved.ctypes.data_as(B._i32p))
        assert (carry == CANARY).all() and held.value == 0
        return rc

    def clean(eng, usable):
        carry, held = np.full((length - 1, 1, usable, 2), CANARY, np.float32), C.c_int32(0)
        c = B.csm_of(bins, 1, CU.CONVENTIONAL)
        rc = eng._lib.awpu_hip_csm_clean_samples(eng._h, B._f32(x), x.shape[1], n_blocks, C.byref(w), C.byref(c), length, -1, None, B._f32(carry),
                                                 C.cast(C.byref(held), B._i32p), C.byref(cl), B.CSM_CLEAN_CLEAN, image.ctypes.data_as(B._u8p), None,
                                                 B._f32(power), None, None, B._f32(planes), steps.ctypes.data_as(C.c_void_p))
        assert (carry == CANARY).all() and held.value == 0
        return rc

    with engine_with_too_many(pkg, max_batch=2) as eng:
        # a run the handle takes, on five of its mics, leaves the recording's tail in the ring
        eng.set_active_mics(np.array([6, 1, 3, 0, 2048], np.int32))
        ok = eng.csm_watch_samples(x, 1, 2, bins, 1, CU.CAPON, 0.05, length, -1, 0, 1, want_power=True)
        assert np.isfinite(ok.power).all() and ok.power.max() > 0
        before = eng.ring_snapshot()
        assert before.any()
        eng.set_active_mics(None)
        assert watch(eng, CU.CONVENTIONAL, TOO_MANY) == B.ERR_RANGE and b"2048" in eng._lib.awpu_hip_last_error()
        assert clean(eng, TOO_MANY) == B.ERR_RANGE
        eng.set_active_mics(np.arange(513, dtype=np.int32))
        assert watch(eng, CU.CAPON, 513) == B.ERR_RANGE and b"512" in eng._lib.awpu_hip_last_error()
        assert np.array_equal(eng.ring_snapshot(), before)  # a refused run leaves the ring as it was
    assert (power == CANARY).all() and (planes == CANARY).all() and (solved == -7).all() and (steps == CANARY).all() and (image == 0xA5).all()
