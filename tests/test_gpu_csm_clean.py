"""CLEAN-SC (step 7 of include/awpu_hip_csm.h; awpu_hip_csm_clean.h) on the device.

1. csm_clean_step_device, csm_clean and csm_clean_device equal the host rule (awpu_hip_csm_clean_*_host) bit for bit -- D, v, qs,
   steps, clean, residual, map, each output alone and together -- on the smallest shapes at which the kernels can go wrong: usable
   in {1, 2, 63, 64, 65} (a wave's edge; more than one 16 x 16 tile of the update kernel), 257 (of 320, ragged: more rows than the
   component kernel's 256 a pass, and the map kernel at 32 pixels a workgroup) and 256 (144 KiB of LDS in the map); one bin and
   eight; guard floats around every device output.
2. The loop equals the hand-driven composition: csm_map_device, the pick on the host, csm_clean_step_device.
3. The CPU edge cases on the device: a zero bin, the identity, an early stop, a non-finite bin, a bin done while the others go on.
4. EXACT and FAST handles give the same bits.
5. One call behind pending work on its stream gives a settled handle's bits (tests/stream_order.py).
6. A second call with more bins and more mics after a small one.
7. The handle refusals: nothing is enqueued and nothing is written.
8. 545 of 640 and 2048 mics (three and eight passes of the component kernel's rows) and the refusal at 2049: test_gpu_csm_large.py,
   with this file's helpers."""
import ctypes as C

import numpy as np
import pytest

import csm_clean_util as KU
import csm_util as CU
import stream_order as H
from test_gpu_csm import CANARY, GUARD, Shape, guarded, inner, shapes  # noqa: F401
from test_gpu_stream_order import busy, check, scenes  # noqa: F401

pytestmark = pytest.mark.gpu

OUTPUTS = ("steps", "clean", "residual", "map", "residual_matrix")
EIGHT = [0, 5, 17, 40, 64, 99, 127, 128]
# (bins, window, n_blocks, steps, gain)
SETTINGS = [([5], 0, 17, 6, 1.0), (EIGHT, 1, 17, 4, 0.5)]
BIG_SETTINGS = [([3, 47, 128], 1, 3, 3, 0.5)]


def same(got, want, where):
    """Bits wherever the host's value is finite or infinite; NaN exactly where the host has NaN."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, where
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (where, "NaN positions")
    assert np.array_equal(CU.bits(got)[~nan], CU.bits(want)[~nan]), where


def same_outputs(got, want, where, names=OUTPUTS):
    for name in names:
        if name == "steps":
            assert np.array_equal(got[name]["pixel"], want[name]["pixel"]), (where, got[name]["pixel"], want[name]["pixel"])
            same(got[name]["before"], want[name]["before"], (where, "before"))
            same(got[name]["removed"], want[name]["removed"], (where, "removed"))
        else:
            same(got[name], want[name], (where, name))


def sizes(eng, K, steps):
    U, P = eng._usable, eng.pixel_count
    return {"steps": (K, steps, 3), "clean": (K, P), "residual": (K, P), "map": (K, P), "residual_matrix": (K, U, U, 2)}


def device_clean(eng, B, matrix, block_count, bins, window, steps, gain, stop=0.0, want=OUTPUTS, stream=0):
    """csm_clean_device of a host matrix; every output sits between guards, which must survive; the input must stay as it was."""
    import torch

    shape = sizes(eng, len(bins), steps)
    d_C = torch.from_numpy(np.array(matrix, np.float32)).cuda()
    raw = {name: guarded(int(np.prod(shape[name]))) for name in want}
    torch.cuda.synchronize()
    eng.csm_clean_device(d_C.data_ptr(), block_count, bins, steps, gain, stop, window, stream=stream,
                         **{f"d_{name}_ptr": raw[name].data_ptr() + 4 * GUARD for name in want})
    eng.synchronize()
    assert CU.same_bits(d_C.cpu().numpy(), np.array(matrix, np.float32)), "d_matrix written"
    out = {name: inner(raw[name], shape[name], name) for name in want}
    if "steps" in out:
        out["steps"] = np.ascontiguousarray(out["steps"]).view(B.CSM_CLEAN_STEP_DTYPE).reshape(len(bins), steps)
    return out


def device_step(eng, matrix, pixels, bins, window, gain, want=("component", "qs")):
    import torch

    K, U = len(bins), eng._usable
    d_D = guarded(K * U * U * 2)
    d_D[GUARD:-GUARD] = torch.from_numpy(np.ascontiguousarray(matrix, np.float32).reshape(-1)).cuda()
    d_p = torch.from_numpy(np.ascontiguousarray(pixels, np.int32)).cuda()
    shape = {"component": (K, U, 2), "qs": (K,)}
    raw = {name: guarded(int(np.prod(shape[name]))) for name in want}
    torch.cuda.synchronize()
    eng.csm_clean_step_device(d_D.data_ptr() + 4 * GUARD, d_p.data_ptr(), bins, gain, window, **{f"d_{name}_ptr": raw[name].data_ptr() + 4 * GUARD for name in want})
    eng.synchronize()
    return inner(d_D, (K, U, U, 2), "matrix"), {name: inner(raw[name], shape[name], name) for name in want}


def host_clean(pkg, sh, Cm, n, bins, window, steps, gain, stop=0.0):
    return pkg.csm_clean_host(Cm, n, sh.off, sh.frac, bins, steps, gain, stop, window, index=sh.index, want=OUTPUTS)


# ------------------------------------------------------------------------------------------------ 1. the rule's bits

def check_against_host_rule(pkg, sh, settings, alone=True):
    B = pkg.binding
    with sh.engine() as eng:
        before = eng.stats().kernel_variant
        for bins, window, n_blocks, steps, gain in settings:
            where = (sh.name, bins)
            Cm = sh.rule(bins, window, n_blocks)["C"]
            want = host_clean(pkg, sh, Cm, n_blocks, bins, window, steps, gain)
            assert (want["steps"]["pixel"][:, 0] >= 0).all(), where
            got = device_clean(eng, B, Cm, n_blocks, bins, window, steps, gain)
            same_outputs(got, want, where)
            if alone:
                for name in OUTPUTS:  # each output alone: the same bits (without residual_matrix the working D is the handle's)
                    same_outputs(device_clean(eng, B, Cm, n_blocks, bins, window, steps, gain, want=(name,)), got, (where, name, "alone"), (name,))
            same_outputs(eng.csm_clean(Cm, n_blocks, bins, steps, gain, 0.0, window, want=OUTPUTS), got, (where, "host form"))
            same_outputs(eng.csm_clean(Cm, n_blocks, bins, steps, gain, 0.0, window, want=("clean",)), got, (where, "host form, alone"), ("clean",))
            # the step at the first picks, on a matrix whose upper triangle and diagonal im are garbage; one bin skipped where there are several
            pixels = want["steps"]["pixel"][:, 0].astype(np.int32)
            if len(bins) > 1:
                pixels[1] = -1
                pixels[-1] = sh.P  # (outside the table: skipped too)
            dirty = np.array(Cm)
            upper = np.triu(np.ones((sh.U, sh.U), bool), 1)
            dirty[:, upper] = 7.0e5
            dirty[:, np.arange(sh.U), np.arange(sh.U), 1] = -2.0
            D_want, out_want = pkg.csm_clean_step_host(dirty, pixels, sh.off, sh.frac, bins, gain, window, index=sh.index)
            D_got, out_got = device_step(eng, dirty, pixels, bins, window, gain)
            same(D_got, D_want, (where, "step D"))
            same(out_got["component"], out_want["component"], (where, "v"))
            same(out_got["qs"], out_want["qs"], (where, "qs"))
            D_alone, _ = device_step(eng, dirty, pixels, bins, window, gain, want=())
            same(D_alone, D_want, (where, "step D, no exports"))
        assert eng.stats().kernel_variant == before  # CSM calls leave it alone


@pytest.fixture(scope="module")
def sixty_three(pkg):
    return Shape(pkg, "sixty_three", 64, 64, list(range(63)), 100, False, 9)


@pytest.mark.parametrize("name", ["one_mic", "two_mics", "sixty_four", "sixty_five_of_128"])
def test_device_equals_the_host_rule(pkg, shapes, name):  # noqa: F811
    check_against_host_rule(pkg, shapes[name], SETTINGS)


def test_device_equals_the_host_rule_at_63_mics(pkg, sixty_three):
    check_against_host_rule(pkg, sixty_three, SETTINGS)


@pytest.mark.parametrize("name", ["two_fifty_six", "two_fifty_seven_of_320"])
def test_device_equals_the_host_rule_above_a_pass_of_rows(pkg, shapes, name):  # noqa: F811
    """257 active mics (of 320, ragged, with gains): the component kernel's lanes take a second pass for row 256, the update kernel
    a 17th tile, and the map kernel 32 pixels a workgroup; 256: the last full pass, and 144 KiB of LDS in the map."""
    check_against_host_rule(pkg, shapes[name], BIG_SETTINGS, alone=False)


# ------------------------------------------------------------------------------------------------ 2. composition

def test_the_loop_equals_the_hand_driven_composition(pkg, shapes):  # noqa: F811
    import torch

    B = pkg.binding
    sh = shapes["sixty_five_of_128"]
    bins, window, n_blocks, steps, gain, stop = EIGHT, 1, 17, 5, 0.5, 0.3
    K, U, P = len(bins), sh.U, sh.P
    Cm = sh.rule(bins, window, n_blocks)["C"]
    with sh.engine() as eng:
        got = device_clean(eng, B, Cm, n_blocks, bins, window, steps, gain, stop)
        d_D = torch.from_numpy(np.array(Cm)).cuda()
        d_plane = torch.empty(K * P, device="cuda")
        rec = np.zeros((K, steps), B.CSM_CLEAN_STEP_DTYPE)
        rec["pixel"] = -1
        done, first = np.zeros(K, bool), np.zeros(K, np.float32)
        for i in range(steps):
            eng.csm_map_device(d_D.data_ptr(), n_blocks, bins, window, CU.CONVENTIONAL, d_plane.data_ptr())
            eng.synchronize()
            rows = d_plane.cpu().numpy().reshape(K, P)
            pixels = np.full(K, -1, np.int32)
            for k in np.flatnonzero(~done):
                p = KU.pick(rows[k])
                if p >= 0 and i == 0:
                    first[k] = rows[k, p]
                if p < 0 or rows[k, p] < np.float32(stop) * first[k]:
                    done[k] = True
                else:
                    pixels[k] = p
            d_p = torch.from_numpy(pixels).cuda()
            d_qs = torch.empty(K, device="cuda")
            eng.csm_clean_step_device(d_D.data_ptr(), d_p.data_ptr(), bins, gain, window, d_qs_ptr=d_qs.data_ptr())
            eng.synchronize()
            qs = d_qs.cpu().numpy()
            for k in np.flatnonzero(pixels >= 0):
                if qs[k] > 0 and np.isfinite(qs[k]):
                    rec[k, i] = (pixels[k], rows[k, pixels[k]], np.float32(gain) * rows[k, pixels[k]])
                else:
                    done[k] = True
        eng.csm_map_device(d_D.data_ptr(), n_blocks, bins, window, CU.CONVENTIONAL, d_plane.data_ptr())
        eng.synchronize()
        taken = (rec["pixel"] >= 0).sum(axis=1)
        print("steps taken per bin:", taken)
        assert taken.min() < steps and taken.max() >= 2  # (some bin stops early while the others go on)
        assert np.array_equal(got["steps"], rec)
        assert CU.same_bits(got["residual"], d_plane.cpu().numpy().reshape(K, P))
        assert CU.same_bits(got["residual_matrix"], d_D.cpu().numpy().reshape(K, U, U, 2))


# ------------------------------------------------------------------------------------------------ 3. edges

def test_edges_on_the_device(pkg, shapes):  # noqa: F811
    B = pkg.binding
    sh = shapes["ragged5"]
    bins, window, n_blocks = [3, 47, 128], 1, 17
    Cm = sh.rule(bins, window, n_blocks)["C"]
    zero = np.array(Cm)
    zero[1] = 0.0
    eye = np.zeros_like(Cm)
    eye[:, np.arange(sh.U), np.arange(sh.U), 0] = 1.0
    inf, nan = np.array(Cm), np.array(Cm)
    inf[1, 3, 1, 0] = np.inf
    nan[1, 3, 1, 1] = np.nan
    with sh.engine() as eng, np.errstate(all="ignore"):
        for what, matrix, steps, gain, stop in (("zero bin", zero, 4, 1.0, 0.0), ("identity", eye, 2, 1.0, 0.0), ("early stop", Cm, 8, 0.5, 0.5),
                                               ("inf", inf, 4, 1.0, 0.0), ("nan", nan, 4, 1.0, 0.0)):
            want = host_clean(pkg, sh, matrix, n_blocks, bins, window, steps, gain, stop)
            got = device_clean(eng, B, matrix, n_blocks, bins, window, steps, gain, stop)
            same_outputs(got, want, what)
            same_outputs(eng.csm_clean(matrix, n_blocks, bins, steps, gain, stop, window, want=OUTPUTS), want, (what, "host form"))
            taken = (want["steps"]["pixel"] >= 0).sum(axis=1)
            print(what, "steps taken:", taken)
            if what == "zero bin":
                assert taken[1] == 0 and taken[0] == taken[2] == 4 and not got["clean"][1].any() and not got["residual"][1].any()
            if what == "identity":
                assert (got["steps"]["pixel"][:, 0] == 0).all()
            if what == "early stop":
                assert (taken >= 1).all() and (taken < 8).all()
            if what in ("inf", "nan"):
                base = host_clean(pkg, sh, Cm, n_blocks, bins, window, steps, gain, stop)
                same_outputs({k: v[[0, 2]] for k, v in got.items()}, {k: v[[0, 2]] for k, v in base.items()}, (what, "the other bins"))


# ------------------------------------------------------------------------------------------------ 4. math modes

def test_exact_and_fast_handles_give_the_same_bits(pkg, shapes):  # noqa: F811
    B = pkg.binding
    sh = shapes["sixty_five_of_128"]
    bins, window, n_blocks, steps, gain = SETTINGS[1]
    Cm = sh.rule(bins, window, n_blocks)["C"]
    want = host_clean(pkg, sh, Cm, n_blocks, bins, window, steps, gain)
    for math in (pkg.MATH_F32_EXACT, pkg.MATH_F32_FAST):
        with sh.engine(math=math) as eng:
            same_outputs(device_clean(eng, B, Cm, n_blocks, bins, window, steps, gain), want, math)


# ------------------------------------------------------------------------------------------------ 5. stream order

def test_csm_clean_device_behind_pending_work(pkg, scenes, busy):  # noqa: F811
    sc = scenes(16)
    bins, steps = [3, 47, 128], 4
    matrices = tuple(pkg.csm_accumulate_host(x, bins, 1)[0] for x in sc.samples)
    outs = {"steps": ((3, steps, 3), np.float32), "clean": ((3, sc.P), np.float32), "residual": ((3, sc.P), np.float32), "map": ((3, sc.P), np.float32),
            "residual_matrix": ((3, 64, 64, 2), np.float32)}
    case = H.Case(sc.engine(), {"matrix": matrices}, outs,
                  lambda e, i, o, s: e.csm_clean_device(i["matrix"], 5, bins, steps, 0.5, 0.0, 1, CU.CONVENTIONAL, o["steps"], o["clean"], o["residual"],
                                                        o["map"], o["residual_matrix"], s))
    got = check(case, busy)
    want = pkg.csm_clean_host(matrices[0], 5, sc.off, sc.frac, bins, steps, 0.5, 0.0, 1, want=OUTPUTS)
    got["steps"] = np.ascontiguousarray(got["steps"]).view(pkg.binding.CSM_CLEAN_STEP_DTYPE).reshape(3, steps)
    same_outputs(got, want, "behind pending work")


def test_csm_clean_step_device_behind_pending_work(pkg, scenes, busy):  # noqa: F811
    sc = scenes(16)
    bins = [3, 47, 128]
    matrices = tuple(pkg.csm_accumulate_host(x, bins, 1)[0] for x in sc.samples)
    pixels = (np.array([40, -1, 200], np.int32), np.array([7, 9, 11], np.int32))
    case = H.Case(sc.engine(), {"matrix": matrices, "pixel": pixels}, {"component": ((3, 64, 2), np.float32), "qs": ((3,), np.float32)},
                  lambda e, i, o, s: e.csm_clean_step_device(i["matrix"], i["pixel"], bins, 1.0, 1, CU.CONVENTIONAL, o["component"], o["qs"], s),
                  inout=("matrix",))
    got = check(case, busy)
    D, out = pkg.csm_clean_step_host(matrices[0], pixels[0], sc.off, sc.frac, bins, 1.0, 1)
    assert CU.same_bits(got["matrix"], D) and CU.same_bits(got["component"], out["component"]) and CU.same_bits(got["qs"], out["qs"])


# ------------------------------------------------------------------------------------------------ 6. growth

def test_a_larger_call_after_a_small_one(pkg, shapes):  # noqa: F811
    """The handle's buffers (the working matrix, v, the planes, a host form's staging) are sized by the first call; a second call
    with more mics and more bins allocates them again."""
    B = pkg.binding
    sh = shapes["sixty_five_of_128"]
    half = sh.index[::3]
    with sh.engine() as eng:
        eng.set_active_mics(half)
        gl = None if sh.gains is None else sh.gains[half]
        Cs, n = pkg.csm_accumulate_host(sh.samples_of(17), [5], 0, index=half, gain=gl, n_blocks=17)
        want = pkg.csm_clean_host(Cs, n, sh.off, sh.frac, [5], 3, 1.0, 0.0, 0, index=half, want=OUTPUTS)
        same_outputs(device_clean(eng, B, Cs, n, [5], 0, 3, 1.0, want=("steps", "clean", "residual", "map")), want, "small", ("steps", "clean", "residual", "map"))
        same_outputs(eng.csm_clean(Cs, n, [5], 3, 1.0, 0.0, 0, want=OUTPUTS), want, "small, host form")
        eng.set_active_mics(sh.index)
        bins, window, n_blocks, steps, gain = SETTINGS[1]
        Cm = sh.rule(bins, window, n_blocks)["C"]
        want = host_clean(pkg, sh, Cm, n_blocks, bins, window, steps, gain)
        same_outputs(device_clean(eng, B, Cm, n_blocks, bins, window, steps, gain, want=("steps", "clean", "residual", "map")), want, "large",
                     ("steps", "clean", "residual", "map"))
        same_outputs(eng.csm_clean(Cm, n_blocks, bins, steps, gain, 0.0, window, want=OUTPUTS), want, "large, host form")


# ------------------------------------------------------------------------------------------------ 7. refusals

def test_handle_forms_refuse(pkg, shapes, scenes):  # noqa: F811
    """FIR8, a band on the handle, a device group, a call during process_async, a slab handle, no table: AWPU_ERR_STATE; kinds 1, 2
    and 3, a bad cl or gain, a bad request, a block count of 0, null buffers, no output, an overlapping residual matrix:
    AWPU_ERR_INVALID.  Nothing is written."""
    import torch

    B = pkg.binding
    sc = scenes(16)
    bins, steps = [3, 47], 4
    d_C = torch.full((2 * 64 * 64 * 2,), float(CANARY), dtype=torch.float32, device="cuda")
    d_o = torch.full((2 * 64 * 64 * 2,), float(CANARY), dtype=torch.float32, device="cuda")
    d_p = torch.zeros(2, dtype=torch.int32, device="cuda")
    host_C = np.full((2, 64, 64, 2), CANARY, np.float32)
    host_o = np.full((2, sc.P), CANARY, np.float32)

    def refused(eng, which=(0, 1, 2), bins=bins, kind=CU.CONVENTIONAL, cl=(steps, 1.0, 0.0), matrix=True, out=True, pixel=True, blocks=5, rm=0):
        """The statuses of 0 csm_clean_device, 1 csm_clean_step_device, 2 awpu_hip_csm_clean."""
        c, k = B.csm_of(bins, 1, kind), B.CsmClean(*cl)
        calls = (lambda: eng._lib.awpu_hip_csm_clean_device(eng._h, C.c_void_p(d_C.data_ptr() if matrix else 0), blocks, C.byref(c), C.byref(k), None,
                                                            C.c_void_p(d_o.data_ptr() if out else 0), None, None, C.c_void_p(rm), None),
                 lambda: eng._lib.awpu_hip_csm_clean_step_device(eng._h, C.c_void_p(d_C.data_ptr() if matrix else 0), C.c_void_p(d_p.data_ptr() if pixel else 0),
                                                                 C.byref(c), cl[1], C.c_void_p(d_o.data_ptr() if out else 0), None, None),
                 lambda: eng._lib.awpu_hip_csm_clean(eng._h, B._f32(host_C) if matrix else None, blocks, C.byref(c), C.byref(k), None,
                                                     B._f32(host_o) if out else None, None, None, None))
        return [calls[i]() for i in which]

    inv, state = B.ERR_INVALID, B.ERR_STATE
    with sc.engine()() as eng:
        for kind in (CU.DIAGONAL_REMOVED, CU.CAPON, 3):
            assert refused(eng, kind=kind) == [inv] * 3, kind
        assert refused(eng, bins=[47, 3]) == [inv] * 3 and refused(eng, bins=[3, 129]) == [inv] * 3
        for cl in ((0, 1.0, 0.0), (33, 1.0, 0.0), (4, 1.0, 1.0), (4, 1.0, -0.5)):
            assert refused(eng, (0, 2), cl=cl) == [inv] * 2, cl
        for gain in (0.0, 1.5, float("nan")):
            assert refused(eng, cl=(4, gain, 0.0)) == [inv] * 3, gain
        assert refused(eng, matrix=False) == [inv] * 3
        assert refused(eng, (0, 2), out=False) == [inv] * 2
        assert refused(eng, (1,), pixel=False) == [inv]
        assert refused(eng, (0, 2), blocks=0) == [inv] * 2
        assert refused(eng, (0,), rm=d_C.data_ptr() + 64) == [inv]  # the residual matrix overlaps the input
        eng.set_band(pkg.band_design(1000.0, 4000.0, 31))
        assert refused(eng) == [state] * 3
        eng.set_band(None)
        eng.process_async(sc.frames[0][:1])
        assert refused(eng) == [state] * 3
        eng.wait()
    with pkg.Engine(n_pixels=sc.P, n_streams=64, interp=B.INTERP_FIR8) as eng:
        eng.set_delay_table(sc.off, sc.frac)
        eng.set_active_mics(None)
        assert refused(eng) == [state] * 3
    with pkg.Engine(n_pixels=sc.P, n_streams=64, grid_columns=16, devices=[0, 0]) as eng:  # a device group
        eng.set_delay_table(sc.off, sc.frac)
        eng.set_active_mics(None)
        assert refused(eng) == [state] * 3
    with pkg.Engine(n_pixels=sc.P, n_streams=64, pixel_begin=32, pixel_count=64) as eng:  # a slab handle: the pick needs the whole map
        eng.set_delay_table(sc.off[32:96], sc.frac[32:96])
        eng.set_active_mics(None)
        assert refused(eng) == [state] * 3
    with pkg.Engine(n_pixels=sc.P, n_streams=64) as eng:  # no table, no mics
        assert refused(eng) == [state] * 3
    null = pkg.Engine(n_pixels=sc.P, n_streams=64)
    with null as eng:
        h, eng._h = eng._h, None
        try:
            assert refused(eng) == [inv] * 3
        finally:
            eng._h = h
    torch.cuda.synchronize()
    assert (d_C.cpu().numpy() == CANARY).all() and (d_o.cpu().numpy() == CANARY).all() and (host_C == CANARY).all() and (host_o == CANARY).all()
