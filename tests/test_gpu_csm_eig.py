"""Step 8 of include/awpu_hip_csm.h on the device (include/awpu_hip_csm_eig.h): the eigendecomposition, the weighed matrix and the
two subspace maps.

1. csm_eig_device equals csm_eig_host bit for bit -- values, vectors, solved and sweep words -- on 1, 2, 3, 5, 8, 9, 32, 33, 63, 64,
   65 and 96 mics (one entry; odd sizes with the dummy that sits out; the Jacobi kernel's 64 threads up to 8 mics, 256 from 9 to
   32 and 1024 from 33 on, each tier at both of its edges; the last size whose A and V live in LDS and the first that lives in
   the scratch) with 1, 3 and 8 bins, a rank-deficient matrix included; guards intact; the synchronous csm_eig gives the same.
   The sizes from 128 mics to the bound of 256 are test_gpu_csm_eig_edges.py's (BOUND_MICS below are its lists).
2. Composition: csm_eig_weigh_device equals csm_eig_weigh_host, both kinds, root 0 and 4, n_sources 0, 2 and U - 1;
   csm_eig_map_device equals csm_eig_map_host of the host's decomposition, and equals the steps one by one on the device -- eig,
   weigh, csm_map_device's q, the finish (restated in numpy float32); a slab handle maps its own pixels.
3. Edges: an unsolved bin among solved ones, in both forms; work pending on the stream in front and behind with no host
   synchronisation (tests/stream_order.py); the refusals, each leaving the outputs untouched."""
import ctypes as C

import numpy as np
import pytest

import csm_eig_util as EU
import csm_util as CU
import stream_order as H
from test_gpu_stream_order import busy, check, scenes  # noqa: F401

pytestmark = pytest.mark.gpu

GUARD = 64
CANARY = np.float32(-3.0)
EIGHT = [0, 3, 16, 47, 100, 101, 127, 128]
THREE = [3, 16, 128]
PIXELS = 300  # more than one workgroup of the map kernel and of the finish
# U -> (n_streams, active list): ragged lists from three mics on
MICS = {1: (8, [3]),
        2: (8, [5, 2]),
        3: (8, [6, 1, 3]),
        5: (8, [6, 1, 3, 0, 7]),
        8: (8, list(range(8))),                               # the last size of 64 threads
        9: (12, [i for i in range(12) if i % 4 != 1]),        # the first of 256, ragged
        32: (32, list(range(32))),                            # the last of 256
        33: (40, [i for i in range(40) if i % 6 != 5][1:]),   # the first of 1024
        63: (64, [i for i in range(64) if i != 40]),
        64: (64, list(range(64))),
        65: (128, list(range(0, 128, 2)) + [127]),
        96: (96, list(range(96)))}
# the lists of test_gpu_csm_eig_edges.py, up to AWPU_CSM_EIG_MAX_MICS: too large for the eight-bin settings of this file's tests
BOUND_MICS = {128: (128, list(range(128))),
              129: (160, [i for i in range(160) if i % 5 != 4] + [159]),  # ragged and odd
              255: (256, [i for i in range(256) if i != 100]),
              256: (256, list(range(256)))}
assert all(len(index) == U for U, (_, index) in {**MICS, **BOUND_MICS}.items())


class Rig:
    """The table of a mic list, seeded: off and frac [PIXELS, n_streams], and handles on it."""

    def __init__(self, pkg, U):
        self.pkg, self.U = pkg, U
        self.S, index = MICS[U] if U in MICS else BOUND_MICS[U]
        self.index = np.asarray(index, np.int32)
        rng = np.random.default_rng(900 + U)
        self.off = rng.integers(0, 700, (PIXELS, self.S)).astype(np.int32)
        self.frac = rng.random((PIXELS, self.S)).astype(np.float32)

    def engine(self, pixel_begin=0, pixel_count=0, **kw):
        lo, hi = pixel_begin, pixel_begin + (pixel_count or PIXELS)
        eng = self.pkg.Engine(n_pixels=PIXELS, n_streams=self.S, pixel_begin=pixel_begin, pixel_count=pixel_count, **kw)
        eng.set_delay_table(self.off[lo:hi], self.frac[lo:hi])
        eng.set_active_mics(self.index)
        return eng


_matrices = {}


def matrix_of(U, K, n_blocks):
    """A seeded matrix of two strong sources in noise (computed once per setting, left unchanged)."""
    key = (U, K, n_blocks)
    if key not in _matrices:
        Cm = EU.random_matrix(np.random.default_rng(31 * U + 7 * K + n_blocks), K, U, n_blocks)
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


def device_eig(eng, Cm, n, bins, want_words=True, stream=0):
    """csm_eig_device on guarded buffers -> (values, vectors, solved, sweeps) on the host, and the device tensors of the first two."""
    import torch

    K, U = Cm.shape[0], Cm.shape[1]
    d_C = torch.from_numpy(np.array(Cm, np.float32)).cuda()
    d_val, d_vec = guarded(K * U, torch.float32, float(CANARY)), guarded(K * U * U * 2, torch.float32, float(CANARY))
    d_s, d_w = guarded(K, torch.int32, -7), guarded(K, torch.int32, -7)
    torch.cuda.synchronize()
    eng.csm_eig_device(d_C.data_ptr(), n, bins, d_val.data_ptr() + 4 * GUARD, d_vec.data_ptr() + 4 * GUARD,
                       d_s.data_ptr() + 4 * GUARD if want_words else 0, d_w.data_ptr() + 4 * GUARD if want_words else 0, stream)
    eng.synchronize()
    solved, sweeps = inner(d_s, (K,), -7, "solved"), inner(d_w, (K,), -7, "sweeps")
    assert want_words or ((solved == -7).all() and (sweeps == -7).all())
    return (inner(d_val, (K, U), CANARY, "values"), inner(d_vec, (K, U, U, 2), CANARY, "vectors"), solved, sweeps), (d_val, d_vec)


def device_weigh(eng, d_val, d_vec, K, U, bins, kind, n_sources, root):
    import torch

    d_H = guarded(K * U * U * 2, torch.float32, float(CANARY))
    eng.csm_eig_weigh_device(d_val.data_ptr() + 4 * GUARD, d_vec.data_ptr() + 4 * GUARD, bins, d_H.data_ptr() + 4 * GUARD, kind, n_sources, root)
    eng.synchronize()
    return inner(d_H, (K, U, U, 2), CANARY, "weighed"), d_H


def device_eig_map(eng, Cm, n, bins, kind, n_sources, root, window, want=("values", "solved"), stream=0):
    import torch

    K, U, P = Cm.shape[0], Cm.shape[1], eng.pixel_count
    d_C = torch.from_numpy(np.array(Cm, np.float32)).cuda()
    d_map, d_val, d_s = guarded(K * P, torch.float32, float(CANARY)), guarded(K * U, torch.float32, float(CANARY)), guarded(K, torch.int32, -7)
    torch.cuda.synchronize()
    eng.csm_eig_map_device(d_C.data_ptr(), n, bins, d_map.data_ptr() + 4 * GUARD, kind, n_sources, root, window,
                           d_val.data_ptr() + 4 * GUARD if "values" in want else 0, d_s.data_ptr() + 4 * GUARD if "solved" in want else 0, stream)
    eng.synchronize()
    values, solved = inner(d_val, (K, U), CANARY, "values"), inner(d_s, (K,), -7, "solved")
    assert "values" in want or (values == CANARY).all()
    assert "solved" in want or (solved == -7).all()
    return inner(d_map, (K, P), CANARY, "map"), values, solved


def same(got, want):
    return all(CU.same_bits(g, w) for g, w in zip(got, want))


# ------------------------------------------------------------------------------------------------ 1. the rule's bits

def device_equals(eng, Cm, n, bins, want):
    """csm_eig_device against `want`, a result of csm_eig_host -> the device's own (values, vectors, solved, sweeps)."""
    got, _ = device_eig(eng, Cm, n, bins)
    print(Cm.shape, n, "sweeps", want[3].tolist(), got[3].tolist())
    assert got[2].tolist() == want[2].tolist() and got[3].tolist() == want[3].tolist()
    assert same(got, want)
    assert same(device_eig(eng, Cm, n, bins, want_words=False)[0][:2], want[:2])  # without the words: the same bits
    return got


def check_bits(pkg, eng, Cm, n, bins, expect=None):
    want = pkg.csm_eig_host(Cm, n, bins)
    assert want[2].tolist() == (expect or [1] * len(bins))
    device_equals(eng, Cm, n, bins, want)
    return want


@pytest.mark.parametrize("U", sorted(MICS))
def test_device_eig_equals_the_host_rule(pkg, U):
    with Rig(pkg, U).engine() as eng:
        for bins in ([16], THREE, EIGHT):
            if U in (63, 96) and len(bins) == 8:
                continue  # (eight bins at 64 and 65 mics, on both sides of the LDS bound)
            check_bits(pkg, eng, matrix_of(U, len(bins), 2 * U + 3), 2 * U + 3, bins)
        if U >= 5:  # rank-deficient: fewer blocks than mics
            check_bits(pkg, eng, matrix_of(U, 3, U // 4), U // 4, THREE)
        Cm, n = matrix_of(U, 3, 2 * U + 3), 2 * U + 3
        assert same(eng.csm_eig(Cm, n, THREE), pkg.csm_eig_host(Cm, n, THREE))  # the synchronous form


# ------------------------------------------------------------------------------------------------ 2. composition

REQUESTS = [(EU.MUSIC, 0, 0), (EU.MUSIC, 2, 0), (EU.MUSIC, -1, 0), (EU.FUNCTIONAL, 0, 0), (EU.FUNCTIONAL, 0, 4)]  # n_sources -1: U - 1


def check_composition(pkg, rig, eng, Cm, n, bins, window, requests, host):
    """Steps 8a to 8c of Cm on the device against the host functions, with `host` the (values, vectors, solved) of csm_eig_host:
    the weighed matrix, the map, the map without its optional outputs, the steps one by one, and the synchronous form."""
    import torch

    U, K = rig.U, len(bins)
    val, vec, solved = host
    got, (d_val, d_vec) = device_eig(eng, Cm, n, bins)
    assert same(got[:3], (val, vec, solved))
    for kind, n_sources, root in requests:
        n_sources = U - 1 if n_sources < 0 else n_sources
        Hw = pkg.csm_eig_weigh_host(val, vec, bins, kind, n_sources, root)
        Hd, d_H = device_weigh(eng, d_val, d_vec, K, U, bins, kind, n_sources, root)
        assert CU.same_bits(Hd, Hw), (kind, n_sources, root)
        want = pkg.csm_eig_map_host(Hw, solved, rig.off, rig.frac, bins, kind, n_sources, root, window, index=rig.index)
        m, v, s = device_eig_map(eng, Cm, n, bins, kind, n_sources, root, window)
        assert CU.same_bits(m, want) and CU.same_bits(v, val) and s.tolist() == [1] * K, (kind, n_sources, root)
        assert CU.same_bits(device_eig_map(eng, Cm, n, bins, kind, n_sources, root, window, want=())[0], want)
        # the steps one by one: q of the weighed matrix by the map's own call, then the finish
        d_q = guarded(K * PIXELS, torch.float32, float(CANARY))
        eng.csm_map_device(d_H.data_ptr() + 4 * GUARD, 1, bins, window, CU.CONVENTIONAL, d_q_ptr=d_q.data_ptr() + 4 * GUARD)
        eng.synchronize()
        q = inner(d_q, (K, PIXELS), CANARY, "q")
        assert CU.same_bits(EU.finish(q, solved, bins, window, U, kind, root), m), (kind, n_sources, root)
        # the synchronous form
        out = eng.csm_eig_map(Cm, n, bins, kind, n_sources, root, window, want=("map", "values", "solved"))
        assert CU.same_bits(out["map"], want) and CU.same_bits(out["values"], val) and out["solved"].tolist() == [1] * K


@pytest.mark.parametrize("U", [5, 64, 65])
def test_composition(pkg, U):
    rig = Rig(pkg, U)
    bins, window = THREE, 1
    n = 2 * U + 3
    Cm = matrix_of(U, 3, n)
    val, vec, solved, _ = pkg.csm_eig_host(Cm, n, bins)
    with rig.engine() as eng:
        check_composition(pkg, rig, eng, Cm, n, bins, window, REQUESTS, (val, vec, solved))
    # a slab handle maps its own pixels
    lo, count = 32, 70
    kind, n_sources, root = EU.MUSIC, 2, 0
    want = pkg.csm_eig_map_host(pkg.csm_eig_weigh_host(val, vec, bins, kind, n_sources, root), solved, rig.off, rig.frac, bins, kind, n_sources, root,
                                window, index=rig.index)
    with rig.engine(pixel_begin=lo, pixel_count=count) as eng:
        assert eng.pixel_count == count
        m, _, _ = device_eig_map(eng, Cm, n, bins, kind, n_sources, root, window)
        assert m.shape == (3, count) and CU.same_bits(m, want[:, lo:lo + count])
        assert CU.same_bits(eng.csm_eig_map(Cm, n, bins, kind, n_sources, root, window)["map"], want[:, lo:lo + count])


# ------------------------------------------------------------------------------------------------ 3. edges

@pytest.mark.parametrize("U", [5, 65])
def test_an_unsolved_bin_among_solved_ones(pkg, U):
    """A NaN below the diagonal, an inf on it, a negative trace and all zeros, each in one bin of three: that bin +0 with solved 0
    -- and a +0 plane in both maps --, the others the rule's bits."""
    rig = Rig(pkg, U)
    n = 2 * U + 3
    base = matrix_of(U, 3, n)
    with rig.engine() as eng:
        for what, bin_ in (("nan", 1), ("inf", 0), ("negative", 2), ("zeros", 1)):
            Cm = base.copy()
            if what == "nan":
                Cm[bin_, U - 1, U // 2, 1] = np.nan
            elif what == "inf":
                Cm[bin_, U // 2, U // 2, 0] = np.inf
            elif what == "negative":
                Cm[bin_, np.arange(U), np.arange(U), 0] *= -1.0
            else:
                Cm[bin_] = 0.0
            expect = [0 if k == bin_ else 1 for k in range(3)]
            val, vec, solved, _ = check_bits(pkg, eng, Cm, n, THREE, expect)
            assert not val[bin_].any() and not vec[bin_].any() and not np.signbit(vec[bin_]).any()
            for kind, n_sources, root in ((EU.MUSIC, 2, 0), (EU.FUNCTIONAL, 0, 4)):
                Hw = pkg.csm_eig_weigh_host(val, vec, THREE, kind, n_sources, root)
                want = pkg.csm_eig_map_host(Hw, solved, rig.off, rig.frac, THREE, kind, n_sources, root, 0, index=rig.index)
                m, v, s = device_eig_map(eng, Cm, n, THREE, kind, n_sources, root, 0)
                assert s.tolist() == expect and CU.same_bits(m, want) and CU.same_bits(v, val)
                assert not m[bin_].any() and not np.signbit(m[bin_]).any() and not np.isnan(m).any()


def test_behind_pending_work(pkg, scenes, busy):  # noqa: F811
    sc = scenes(16)
    bins = [3, 47, 128]
    matrices = tuple(pkg.csm_accumulate_host(x, bins, 1)[0] for x in sc.samples)  # (fewer blocks than mics: rank-deficient)
    n = sc.samples[0].shape[1] // 256
    val, vec, solved, sweeps = pkg.csm_eig_host(matrices[0], n, bins)
    case = H.Case(sc.engine(), {"matrix": matrices},
                  {"values": ((3, 64), np.float32), "vectors": ((3, 64, 64, 2), np.float32), "solved": ((3,), np.int32), "sweeps": ((3,), np.int32)},
                  lambda e, i, o, s: e.csm_eig_device(i["matrix"], n, bins, o["values"], o["vectors"], o["solved"], o["sweeps"], s))
    got = check(case, busy)
    assert same((got["values"], got["vectors"], got["solved"], got["sweeps"]), (val, vec, solved, sweeps))
    for kind, n_sources, root in ((EU.MUSIC, 2, 0), (EU.FUNCTIONAL, 0, 4)):
        case = H.Case(sc.engine(), {"matrix": matrices}, {"map": ((3, sc.P), np.float32), "values": ((3, 64), np.float32), "solved": ((3,), np.int32)},
                      lambda e, i, o, s: e.csm_eig_map_device(i["matrix"], n, bins, o["map"], kind, n_sources, root, 1, o["values"], o["solved"], s))
        got = check(case, busy)
        want = pkg.csm_eig_map_host(pkg.csm_eig_weigh_host(val, vec, bins, kind, n_sources, root), solved, sc.off, sc.frac, bins, kind, n_sources, root, 1)
        assert CU.same_bits(got["map"], want) and CU.same_bits(got["values"], val) and got["solved"].tolist() == [1, 1, 1]


def test_refusals_leave_the_outputs_untouched(pkg, scenes):  # noqa: F811
    import torch

    B = pkg.binding
    sc = scenes(16)
    bins = [3]
    Cs = np.zeros((1, 64, 64, 2), np.float32)
    Cs[0, np.arange(64), np.arange(64), 0] = 1.0
    d = torch.full((Cs.size,), float(CANARY), dtype=torch.float32, device="cuda")
    out = np.full(Cs.size, CANARY, np.float32)
    p = d.data_ptr()

    def status(call):
        try:
            call()
            return B.OK
        except pkg.AwpuError as e:
            return e.status

    def calls(eng, kind=EU.MUSIC, n_sources=0, root=0, c_kind=0):
        c, e = B.csm_of(bins, 0, c_kind), B.csm_eig_of(kind, n_sources, root)
        return [lambda: eng.csm_eig_weigh_device(p, p, c, p, e),
                lambda: eng.csm_eig_map_device(p, 1, c, p, e),
                lambda: B._check(eng._lib.awpu_hip_csm_eig_map(eng._h, B._f32(Cs), 1, C.byref(c), C.byref(e), B._f32(out), None, None), "csm_eig_map")]

    def every(eng):
        return [lambda: eng.csm_eig_device(p, 1, bins, p, p),
                lambda: B._check(eng._lib.awpu_hip_csm_eig(eng._h, B._f32(Cs), 1, C.byref(B.csm_of(bins)), B._f32(out), B._f32(out), None, None), "csm_eig"),
                *calls(eng)]

    with sc.engine()() as eng:
        # the invalid requests: awpu_csm_eig_t, c->kind, nulls, the block count
        for bad in (dict(kind=2), dict(kind=-1), dict(n_sources=64), dict(n_sources=-1), dict(root=7), dict(root=-1),
                    dict(kind=EU.FUNCTIONAL, n_sources=64), dict(c_kind=CU.CAPON), dict(c_kind=CU.DIAGONAL_REMOVED)):
            assert [status(call) for call in calls(eng, **bad)] == [B.ERR_INVALID] * 3, bad
        reserved = B.CsmEig(0, 0, 0, 5)
        assert status(lambda: eng.csm_eig_map_device(p, 1, bins, p, reserved)) == status(lambda: eng.csm_eig_weigh_device(p, p, bins, p, reserved)) == B.ERR_INVALID
        for call in (lambda: eng.csm_eig_device(0, 1, bins, p, p), lambda: eng.csm_eig_device(p, 1, bins, 0, p), lambda: eng.csm_eig_device(p, 1, bins, p, 0),
                     lambda: eng.csm_eig_device(p, 0, bins, p, p), lambda: eng.csm_eig_device(p, 1, [16, 3], p, p),
                     lambda: eng.csm_eig_weigh_device(0, p, bins, p), lambda: eng.csm_eig_weigh_device(p, p, bins, 0),
                     lambda: eng.csm_eig_map_device(0, 1, bins, p), lambda: eng.csm_eig_map_device(p, 1, bins, 0), lambda: eng.csm_eig_map_device(p, 0, bins, p),
                     lambda: eng.csm_eig(Cs, 0, bins), lambda: eng.csm_eig_map(Cs, 0, bins)):
            assert status(call) == B.ERR_INVALID
        c, e = B.csm_of(bins), B.csm_eig_of(EU.MUSIC)
        assert eng._lib.awpu_hip_csm_eig_map(eng._h, B._f32(Cs), 1, C.byref(c), None, B._f32(out), None, None) == B.ERR_INVALID
        assert eng._lib.awpu_hip_csm_eig_map(None, B._f32(Cs), 1, C.byref(c), C.byref(e), B._f32(out), None, None) == B.ERR_INVALID
        # the state refusals of the cross-spectral calls
        eng.set_band(pkg.band_design(1000.0, 4000.0, 31))
        assert [status(call) for call in every(eng)] == [B.ERR_STATE] * 5
        eng.set_band(None)
        eng.process_async(sc.frames[0][:1])
        assert [status(call) for call in every(eng)] == [B.ERR_STATE] * 5
        eng.wait()
        assert status(every(eng)[1]) == B.OK  # (and the handle serves the call once it may)
        out[:] = CANARY
    with pkg.Engine(n_pixels=sc.P, n_streams=64, interp=B.INTERP_FIR8) as eng:
        eng.set_delay_table(sc.off, sc.frac)
        eng.set_active_mics(None)
        assert [status(call) for call in every(eng)] == [B.ERR_STATE] * 5
    with pkg.Engine(n_pixels=sc.P, n_streams=64, grid_columns=16, devices=[0, 0]) as eng:  # a device group
        eng.set_delay_table(sc.off, sc.frac)
        eng.set_active_mics(None)
        assert [status(call) for call in every(eng)] == [B.ERR_STATE] * 5
    # more active mics than the bound
    S = B.CSM_EIG_MAX_MICS + 1
    with pkg.Engine(n_pixels=2, n_streams=S) as eng:
        eng.set_delay_table(np.zeros((2, S), np.int32), np.zeros((2, S), np.float32))
        eng.set_active_mics(None)
        big = np.zeros((1, S, S, 2), np.float32)
        big[0, np.arange(S), np.arange(S), 0] = 1.0
        c, e = B.csm_of(bins), B.csm_eig_of(EU.MUSIC)
        assert eng._lib.awpu_hip_csm_eig(eng._h, B._f32(big), 1, C.byref(c), B._f32(out), B._f32(out), None, None) == B.ERR_RANGE
        assert eng._lib.awpu_hip_csm_eig_map(eng._h, B._f32(big), 1, C.byref(c), C.byref(e), B._f32(out), None, None) == B.ERR_RANGE
        for call in (lambda: eng.csm_eig_device(p, 1, bins, p, p), lambda: eng.csm_eig_weigh_device(p, p, bins, p), lambda: eng.csm_eig_map_device(p, 1, bins, p)):
            assert status(call) == B.ERR_RANGE
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == CANARY).all() and (out == CANARY).all()
