"""Step 8 of include/awpu_hip_csm.h on the device where test_gpu_csm_eig.py does not go: from 128 mics to the bound of
AWPU_CSM_EIG_MAX_MICS = 256, and the kinds of matrix other than two sources in noise.  The device against the host rule bit for
bit, every output between guard floats; the host rule at these sizes and classes is test_csm_eig_edges_cpu.py's question, and
csm_eig_util states the matrices, the bounds and what each class must show, once for both files.

1. The bound: 128 of 128 mics, 129 of 160 (ragged, odd: the dummy sits out in the scratch path), 255 of 256 and 256 of 256 --
   1024 threads, A and V in the scratch (2 x 1 MiB a bin at 256, where the second bin lies kb * U * U entries in), the sort's
   grid of 256 workgroups a bin.  128 and 129: bins [16] and [3, 16, 128] of 2 U + 3 blocks and a rank-deficient matrix of U // 4
   blocks; 255: one bin; 256: two bins.  Values, vectors, solved and sweep words equal csm_eig_host's (computed once per module);
   the synchronous form too; and the device's own output meets numpy.linalg.eigh of the loaded matrix within the derived bounds,
   so that "device = host rule = numpy" does not rest on two files agreeing about sizes.
2. Composition at 9 mics (256 threads), 129 and 256 (the weigh kernel's 16 x 16 tiles, its w[256] filled in exactly one pass; the
   finish behind the map's q of a 256-mic weighed matrix): test_gpu_csm_eig.py's check_composition with MUSIC of 0, 2 and U - 1
   sources and functional beamforming of root 0, 4 and 6, the largest root; 300 pixels leave a tail workgroup in the map (64
   pixels each) and in the finish (256).
3. Matrix classes, each at 5, 64 and 65 mics (64 threads; the LDS-resident path; the scratch path): 3 I and a diagonal with
   repeated values -- bins that rotate nothing, whose sweep flag is never raised and whose rotation words are never written;
   every entry (2, 0), whose eigenvalues tie exactly behind rotations, so that csm_eig_before's index order decides ranks in the
   sort kernel (a wrong tie-break writes one row twice and leaves another its canary), and 2 x 2 blocks down the diagonal, whose
   exact ties have an order that can be stated without the rule; an indefinite matrix with a positive trace; the matrix times 2^100, 2^-100 and 2^60 against the matrix itself; subnormal entries; and an eigenvalue that fits no
   float, which makes its bin unsolved (csm_eig_fits) in the eig and the map forms, beside a diagonal of 3e38 that is solved.

Not covered: a bin that still rotates in its 32nd sweep.  No natural input is known to reach it, and AWPU_CSM_EIG_MAX_SWEEPS is a
fixed define of the public header."""
import time

import numpy as np
import pytest

import csm_eig_util as EU
import csm_util as CU
import test_gpu_csm_eig as E
from test_gpu_csm_eig import CANARY, Rig, check_bits, device_eig, device_eig_map, device_equals, device_weigh, matrix_of

pytestmark = pytest.mark.gpu

BINS_OF = {1: [16], 2: [16, 128], 3: E.THREE}
# U -> the settings (n_bins, n_blocks) of the bit test; the last one is also given to the synchronous form
SETTINGS = {128: [(1, 259), (1, 32), (3, 259)],
            129: [(1, 261), (1, 32), (3, 261)],
            255: [(1, 513)],
            256: [(2, 515)]}
assert all(n in (2 * U + 3, U // 4) for U, settings in SETTINGS.items() for _, n in settings)
REQUESTS = E.REQUESTS + [(EU.FUNCTIONAL, 0, 6)]
assert sorted(r for k, _, r in REQUESTS if k == EU.FUNCTIONAL) == [0, 4, 6] and sorted(s for k, s, _ in REQUESTS if k == EU.MUSIC) == [-1, 0, 2]

_host = {}


def host_of(pkg, U, K, n_blocks):
    """csm_eig_host of matrix_of(U, K, n_blocks), computed once per module (3.4 s a bin at 256 mics) and left unchanged."""
    key = (U, K, n_blocks)
    if key not in _host:
        t0 = time.perf_counter()
        out = pkg.csm_eig_host(matrix_of(*key), n_blocks, BINS_OF[K])
        print(key, f"host rule: {time.perf_counter() - t0:.2f} s")
        for a in out:
            a.setflags(write=False)
        _host[key] = out
    return _host[key]


# ------------------------------------------------------------------------------------------------ 1. the bound

@pytest.mark.parametrize("U", sorted(SETTINGS))
def test_device_eig_up_to_the_bound(pkg, U):
    assert U in E.BOUND_MICS and pkg.binding.CSM_EIG_MAX_MICS == 256 == max(SETTINGS)
    with Rig(pkg, U).engine() as eng:
        for K, n in SETTINGS[U]:
            Cm, bins, want = matrix_of(U, K, n), BINS_OF[K], host_of(pkg, U, K, n)
            assert want[2].tolist() == [1] * K
            t0 = time.perf_counter()
            got = device_equals(eng, Cm, n, bins, want)
            worst = EU.against_numpy(Cm, n, got[0], got[1])  # the device's own words
            print(U, K, n, "fractions of the bounds on the device", worst, f"device and checks: {time.perf_counter() - t0:.2f} s")
            assert max(worst.values()) <= 1.0, worst
        assert E.same(eng.csm_eig(Cm, n, bins), want)  # the synchronous form


# ------------------------------------------------------------------------------------------------ 2. composition

@pytest.mark.parametrize("U", [9, 129, 256])
def test_composition_at_a_tier_edge_and_the_bound(pkg, U):
    K = 2 if U == 256 else 3
    n = 2 * U + 3
    rig = Rig(pkg, U)
    assert E.PIXELS % 64 and E.PIXELS % 256 and E.PIXELS > 256  # a tail workgroup in the map's q and in the finish
    with rig.engine() as eng:
        E.check_composition(pkg, rig, eng, matrix_of(U, K, n), n, BINS_OF[K], 1, REQUESTS, host_of(pkg, U, K, n)[:3])


# ------------------------------------------------------------------------------------------------ 3. matrix classes

def no_canary(got):
    assert not (got[0] == CANARY).any() and not (got[1] == CANARY).any()  # every word of values and vectors was written


@pytest.mark.parametrize("U", EU.EDGE_MICS)
def test_bins_that_rotate_nothing(pkg, U):
    with Rig(pkg, U).engine() as eng:
        Cm, n = EU.identity_times_three(U)
        EU.check_identity(device_equals(eng, Cm, n, [16], pkg.csm_eig_host(Cm, n, [16])), U)
        Cm, n, _, _ = EU.repeated_diagonal(U)
        EU.check_repeated(device_equals(eng, Cm, n, [16], pkg.csm_eig_host(Cm, n, [16])), U)
        # ... and as one bin among bins that rotate: each workgroup's flags are its own
        mixed = np.array(matrix_of(U, 3, 2 * U + 3))
        mixed[1] = Cm[0]
        want = check_bits(pkg, eng, mixed, 2, E.THREE)
        assert want[3][1] == 1 and want[3][0] > 1 and want[3][2] > 1


@pytest.mark.parametrize("U", EU.EDGE_MICS)
def test_exact_ties_behind_rotations(pkg, U):
    with Rig(pkg, U).engine() as eng:
        Cm, n = EU.equal_entries(U)
        got = device_equals(eng, Cm, n, [16], pkg.csm_eig_host(Cm, n, [16]))
        no_canary(got)
        EU.check_equal_entries(got, U)
        # (any consistent order of those ties is a decomposition; the paired blocks tie exactly too, in an order that can be stated)
        Cm, n, _ = EU.paired_blocks(U)
        got = device_equals(eng, Cm, n, [16], pkg.csm_eig_host(Cm, n, [16]))
        no_canary(got)
        EU.check_paired_blocks(got, U)


@pytest.mark.parametrize("U", EU.EDGE_MICS)
def test_indefinite_matrix_with_a_positive_trace(pkg, U):
    n = 2 * U + 3
    Cm = EU.indefinite_matrix(np.random.default_rng(600 + U), 3, U, n)
    rig = Rig(pkg, U)
    with rig.engine() as eng:
        want = check_bits(pkg, eng, Cm, n, E.THREE)
        got, (d_val, d_vec) = device_eig(eng, Cm, n, E.THREE)
        F0, _ = device_weigh(eng, d_val, d_vec, 3, U, E.THREE, EU.FUNCTIONAL, 0, 0)
        assert CU.same_bits(F0, pkg.csm_eig_weigh_host(want[0], want[1], E.THREE, EU.FUNCTIONAL, 0, 0))
        EU.check_indefinite(Cm, n, got, F0)
        for kind, n_sources, root in ((EU.MUSIC, 2, 0), (EU.FUNCTIONAL, 0, 4)):
            Hw = pkg.csm_eig_weigh_host(want[0], want[1], E.THREE, kind, n_sources, root)
            m, v, s = device_eig_map(eng, Cm, n, E.THREE, kind, n_sources, root, 1)
            assert CU.same_bits(m, pkg.csm_eig_map_host(Hw, want[2], rig.off, rig.frac, E.THREE, kind, n_sources, root, 1, index=rig.index))
            assert np.isfinite(m).all() and (m >= 0).all() and CU.same_bits(v, want[0]) and s.tolist() == [1, 1, 1]


@pytest.mark.parametrize("U", EU.EDGE_MICS)
def test_powers_of_two_scale_exactly(pkg, U):
    n = 2 * U + 3
    Cm = matrix_of(U, 3, n)
    with Rig(pkg, U).engine() as eng:
        base = device_equals(eng, Cm, n, E.THREE, pkg.csm_eig_host(Cm, n, E.THREE))
        assert base[2].tolist() == [1, 1, 1]
        for power in EU.EDGE_SCALES:
            scaled = EU.scaled_by_power_of_two(Cm, power)
            got = device_equals(eng, scaled, n, E.THREE, pkg.csm_eig_host(scaled, n, E.THREE))
            EU.check_scaled(base, got, power)  # between two device results


@pytest.mark.parametrize("U", EU.EDGE_MICS)
def test_subnormal_entries(pkg, U):
    """The largest entry 1e-44.  No accuracy bound: the float result is itself subnormal."""
    n = 2 * U + 3
    tiny = EU.scaled_to_largest(matrix_of(U, 3, n), 1e-44)
    assert tiny.any() and np.abs(tiny).max() < 2.0 ** -126
    rig = Rig(pkg, U)
    with rig.engine() as eng:
        want = pkg.csm_eig_host(tiny, n, E.THREE)
        got = device_equals(eng, tiny, n, E.THREE, want)
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
        for kind, n_sources, root in ((EU.MUSIC, 2, 0), (EU.FUNCTIONAL, 0, 4)):
            Hw = pkg.csm_eig_weigh_host(want[0], want[1], E.THREE, kind, n_sources, root)
            m, _, _ = device_eig_map(eng, tiny, n, E.THREE, kind, n_sources, root, 0)
            assert CU.same_bits(m, pkg.csm_eig_map_host(Hw, want[2], rig.off, rig.frac, E.THREE, kind, n_sources, root, 0, index=rig.index))
            assert np.isfinite(m).all()


@pytest.mark.parametrize("U", EU.EDGE_MICS)
def test_an_eigenvalue_that_fits_no_float_makes_the_bin_unsolved(pkg, U):
    """Every entry (1e38, 0), one block, as bin 1 of three: finite entries and a finite double eigenvalue U * 1e38.  That bin is
    +0 with solved 0 in the eig and the map forms, its plane +0 in both maps, no NaN anywhere; the other bins keep the rule's bits."""
    n = 1
    Cm = np.array(matrix_of(U, 3, 2 * U + 3))
    ordinary = pkg.csm_eig_host(Cm, n, E.THREE)
    Cm[1] = EU.overflowing(U)[0][0]
    rig = Rig(pkg, U)
    with rig.engine() as eng:
        val, vec, solved, _ = want = pkg.csm_eig_host(Cm, n, E.THREE)
        got = device_equals(eng, Cm, n, E.THREE, want)
        EU.check_unsolved_bin(got, 1)
        assert got[3][1] >= 1  # (the sweeps ran: the bin fails behind them)
        for k in (0, 2):
            assert CU.same_bits(got[0][k], ordinary[0][k]) and CU.same_bits(got[1][k], ordinary[1][k]) and got[3][k] == ordinary[3][k]
        assert E.same(eng.csm_eig(Cm, n, E.THREE), want)
        for kind, n_sources, root in ((EU.MUSIC, 2, 0), (EU.FUNCTIONAL, 0, 0), (EU.FUNCTIONAL, 0, 4)):
            Hw = pkg.csm_eig_weigh_host(val, vec, E.THREE, kind, n_sources, root)
            assert not np.isnan(Hw).any()
            plane = pkg.csm_eig_map_host(Hw, solved, rig.off, rig.frac, E.THREE, kind, n_sources, root, 0, index=rig.index)
            m, v, s = device_eig_map(eng, Cm, n, E.THREE, kind, n_sources, root, 0)
            assert s.tolist() == [1, 0, 1] and CU.same_bits(m, plane) and CU.same_bits(v, val)
            assert not m[1].any() and not np.signbit(m[1]).any() and not np.isnan(m).any() and (m[[0, 2]] > 0).all()
            out = eng.csm_eig_map(Cm, n, E.THREE, kind, n_sources, root, 0, want=("map", "values", "solved"))
            assert CU.same_bits(out["map"], plane) and CU.same_bits(out["values"], val) and out["solved"].tolist() == [1, 0, 1]
        # the largest eigenvalue that fits: a diagonal of 3e38 is solved with values 3e38 (against the host's bits only)
        big = EU.diagonal_matrix(np.full(U, 3e38))
        got = device_equals(eng, big, 1, [16], pkg.csm_eig_host(big, 1, [16]))
        assert got[2].tolist() == [1] and CU.same_bits(got[0], np.full((1, U), 3e38, np.float32))
