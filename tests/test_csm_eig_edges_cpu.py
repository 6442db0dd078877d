"""Step 8a of include/awpu_hip_csm.h on the host at the sizes and on the kinds of matrix that test_csm_eig_cpu.py leaves out, so
that test_gpu_csm_eig_edges.py compares the device with a host rule that has itself been checked there.  On a box without a GPU.

1. awpu_hip_csm_eig_host against numpy.linalg.eigh (csm_eig_util.against_numpy, the bounds derived there) at the edges of the
   Jacobi kernel's thread tiers, 8, 9 and 32 mics, and from 128 mics to the bound: 128, 129, 255 and 256.  Three bins, one at 255
   and 256 (about 3.5 s a bin there); more blocks than mics and, but for 255, a rank-deficient matrix of U // 4 blocks.
2. The classes of matrix, each at 5, 64 and 65 mics (csm_eig_util states the matrices and what their decomposition must show):
   3 I and a diagonal with repeated values, which rotate nothing -- one sweep, equal values in index order, unit vectors with
   neither a NaN nor a negative zero --; every entry (2, 0), rank one, with exact ties behind rotations, and 2 x 2 blocks
   down the diagonal, whose exact ties come in an order that can be stated without the rule; an indefinite matrix
   with a positive trace, its values descending through zero and its functional weight 0 from zero down; the matrix times 2^100,
   2^-100 and 2^60, through which every operation of the rule scales exactly; a matrix of subnormal entries.
3. An eigenvalue that does not fit a float makes its bin unsolved: every entry (1e38, 0) as one bin of three, and 64 mics of two
   sources scaled to a largest entry of 3e37 (each gave `inf` values with solved 1 before csm_eig_fits); a diagonal of 3e38, the
   largest that fits, is solved.  The maps of such a call hold no NaN.

Not covered, here or on the device: a bin that still rotates in its 32nd sweep.  No natural input is known to reach it, and
AWPU_CSM_EIG_MAX_SWEEPS is a fixed define of the public header."""
import time

import numpy as np
import pytest

import csm_eig_util as EU
import csm_util as CU

BINS = [3, 16, 128]
SIZES = [(U, n) for U in (8, 9, 32, 128, 129, 255, 256) for n in ([2 * U + 3] + ([U // 4] if U != 255 else []))]


def ordinary(U, K=3):
    """Two strong sources in noise, 2 U + 3 blocks, seeded by the size."""
    return EU.random_matrix(np.random.default_rng(4000 + U), K, U, 2 * U + 3), 2 * U + 3


def table(U, pixels=5):
    rng = np.random.default_rng(70 + U)
    return rng.integers(0, 200, (pixels, U)).astype(np.int32), rng.random((pixels, U)).astype(np.float32)


@pytest.mark.parametrize("U,n", SIZES)
def test_eig_host_against_numpy_at_the_tiers_and_the_bound(pkg, U, n):
    bins = BINS if U < 255 else [16]
    Cm = EU.random_matrix(np.random.default_rng(1000 + 7 * U + n), len(bins), U, n)
    t0 = time.perf_counter()
    val, vec, solved, sweeps = pkg.csm_eig_host(Cm, n, bins)
    seconds = time.perf_counter() - t0
    assert solved.tolist() == [1] * len(bins) and (sweeps >= 1).all() and (sweeps <= 16).all()
    worst = EU.against_numpy(Cm, n, val, vec)
    print(U, n, "sweeps", sweeps.tolist(), "fractions of the bounds", worst, f"{seconds:.2f} s")
    assert max(worst.values()) <= 1.0, worst
    assert (val[:, :-1] >= val[:, 1:]).all()


@pytest.mark.parametrize("U", EU.EDGE_MICS)
def test_matrices_that_rotate_nothing(pkg, U):
    Cm, n = EU.identity_times_three(U)
    EU.check_identity(pkg.csm_eig_host(Cm, n, [16]), U)
    Cm, n, _, _ = EU.repeated_diagonal(U)
    EU.check_repeated(pkg.csm_eig_host(Cm, n, [16]), U)


@pytest.mark.parametrize("U", EU.EDGE_MICS)
def test_equal_entries_give_exact_ties(pkg, U):
    Cm, n = EU.equal_entries(U)
    EU.check_equal_entries(pkg.csm_eig_host(Cm, n, [16]), U)
    # (any consistent order of those ties is a decomposition; the paired blocks tie exactly too, in an order that can be stated)
    Cm, n, _ = EU.paired_blocks(U)
    EU.check_paired_blocks(pkg.csm_eig_host(Cm, n, [16]), U)


@pytest.mark.parametrize("U", EU.EDGE_MICS + (33,))
def test_indefinite_matrix_with_a_positive_trace(pkg, U):
    n = 2 * U + 3
    Cm = EU.indefinite_matrix(np.random.default_rng(600 + U), 3, U, n)
    out = pkg.csm_eig_host(Cm, n, BINS)
    val, vec, solved, _ = out
    EU.check_indefinite(Cm, n, out, pkg.csm_eig_weigh_host(val, vec, BINS, EU.FUNCTIONAL, 0, 0))
    off, frac = table(U)
    for kind, n_sources, root in ((EU.MUSIC, 2, 0), (EU.FUNCTIONAL, 0, 0), (EU.FUNCTIONAL, 0, 4)):
        m = pkg.csm_eig_map_host(pkg.csm_eig_weigh_host(val, vec, BINS, kind, n_sources, root), solved, off, frac, BINS, kind, n_sources, root)
        assert np.isfinite(m).all() and (m >= 0).all(), (kind, root)


@pytest.mark.parametrize("U", EU.EDGE_MICS + (33,))
def test_powers_of_two_scale_exactly(pkg, U):
    Cm, n = ordinary(U)
    base = pkg.csm_eig_host(Cm, n, BINS)
    assert base[2].tolist() == [1, 1, 1]
    for power in EU.EDGE_SCALES:
        EU.check_scaled(base, pkg.csm_eig_host(EU.scaled_by_power_of_two(Cm, power), n, BINS), power)


@pytest.mark.parametrize("U", EU.EDGE_MICS)
def test_subnormal_entries(pkg, U):
    """The largest entry 1e-44: every entry a few units of 2^-149.  The doubles are ordinary; the float results are themselves
    subnormal, so no accuracy is asserted: the call must end with finite outputs, the values descending."""
    Cm, n = ordinary(U)
    tiny = EU.scaled_to_largest(Cm, 1e-44)
    assert tiny.any() and np.abs(tiny).max() < 2.0 ** -126
    val, vec, solved, sweeps = pkg.csm_eig_host(tiny, n, BINS)
    print(U, "subnormal: solved", solved.tolist(), "sweeps", sweeps.tolist(), "largest value", val[:, 0].tolist())
    assert np.isfinite(val).all() and np.isfinite(vec).all() and (val[:, :-1] >= val[:, 1:]).all()
    assert solved.tolist() == [1, 1, 1]


@pytest.mark.parametrize("U", EU.EDGE_MICS)
def test_an_eigenvalue_that_fits_no_float_makes_the_bin_unsolved(pkg, U):
    Cm, _ = ordinary(U)
    n = 1  # (the overflowing matrix is one block; the ordinary bins are then 2 U + 3 times larger, no more)
    want = pkg.csm_eig_host(Cm, n, BINS)
    assert want[2].tolist() == [1, 1, 1]
    bad = Cm.copy()
    bad[1] = EU.overflowing(U)[0][0]
    assert np.isfinite(bad).all()
    out = pkg.csm_eig_host(bad, n, BINS)
    val, vec, solved, sweeps = out
    print(U, "overflow: solved", solved.tolist(), "sweeps", sweeps.tolist())
    EU.check_unsolved_bin(out, 1)
    for k in (0, 2):
        assert CU.same_bits(val[k], want[0][k]) and CU.same_bits(vec[k], want[1][k]) and sweeps[k] == want[3][k]
    off, frac = table(U)
    for kind, n_sources, root in ((EU.MUSIC, 2, 0), (EU.FUNCTIONAL, 0, 0), (EU.FUNCTIONAL, 0, 4)):
        H = pkg.csm_eig_weigh_host(val, vec, BINS, kind, n_sources, root)
        assert not np.isnan(H).any() and not H[1].any()
        m = pkg.csm_eig_map_host(H, solved, off, frac, BINS, kind, n_sources, root)
        assert not np.isnan(m).any() and not m[1].any() and not np.signbit(m[1]).any() and (m[[0, 2]] > 0).all()
    # the largest eigenvalue that fits: a diagonal of 3e38 is solved, its values 3e38
    val, vec, solved, sweeps = pkg.csm_eig_host(EU.diagonal_matrix(np.full(U, 3e38)), 1, [16])
    assert solved.tolist() == [1] and sweeps.tolist() == [1]
    assert CU.same_bits(val, np.full((1, U), 3e38, np.float32)) and CU.same_bits(vec, EU.unit_rows(np.arange(U)))


def test_two_sources_scaled_past_the_floats_are_unsolved(pkg):
    """64 mics of two sources in noise, the largest entry 3e37: every entry is an ordinary float and the two largest eigenvalues
    are not.  Before csm_eig_fits the bin came back solved with two infinite values, and its functional weighed matrix held NaN."""
    U, n = 64, 1
    Cm = EU.scaled_to_largest(ordinary(U, 1)[0], 3e37)
    top = np.linalg.eigvalsh(EU.loaded(Cm, n))[0, ::-1]
    assert top[1] > np.finfo(np.float32).max > top[2] > 0
    out = pkg.csm_eig_host(Cm, n, [16])
    EU.check_unsolved_bin(out, 0)
    assert 1 <= out[3][0] <= 16  # (the sweeps ran; the bin fails behind them)
    assert not pkg.csm_eig_weigh_host(out[0], out[1], [16], EU.FUNCTIONAL, 0, 4).any()
