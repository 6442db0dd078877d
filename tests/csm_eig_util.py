"""What the tests of step 8 of include/awpu_hip_csm.h share (test_csm_eig_cpu.py, test_csm_eig_edges_cpu.py, test_gpu_csm_eig.py,
test_gpu_csm_eig_edges.py): seeded matrices, the matrix A the rule loads in complex128, the bounds against numpy.linalg.eigh and
the comparison itself, the matrix classes both sides run (identity, repeated diagonal, equal entries, indefinite, scaled,
subnormal, overflowing), step 8c's finish restated in numpy float32, and a one-source variant of csm_util's scene.  A plain
helper, not a conftest."""
from __future__ import annotations

import numpy as np

import csm_util as CU

F32 = np.float32
MUSIC, FUNCTIONAL = 0, 1
# Eigenvalues agree within 2^-22 of the bin's largest: Jacobi in double is exact to about 1e-14 of it and is then rounded to float
# once (2^-24 relative); numpy's are exact to about 1e-15.  The factor 2 on one rounding of the largest value (2^-23, as
# test_csm_invert_cpu.py argues for G) is slack.
VALUE_BOUND = 2.0 ** -22


def vector_bound(U):
    """|A v - lambda v| over lambda_max, and |V^H V - I|: v's U entries and lambda are each rounded to float once (2^-24 of
    at most 1, and of lambda_max), so a row of A v - lambda v is off by at most (|A| 1 + lambda_max) 2^-24 <= (sqrt(U) + 1) 2^-24
    lambda_max and an entry of V^H V by 2 U 2^-24 / 2 in the worst case; (U + 2) 2^-23 covers both."""
    return (U + 2) * 2.0 ** -23


def vectors_of(vec):
    """vectors [K, U, U, 2] -> V [K, U, U] complex128 with the eigenvectors as COLUMNS."""
    return np.swapaxes(CU.as_complex(vec), 1, 2)


def against_numpy(Cm, n, val, vec):
    """A decomposition (float values [K, U] and vectors [K, U, U, 2]) against numpy.linalg.eigvalsh of the loaded matrix in
    complex128 -> the worst fraction reached of each bound: |lambda - ref| / max|ref| over VALUE_BOUND, the residual
    |A v - lambda v| / max|ref| and the Gram error |V^H V - I| over vector_bound(U).  At most 1 where the bounds hold."""
    U = Cm.shape[1]
    A = loaded(Cm, n)
    ref = np.linalg.eigvalsh(A)[:, ::-1]
    top = np.abs(ref).max(axis=1)
    V = vectors_of(vec)
    lam = np.asarray(val, np.float64)
    return {"values": float((np.abs(lam - ref).max(axis=1) / top).max() / VALUE_BOUND),
            "residual": float((np.abs(A @ V - V * lam[:, None, :]).max(axis=(1, 2)) / top).max() / vector_bound(U)),
            "gram": float(np.abs(np.conj(np.swapaxes(V, 1, 2)) @ V - np.eye(U)).max() / vector_bound(U))}


def random_matrix(rng, K, U, n_blocks, sources=2):
    """C = sum over blocks of X X^H, as step 2 lays it out, of `sources` strong sources in noise: [K, U, U, 2] float32, Hermitian,
    with an exactly real diagonal.  Fewer blocks than mics make it rank-deficient."""
    X = rng.standard_normal((K, U, n_blocks)) + 1j * rng.standard_normal((K, U, n_blocks))
    for s in range(min(sources, U)):
        steer = np.exp(2j * np.pi * rng.random((K, U, 1)))
        X = X + (8.0 - 3.0 * s) * steer * (rng.standard_normal((K, 1, n_blocks)) + 1j * rng.standard_normal((K, 1, n_blocks)))
    Cc = X @ np.conj(np.swapaxes(X, 1, 2))
    out = np.stack([Cc.real, Cc.imag], axis=-1).astype(F32)
    out[:, np.arange(U), np.arange(U), 1] = 0.0
    return out


def loaded(Cm, n):
    """A of step 8a, in complex128, from the entries the rule reads (the lower triangle and the diagonal's real parts)."""
    U = Cm.shape[1]
    low = np.tril(CU.as_complex(Cm), -1)
    d = np.diagonal(Cm[..., 0], axis1=1, axis2=2).astype(np.float64) / n
    return (low + np.conj(np.swapaxes(low, 1, 2))) / n + d[:, :, None] * np.eye(U)


# ---- the matrix classes of test_csm_eig_edges_cpu.py and test_gpu_csm_eig_edges.py: each -> (matrix [K, U, U, 2], block count)

REPEATED = [4.0, 8.0, 4.0, 2.0, 8.0, 4.0]  # the pattern test_csm_eig_cpu.py's diagonal case has at six mics
EDGE_MICS = (5, 64, 65)  # 64 threads; the last size whose A and V live in LDS; the first that lives in the scratch
EDGE_SCALES = (100, -100, 60)  # powers of two the rule must carry through exactly


def diagonal_matrix(d):
    """One bin with the diagonal d and nothing else: no pair rotates."""
    d = np.asarray(d, F32)
    U = len(d)
    Cm = np.zeros((1, U, U, 2), F32)
    Cm[0, np.arange(U), np.arange(U), 0] = d
    return Cm


def identity_times_three(U):
    """3 I of two blocks: every eigenvalue 1.5."""
    return diagonal_matrix(np.full(U, 3.0)), 2


def repeated_diagonal(U):
    """REPEATED tiled to U mics, two blocks -> (matrix, block count, expected values, expected order): the values descend and
    equal ones keep index order, so row r of `vectors` is the unit vector of index order[r]."""
    d = np.resize(np.asarray(REPEATED), U)
    order = np.argsort(-d, kind="stable")
    return diagonal_matrix(d), 2, (d[order] / 2.0).astype(F32), order


def equal_entries(U, value=2.0):
    """Every entry (value, 0), one block: rank one, so all eigenvalues but one are zero -- in the rule's arithmetic many of them
    exactly, which makes the sort's tie-break run on a matrix that was rotated."""
    Cm = np.zeros((1, U, U, 2), F32)
    Cm[..., 0] = value
    return Cm, 1


def paired_blocks(U, a=3.0, b=1.0):
    """2 x 2 blocks ((a, b), (b, a)) down the diagonal -- a alone at the last index of an odd U --, one block -> (matrix, block
    count, the eigenvalues by index as the rotations leave them).  Only the pairs (2k, 2k + 1) rotate, each once, with
    theta = 0: the pair's closed form leaves a - b at 2k and a + b at 2k + 1, exactly and the same in every block.  So the ties
    are exact, they come out of rotations, and which block a row of `vectors` lives in says which index its value had."""
    Cm = diagonal_matrix(np.full(U, a))
    even = np.arange(0, U - 1, 2)
    Cm[0, even + 1, even, 0] = Cm[0, even, even + 1, 0] = b
    lam = np.full(U, a)
    lam[even], lam[even + 1] = a - b, a + b
    return Cm, 1, lam


def indefinite_matrix(rng, K, U, n_blocks):
    """random_matrix with its diagonal multiplied by 0.05: Hermitian, the trace still positive, eigenvalues of both signs."""
    Cm = random_matrix(rng, K, U, n_blocks)
    Cm[:, np.arange(U), np.arange(U), 0] *= F32(0.05)
    return Cm


def scaled_by_power_of_two(Cm, power):
    """Cm * 2^power in float32, checked to be exact (no entry overflows or loses bits to a subnormal)."""
    out = np.ldexp(np.asarray(Cm, F32), power).astype(F32)
    assert np.isfinite(out).all() and np.array_equal(np.ldexp(out.astype(np.float64), -power), np.asarray(Cm, np.float64))
    return out


def scaled_to_largest(Cm, largest):
    """Cm scaled so that its largest |entry| is `largest`, rounded to float32 (1e-44: a matrix of subnormals, a few units of
    2^-149 each; 3e37: eigenvalues past FLT_MAX from finite entries)."""
    Cd = np.asarray(Cm, np.float64)
    out = (Cd * (largest / np.abs(Cd).max())).astype(F32)
    assert np.isfinite(out).all()
    return out


def overflowing(U):
    """Every entry (1e38, 0), one block: finite entries, a finite double eigenvalue U * 1e38 that no float holds from 4 mics on."""
    return equal_entries(U, 1e38)


# ---- what a decomposition out = (values, vectors, solved, sweeps) of each class must show, whoever computed it

def unit_rows(order):
    """vectors [1, U, U, 2] whose row r is the unit vector of index order[r]: +1 there, +0 elsewhere, both parts."""
    U = len(order)
    vec = np.zeros((1, U, U, 2), F32)
    vec[0, np.arange(U), np.asarray(order), 0] = 1.0
    return vec


def check_identity(out, U):
    """3 I of two blocks rotates nothing: one sweep, every value 1.5, the unit vectors in index order -- to the bit, so no NaN
    and no negative zero."""
    val, vec, solved, sweeps = out
    assert solved.tolist() == [1] and sweeps.tolist() == [1]
    assert CU.same_bits(val, np.full((1, U), 1.5, F32)) and CU.same_bits(vec, unit_rows(np.arange(U)))


def check_repeated(out, U):
    """The repeated diagonal rotates nothing either; equal values keep index order."""
    val, vec, solved, sweeps = out
    _, _, values, order = repeated_diagonal(U)
    assert solved.tolist() == [1] and sweeps.tolist() == [1]
    assert CU.same_bits(val[0], values) and CU.same_bits(vec, unit_rows(order)), (val[0], np.argmax(vec[0, :, :, 0], axis=1))


def check_equal_entries(out, U, value=2.0):
    """Rank one: at least two values exactly equal (the ties the sort must break), values descending, the decomposition within
    the bounds against numpy -> how many values repeat another."""
    val, vec, solved, sweeps = out
    Cm, n = equal_entries(U, value)
    assert solved.tolist() == [1] and (val[0, :-1] >= val[0, 1:]).all()
    ties = U - len(np.unique(val[0]))
    assert ties >= 1, val[0]
    worst = against_numpy(Cm, n, val, vec)
    print(U, "equal entries: sweeps", sweeps.tolist(), "repeated values", ties, "zeros", int((val[0] == 0).sum()), worst)
    assert max(worst.values()) <= 1.0, worst
    return ties


def check_paired_blocks(out, U):
    """Exact ties behind rotations, with an order that can be stated without the rule: the values descend, equal ones in index
    order (numpy's stable sort of the eigenvalues by index), and row r of `vectors` is supported on the block of index order[r]."""
    val, vec, solved, sweeps = out
    _, _, lam = paired_blocks(U)
    order = np.argsort(-lam, kind="stable")
    assert solved.tolist() == [1] and sweeps.tolist() == [2] and CU.same_bits(val[0], lam[order].astype(F32))
    support = np.abs(vec[0]).sum(axis=2) > 0  # [row, mic]
    for r, j in enumerate(order):
        block = [j] if j == U - 1 and U % 2 else [j - j % 2, j - j % 2 + 1]
        assert np.flatnonzero(support[r]).tolist() == block, (r, int(j), np.flatnonzero(support[r]).tolist())
    assert max(against_numpy(paired_blocks(U)[0], 1, val, vec).values()) <= 1.0


def check_indefinite(Cm, n, out, F0):
    """Eigenvalues of both signs: solved, descending through zero, within the bounds against numpy (taken against the largest
    |lambda|); F0, the functional weighed matrix of root 0, is V max(L, 0) V^H of numpy within 2 vector_bound(U) max|lambda|
    (test_weighed_matrix's bound for root 0): the weight of an eigenvalue <= 0 is 0."""
    val, vec, solved, sweeps = out
    U = Cm.shape[1]
    assert solved.all() and (val[:, :-1] >= val[:, 1:]).all() and (val[:, 0] > 0).all() and (val[:, -1] < 0).all()
    worst = against_numpy(Cm, n, val, vec)
    lam, Q = np.linalg.eigh(loaded(Cm, n))
    positive = (Q * np.maximum(lam, 0.0)[:, None, :]) @ np.conj(np.swapaxes(Q, 1, 2))
    worst["root 0"] = float((np.abs(CU.as_complex(F0) - positive).max(axis=(1, 2)) / np.abs(lam).max(axis=1)).max() / (2 * vector_bound(U)))
    print(U, "indefinite: sweeps", sweeps.tolist(), "values", val[:, 0].tolist(), "down to", val[:, -1].tolist(), worst)
    assert max(worst.values()) <= 1.0, worst


def check_scaled(base, out, power):
    """The decomposition of a matrix times 2^power: the base's values times 2^power to the bit, its vectors and words as they are."""
    want = np.ldexp(base[0], power).astype(F32)
    assert np.isfinite(want).all() and (want != 0).sum() == (base[0] != 0).sum()
    assert CU.same_bits(out[0], want) and CU.same_bits(out[1], base[1]), power
    assert out[2].tolist() == base[2].tolist() and out[3].tolist() == base[3].tolist(), power


def check_unsolved_bin(out, k):
    """Bin k is unsolved: +0 values and vectors, solved 0; nothing anywhere is a NaN or infinite."""
    val, vec, solved, _ = out
    assert solved[k] == 0 and all(s == 1 for i, s in enumerate(solved.tolist()) if i != k)
    for a in (val[k], vec[k]):
        assert not a.any() and not np.signbit(a).any()
    assert np.isfinite(val).all() and np.isfinite(vec).all()


def finish(q, solved, bins, window, usable, kind, root):
    """Step 8c's finish as written, one float32 rounding an operation: q [n_bins, n_pixels] -> map."""
    q = np.asarray(q, F32)
    uf = F32(usable)
    with np.errstate(**CU.quiet):
        if kind == MUSIC:
            floor = uf * F32(2.0 ** -24)
            out = (uf / np.where(q > floor, q, floor)).astype(F32)
        else:
            ck = np.where((np.asarray(bins) == 0) | (np.asarray(bins) == 128), F32(1.0), F32(2.0)).astype(F32)[:, None]
            wss = F32(96.0) if window == 1 else F32(256.0)
            y = (np.where(q > 0, q, F32(0.0)).astype(F32) / uf).astype(F32)
            for _ in range(root):
                y = (y * y).astype(F32)
            out = ((ck * y).astype(F32) / ((wss * F32(256.0)) * uf)).astype(F32)
    out[np.asarray(solved) == 0] = F32(0.0)
    assert out.dtype == F32
    return out


def one_source_samples(pkg, spec, xyz, seed=77, n_blocks=64):
    """csm_util's scene with its first source alone: band-limited noise of rms 1 around bin 16 from the pixel (16, 12), and the
    mics' unequal self-noise -> samples [n_mics, 256 * n_blocks] float32."""
    S = pkg.synthetic
    n = 256 * n_blocks
    rng = np.random.default_rng(seed)
    f = np.fft.rfftfreq(n, 1.0 / S.SAMPLE_RATE)
    band = np.abs(f - CU.SCENE_BIN * S.SAMPLE_RATE / 256.0) <= CU.SCENE_BAND_HZ
    theta, phi = CU.scene_directions(spec)[0]
    tau = pkg.binding.steering_delays(xyz, theta, phi).astype(np.float64)
    spectrum = np.where(band, rng.standard_normal(len(f)) + 1j * rng.standard_normal(len(f)), 0.0)
    waves = np.fft.irfft(spectrum[None, :] * np.exp(2j * np.pi * f[None, :] * tau[:, None] / S.SAMPLE_RATE), n, axis=1)
    x = waves / waves.std()
    levels = np.exp(rng.uniform(np.log(CU.SCENE_NOISE[0]), np.log(CU.SCENE_NOISE[1]), xyz.shape[1]))
    return (x + levels[:, None] * rng.standard_normal(x.shape)).astype(F32)
