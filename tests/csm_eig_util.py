"""What the tests of step 8 of include/awpu_hip_csm.h share (test_csm_eig_cpu.py, test_gpu_csm_eig.py): seeded matrices, the matrix
A the rule loads in complex128, step 8c's finish restated in numpy float32, and a one-source variant of csm_util's scene.  A plain
helper, not a conftest."""
from __future__ import annotations

import numpy as np

import csm_util as CU

F32 = np.float32
MUSIC, FUNCTIONAL = 0, 1


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
