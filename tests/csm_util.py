"""The rule of include/awpu_hip_csm.h restated in numpy, for the cross-spectral tests (test_csm_cpu.py, test_gpu_csm.py): every
operation one float32 rounding, every fmaf through cohere_util.fmaf (exact: the product of two float32 is exact in float64 and
the sum is rounded to odd there), in the rule's order; the two tables are read from the library.  And the scene the feature was
argued with: two independent band-limited noise sources closer than a beam width, and self-noise of a different level on every mic.
A plain helper, not a conftest."""
from __future__ import annotations

import numpy as np

from cohere_util import F32, bits, fmaf, median_over_max_db, same_bits  # noqa: F401

CONVENTIONAL, DIAGONAL_REMOVED, CAPON = 0, 1, 2
ANGLE = F32(0.024543693)  # (float) (2 pi / 256)
quiet = dict(over="ignore", invalid="ignore", under="ignore", divide="ignore")


def twiddle(tw, j):
    """t_j for j in [0, 255] from the library's 128-entry table: (re, im)."""
    j = np.asarray(j)
    sign = np.where(j & 128, F32(-1.0), F32(1.0)).astype(F32)
    return tw[j & 127, 0] * sign, tw[j & 127, 1] * sign


def spectra(pkg, samples, bins, window=0, index=None, gain=None, n_blocks=None):
    """Step 1: [n_blocks, n_bins, usable, 2]."""
    samples = np.asarray(samples, F32)
    index = np.arange(samples.shape[0]) if index is None else np.asarray(index)
    n_blocks = samples.shape[1] // 256 if n_blocks is None else n_blocks
    w, tw = pkg.tones_window(window), pkg.tones_twiddles()
    with np.errstate(**quiet):
        x = samples[index][:, :256 * n_blocks].reshape(len(index), n_blocks, 256)
        if gain is not None:
            x = x * np.asarray(gain, F32)[:, None, None]
        v = (x * w[None, None, :]).astype(F32)  # [U, B, 256]
        k = np.asarray(bins)
        re = np.zeros((n_blocks, len(k), len(index)), F32)
        im = np.zeros_like(re)
        for i in range(256):
            tr, ti = twiddle(tw, (k * i) & 255)
            vi = v[:, :, i].T[:, None, :]  # [B, 1, U]
            re = fmaf(vi, tr[None, :, None], re)
            im = fmaf(vi, ti[None, :, None], im)
    return np.stack([re, im], axis=-1)


def accumulate(X, matrix=None):
    """Step 2: the blocks of X [n_blocks, n_bins, usable, 2] into matrix [n_bins, usable, usable, 2] (default zeros) -> a new matrix."""
    n_blocks, K, U, _ = X.shape
    C = np.zeros((K, U, U, 2), F32) if matrix is None else np.array(matrix, F32)
    lower = np.tril(np.ones((U, U), bool), -1)
    re, im = C[..., 0].copy(), C[..., 1].copy()  # (every pair is computed; the entries b < a are kept)
    diag = C[:, np.arange(U), np.arange(U), 0].copy()
    with np.errstate(**quiet):
        for b in range(n_blocks):
            ar, ai = X[b, :, :, None, 0], X[b, :, :, None, 1]  # Xa: rows
            br, bi = X[b, :, None, :, 0], X[b, :, None, :, 1]  # Xb: columns
            re = fmaf(ar, br, re)
            re = fmaf(ai, bi, re)
            im = fmaf(ai, br, im)
            im = fmaf(-ar, bi, im)
            diag = fmaf(X[b, :, :, 0], X[b, :, :, 0], diag)
            diag = fmaf(X[b, :, :, 1], X[b, :, :, 1], diag)
    upper = lower.T
    eye = np.eye(U, dtype=bool)
    re_t, im_t = np.swapaxes(re, 1, 2), np.swapaxes(im, 1, 2)
    out = np.zeros((K, U, U, 2), F32)
    out[..., 0] = np.where(lower, re, np.where(upper, re_t, np.where(eye, diag[:, :, None], F32(0))))
    out[..., 1] = np.where(lower, im, np.where(upper, -im_t, F32(0)))
    return out


def steer(pkg, off, frac, bins, index=None):
    """Step 3: [n_pixels, n_bins, usable, 2]."""
    off, frac = np.asarray(off, np.int64), np.asarray(frac, F32)
    index = np.arange(off.shape[1]) if index is None else np.asarray(index)
    tw = pkg.tones_twiddles()
    k = np.asarray(bins, np.int64)[None, :, None]
    n = (256 - off[:, index])[:, None, :]
    f = frac[:, index][:, None, :]
    with np.errstate(**quiet):
        g = (k.astype(F32) * f).astype(F32)
        gi = g.astype(np.int64)
        gf = (g - gi.astype(F32)).astype(F32)
        tr, ti = twiddle(tw, (k * n + gi) & 255)
        th = (gf * ANGLE).astype(F32)
        t2 = (th * th).astype(F32)
        cr = fmaf(t2, F32(1.0) / F32(24.0), F32(-0.5))
        cr = fmaf(cr, t2, F32(1.0))
        sn = fmaf(t2, F32(1.0) / F32(120.0), F32(-1.0) / F32(6.0))
        sn = fmaf(sn, t2, F32(1.0))
        sn = (sn * th).astype(F32)
        re = (tr * cr).astype(F32) + (ti * sn).astype(F32)
        im = (ti * cr).astype(F32) - (tr * sn).astype(F32)
    assert re.dtype == F32 and im.dtype == F32
    return np.stack([re, im], axis=-1)


def quadratic(H, s, kind):
    """Step 4: H [n_bins, usable, usable, 2], s [n_pixels, n_bins, usable, 2] -> q [n_bins, n_pixels]."""
    K, U = H.shape[0], H.shape[1]
    P = s.shape[0]
    sr, si = np.moveaxis(s[..., 0], 0, 1), np.moveaxis(s[..., 1], 0, 1)  # [K, P, U]
    yr, yi = np.zeros((K, P, U), F32), np.zeros((K, P, U), F32)
    with np.errstate(**quiet):
        for b in range(U - 1):
            rows = slice(b + 1, U)
            hr, hi = H[:, None, rows, b, 0], H[:, None, rows, b, 1]  # [K, 1, rows]
            sbr, sbi = sr[:, :, b, None], si[:, :, b, None]
            yr[:, :, rows] = fmaf(hr, sbr, yr[:, :, rows])
            yr[:, :, rows] = fmaf(hi, sbi, yr[:, :, rows])
            yi[:, :, rows] = fmaf(hi, sbr, yi[:, :, rows])
            yi[:, :, rows] = fmaf(-hr, sbi, yi[:, :, rows])
        d = np.zeros(K, F32)
        x = np.zeros((K, P), F32)
        for a in range(U):
            d = d + H[:, a, a, 0]
            x = fmaf(sr[:, :, a], yr[:, :, a], x)
            x = fmaf(-si[:, :, a], yi[:, :, a], x)
        twice = x + x
        q = twice if kind == DIAGONAL_REMOVED else d[:, None] + twice
    assert q.dtype == F32
    return q


def maps(q, bins, window, kind, usable, block_count):
    """Step 5: [n_bins, n_pixels]."""
    ck = np.where((np.asarray(bins) == 0) | (np.asarray(bins) == 128), F32(1.0), F32(2.0)).astype(F32)[:, None]
    wss = F32(96.0) if window == 1 else F32(256.0)
    with np.errstate(**quiet):
        if kind == CAPON:
            scale = wss * F32(256.0)
            return np.where(q > 0, ck / (scale * q), F32(0.0)).astype(F32)
        pairs = usable * (usable - 1) if kind == DIAGONAL_REMOVED else usable * usable
        scale = (wss * F32(256.0)) * (F32(pairs) * F32(block_count))
        v = ((ck * q) / scale).astype(F32)
        return np.where(v < 0, F32(0.0), v).astype(F32) if kind == DIAGONAL_REMOVED else v


def rule_map(pkg, matrix, block_count, off, frac, bins, window=0, kind=CONVENTIONAL, index=None):
    """{"map", "q"} by the rule as written."""
    usable = off.shape[1] if index is None else len(index)
    q = quadratic(np.asarray(matrix, F32), steer(pkg, off, frac, bins, index), kind)
    return dict(q=q, map=maps(q, bins, window, kind, usable, block_count))


def as_complex(a):
    a = np.asarray(a, np.float64)
    return a[..., 0] + 1j * a[..., 1]


# ---- the scene: the c1 array, two independent noise sources band-limited around bin 16 (3.05 kHz) SCENE_COLS apart on one grid
# row, 256 blocks, white self-noise of a different level on every mic.  Picked so that, for the host rule alone, find_peaks sees
# one source in the conventional plane and both, at their pixels, in the Capon plane (tests/test_csm_cpu.py).

SCENE_BIN = 16
SCENE_BLOCKS = 256
SCENE_ROW = 16
SCENE_COLS = (12, 19)     # the sources' pixels on the 32 x 32 grid: 7 pixels = 0.44 in sine space; the beam is about 0.8 wide
SCENE_AMP = (1.0, 0.8)    # rms of each source at a mic
SCENE_BAND_HZ = 100.0     # half width of the sources' band around the bin's centre
SCENE_NOISE = (0.5, 2.0)  # rms of the mics' self-noise: log-uniform in this range, a level of its own for every mic
SCENE_LOADING = 1e-2
SCENE_FIND = dict(radius=2, max_sources=4, min_ratio=0.25)


def scene_directions(spec):
    """(theta, phi) of the two sources: the centres of their pixels on the sine-space grid of `spec`."""
    sep = np.sin(np.deg2rad(spec.fov) / 2.0) / (spec.res / 2.0)
    out = []
    for col in SCENE_COLS:
        x, y = (col - spec.res / 2.0 + 0.5) * sep, (SCENE_ROW - spec.res / 2.0 + 0.5) * sep
        out.append((float(np.arcsin(np.hypot(x, y))), float(np.arctan2(y, x))))
    return out


def scene_samples(pkg, spec, xyz, seed=2024, n_blocks=SCENE_BLOCKS):
    """samples [n_mics, 256 * n_blocks] float32 of the scene, and the mics' noise levels."""
    S = pkg.synthetic
    n = 256 * n_blocks
    rng = np.random.default_rng(seed)
    f = np.fft.rfftfreq(n, 1.0 / S.SAMPLE_RATE)
    centre = SCENE_BIN * S.SAMPLE_RATE / 256.0
    band = np.abs(f - centre) <= SCENE_BAND_HZ
    x = np.zeros((xyz.shape[1], n))
    for (theta, phi), amp in zip(scene_directions(spec), SCENE_AMP):
        tau = pkg.binding.steering_delays(xyz, theta, phi).astype(np.float64)
        spectrum = np.where(band, rng.standard_normal(len(f)) + 1j * rng.standard_normal(len(f)), 0.0)
        # mic m hears the wave advanced by tau_m samples (synthetic.make_frames' convention)
        waves = np.fft.irfft(spectrum[None, :] * np.exp(2j * np.pi * f[None, :] * tau[:, None] / S.SAMPLE_RATE), n, axis=1)
        x += amp * waves / waves.std()
    levels = np.exp(rng.uniform(np.log(SCENE_NOISE[0]), np.log(SCENE_NOISE[1]), xyz.shape[1]))
    x += levels[:, None] * rng.standard_normal(x.shape)
    return x.astype(F32), levels


def scene_pixels(spec):
    return [SCENE_ROW * spec.res + col for col in SCENE_COLS]
