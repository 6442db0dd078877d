"""Step 7 of include/awpu_hip_csm.h (awpu_hip_csm_clean.h states it), CLEAN-SC, restated in numpy on top of csm_util for the
CLEAN-SC tests (test_csm_clean_cpu.py, test_gpu_csm_clean.py): every operation one float32 rounding, every fmaf through
cohere_util.fmaf, every sum in the rule's order.  A float64 CLEAN-SC of the same matrix to compare the rule with.  And the scene
the feature was argued with: two independent sources 15 dB apart on one grid row, the weak one among the strong one's side
lobes, low self-noise of a different level on every mic.  A plain helper, not a conftest."""
from __future__ import annotations

import numpy as np

import csm_util as CU
from csm_util import F32, fmaf, quiet

STEP_DTYPE = np.dtype([("pixel", "<i4"), ("before", "<f4"), ("removed", "<f4")])


def load(C):
    """Load: the entries b < a as they are, the diagonal (re, +0), the upper triangle the exact conjugate."""
    C = np.asarray(C, F32)
    U = C.shape[1]
    lower = np.tril(np.ones((U, U), bool), -1)
    eye = np.eye(U, dtype=bool)
    re, im = C[..., 0], C[..., 1]
    D = np.zeros_like(C)
    D[..., 0] = np.where(lower | eye, re, np.swapaxes(re, 1, 2))
    D[..., 1] = np.where(lower, im, np.where(eye, F32(0.0), -np.swapaxes(im, 1, 2)))
    return D


def component(D, s):
    """D [K, U, U, 2] loaded, s [K, U, 2] -> v [K, U, 2], qs [K]."""
    K, U = D.shape[0], D.shape[1]
    vr, vi = np.zeros((K, U), F32), np.zeros((K, U), F32)
    with np.errstate(**quiet):
        for b in range(U):
            dr, di = D[:, :, b, 0], D[:, :, b, 1]  # D[a][b], every a
            sr, si = s[:, b, 0][:, None], s[:, b, 1][:, None]
            vr = fmaf(dr, sr, vr)
            vr = fmaf(di, si, vr)
            vi = fmaf(di, sr, vi)
            vi = fmaf(-dr, si, vi)
        qs = np.zeros(K, F32)
        for a in range(U):
            qs = fmaf(s[:, a, 0], vr[:, a], qs)
            qs = fmaf(-s[:, a, 1], vi[:, a], qs)
    return np.stack([vr, vi], axis=-1), qs


def update(D, v, r, active):
    """D -= t v^H with t = v r, for the bins where `active`; -> a new D."""
    U = D.shape[1]
    lower = np.tril(np.ones((U, U), bool), -1)
    eye = np.eye(U, dtype=bool)
    with np.errstate(**quiet):
        tr = (v[:, :, 0] * r[:, None]).astype(F32)[:, :, None]  # by row a
        ti = (v[:, :, 1] * r[:, None]).astype(F32)[:, :, None]
        br, bi = v[:, None, :, 0], v[:, None, :, 1]  # by column b
        re = fmaf(-tr, br, D[..., 0])
        re = fmaf(-ti, bi, re)
        im = fmaf(-ti, br, D[..., 1])
        im = fmaf(tr, bi, im)
    out = np.zeros_like(D)
    out[..., 0] = np.where(lower | eye, re, np.swapaxes(re, 1, 2))
    out[..., 1] = np.where(lower, im, np.where(eye, F32(0.0), -np.swapaxes(im, 1, 2)))
    return np.where(np.asarray(active, bool)[:, None, None, None], out, D)


def pick(row):
    """Peel's pick of one dirty row: the pixel, or -1."""
    row = np.asarray(row, F32)
    with np.errstate(**quiet):
        ok = np.isfinite(row) & (row > 0)
    if not ok.any():
        return -1
    return int(np.argmax(np.where(ok, row, F32(-1.0))))  # (argmax: the first of equals, the lower index)


def dirty(pkg, D, block_count, s_all, bins, window):
    U = D.shape[1]
    return CU.maps(CU.quadratic(D, s_all, CU.CONVENTIONAL), bins, window, CU.CONVENTIONAL, U, block_count)


def step(pkg, matrix, pixel, off, frac, bins, gain=1.0, index=None):
    """awpu_hip_csm_clean_step_host restated: -> (D, v, qs)."""
    s_all = CU.steer(pkg, off, frac, bins, index)  # [P, K, U, 2]
    D = load(matrix)
    K = D.shape[0]
    pixel = np.asarray(pixel)
    takes = (pixel >= 0) & (pixel < s_all.shape[0])
    s = np.stack([s_all[pixel[k] if takes[k] else 0, k] for k in range(K)])
    v, qs = component(D, s)
    with np.errstate(**quiet):
        ok = takes & (qs > 0) & np.isfinite(qs)
        r = (F32(gain) / qs).astype(F32)
    D = update(D, v, r, ok)
    v = np.where(takes[:, None, None], v, F32(0.0))
    return D, v, np.where(takes, qs, F32(0.0)).astype(F32)


def clean(pkg, matrix, block_count, off, frac, bins, steps, gain=1.0, stop_ratio=0.0, window=0, index=None):
    """awpu_hip_csm_clean_host restated -> a dict: steps, clean, residual, map, residual_matrix, and `trace`: per iteration
    (the pixels stepped at [K] (-1: no step), D after it, v, qs, the pixels picked [K] -- a pick whose qs fails its test steps nowhere)."""
    s_all = CU.steer(pkg, off, frac, bins, index)
    P, K = s_all.shape[0], len(bins)
    D = load(matrix)
    rec = np.zeros((K, steps), STEP_DTYPE)
    rec["pixel"] = -1
    done = np.zeros(K, bool)
    first = np.zeros(K, F32)
    trace = []
    for i in range(steps):
        if done.all():
            break
        rows = dirty(pkg, D, block_count, s_all, bins, window)
        pixels = np.full(K, -1)
        before = np.zeros(K, F32)
        for k in range(K):
            if done[k]:
                continue
            p = pick(rows[k])
            if p >= 0:
                if i == 0:
                    first[k] = rows[k, p]
                with np.errstate(**quiet):
                    floor = F32(0.0) if stop_ratio == 0 else F32(stop_ratio) * first[k]
                if rows[k, p] < floor:
                    p = -1
            if p < 0:
                done[k] = True
                continue
            pixels[k], before[k] = p, rows[k, p]
        s = np.stack([s_all[max(pixels[k], 0), k] for k in range(K)])
        v, qs = component(D, s)
        with np.errstate(**quiet):
            ok = (pixels >= 0) & (qs > 0) & np.isfinite(qs)
            r = (F32(gain) / qs).astype(F32)
        done |= (pixels >= 0) & ~ok
        D = update(D, v, r, ok)
        for k in np.flatnonzero(ok):
            rec[k, i] = (pixels[k], before[k], F32(gain) * before[k])
        trace.append((np.where(ok, pixels, -1), D.copy(), v, qs, pixels))
    residual = dirty(pkg, D, block_count, s_all, bins, window)
    cleaned = np.zeros((K, P), F32)
    for k in range(K):
        for i in range(steps):
            if rec[k, i]["pixel"] >= 0:
                cleaned[k, rec[k, i]["pixel"]] = cleaned[k, rec[k, i]["pixel"]] + rec[k, i]["removed"]
    with np.errstate(**quiet):
        total = cleaned + residual
    return dict(steps=rec, clean=cleaned, residual=residual, map=total, residual_matrix=D, trace=trace)


def clean_f64(pkg, matrix, block_count, off, frac, bins, steps, gain=1.0, window=0, index=None):
    """CLEAN-SC of the same matrix in float64 (the rule's steering vectors, exact sums): -> (pixels [K, steps], removed [K, steps],
    residual [K, P])."""
    s_all = CU.as_complex(CU.steer(pkg, off, frac, bins, index))  # [P, K, U]
    P, K, U = s_all.shape
    C = CU.as_complex(load(matrix))
    ck = np.where((np.asarray(bins) == 0) | (np.asarray(bins) == 128), 1.0, 2.0)
    scale = (96.0 if window == 1 else 256.0) * 256.0 * U * U * block_count
    pixels, removed = np.full((K, steps), -1), np.zeros((K, steps))
    residual = np.zeros((K, P))
    for k in range(K):
        D, e = C[k].copy(), np.conj(s_all[:, k, :])  # e [P, U]
        rows = lambda: ck[k] * np.einsum("pa,ab,pb->p", np.conj(e), D, e).real / scale  # noqa: E731
        for i in range(steps):
            row = rows()
            p = int(np.argmax(row))
            if not row[p] > 0:
                break
            v = D @ e[p]
            qs = (np.conj(e[p]) @ v).real
            if not qs > 0:
                break
            D = D - gain * np.outer(v, np.conj(v)) / qs
            pixels[k, i], removed[k, i] = p, gain * row[p]
        residual[k] = rows()
    return pixels, removed, residual


# ---- the scene: the c1 array (8 x 8, 2 cm), bin 40 (7.6 kHz), a 32 x 32 sine-space grid; two independent noise sources on row 16,
# the weak one 15 dB down, nine pixels from the strong one, in its side-lobe region (the row's side lobes there are -12 .. -14 dB); 256 blocks; per-mic self-noise log-uniform
# in 0.05 .. 0.2 rms of the strong source.

SCENE_BIN = 40
SCENE_BLOCKS = 256
SCENE_ROW = 16
SCENE_COLS = (10, 19)
SCENE_DB = -15.0
SCENE_AMP = (1.0, 10.0 ** (SCENE_DB / 20.0))
SCENE_BAND_HZ = 100.0
SCENE_NOISE = (0.05, 0.2)
SCENE_SEED = 2024
SCENE_FIND = dict(radius=2, max_sources=4, min_ratio=0.01)


def scene_pixels(spec):
    return [SCENE_ROW * spec.res + col for col in SCENE_COLS]


def scene_samples(pkg, spec, xyz, seed=SCENE_SEED, n_blocks=SCENE_BLOCKS):
    """samples [n_mics, 256 * n_blocks] float32 of the scene (built as csm_util.scene_samples builds its own)."""
    S = pkg.synthetic
    n = 256 * n_blocks
    rng = np.random.default_rng(seed)
    f = np.fft.rfftfreq(n, 1.0 / S.SAMPLE_RATE)
    centre = SCENE_BIN * S.SAMPLE_RATE / 256.0
    band = np.abs(f - centre) <= SCENE_BAND_HZ
    sep = np.sin(np.deg2rad(spec.fov) / 2.0) / (spec.res / 2.0)
    x = np.zeros((xyz.shape[1], n))
    for col, amp in zip(SCENE_COLS, SCENE_AMP):
        px, py = (col - spec.res / 2.0 + 0.5) * sep, (SCENE_ROW - spec.res / 2.0 + 0.5) * sep
        theta, phi = float(np.arcsin(np.hypot(px, py))), float(np.arctan2(py, px))
        tau = pkg.binding.steering_delays(xyz, theta, phi).astype(np.float64)
        spectrum = np.where(band, rng.standard_normal(len(f)) + 1j * rng.standard_normal(len(f)), 0.0)
        waves = np.fft.irfft(spectrum[None, :] * np.exp(2j * np.pi * f[None, :] * tau[:, None] / S.SAMPLE_RATE), n, axis=1)
        x += amp * waves / waves.std()
    levels = np.exp(rng.uniform(np.log(SCENE_NOISE[0]), np.log(SCENE_NOISE[1]), xyz.shape[1]))
    x += levels[:, None] * rng.standard_normal(x.shape)
    return x.astype(F32)


def db(x, ref):
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(np.asarray(x, np.float64) / float(ref))
