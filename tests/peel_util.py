"""The rule of include/awpu_hip_peel.h restated in numpy, and the two-source scene, for the peel tests (test_peel_cpu.py,
test_gpu_peel.py): every operation one float32 rounding, in the rule's order.  A plain helper, not a conftest."""
from __future__ import annotations

import numpy as np

import cohere_util as CU

F32 = np.float32
fmaf = CU.fmaf


def reach(off, index):
    """(lo, length) of the beam for the table `off` [P, stride] at the active mics."""
    o = np.asarray(off)[:, np.asarray(index)]
    E = int(o.max()) - int(o.min())
    return -E - 1, 256 + 2 * E + 2


def u_of(gamma, gain, usable):
    """u[] of the rule: gamma without gains, gamma / g with, 0 where g == 0 (one float32 division)."""
    if gain is None:
        return np.full(usable, F32(gamma), F32)
    g = np.asarray(gain, F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(g == 0, F32(0), F32(gamma) / g).astype(F32)


def step(frame, off, frac, p, gamma, index=None, gain=None):
    """One step of one frame [n_streams, hist] at pixel p by the rule as written -> (the frame after it, the beam)."""
    frame = np.array(frame, F32)
    off, frac = np.asarray(off, np.int32), np.asarray(frac, F32)
    index = np.arange(off.shape[1]) if index is None else np.asarray(index)
    U = len(index)
    lo, L = reach(off, index)
    if p < 0:
        return frame, np.zeros(L, F32)
    u = u_of(gamma, gain, U)
    norm = F32(1.0) / F32(U)
    out = np.zeros(L, F32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for s, m in enumerate(index):
            base = int(off[p, m]) + lo
            x = frame[m, base:base + L + 1]
            if gain is not None:
                x = x * F32(gain[s])
            out = out + fmaf(frac[p, m], x[:-1] - x[1:], x[1:])
        b = out * norm
        assert b.dtype == F32
        for s, m in enumerate(index):
            base = int(off[p, m]) + lo + 1
            c = fmaf(frac[p, m], b[1:] - b[:-1], b[:-1])
            frame[m, base:base + L - 1] = fmaf(-u[s], c, frame[m, base:base + L - 1])
    return frame, b


def pick(row):
    """The loop's pick on a power row: the greatest finite power > 0, the lower index on a tie; -1 if there is none."""
    row = np.asarray(row, F32)
    ok = np.isfinite(row) & (row > 0)
    if not ok.any():
        return -1
    return int(np.where(ok, row, F32(-1)).argmax())


def floor_ratio(stop_ratio, first):
    return F32(0) if stop_ratio == 0 else F32(stop_ratio) * F32(first)


def loop(frame, sweep, do_step, steps, stop_ratio=0.0):
    """The loop of the rule on one frame with the sweep and the step given as functions (frame -> power row; (frame, pixel) ->
    frame): -> dict(steps [steps] records (pixel, before, removed), clean, residual, map, frame, rows = every P_k)."""
    rec = [(-1, F32(0), F32(0))] * steps
    row = np.asarray(sweep(frame), F32)
    rows = [row]
    first = F32(0)
    for k in range(steps):
        p = pick(row)
        if p < 0:
            break
        before = row[p]
        if k == 0:
            first = before
        if before < floor_ratio(stop_ratio, first):
            break
        frame = do_step(frame, p)
        row = np.asarray(sweep(frame), F32)
        rows.append(row)
        d = F32(before - row[p])
        rec[k] = (p, before, d if d > 0 else F32(0))
    clean = np.zeros(len(row), F32)
    for p, _, removed in rec:
        if p >= 0:
            clean[p] = clean[p] + removed
    return dict(steps=rec, clean=clean, residual=row, map=clean + row, frame=frame, rows=rows)


def steps_equal(got, want) -> bool:
    """got: PEEL_STEP_DTYPE records of one frame; want: the (pixel, before, removed) list of loop()."""
    return len(got) == len(want) and all(int(g["pixel"]) == w[0] and CU.same_bits(g["before"], w[1]) and CU.same_bits(g["removed"], w[2])
                                         for g, w in zip(got, want))


# ---- the scene: two independent band-limited noise sources, the second 15 dB under the first, on the 8 x 8 array

RATE, PITCH, RES, FOV, HIST = 48828.0, 0.02, 24, 120.0, 1024
STRONG, WEAK = (12, 12), (5, 17)  # (row, column) on the 24 x 24 grid
WEAK_DB = -15.0


def scene_table(pkg):
    xyz = pkg.create_antenna(8, 8, PITCH)
    return pkg.build_delay_table(xyz, RES, RES, FOV)


def scene_frame(off, frac, seed, weak_db=WEAK_DB, sigma=0.05):
    """One frame [64, 1024]: each source is 2-9 kHz noise of unit (the weak one: weak_db) variance that the table's own delays
    of its pixel align -- mic m hears s(n - (off + 1 - frac)) --, plus white noise of `sigma` per mic."""
    rng = np.random.default_rng(seed)
    n = 2 * HIST
    f = np.fft.rfftfreq(n, 1.0 / RATE)
    band = (f >= 2000.0) & (f <= 9000.0)
    frame = np.zeros((off.shape[1], HIST))
    for (r, c), db in ((STRONG, 0.0), (WEAK, weak_db)):
        spec = np.where(band, rng.normal(size=f.size) + 1j * rng.normal(size=f.size), 0.0)
        spec = spec / np.fft.irfft(spec, n).std()  # unit variance in time
        p = r * RES + c
        delay = off[p].astype(np.float64) + 1.0 - frac[p].astype(np.float64)
        for m in range(off.shape[1]):
            frame[m] += 10.0 ** (db / 20.0) * np.fft.irfft(spec * np.exp(-2j * np.pi * f * delay[m] / RATE), n)[:HIST]
    frame += sigma * rng.normal(size=frame.shape)
    return frame.astype(F32)


def db(x, ref):
    return 10.0 * np.log10(np.float64(x) / np.float64(ref))
