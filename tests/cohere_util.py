"""The rule of include/awpu_hip_cohere.h restated in numpy, for the coherence tests (test_cohere_cpu.py, test_gpu_cohere.py): every
operation one float32 rounding, in the rule's order, all pixels of a frame at once.  A plain helper, not a conftest."""
from __future__ import annotations

import numpy as np

F32 = np.float32


def fmaf(a, b, c):
    """fmaf(a, b, c) on float32 arrays: a * b + c rounded once.  The product is exact in float64; the sum is rounded to odd there
    (TwoSum gives the sign of what the float64 addition dropped), so that the rounding to float32 sees which side of a tie the
    exact value lies on."""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        p = np.asarray(a, np.float64) * np.asarray(b, np.float64)
        c64 = np.broadcast_to(np.asarray(c, np.float64), p.shape)
        s = p + c64
        bb = s - p
        err = (p - (s - bb)) + (c64 - bb)
        other = np.where(err > 0, np.nextafter(s, np.inf), np.where(err < 0, np.nextafter(s, -np.inf), s))
        odd = (s.view(np.int64) & 1) == 1
        return np.where((err == 0) | odd | ~np.isfinite(s), s, other).astype(F32)


def rule(frame, off, frac, index=None, gain=None):
    """(power, coherence, weighted [P], sums, energy [P, 256]) of one frame [n_streams, hist] by the rule as written."""
    frame = np.asarray(frame, F32)
    off, frac = np.asarray(off, np.int32), np.asarray(frac, F32)
    index = np.arange(off.shape[1]) if index is None else np.asarray(index)
    P, U = off.shape[0], len(index)
    out = np.zeros((P, 256), F32)
    e = np.zeros((P, 256), F32)
    taps = np.arange(257)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for s, m in enumerate(index):
            x = frame[m][off[:, m][:, None] + taps[None, :]]  # [P, 257]
            if gain is not None:
                x = x * F32(gain[s])
            f = frac[:, m][:, None]
            t = fmaf(f, x[:, :256] - x[:, 1:], x[:, 1:])
            out = out + t
            ma = t[:, 1:255] * F32(0.5) - F32(0.25) * (t[:, 2:256] + t[:, 0:254])
            e[:, 1:255] = fmaf(ma, ma, e[:, 1:255])
        MA = out[:, 1:255] * F32(0.5) - F32(0.25) * (out[:, 2:256] + out[:, 0:254])
        sq = MA * MA
        num = np.zeros(P, F32)
        den = np.zeros(P, F32)
        for i in range(254):
            num = num + sq[:, i]
        for i in range(1, 255):
            den = den + e[:, i]
        assert num.dtype == F32 and den.dtype == F32 and out.dtype == F32
        power = num / F32(256 * U)
        c = np.where(den > 0, num / (F32(U) * den), F32(0.0)).astype(F32)
        c = np.where(c > 1, F32(1.0), c).astype(F32)
        weighted = power * c
    return power, c, weighted, out, e


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same_bits(a, b) -> bool:
    return np.array_equal(bits(a), bits(b))


def rel_err(got, want) -> float:
    """max |got - want| / |want| over every entry, no floor: where want is 0, got must be."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    d = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(want != 0.0, d / np.abs(want), np.where(d == 0.0, 0.0, np.inf))
    return float(r.max())


def median_over_max_db(row) -> float:
    row = np.asarray(row, np.float64)
    return float(10.0 * np.log10(np.median(row) / row.max()))
