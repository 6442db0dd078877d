"""What the exposure tests (test_expose_cpu.py, test_gpu_expose.py) share: the rule of include/awpu_hip_expose.h restated in numpy,
and power rows at the value edges.  A plain helper, not a conftest."""
from __future__ import annotations

import numpy as np

MEAN, PEAK = 0, 1


def expose_np(power: np.ndarray, first: int, every: int, length: int, mode: int, carry: np.ndarray):
    """-> (frames [n_frames, n_pixels], acc after the last block).  float32 adds in block order, one division by np.float32(L),
    the PEAK order on the rows' uint32 views; `carry` is acc before block 0 and is not written."""
    power = np.ascontiguousarray(power, np.float32)
    acc = np.array(carry, np.float32)
    frames = []
    with np.errstate(all="ignore"):
        for k in range(len(power)):
            t = k - first + length - 1
            if t < 0 or t % every >= length:
                continue
            q, p = t % every, power[k]
            if q == 0:
                acc = p.copy()
            elif mode == MEAN:
                acc = acc + p
            else:
                acc = np.where(p.view(np.uint32) > acc.view(np.uint32), p, acc)
            if q == length - 1:
                frames.append(acc / np.float32(length) if mode == MEAN else acc.copy())
    return (np.stack(frames) if frames else np.zeros((0, power.shape[1]), np.float32)), acc


def edge_rows(n_blocks: int, n_pixels: int, seed: int = 5) -> np.ndarray:
    """Non-negative random rows with, scattered over them: subnormals, zeros of both signs, the largest finite value, +inf and
    the quiet NaN 0x7fc00000 (one payload only: which of two different NaNs an addition returns is the adder's business, and no
    -inf: inf - inf makes a NaN whose sign is the adder's too)."""
    rng = np.random.default_rng(seed)
    rows = rng.random((n_blocks, n_pixels), dtype=np.float32) * np.float32(3.0)
    specials = np.array([0x00000001, 0x007FFFFF, 0x00400000, 0x00800000, 0x00000000, 0x80000000, 0x7F7FFFFF, 0x7F800000, 0x7FC00000],
                        np.uint32).view(np.float32)
    where = rng.random((n_blocks, n_pixels)) < 0.3
    rows[where] = specials[rng.integers(0, len(specials), int(where.sum()))]
    # whole windows of subnormals (sums that stay subnormal, and a subnormal divided), and of -0.0
    rows[:, 0] = np.uint32(0x00000003).view(np.float32)
    if n_pixels > 1:
        rows[:, 1] = np.float32(-0.0)
    return rows


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
