"""The rule of include/awpu_hip_tones.h restated in numpy, for the tone tests (test_tones_cpu.py, test_gpu_tones.py): every operation
one float32 rounding, in the rule's order, all pixels of a frame at once; the two tables are read from the library.  And the
two-source scene the feature was argued with.  A plain helper, not a conftest."""
from __future__ import annotations

import numpy as np

from cohere_util import F32, bits, fmaf, rel_err, same_bits  # noqa: F401

BINS = 129
REV8 = np.array([int(f"{n:08b}"[::-1], 2) for n in range(256)])


def sums(frame, off, frac, index=None, gain=None):
    """Step 1: out[P, 256] of one frame, cohere_util.rule's out[]."""
    frame = np.asarray(frame, F32)
    off, frac = np.asarray(off, np.int32), np.asarray(frac, F32)
    index = np.arange(off.shape[1]) if index is None else np.asarray(index)
    out = np.zeros((off.shape[0], 256), F32)
    taps = np.arange(257)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for s, m in enumerate(index):
            x = frame[m][off[:, m][:, None] + taps[None, :]]  # [P, 257]
            if gain is not None:
                x = x * F32(gain[s])
            out = out + fmaf(frac[:, m][:, None], x[:, :256] - x[:, 1:], x[:, 1:])
    assert out.dtype == F32
    return out


def transform(out, w, tw, wss, usable):
    """Steps 2 to 4: out [P, 256] -> (spectrum [P, 129, 2], bins [P, 129]); w [256] and tw [128, 2] are the library's tables."""
    out, w, tw = np.asarray(out, F32), np.asarray(w, F32), np.asarray(tw, F32)
    P = out.shape[0]
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        y = np.zeros((P, 256), F32)
        ma = out[:, 1:255] * F32(0.5) - F32(0.25) * (out[:, 2:256] + out[:, 0:254])
        y[:, 1:255] = ma * w[1:255]
        re, im = y[:, REV8].copy(), np.zeros((P, 256), F32)
        h = 1
        while h < 256:
            pos = np.arange(256)
            a = pos[(pos & h) == 0]
            b = a + h
            j = a & (h - 1)
            wr, wi = tw[j * (128 // h), 0], tw[j * (128 // h), 1]
            tr = re[:, b] * wr - im[:, b] * wi
            ti = re[:, b] * wi + im[:, b] * wr
            ar, ai = re[:, a].copy(), im[:, a].copy()
            re[:, a], im[:, a] = ar + tr, ai + ti
            re[:, b], im[:, b] = ar - tr, ai - ti
            h *= 2
        assert re.dtype == F32 and im.dtype == F32
        re, im = re[:, :BINS], im[:, :BINS]
        s = re * re + im * im
        c = np.full(BINS, 2.0, F32)
        c[0] = c[BINS - 1] = 1.0
        bins = (c * s) / (F32(wss) * F32(256 * usable))
        assert bins.dtype == F32
    return np.stack([re, im], axis=-1), bins


def groups(bins, edges):
    """Step 5: tone [n_groups, P], k ascending from +0.0."""
    tone = np.zeros((len(edges) - 1, bins.shape[0]), F32)
    with np.errstate(over="ignore", invalid="ignore"):
        for g in range(len(edges) - 1):
            for k in range(edges[g], edges[g + 1]):
                tone[g] = tone[g] + bins[:, k]
    return tone


def pitch(bins, edges):
    """Step 6: the greater bits win, equal bits go to the lower k."""
    u = bits(bins)[:, edges[0]:edges[-1]]
    return (edges[0] + np.argmax(u, axis=1)).astype(np.int32)  # argmax: the first of equal maxima


def rule(pkg, frame, off, frac, edges, window=0, index=None, gain=None):
    """{tone [G, P], pitch [P], bins [P, 129], spectrum [P, 129, 2], sums [P, 256]} of one frame by the rule as written."""
    usable = off.shape[1] if index is None else len(index)
    out = sums(frame, off, frac, index, gain)
    spectrum, b = transform(out, pkg.tones_window(window), pkg.tones_twiddles(), 96.0 if window == 1 else 256.0, usable)
    edges = [int(e) for e in edges]
    return dict(tone=groups(b, edges), pitch=pitch(b, edges), bins=b, spectrum=spectrum, sums=out)


def bins64(out, window_table, wss, usable, want_floor=False):
    """Steps 2 to 4 in float64 on the rule's own out[]: numpy's rfft.  With want_floor also what step 2's one fp32 addition can
    move a bin by, whatever follows it (stencil_floor)."""
    out32 = np.asarray(out, F32)
    out = out32.astype(np.float64)
    w = np.asarray(window_table, np.float64)
    y = np.zeros_like(out)
    y[:, 1:255] = (0.5 * out[:, 1:255] - 0.25 * (out[:, 2:256] + out[:, 0:254])) * w[1:255]
    z = np.fft.rfft(y, axis=1)
    c = np.full(BINS, 2.0)
    c[0] = c[BINS - 1] = 1.0
    scale = float(wss) * 256.0 * usable
    bins = c * (z.real ** 2 + z.imag ** 2) / scale
    if not want_floor:
        return bins
    return bins, stencil_floor(out32, w, np.abs(z), c, scale)


def stencil_floor(out32, w, z_abs, c, scale):
    """[P, 129]: how far the rounding of out[i+1] + out[i-1] in fp32 alone can move bins[k], derived from the number format.  That
    sum s_i is off by at most ulp(s_i) / 2; the stencil's 0.25 and the window carry it into y[i] as e_i <= 0.125 ulp(s_i) w[i]; a
    transform is linear with unit-modulus weights, so every z[k] moves by at most E = sum_i e_i; and c |z|^2 / scale moves by at
    most c (2 |z[k]| E + E^2) / scale.  (0.5 out[i] is exact, and every later rounding is relative to the value it rounds.)"""
    with np.errstate(over="ignore", invalid="ignore"):
        s = (out32[:, 2:256] + out32[:, 0:254]).astype(F32)
    E = (0.125 * np.spacing(np.abs(s)).astype(np.float64) * w[1:255]).sum(axis=1)[:, None]
    return c * (2.0 * z_abs * E + E * E) / scale


# ---- the two-source scene: c1, plane waves A (9 kHz, bin 47) and B (3.05 kHz, bin 16, 26.5 dB under A in the power map)

SCENE = (dict(hz=9000.0, amp=1e-2, theta=20.0, phi=35.0, bin=47), dict(hz=3050.0, amp=3e-3, theta=40.0, phi=200.0, bin=16))
SCENE_NOISE = 1e-3


def scene_frame(pkg, xyz, seed=4321, hist=1024):
    """One frame [n_mics, hist] of the two-source scene, built as synthetic.make_frames builds its one source."""
    S = pkg.synthetic
    t = np.arange(hist, dtype=np.float64)
    frame = SCENE_NOISE * (np.random.RandomState(seed).rand(xyz.shape[1], hist) * 2.0 - 1.0)
    for src in SCENE:
        tau = pkg.binding.steering_delays(xyz, np.deg2rad(src["theta"]), np.deg2rad(src["phi"])).astype(np.float64)
        frame = frame + src["amp"] * np.sin(2.0 * np.pi * src["hz"] * (t[None, :] + tau[:, None]) / S.SAMPLE_RATE)
    return frame.astype(F32)


def scene_pixels(pkg, spec):
    """The pixels of sources A and B on the grid of `spec`."""
    out = []
    for src in SCENE:
        r, c = pkg.synthetic.source_pixel(spec, np.deg2rad(src["theta"]), np.deg2rad(src["phi"]))
        out.append(r * spec.res + c)
    return out
