"""The shapes of the peel edge tests (test_peel_edges_cpu.py, test_gpu_peel_edges.py), defined once: synthetic tables whose mic
count, beam length and pixel count sit on the branches of csrc/peel_kernels.hip, and the tied scene table.

The step's kernel walks the active mics sixteen at a time and then a tail (the beam pass), two at a time eight apart (the
subtraction), beam samples 512 a trip (the beam pass) and 4 x 64 a trip (the subtraction):

    mic counts    U = 1, 8, 9, 15, 16, 17, 24, 31, 32, 33 of 40 streams, E = 40 (len 338), 5 pixels; U = 256 of 300, E = 30, 2 pixels
    beam lengths  8 streams, all active: E = 0 (len 258, n = 257: one lane alone in the second trip of the subtraction), E = 127
                  (len 512: exactly one trip of the beam pass), E = 128 (len 514), E = 255 (len 768) on a table that fits the
                  history exactly: min off 256, max off 511, the step reads samples 0 .. 1023

A plain helper, not a conftest."""
from __future__ import annotations

import numpy as np

import peel_util as PU

GAINS = (1.5, 0.0, -0.75, 1.0, 0.25)
MIC_COUNTS = (1, 8, 9, 15, 16, 17, 24, 31, 32, 33)
BEAM_REACHES = (0, 127, 128, 255)


def synthetic(n_streams, usable, E, n_pixels, seed, hist=1024, fit=False, shuffled=True, n_frames=3):
    """A dict like test_peel_cpu.small_shape(): off, frac [n_pixels, n_streams], index [usable], gain [usable] (list order), frames
    [n_frames, n_streams, hist], pixel [n_frames].

    off is uniform in [base, base + E], at every stream; entry (pixel 0, index[0]) is base and entry (pixel P-1, index[-1]) is
    base + E, so the reach is E at the active mics whatever the draw.  With `fit`, base = E + 1: the lowest sample the step reads
    is 0, and with hist = 3 E + 259 the highest is hist - 1; without, the reach lies in the middle of the history.  frac is random,
    with exact 0 and 1 mixed into row 0 and whole rows of 0 and of 1 between the first and the last.  The first frame takes pixel
    0, the last P - 1, the second none (-1); further ones walk the table."""
    assert 1 <= usable <= n_streams and E >= 0 and n_pixels >= 1 and n_frames >= 3
    rng = np.random.default_rng(seed)
    top = hist - 258 - 2 * E  # the highest base the range rule takes: base + 3 E + 257 <= hist - 1
    base = E + 1 if fit else (E + 1 + top) // 2
    assert E + 1 <= base <= top, "the reach does not fit the history"
    off = rng.integers(base, base + E + 1, size=(n_pixels, n_streams)).astype(np.int32)
    frac = rng.random((n_pixels, n_streams)).astype(np.float32)
    frac[0, 0::3] = 0.0
    frac[0, 1::3] = 1.0
    for p in range(1, n_pixels - 1):
        if p % 5 in (1, 2):
            frac[p, :] = 0.0 if p % 5 == 1 else 1.0
    index = (rng.permutation(n_streams)[:usable] if shuffled else np.arange(usable)).astype(np.int32)
    off[0, index[0]], off[n_pixels - 1, index[-1]] = base, base + E
    assert PU.reach(off, index) == (-E - 1, 258 + 2 * E)
    gain = np.array([GAINS[s % len(GAINS)] for s in range(usable)], np.float32)
    frames = (rng.random((n_frames, n_streams, hist)) * 2 - 1).astype(np.float32)
    pixel = np.array([(k - 1) % (n_pixels + 1) - 1 for k in range(n_frames)], np.int32)  # k = 1: -1, then 0, 1, ..
    pixel[0], pixel[-1] = 0, n_pixels - 1
    assert (pixel == -1).any()
    return dict(off=off, frac=frac, index=index, gain=gain, frames=frames, pixel=pixel)


def mic_shape(U, n_frames=3):
    if U == 256:
        return synthetic(300, 256, 30, 2, seed=7256, n_frames=n_frames)
    return synthetic(40, U, 40, 5, seed=7000 + U, n_frames=n_frames)


def beam_shape(E):
    if E == 0:  # every offset equal
        return synthetic(8, 8, 0, 3, seed=8000)
    if E == 255:  # the exact fit: a sorted list, so that stream 0 reads sample 0 and stream 7 sample hist - 1
        return synthetic(8, 8, 255, 4, seed=8255, fit=True, shuffled=False)
    return synthetic(8, 8, E, 4, seed=8000 + E)


SHAPES = {**{f"U{U}": (lambda U=U: mic_shape(U)) for U in MIC_COUNTS + (256,)}, **{f"E{E}": (lambda E=E: beam_shape(E)) for E in BEAM_REACHES}}


def reach_of(s):
    """E of a shape."""
    o = s["off"][:, s["index"]]
    return int(o.max()) - int(o.min())


def by_stream(s):
    """The shape's gains as Engine.set_mic_gains takes them: [n_streams] by stream id, 1 off the list."""
    g = np.ones(s["off"].shape[1], np.float32)
    g[s["index"]] = s["gain"]
    return g


def rotated(pixel):
    """The pixels of a second step: every frame takes its neighbour's."""
    return np.roll(np.asarray(pixel, np.int32), -1)


# ---- the tied scene table: rows of the strong source's pixel at two more pixels

STRONG = PU.STRONG[0] * PU.RES + PU.STRONG[1]  # 300
WEAK = PU.WEAK[0] * PU.RES + PU.WEAK[1]        # 137


def tied_table(off, frac, at=(5, 570)):
    """The scene table with the rows `at` replaced by the strong pixel's: those pixels' powers have the strong pixel's bits."""
    off, frac = np.array(off), np.array(frac)
    for p in at:
        off[p], frac[p] = off[STRONG], frac[STRONG]
    return off, frac
