"""The sample-value tiers of the value-edge tests (test_value_edges_cpu.py, test_gpu_value_edges.py), defined once.

Every input is built from X0 = util.hash_frames(..., scale=2**-6): a tier is exactly 2^k X0 (two float32 multiplications by powers of
two, each exact -- X0's samples are 24-bit integers times 2^-29, so even 2^-120 X0 is a whole number of 2^-149, the subnormal step),
or X0 with a few samples replaced.  What a tier is, in terms of the IEEE restatement (oracle/das_oracle.c):

    small  k = -40   everything normal: sums and powers scale exactly
    big    k = +55   the same
    top    k = +120  sums finite and exactly scaled, every square overflows: every power +inf
    dusk   k = -56   sums and most squares normal; the division by 256 * usable rounds into the subnormal range: every power
                     subnormal and none 0 (about 1 M to 4.5 M units of 2^-149)
    dim    k = -64   sums normal, every non-zero square subnormal, every power subnormal and none 0 (16 to 68 units); the sum of
                     squares is a whole number of units below 2^24, so it is exact in any order
    under  k = -100  samples normal (or 0); differences and products partly subnormal; every power 0
    sub    k = -120  every non-zero sample subnormal, the sums subnormal; every power 0
    zeros            a frame of -0.0, and X0 with one active mic's row set to -0.0
    nonfinite        X0 with +inf, NaN, a +3e38 / -3e38 pair (its difference overflows) and a (+inf, finite) pair where a pixel's
                     fraction is exactly 0 (fma(0, inf, next) = NaN), each in an active mic's row at a history sample that some
                     pixels' windows reach and others do not

All of this is host arithmetic on subnormals: it means what it says only while the host is not flushing them (host_flushes()).
A plain helper, not a conftest: the GPU tests' child processes import it too."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import util

SCALED = {"small": -40, "big": 55, "top": 120, "dusk": -56, "dim": -64, "under": -100, "sub": -120}
EPILOGUE = ("dusk", "dim")      # the tiers whose powers are subnormal and not 0: what the epilogue does below the normal range
# awpu_hip_beams divides by 256 alone, not by 256 * usable: on the golden beams_c1 table 2^-56 X0 gives normal powers (93 M to 239 M
# units of 2^-149; the smallest normal is 8.4 M).  No single k serves both: the table needs k <= -59 for subnormal powers, and below
# k = -57 the sweeps' powers are so few units that a reordered sum of squares moves them by more than the flat 1e-5.  So the beams'
# dusk is k = -59 -- 1.45 M to 3.73 M units, the band the sweeps' dusk is in -- and its dim is the sweeps' (1416 to 3642 units).
BEAMS_SCALED = {"dusk": -59, "dim": -64}
TINY = np.float32(2.0 ** -126)  # the smallest normal
UNIT = 2.0 ** -149              # the subnormal step (a double: units() counts in it exactly)


def host_flushes() -> bool:
    """Does this thread flush subnormal results (FTZ) or operands (DAZ)?  (numpy follows the thread's mode.)"""
    a = np.float32(1e-30) * np.float32(1e-10)        # a subnormal result
    b = np.float32(2.0 ** -140) * np.float32(4.0)    # a subnormal operand
    return not (a != 0 and b == np.float32(2.0 ** -138))


def scale_pow2(x: np.ndarray, k: int) -> np.ndarray:
    """2^k x in float32 by two multiplications by powers of two (2^k itself need not be a float32)."""
    assert not host_flushes()
    a = k // 2
    with np.errstate(under="ignore", over="ignore"):
        return (np.asarray(x, np.float32) * np.float32(2.0 ** a)) * np.float32(2.0 ** (k - a))


def ldexp32(x: np.ndarray, k: int) -> np.ndarray:
    """ldexp in float32 (rounds once; exact wherever the result is normal)."""
    with np.errstate(under="ignore", over="ignore"):
        return np.ldexp(np.asarray(x, np.float32), k).astype(np.float32)


def units(x) -> np.ndarray:
    """x in units of 2^-149, as doubles (exact for every float32)."""
    return np.asarray(x, np.float64) / UNIT


def subnormal(x) -> np.ndarray:
    return (np.abs(x) < TINY) & (x != 0)


def epilogue32(sums: np.ndarray, divisor: int, order: str) -> np.ndarray:
    """The epilogue of the restatement (oracle/das_oracle.c epilogue_f32) on sums [P, 256] in float32 numpy, one rounding per
    operation: MA = out[i] * 0.5 - 0.25 * (out[i + 1] + out[i - 1]) for i = 1 .. 254, the sum of MA^2 in the order `forward` (the
    restatement's own), `reversed` or `pairwise` (a tree over neighbours), then one division by `divisor` (256 * usable)."""
    assert not host_flushes()
    s = np.asarray(sums, np.float32)
    with np.errstate(under="ignore", over="ignore", invalid="ignore"):
        ma = s[:, 1:255] * np.float32(0.5) - np.float32(0.25) * (s[:, 2:256] + s[:, 0:254])
        sq = ma * ma
        assert sq.dtype == np.float32
        if order == "pairwise":
            while sq.shape[1] > 1:
                if sq.shape[1] % 2:
                    sq = np.concatenate([sq, np.zeros((len(sq), 1), np.float32)], axis=1)
                sq = sq[:, 0::2] + sq[:, 1::2]
            acc = sq[:, 0]
        else:
            acc = np.zeros(len(sq), np.float32)
            for i in (range(sq.shape[1]) if order == "forward" else range(sq.shape[1] - 1, -1, -1)):
                acc = acc + sq[:, i]
        return (acc / np.float32(divisor)).astype(np.float32)


def bits(x: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def same_bits(a, b) -> bool:
    return np.array_equal(bits(a), bits(b))


def same_nonfinite(got: np.ndarray, want: np.ndarray) -> bool:
    """Finite entries bit-equal; NaN where NaN, +inf where +inf, -inf where -inf."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    fin = np.isfinite(want)
    return bool(np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isposinf(got), np.isposinf(want)) and
                np.array_equal(np.isneginf(got), np.isneginf(want)) and np.array_equal(bits(got)[fin], bits(want)[fin]))


@dataclass
class Case:
    """A table, a mic list and X0.  `pixels`: the pixels the oracle is run on (all of them for the small grid)."""
    name: str
    xyz: np.ndarray
    rows: int
    cols: int
    off: np.ndarray
    frac: np.ndarray
    index: np.ndarray
    x0: np.ndarray            # [batch, n_streams, hist]
    pixels: np.ndarray
    bad: dict = field(default_factory=dict)  # nonfinite tier: name -> (stream, history sample)

    @property
    def n_pixels(self) -> int:
        return self.rows * self.cols

    @property
    def batch(self) -> int:
        return self.x0.shape[0]

    def tier(self, name: str) -> np.ndarray:
        """[batch, n_streams, hist] of a tier.  zeros: frame 0 all -0.0, the others X0 with the row of index[1] set to -0.0;
        zero_row: every frame the latter (the single-frame cases)."""
        if name == "x0":
            return self.x0
        if name in SCALED:
            return scale_pow2(self.x0, SCALED[name])
        if name == "nonfinite":
            return self.with_bad_samples(self.x0)
        assert name in ("zeros", "zero_row"), name
        x = self.x0.copy()
        x[:, self.index[1], :] = -0.0
        if name == "zeros":
            x[0] = -0.0
        return x

    def with_bad_samples(self, x: np.ndarray) -> np.ndarray:
        """x [..., n_streams, hist] with the nonfinite tier's samples put in."""
        x = x.copy()
        for what, (m, t) in self.bad.items():
            x[..., m, t:t + len(BAD[what])] = BAD[what]
        return x


BAD = {"inf": (np.float32(np.inf),), "nan": (np.float32(np.nan),), "overflow": (np.float32(3e38), np.float32(-3e38)),
       "frac0": (np.float32(np.inf), np.float32(0.5))}


def tile_edge_pixels(rows: int, cols: int, tile_cols: int, at_least: int = 512) -> np.ndarray:
    """The four corner pixels of the single-frame kernels' tiles (4 rows x tile_cols columns, clipped at the grid's edge): of every
    tile on the grid's border and of every second tile inside, checkerboard fashion -- so the first and last row of every tile row
    and the first and last column of every tile column are there -- plus fixed others up to `at_least`."""
    chosen = set()
    n_tr, n_tc = (rows + 3) // 4, (cols + tile_cols - 1) // tile_cols
    for tr in range(n_tr):
        for tc in range(n_tc):
            if (tr + tc) % 2 == 0 or tr in (0, n_tr - 1) or tc in (0, n_tc - 1):
                for r in (4 * tr, min(4 * tr + 3, rows - 1)):
                    for c in (tile_cols * tc, min(tile_cols * (tc + 1), cols) - 1):
                        chosen.add(r * cols + c)
    others = [int(p) for p in np.random.default_rng(11).permutation(rows * cols) if int(p) not in chosen]
    chosen |= set(others[:max(0, at_least - len(chosen))])
    return np.array(sorted(chosen), np.int64)


def make_case(name: str, oracle_py, build_delay_table=None) -> Case:
    """The cases of the GPU tests.  Tables from `build_delay_table` (the library's) or the oracle's compute_delay_lut: the same
    arrays (tests/test_host_mirror.py)."""
    arrays, rows, cols, mics, batch, seed, tile_cols = CASES[name]
    xyz = oracle_py.create_tiled_antenna(arrays, 1)
    n = xyz.shape[1]
    off, frac = (build_delay_table or oracle_py.compute_delay_lut)(xyz, rows, cols, 180.0)
    if mics == n:
        index = np.arange(n, dtype=np.int32)
    else:  # a ragged list; the corner mics are the ones whose delay is the minimum (fraction exactly 0) for a quarter of the sky
        pick = np.random.default_rng(7).choice(np.arange(1, n), mics - 1, replace=False)
        index = np.sort(np.concatenate([[0], pick])).astype(np.int32)
    x0 = util.hash_frames(n, 1024, seed=seed, batch=batch)
    pixels = np.arange(rows * cols) if rows * cols <= 1024 else tile_edge_pixels(rows, cols, tile_cols)
    case = Case(name, xyz, rows, cols, off, frac, index, x0, pixels)
    case.bad = place_bad_samples(case)
    return case


def place_bad_samples(case: Case) -> dict:
    """Where the nonfinite tier's bad samples go.  A pixel reads samples off .. off + 256 of a mic: a bad sample at history position
    t = (the q-quantile of that mic's offsets) + 255 is inside the window of the pixels whose offset is at most 255 below it and
    past the end of the others' -- "mid-history": well inside the frame, at the edge of the windows."""
    off, frac, index = case.off[case.pixels], case.frac[case.pixels], case.index
    bad = {}
    for what, s, q in (("inf", 3, 0.1), ("nan", len(index) // 2, 0.1), ("overflow", len(index) - 2, 0.1)):
        m = int(index[s])
        lo = int(np.quantile(off[:, m], 1.0 - q))  # pixels with off >= lo reach lo + 255
        bad[what] = (m, lo + 255)
    # a (cur, next) = (+inf, finite) pair at the last output sample of a pixel whose fraction for that mic is exactly 0 (the mic with
    # the smallest delay: its offset is the largest there, so pixels that look elsewhere do not reach the pair)
    taken = {m for m, _ in bad.values()}
    for m in (int(m) for m in index if int(m) not in taken):
        zero = np.flatnonzero(frac[:, m] == 0.0)
        if zero.size:
            bad["frac0"] = (m, int(off[zero, m].max()) + 255)
            break
    assert "frac0" in bad, "no active mic has a pixel with fraction 0"
    return bad


# name: arrays side by side, rows, cols, active mics, batch, seed of X0, columns of a tile (0: the oracle runs on every pixel)
CASES = {
    # c2's geometry on a 24 x 40 grid: 3 x 3 tiles of 8 x 16, the last column of tiles partial; 37 ragged mics; batch 3: the last
    # pair is a frame with itself
    "grid37": (4, 24, 40, 37, 3, 4009013, 0),
    "grid36": (4, 24, 40, 36, 3, 4009013, 0),   # whole groups of four: the packed entry points
    # the single-frame kernels take grids of more than 32 pixels per CU: the shapes of test_gpu_dispatch.py's census
    "one_array_100": (1, 100, 100, 64, 1, 9002, 16),    # exact_ndh_stationary
    "four_arrays_96": (4, 96, 96, 256, 1, 9003, 16),    # exact_ndh
    "c2_64": (4, 64, 64, 256, 1, 9004, 4),             # exact_ndp
}


def oracle_sums(oracle_py, case: Case, frame: np.ndarray, fir=None):
    """(power, sums) of one frame on case.pixels by the IEEE restatement."""
    off, frac = case.off[case.pixels], case.frac[case.pixels]
    if fir is not None:
        return oracle_py.das_fir8_f32(frame, off, frac, fir, index=case.index, want_out=True)
    return oracle_py.das_f32(frame, off, frac, index=case.index, want_out=True)
