"""(no device) Value edges behind the sweep: the sweeps write exact 0, subnormals, +inf and NaN (README), and the display step, the
peak finder and calibration take those rows and samples as they are.  Here are the frames the GPU tests (test_gpu_behind_sweep.py)
share, the plain numpy restatements of the three rules -- float32 where the rule says float, float64 where it says double --, and
the host entry points against them: awpu_hip_heatmap_u8, awpu_hip_find_peaks and the oracle's calibration.  Two defects are pinned:
`min_ratio = 0` was no "no ratio threshold" on a frame holding +inf or NaN (0 * inf is NaN), and calibration sorted mean squares
that may hold NaN with operator<, so its median depended on which mic held the NaN and the NaN stream came out usable."""
import functools

import numpy as np
import pytest

import util
import value_edges as V
from test_find_cpu import assert_same, restated

FLT_MAX = np.finfo(np.float32).max
INF = np.float32(np.inf)
NAN_BITS = (0x7FC00000, 0xFFC00000)  # the quiet NaN of either sign


def put_bits(x, where, pattern):
    """x[where] = the float32 of that bit pattern, whatever a conversion would make of a NaN's sign."""
    x.view(np.uint32)[where] = pattern


# ------------------------------------------------------------------------------------------------ display

PEAKS = {"one": np.float32(1.0), "flt_max": FLT_MAX, "tiny": np.float32(1.5 * 2.0 ** -126), "sub64": np.float32(64 * 2.0 ** -149)}
DISPLAY_N = [1, 63, 1025, 16385]  # the last: more than one pass of the 64 x 256 grid-stride launch


@functools.lru_cache(maxsize=None)
def dim_row():
    """A power row of the dim tier (value_edges.py) by the oracle: 960 subnormal powers, 16 to 68 units of 2^-149."""
    from oracle import oracle_py

    case = V.make_case("grid37", oracle_py)
    power, _ = V.oracle_sums(oracle_py, case, case.tier("dim")[0])
    assert V.subnormal(power).all()
    power.setflags(write=False)
    return power


def staircase(M, n):
    """For j = 0 .. 255 the three floats at and next to float32(M * j / 255), clipped to [0, M]: the pixels whose level is about to
    change, where a division that is not correctly rounded shows.  n - 1 of them (all 768 from n = 769 on), and M itself LAST: a
    maximum that drops the tail of the frame shows too."""
    M = np.float32(M)
    t = (np.float64(M) * np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)
    with np.errstate(over="ignore"):  # (the float after FLT_MAX is +inf: clipped to M)
        steps = np.stack([np.nextafter(t, -INF), t, np.nextafter(t, INF)], axis=1).reshape(-1)
    steps = np.clip(steps, np.float32(0.0), M)
    return np.concatenate([steps[(np.arange(n - 1) * 7) % 768], [M]]).astype(np.float32)


def display_frames(n):
    """name -> (frame [n] float32, M: what peak_given's values are built from)."""
    assert not V.host_flushes()
    rng = np.random.default_rng(n)
    base = rng.uniform(0.0, 1.0, n).astype(np.float32)
    frames = {f"stairs_{k}": (staircase(M, n), M) for k, M in PEAKS.items()}
    frames["dim_row"] = (np.resize(dim_row(), n), np.float32(68 * 2.0 ** -149))
    x = base.copy()
    x[rng.integers(0, n, max(1, n // 50))] = INF
    frames["inf_among_finite"] = (x, np.float32(1.0))
    frames["all_inf"] = (np.full(n, INF), INF)
    x = base.copy()
    put_bits(x, slice(0, None, 5), NAN_BITS[0])
    put_bits(x, slice(2, None, 7), NAN_BITS[1])
    frames["nans"] = (x, np.float32(1.0))
    frames["minus_zero"] = (np.full(n, -0.0, np.float32), np.float32(1.0))
    x = base.copy()
    x[::3] = -x[::3] - np.float32(0.5)
    frames["negatives"] = (x, np.float32(1.0))
    frames["zero"] = (np.zeros(n, np.float32), np.float32(1.0))
    return {k: (np.ascontiguousarray(f, np.float32), M) for k, (f, M) in frames.items()}


def given_peaks(M):
    """What peak_given is handed: above and below the frame's peak, and what no maximum would give."""
    with np.errstate(over="ignore"):
        return [np.float32(2.0) * M, M / np.float32(2.0), np.float32(0.0), INF, np.float32(np.nan), np.float32(-1.0)]


def restated_max(frame):
    """The running maximum starts at +0 and is replaced only where p > m: the largest value above 0, or +0 (never a NaN, -0.0 or
    a negative value)."""
    above = frame[frame > np.float32(0.0)]
    return above.max() if above.size else np.float32(0.0)


def restated_levels(frame, m):
    """level = float64(float32(p / m)) * 255; NaN or negative -> 0; above 255 -> 255; truncated."""
    with np.errstate(all="ignore"):
        q = np.asarray(frame, np.float32) / np.float32(m)
        assert q.dtype == np.float32
        level = q.astype(np.float64) * 255.0
        level = np.where(~(level >= 0.0), 0.0, np.where(level > 255.0, 255.0, level))
    return level.astype(np.uint8)


@pytest.mark.parametrize("n", DISPLAY_N)
def test_display_equals_the_restatement(pkg, n):
    assert not V.host_flushes()
    for name, (frame, _) in display_frames(n).items():
        m = restated_max(frame)
        want = restated_levels(frame, m)
        got = pkg.heatmap_u8(frame)
        assert np.array_equal(got, want), (n, name, np.flatnonzero(got != want)[:4], got[got != want][:4], want[got != want][:4])
        if name.startswith("stairs"):
            assert V.same_bits(m, frame[-1]) and want[-1] == 255
            if n >= 769:  # every level is there, and both sides of every step (64 units of 2^-149 have 65 levels to give)
                assert np.array_equal(np.unique(want), np.arange(256)) or (name == "stairs_sub64" and np.unique(want).size == 65)
    # what the other frames are there for
    frames = {k: f for k, (f, _) in display_frames(n).items()}
    assert not pkg.heatmap_u8(frames["all_inf"]).any()            # inf / inf
    assert not pkg.heatmap_u8(frames["minus_zero"]).any() and not pkg.heatmap_u8(frames["zero"]).any()
    got = pkg.heatmap_u8(frames["inf_among_finite"])
    assert not got.any()                                           # finite / inf = 0, inf / inf = NaN -> 0
    got = pkg.heatmap_u8(frames["nans"])
    assert not got[np.isnan(frames["nans"])].any() and (got.max() == 255 or n < 4)
    got = pkg.heatmap_u8(frames["negatives"])
    assert not got[frames["negatives"] < 0].any() and (got.max() == 255 or n < 2)
    if n >= 960:
        got = pkg.heatmap_u8(frames["dim_row"])
        assert got.max() == 255 and got.min() >= int(255 * 16 / 68)  # subnormal over subnormal: an ordinary image


# ------------------------------------------------------------------------------------------------ find

FIND_GRIDS = [(5, 3), (33, 17), (64, 64)]
FIND_RADII = [1, 2, 8]
FIND_RATIOS = [0.0, 0.25, 1.0]
FIND_SOURCES = [4, 32]
SUB_MIN_POWER = float(np.float32(40 * 2.0 ** -149))  # a subnormal floor, for the plateaus


def find_contents(rows, cols):
    """name -> (frame [rows * cols] float32, min_power)."""
    rng = np.random.default_rng(rows * 1000 + cols)
    n = rows * cols
    r, c = np.divmod(np.arange(n), cols)
    base = rng.uniform(1e-3, 1.0, n).astype(np.float32)
    out = {}
    # plateaus of 2 x 3 equal pixels, whole units 16 .. 68 of 2^-149: ties everywhere, and min_ratio * m rounds on the subnormal grid
    steps = rng.integers(16, 69, size=((rows + 1) // 2, (cols + 2) // 3))
    out["sub_plateaus"] = ((steps[r // 2, c // 3] * V.UNIT).astype(np.float32), SUB_MIN_POWER)
    x = (rng.uniform(0.0, 1.0, n) * float(FLT_MAX)).astype(np.float32)
    x[n // 2] = INF
    out["huge_one_inf"] = (x, 0.0)
    x = base.copy()
    x[sorted({0, 1, n // 2, n // 2 + 1, n // 2 + cols if n // 2 + cols < n else n - 1, n - 1})] = INF  # ties: the lower index wins
    out["several_inf"] = (x, 0.0)
    out["all_inf"] = (np.full(n, INF), 0.0)
    x = base.copy()
    put_bits(x, n // 3, NAN_BITS[0])
    put_bits(x, 2 * n // 3, NAN_BITS[1])
    out["nans"] = (x, 0.0)
    x = base.copy()
    x[n // 4] = -0.0
    x[n // 2] = -3.0
    x[3 * n // 4] = np.float32(-1e-40)
    out["negatives"] = (x, 0.0)
    return {k: (np.ascontiguousarray(f, np.float32), p) for k, (f, p) in out.items()}


def find_edge_cases():
    for rows, cols in FIND_GRIDS:
        for name, (frame, min_power) in find_contents(rows, cols).items():
            for radius in FIND_RADII:
                for min_ratio in FIND_RATIOS:
                    for max_sources in FIND_SOURCES:
                        yield rows, cols, name, frame, dict(radius=radius, max_sources=max_sources, min_power=min_power, min_ratio=min_ratio)


def test_find_equals_the_rule_on_every_bit_pattern(pkg):
    assert not V.host_flushes()
    cases, found = 0, 0
    for rows, cols, name, frame, kw in find_edge_cases():
        got = pkg.find_peaks(frame, rows, cols, **kw)
        want, want_count = restated(frame, rows, cols, kw["radius"], kw["max_sources"], kw["min_power"], kw["min_ratio"], 180.0)
        assert_same(got.sources[0], got.count[0], want, want_count, (rows, cols, name, kw))
        src = got.sources[0][: got.count[0]]
        assert np.isfinite(src["row"]).all() and np.isfinite(src["theta"]).all() and (src["power"] > 0).all()
        near = np.zeros((rows, cols), bool)  # within `radius` of a NaN: never a peak
        for i in np.flatnonzero(np.isnan(frame)):
            near[max(i // cols - kw["radius"], 0): i // cols + kw["radius"] + 1, max(i % cols - kw["radius"], 0): i % cols + kw["radius"] + 1] = True
        assert not near.reshape(-1)[src["pixel"]].any(), (rows, cols, name, kw)
        if name == "all_inf":  # one source, pixel 0, at EVERY ratio: 0 * inf is no threshold
            assert got.count[0] == 1 and src["pixel"][0] == 0 and np.isposinf(src["power"][0]), (rows, cols, kw)
        if name == "several_inf":
            assert got.count[0] >= 1 and src["pixel"][0] == 0 and np.isposinf(src["power"][0]), (rows, cols, kw)
            assert not (src["pixel"] == 1).any()  # pixel 1 ties with pixel 0 and loses
        if name == "nans" and kw["min_ratio"] > 0:
            assert got.count[0] == 0, (rows, cols, kw)  # m is the NaN
        if name == "sub_plateaus":
            assert (src["power"] >= np.float32(SUB_MIN_POWER)).all() and V.subnormal(src["power"]).all()
        cases += 1
        found += int(got.count[0])
    assert cases == 3 * 6 * 3 * 3 * 2 and found > 300, (cases, found)


def test_no_ratio_threshold_is_no_threshold(pkg):
    """The defect: min_ratio = 0 on a frame holding +inf gave min_ratio * m = NaN and no source at all.  It gives what 0.25
    gives on a constant +inf frame, and no fewer sources than 0.25 gives on any frame."""
    for rows, cols in FIND_GRIDS:
        frames = find_contents(rows, cols)
        none = pkg.find_peaks(frames["all_inf"][0], rows, cols, radius=2, max_sources=4, min_ratio=0.0)
        quarter = pkg.find_peaks(frames["all_inf"][0], rows, cols, radius=2, max_sources=4, min_ratio=0.25)
        assert none.count[0] == 1 and none.sources.tobytes() == quarter.sources.tobytes()
        for name, (frame, min_power) in frames.items():
            none = pkg.find_peaks(frame, rows, cols, radius=2, max_sources=32, min_power=min_power, min_ratio=0.0)
            quarter = pkg.find_peaks(frame, rows, cols, radius=2, max_sources=32, min_power=min_power, min_ratio=0.25)
            assert none.count[0] >= quarter.count[0], (rows, cols, name)
        assert pkg.find_peaks(frames["nans"][0], rows, cols, radius=1, max_sources=32, min_ratio=0.0).count[0] >= 1 or rows * cols < 64


def test_mixed_batch_equals_its_frames(pkg):
    for rows, cols in FIND_GRIDS:
        frames = np.stack([f for f, _ in find_contents(rows, cols).values()])
        for min_ratio in FIND_RATIOS:
            whole = pkg.find_peaks(frames, rows, cols, radius=2, max_sources=4, min_ratio=min_ratio)
            for k, frame in enumerate(frames):
                one = pkg.find_peaks(frame, rows, cols, radius=2, max_sources=4, min_ratio=min_ratio)
                assert whole.sources[k].tobytes() == one.sources[0].tobytes() and whole.count[k] == one.count[0], (rows, cols, k)


# ------------------------------------------------------------------------------------------------ calibration

NAN_ROWS = (0, 5, 31, 40, 63)


def calibration_frames():
    """name -> X [64, 1024]: util.hash_frames(64, 1024, seed=21, scale=2^-7) with a few samples or rows replaced."""
    assert not V.host_flushes()
    base = util.hash_frames(64, 1024, seed=21, scale=2.0 ** -7)[0]
    out = {"base": base.copy()}
    for row in NAN_ROWS:
        out[f"nan_row_{row}"] = base.copy()
        out[f"nan_row_{row}"][row, 100 + row] = np.nan
    out["inf_sample"] = base.copy()
    out["inf_sample"][9, 500] = INF
    out["square_overflows"] = base.copy()
    out["square_overflows"][9, 500] = np.float32(3e38)
    out["nan_in_33_rows"] = base.copy()
    out["nan_in_33_rows"][:33, 7] = np.nan
    out["subnormal_row"] = base.copy()
    out["subnormal_row"][12] = V.scale_pow2(base[12], -119)
    out["silence"] = V.scale_pow2(base, -119)  # the sub tier of value_edges.py: 2^-120 times the 2^-6 frames
    return out


def restated_calibration(X, reference_power_level=1e-5):
    """-> (index, correction, median, mean squares): the mean square in float, multiply then add in sample order, one division; the
    sort with NaN last (numpy's own order: finite ascending, +inf, NaN); the median of elements 32 and 33, a float addition
    halved in double and rounded; usable = mean square finite, median finite, |power - median| <= 1e-4 and power >= median * 1e-3,
    both against double bounds."""
    X = np.asarray(X, np.float32)
    with np.errstate(all="ignore"):
        acc = np.zeros(64, np.float32)
        for i in range(X.shape[1]):
            acc = acc + X[:, i] * X[:, i]
        power = acc / np.float32(X.shape[1])
        assert power.dtype == np.float32
        s = np.sort(power)
        median = np.float32(np.float64(s[32] + s[33]) / 2.0)
        far_off = np.abs(power - median).astype(np.float64) > 1e-4
        dead = power.astype(np.float64) < np.float64(median) * 1e-3
        usable = np.isfinite(power) & np.isfinite(median) & ~far_off & ~dead
        index = np.flatnonzero(usable).astype(np.int32)
        correction = np.float32(reference_power_level) / power[index]
    return index, correction.astype(np.float32), median, power


def same_calibration(got, want):
    """index equal; correction and median the same bits."""
    return (np.array_equal(got[0], want[0]) and V.same_bits(got[1], want[1]) and
            V.same_bits(np.float32(got[2]), np.float32(want[2])))


def test_calibration_with_values_that_are_not_finite(oracle):
    frames = calibration_frames()
    for name, X in frames.items():
        got = oracle.calibrate(X)
        want = restated_calibration(X)
        assert same_calibration(got, want[:3]), (name, got[0].size, want[0].size, got[2], want[2])
    base = oracle.calibrate(frames["base"])
    assert base[0].size == 64 and np.isfinite(base[2])
    # the defect: the NaN's place in the list decided the median, and the NaN stream was usable
    for row in NAN_ROWS:
        index, corr, median = oracle.calibrate(frames[f"nan_row_{row}"])
        assert np.array_equal(index, np.delete(np.arange(64), row)) and np.isfinite(corr).all() and np.isfinite(median), row
        _, _, _, power = restated_calibration(frames[f"nan_row_{row}"])
        finite = np.sort(power[np.isfinite(power)])  # 63 of them: elements 32 and 33 of [63 finite ascending, NaN]
        assert V.same_bits(np.float32(median), np.float32(np.float64(finite[32] + finite[33]) / 2.0)), row
    # ... whichever place it has: the SAME 63 finite rows and the NaN row, the NaN row standing at each of the five places, give one
    # median.  (A NaN sample put into row r of the base frame takes row r's mean square out of the list: which two of the other 63
    # are elements 32 and 33 then depends on whether that mean square was below or above them -- two medians, both right, above.)
    medians = []
    for row in NAN_ROWS:
        X = frames["nan_row_0"].copy()
        X[[0, row]] = X[[row, 0]]
        index, corr, median = oracle.calibrate(X)
        medians.append(np.float32(median))
        assert np.array_equal(index, np.delete(np.arange(64), row)), row
        assert same_calibration((index, corr, median), restated_calibration(X)[:3]), row
    assert len({m.view(np.uint32).item() for m in medians}) == 1 and np.isfinite(medians[0]), medians
    for name in ("inf_sample", "square_overflows"):
        index, corr, median = oracle.calibrate(frames[name])
        assert 9 not in index and index.size == 63 and np.isfinite(median), name
        assert np.isposinf(restated_calibration(frames[name])[3][9])
    index, corr, median = oracle.calibrate(frames["nan_in_33_rows"])
    assert index.size == 0 and np.isnan(median)       # elements 32 and 33 are NaN: no finite median, nothing usable
    index, corr, median = oracle.calibrate(frames["subnormal_row"])
    row = frames["subnormal_row"][12]
    assert (V.subnormal(row) | (row == 0)).all() and V.subnormal(row).sum() > 1000
    assert restated_calibration(frames["subnormal_row"])[3][12] == 0 and 12 not in index and index.size == 63  # dead
    # silence: every mean square 0, the median 0, nobody far off or dead: the reference's own answer, 64 usable mics and +inf gains
    index, corr, median = oracle.calibrate(frames["silence"])
    assert (V.subnormal(frames["silence"]) | (frames["silence"] == 0)).all()
    assert index.size == 64 and median == 0.0 and np.isposinf(corr).all()
