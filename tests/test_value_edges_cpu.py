"""(no device) The value tiers of value_edges.py are what their table says, on the very cases the GPU tests sweep, by the IEEE
restatement alone -- and that restatement's bits do not depend on who else is loaded into the process: oracle/_ref is linked with
-Ofast, and loading it used to switch the loading thread to flush-to-zero / denormals-are-zero."""
import functools
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import util
import value_edges as V

REPO = Path(__file__).resolve().parent.parent


@functools.lru_cache(maxsize=None)
def case_of(name):
    from oracle import oracle_py

    return V.make_case(name, oracle_py)


@functools.lru_cache(maxsize=None)
def swept(name, tier, interp="lerp"):
    """(power, sums) of frame 0 of a tier; computed once, left unchanged."""
    from oracle import oracle_py

    fir = util.synthetic_fir_table() if interp == "fir8" else None
    power, sums = V.oracle_sums(oracle_py, case_of(name), case_of(name).tier(tier)[0], fir)
    power.setflags(write=False)
    sums.setflags(write=False)
    return power, sums


subnormal = V.subnormal


def epilogue_tier_conditions(tier, power, sums, divisor):
    """What value_edges.py says of the dusk and dim tiers, on one oracle result; -> figures to print."""
    assert not subnormal(sums).any(), (tier, "a pre-epilogue sum that is not zero is subnormal")
    assert (subnormal(power)).all(), (tier, "an oracle power is zero or normal", V.units(power).min(), V.units(power).max())
    assert V.same_bits(V.epilogue32(sums, divisor, "forward"), power), (tier, "the numpy restatement is not the oracle's epilogue")
    worst = 0.0
    for order in ("reversed", "pairwise"):
        again = V.epilogue32(sums, divisor, order)
        if tier == "dim":  # the sum of squares is a whole number of units below 2^24: exact in any order
            assert V.same_bits(again, power), (tier, order, int((V.bits(again) != V.bits(power)).sum()))
        else:
            worst = max(worst, util.power_rel_err_unfloored(again, power))
            assert worst <= util.POWER_RTOL, (tier, order, worst)
    if tier == "dim":
        assert V.units(power).max() * divisor < 2 ** 24, (tier, "the sum of squares may round")
    return dict(units_min=float(V.units(power).min()), units_max=float(V.units(power).max()), reordered_rel=worst)


# every (case, interpolation) the GPU cases of test_gpu_value_edges.py sweep
SWEPT = [(name, "lerp") for name in V.CASES] + [("grid37", "fir8")]


@pytest.mark.parametrize("name,interp", SWEPT)
def test_the_epilogue_tiers_are_what_they_claim(oracle, name, interp):
    """dusk and dim: sums normal, every oracle power subnormal and not 0; the epilogue restated in float32 numpy on the oracle's
    sums, with the squares added in reversed and in pairwise order, stays within the flat 1e-5 at dusk and is the oracle's bits
    at dim, where the sum of squares is a whole number of 2^-149 below 2^24."""
    assert not V.host_flushes()
    case = case_of(name)
    p0, _ = swept(name, "x0", interp)
    for tier in V.EPILOGUE:
        power, sums = swept(name, tier, interp)
        seen = epilogue_tier_conditions(tier, power, sums, 256 * len(case.index))
        print(name, interp, tier, seen)
        # the powers are the scaled ones rounded onto the subnormal grid, give or take the roundings below it
        assert np.abs(V.units(power) - V.units(V.ldexp32(p0, 2 * V.SCALED[tier]))).max() <= 1.0, tier


def test_the_epilogue_tiers_on_the_golden_beams(oracle):
    """The same conditions for awpu_hip_beams' table (tests/golden/beams_c1.npz): its powers are divided by 256 alone."""
    assert not V.host_flushes()
    g = np.load(REPO / "tests" / "golden" / "beams_c1.npz")
    x0 = util.hash_frames(64, 1024, seed=int(g["seed"]))[0]
    for tier in V.EPILOGUE:
        power, beams = oracle.particle_beams(V.scale_pow2(x0, V.BEAMS_SCALED[tier]), g["off"], g["frac"], g["index"])
        seen = epilogue_tier_conditions(tier, power, beams, 256)
        print("beams_c1", tier, V.BEAMS_SCALED[tier], seen)
    # why the table's dusk is not the sweeps': at their k its powers are normal
    power, _ = oracle.particle_beams(V.scale_pow2(x0, V.SCALED["dusk"]), g["off"], g["frac"], g["index"])
    assert not subnormal(power).any()


@pytest.mark.parametrize("name", list(V.CASES))
def test_the_tiers_are_what_they_claim(oracle, name):
    assert not V.host_flushes()
    case = case_of(name)
    p0, s0 = swept(name, "x0")
    assert np.isfinite(s0).all() and (p0 > 0).all() and not subnormal(s0).any()
    # small, big: everything normal, so a power of two goes through every operation untouched
    for tier in ("small", "big"):
        k = V.SCALED[tier]
        p, s = swept(name, tier)
        assert V.same_bits(s, V.ldexp32(s0, k)) and V.same_bits(p, V.ldexp32(p0, 2 * k)), tier
        assert not subnormal(s).any() and not subnormal(p).any() and np.isfinite(p).all() and (p > 0).all(), tier
    # top: the sums still scale exactly; every square overflows
    p, s = swept(name, "top")
    assert np.isfinite(s).all() and V.same_bits(s, V.ldexp32(s0, V.SCALED["top"]))
    assert np.isposinf(p).all()
    # under: normal samples, subnormal differences and products
    x = case.tier("under")
    assert not subnormal(x).any(), "a sample of the under tier is subnormal: another seed"
    p, s = swept(name, "under")
    assert V.same_bits(p, np.zeros_like(p))
    if oracle.ref_available():  # the reference's build runs flushing (ref_mimo_driver.cpp): other sums
        _, s_ftz = oracle.das_f32(x[0], case.off[case.pixels], case.frac[case.pixels], index=case.index, want_out=True, impl="ref")
        assert not V.same_bits(s, s_ftz)
    # sub: subnormal samples, subnormal sums, nothing lost
    x = case.tier("sub")
    assert (subnormal(x) | (x == 0)).all() and np.array_equal(x == 0, case.x0 == 0)
    p, s = swept(name, "sub")
    assert subnormal(s).mean() >= 0.10 and not (s == 0).any()
    assert V.same_bits(p, np.zeros_like(p))
    # zeros: a frame of -0.0 sums to +0.0 everywhere (-0 - -0 = +0; fma(f, +0, -0) = +0); a mic whose row is -0.0 adds +0.0 to
    # every sum: the sums of the list without it
    p, s = swept(name, "zeros")
    assert V.same_bits(s, np.zeros_like(s)) and V.same_bits(p, np.zeros_like(p))
    _, s = V.oracle_sums(oracle, case, case.tier("zero_row")[0])
    less = V.Case(case.name, case.xyz, case.rows, case.cols, case.off, case.frac, np.delete(case.index, 1), case.x0, case.pixels)
    _, want = V.oracle_sums(oracle, less, case.x0[0])
    assert V.same_bits(s, want)
    # nonfinite: some pixels' windows reach a bad sample, others' do not; each kind of bad sample does what it is there for
    p, s = swept(name, "nonfinite")
    bad_px = ~np.isfinite(p)
    assert bad_px.mean() >= 0.25 and (~bad_px).mean() >= 0.25, bad_px.mean()
    assert bad_px[~np.isfinite(s).all(axis=1)].all()  # (a finite sum near 3e38 squares to +inf as well)
    assert V.same_bits(s[~bad_px], s0[~bad_px]) and V.same_bits(p[~bad_px], p0[~bad_px])
    assert np.isposinf(s).any() and np.isnan(s).any()
    off, frac = case.off[case.pixels], case.frac[case.pixels]
    m, t = case.bad["frac0"]
    hit = np.flatnonzero((frac[:, m] == 0.0) & (off[:, m] + 255 == t))
    assert hit.size and np.isnan(s[hit, 255]).all()  # fma(0, inf, next): NaN, where the reference "should" have read `next`
    m, t = case.bad["overflow"]
    hit = np.flatnonzero((off[:, m] <= t) & (t + 1 <= off[:, m] + 256))
    assert hit.size and all(np.isinf(s[q, t - off[q, m]]) or np.isnan(s[q, t - off[q, m]]) for q in hit)  # 3e38 - (-3e38)


CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import value_edges as V
from oracle import oracle_py
assert oracle_py.fp_flush_bits() == 0 and not V.host_flushes(), "a fresh process flushes subnormals"
case = V.make_case("grid37", oracle_py)
before = {t: V.oracle_sums(oracle_py, case, case.tier(t)[0])[1] for t in ("under", "sub")}
oracle_py.ref("avx2")
oracle_py.ref("fir")
print("flush bits after loading oracle/_ref:", oracle_py.fp_flush_bits())
print("float32(1e-30) * float32(1e-10) =", np.float32(1e-30) * np.float32(1e-10))
for t in ("under", "sub"):
    after = V.oracle_sums(oracle_py, case, case.tier(t)[0])[1]
    print(t, "oracle sums that changed bits:", int((V.bits(after) != V.bits(before[t])).sum()), "of", after.size)
    assert V.same_bits(after, before[t]), t
assert oracle_py.fp_flush_bits() == 0
assert np.float32(1e-30) * np.float32(1e-10) != 0
assert not V.host_flushes()
# where the build and the restatement part: the reference as built flushes what the sub tier is made of
x = case.tier("sub")[0]
_, s_ref = oracle_py.das_f32(x, case.off, case.frac, index=case.index, want_out=True, impl="ref")
assert V.same_bits(s_ref, np.zeros_like(s_ref)) and not (before["sub"] == 0).any()
assert oracle_py.fp_flush_bits() == 0 and not V.host_flushes()  # (the driver restored the caller's mode)
# ... and they are one on normal values, whoever loaded the library
_, s_ref = oracle_py.das_f32(case.x0[0], case.off, case.frac, index=case.index, want_out=True, impl="ref")
_, s_orc = oracle_py.das_f32(case.x0[0], case.off, case.frac, index=case.index, want_out=True)
assert V.same_bits(s_ref, s_orc)
print("CHILD OK")
"""


def test_loading_the_reference_build_leaves_the_host_arithmetic_alone(oracle):
    """In a child process (a fresh MXCSR: this one may have loaded oracle/_ref long ago): the oracle's sums on the under and sub
    tiers are the same bits before and after both reference builds are loaded, numpy still computes subnormals afterwards, and the
    reference's build -- which runs flushing, as the reference executable does -- gives all-zero sums on the sub tier where the
    restatement's are subnormal and none is zero."""
    if oracle._in_reference_tree("src/dsp/delay.cpp") and not (oracle.ref_available("avx2") and oracle.ref_available("fir")):
        oracle.build(ref=True)
    if not (oracle.ref_available("avx2") and oracle.ref_available("fir")):
        pytest.skip("oracle/_ref not built (reference tree absent)")
    proc = subprocess.run([sys.executable, "-c", CHILD, str(REPO)], capture_output=True, text=True, timeout=300)
    print(proc.stdout)
    assert proc.returncode == 0 and "CHILD OK" in proc.stdout, proc.stdout[-2000:] + proc.stderr[-3000:]


def test_the_oracle_clears_and_restores_the_flush_modes(oracle):
    """Every arithmetic entry point runs without FTZ / DAZ whatever the caller's mode is, and hands that mode back."""
    case = case_of("grid37")
    x = case.tier("sub")[0]
    pixels = case.pixels[:32]
    off, frac = case.off[pixels], case.frac[pixels]
    _, want = oracle.das_f32(x, off, frac, index=case.index, want_out=True)
    _, beams_want = oracle.particle_beams(x, off, frac, index=case.index)
    fir = np.zeros((101, 8), np.float32)
    fir[:, 3] = 1.0
    _, fir_want = oracle.das_fir8_f32(x, off, frac, fir, index=case.index, want_out=True)
    assert V.same_bits(beams_want, want) and subnormal(want).any() and subnormal(fir_want).any()
    mode = oracle.fp_flush_bits()
    try:
        oracle.set_fp_flush_bits(oracle.FP_FTZ | oracle.FP_DAZ)
        assert oracle.fp_flush_bits() == (oracle.FP_FTZ | oracle.FP_DAZ)
        _, got = oracle.das_f32(x, off, frac, index=case.index, want_out=True)
        _, beams = oracle.particle_beams(x, off, frac, index=case.index)
        _, fir_got = oracle.das_fir8_f32(x, off, frac, fir, index=case.index, want_out=True)
        out = np.zeros(256, np.float32)
        oracle.oracle().oracle_delay_lerp(oracle._p32(out), oracle._p32(np.ascontiguousarray(x[case.index[0], 200:457])), 0.25)
        assert oracle.fp_flush_bits() == (oracle.FP_FTZ | oracle.FP_DAZ)  # handed back
    finally:
        oracle.set_fp_flush_bits(mode)
    assert V.same_bits(got, want) and V.same_bits(beams, want) and V.same_bits(fir_got, fir_want)
    assert subnormal(out).any()
    assert not V.host_flushes()


def test_a_prebuilt_reference_build_is_run_in_the_reference_mode(oracle):
    """An oracle/_ref left by an earlier ref_mimo_driver.cpp, where it cannot be rebuilt, is called through oracle_py._InReferenceMode:
    flush-to-zero and denormals-are-zero during the call, the caller's mode afterwards (shown on the oracle's own mode reader)."""
    lib = oracle._InReferenceMode(oracle.oracle())
    assert oracle.fp_flush_bits() == 0
    assert lib.oracle_fp_flush_bits() == (oracle.FP_FTZ | oracle.FP_DAZ)
    assert oracle.fp_flush_bits() == 0 and not V.host_flushes()
    assert oracle._sets_fp_mode(oracle.ORACLE_LIB) is False
    if oracle.ref_available():
        oracle.ref("avx2")  # (rebuilt first where the reference tree is there and the library is an earlier driver's)
        assert oracle._sets_fp_mode(oracle.REF_AVX2_LIB) == (not isinstance(oracle._refs["avx2"], oracle._InReferenceMode))
