"""Child process of test_gpu_value_edges.py (the library reads AWPU_SHAPE once per process): one engine, every value tier of
value_edges.py through it, compared here with the IEEE restatement; prints the kernels the handle reported.

    python gpu_value_edges_check.py '<json cfg>'
    cfg: case (value_edges.CASES), math exact | fast, interp lerp | fir8, checks: a list of tiers | packed | isolation | gains

Never loads oracle/_ref (that library's start-up code would switch this thread to flush-to-zero), and says so at both ends."""
import importlib
import json
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))
import util  # noqa: E402
import value_edges as V  # noqa: E402
from oracle import oracle_py  # noqa: E402

pkg = importlib.import_module("beamforming-lk_amd")
B = pkg.binding


class Sweeper:
    """The engine and its device buffers; every result lands in buffers prefilled with NaN."""

    def __init__(self, case, math, interp, max_batch):
        self.case, self.exact = case, math == "exact"
        n, P = case.x0.shape[1], case.n_pixels
        self.fir = util.synthetic_fir_table() if interp == "fir8" else None
        self.eng = pkg.Engine(n_pixels=P, n_streams=n, lut_stride=n, hist=case.x0.shape[2], math=pkg.MATH_F32_EXACT if self.exact else pkg.MATH_F32_FAST,
                              interp=B.INTERP_FIR8 if interp == "fir8" else B.INTERP_LERP, max_batch=max_batch, grid_columns=case.cols)
        self.eng.set_delay_table(case.off, case.frac)
        self.eng.set_active_mics(None if case.index.size == n else case.index)
        if self.fir is not None:
            self.eng.set_fir_table(self.fir)
        self.kernels = set()
        self.sums_ok = self.exact  # (exact_verify exports none: learnt at the first sweep)

    def sweep(self, frames, packed=False):
        """frames [b, n, hist] -> (power [b, P], sums [b, P, 256] or None)"""
        b, P = frames.shape[0], self.case.n_pixels
        d_x = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
        d_p = torch.full((b, P), float("nan"), dtype=torch.float32, device="cuda")
        d_s = None
        torch.cuda.synchronize()
        if packed:
            d_k = torch.full((self.eng.packed_bytes(b) // 4,), float("nan"), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            self.eng.pack_frames(d_x.data_ptr(), b, d_k.data_ptr())
            self.eng.process_packed(d_k.data_ptr(), b, d_p.data_ptr())
        elif self.sums_ok:
            d_s = torch.full((b, P, 256), float("nan"), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            try:
                self.eng.process_device_sums(d_x.data_ptr(), b, d_p.data_ptr(), d_s.data_ptr())
            except pkg.AwpuError as e:  # the round-1 verification kernel exports no sums: its powers are checked
                assert e.status == B.ERR_STATE and expect_no_sums, e
                self.sums_ok, d_s = False, None
                self.eng.process_device(d_x.data_ptr(), b, d_p.data_ptr())
        else:
            self.eng.process_device(d_x.data_ptr(), b, d_p.data_ptr())
        self.eng.synchronize()
        self.kernels.add(B.KERNEL_NAMES[self.eng.stats().kernel_variant])
        return d_p.cpu().numpy(), None if d_s is None else d_s.cpu().numpy()

    def oracle(self, frame):
        return V.oracle_sums(oracle_py, self.case, frame, self.fir)


def check_tier(sw, tier, own, packed=False):
    """One tier through the engine.  `own`: the engine's own powers of X0 (None while this IS X0).  -> the powers"""
    case, px = sw.case, sw.case.pixels
    frames = case.tier(tier)
    power, sums = sw.sweep(frames)
    assert not np.isnan(power).any() or tier == "nonfinite", (tier, "a power was not written, or is NaN")
    if packed:  # the same frames through the packed-exchange entry points: the same bits
        q, _ = sw.sweep(frames, packed=True)
        assert V.same_nonfinite(q, power), (tier, "packed frames: other powers")
    if tier in ("small", "big", "top"):
        k = V.SCALED[tier]
        if tier != "top":  # exact power-of-two scale invariance of the kernel itself
            assert V.same_bits(power, V.ldexp32(own, 2 * k)), (tier, "powers are not 2^2k times the kernel's own powers of X0")
        else:
            assert np.isposinf(power).all(), (tier, "a power is not +inf", power[~np.isposinf(power)][:4])
    if tier in ("under", "sub"):
        assert V.same_bits(power, np.zeros_like(power)), (tier, "a power is not exactly 0", power[power != 0][:4])
    if tier in V.EPILOGUE:
        assert (power != 0).all(), (tier, "a power is 0", int((power == 0).sum()))
    if not sw.exact:  # (this mode's parity with the oracle at X0 is the other tests' subject; its claims here are the ones above)
        if tier in V.EPILOGUE:  # the sums scale exactly: only the roundings onto the subnormal grid differ
            off_by = np.abs(V.units(power) - V.units(V.ldexp32(own, 2 * V.SCALED[tier])))
            print(f"  {tier}: worst |power - 2^2k own| = {off_by.max():g} units of 2^-149, {int((off_by != 0).sum())} of {power.size} not bit-equal")
            assert off_by.max() <= 1.0, (tier, "powers further than one unit of 2^-149 from 2^2k times the kernel's own powers of X0", off_by.max())
        return power
    worst, unequal, compared = 0.0, 0, 0
    for b in range(case.batch):
        p_want, s_want = sw.oracle(frames[b])
        if sums is not None:
            got = sums[b][px]
            if tier == "nonfinite":
                assert V.same_nonfinite(got, s_want), (tier, b, "sums")
            else:
                assert V.same_bits(got, s_want), (tier, b, "sums", np.argwhere(V.bits(got) != V.bits(s_want))[:4].tolist())
        got = power[b][px]
        fin = np.isfinite(p_want)
        assert not np.isfinite(got[~fin]).any(), (tier, b, "a power is finite where the oracle's is not")
        assert np.array_equal(np.isposinf(got), np.isposinf(p_want)), (tier, b, "+inf powers elsewhere than the oracle's")
        if tier == "dim":
            # derived, not measured: MA is exact or one rounding of identical inputs and every addition is exact (whole units below
            # 2^24), so only the square's and the division's roundings can differ: one unit of 2^-149
            off_by = np.abs(V.units(got) - V.units(p_want))
            unequal, compared = unequal + int((off_by != 0).sum()), compared + got.size
            assert off_by.max() <= 1.0, (tier, b, "a power further than one unit of 2^-149 from the oracle's", off_by.max())
        elif fin.any():
            err = util.power_rel_err_unfloored(got[fin], p_want[fin])  # (a zero of the oracle must be exactly 0)
            worst = max(worst, err)
            assert err <= util.POWER_RTOL, (tier, b, err)
    if tier == "dim":
        print(f"  dim: {unequal} of {compared} powers not bit-equal to the oracle's")
    if tier == "dusk":
        print(f"  dusk: worst |power - oracle| / oracle = {worst:.3g}")
    return power


def check_isolation(sw):
    """Batch 4 with frame 1 replaced by a bad frame: the other frames are the clean batch's bits; then the clean batch again."""
    case = sw.case
    n, hist = case.x0.shape[1:]
    x4 = util.hash_frames(n, hist, seed=V.CASES[case.name][5], batch=4)
    assert np.array_equal(x4[:case.batch], case.x0)
    clean_p, clean_s = sw.sweep(x4)
    for what, frame in (("nonfinite", case.with_bad_samples(x4[1])), ("top", V.scale_pow2(x4[1], V.SCALED["top"]))):
        xa = x4.copy()
        xa[1] = frame
        p, s = sw.sweep(xa)
        assert not V.same_nonfinite(p[1], clean_p[1]), (what, "the bad frame changed nothing")
        for b in (0, 2, 3):
            assert V.same_bits(p[b], clean_p[b]), (what, b, "a bad frame leaked into another frame's powers")
            assert s is None or V.same_bits(s[b], clean_s[b]), (what, b, "a bad frame leaked into another frame's sums")
        p, s = sw.sweep(x4)  # nothing stale in tables, packed rows or LDS images
        assert V.same_bits(p, clean_p) and (s is None or V.same_bits(s, clean_s)), (what, "the clean batch after a bad one: other bits")


def check_gains(sw):
    """A gain of 2^-40 on X0 is the small tier; per-mic gains 2^-100 (1, 2, 4, 8, 1, ...) are the frames prescaled in float32."""
    case, px = sw.case, sw.case.pixels
    n = case.x0.shape[1]
    try:
        sw.eng.set_mic_gains(np.full(n, 2.0 ** -40, np.float32))
        _, sums = sw.sweep(case.x0)
        for b in range(case.batch):
            assert V.same_bits(sums[b][px], sw.oracle(case.tier("small")[b])[1]), ("gain 2^-40", b)
        gains = (np.float32(2.0 ** -100) * np.float32(2.0) ** (np.arange(n) % 4)).astype(np.float32)
        sw.eng.set_mic_gains(gains)
        power, sums = sw.sweep(case.x0)
        with np.errstate(under="ignore"):
            scaled = case.x0 * gains[None, :, None]
        assert scaled.dtype == np.float32 and not V.host_flushes()
        for b in range(case.batch):
            assert V.same_bits(sums[b][px], sw.oracle(scaled[b])[1]), ("per-mic gains", b)
        assert V.same_bits(power, np.zeros_like(power))
    finally:
        sw.eng.set_mic_gains(None)
    p, s = sw.sweep(case.x0)
    for b in range(case.batch):
        assert V.same_bits(s[b][px], sw.oracle(case.x0[b])[1]), ("gains off again", b)


def check_beams():
    """awpu_hip_beams on the dusk, dim, under and sub tiers with the golden beams_c1 table: the beams bit for bit; the powers within
    the flat 1e-5 at dusk, within one unit of 2^-149 and none 0 at dim, exactly 0 at under and sub."""
    g = np.load(REPO / "tests" / "golden" / "beams_c1.npz")
    x0 = util.hash_frames(64, 1024, seed=int(g["seed"]))[0]
    with pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=16) as eng:
        eng.set_active_mics(g["index"])
        for tier in ("dusk", "dim", "under", "sub"):
            x = V.scale_pow2(x0, V.BEAMS_SCALED[tier] if tier in V.EPILOGUE else V.SCALED[tier])
            d_x = torch.from_numpy(x).cuda()
            torch.cuda.synchronize()
            power, beams = eng.beams(g["off"], g["frac"], d_x.data_ptr())
            p_want, b_want = oracle_py.particle_beams(x, g["off"], g["frac"], g["index"])
            assert V.subnormal(b_want).any() or tier != "sub"
            assert V.same_bits(beams, b_want), (tier, "beams", int((V.bits(beams) != V.bits(b_want)).sum()))
            if tier in V.EPILOGUE:
                assert V.subnormal(p_want).all() and (power != 0).all(), (tier, "a power is 0")
                off_by = np.abs(V.units(power) - V.units(p_want))
                err = util.power_rel_err_unfloored(power, p_want)
                print(f"  beams {tier}: worst |power - oracle| = {off_by.max():g} units of 2^-149, {err:.3g} relative; "
                      f"{int((off_by != 0).sum())} of {power.size} powers not bit-equal", flush=True)
                if tier == "dim":  # (derived: check_tier)
                    assert off_by.max() <= 1.0, (tier, "powers", off_by.max())
                else:
                    assert err <= util.POWER_RTOL, (tier, "powers", err)
            else:
                assert V.same_bits(power, np.zeros_like(power)) and V.same_bits(p_want, np.zeros_like(p_want)), (tier, "powers")


cfg = json.loads(sys.argv[1])
expect_no_sums = cfg.get("no_sums", False)
assert oracle_py.fp_flush_bits() == 0 and not V.host_flushes(), "the host flushes subnormals"
if cfg["checks"] == ["beams"]:
    check_beams()
    kernels = {"beams"}
else:
    case = V.make_case(cfg["case"], oracle_py, B.build_delay_table)
    sw = Sweeper(case, cfg["math"], cfg["interp"], max_batch=4 if "isolation" in cfg["checks"] else case.batch)
    own = None
    for what in cfg["checks"]:
        if what == "isolation":
            check_isolation(sw)
        elif what == "gains":
            check_gains(sw)
        else:
            power = check_tier(sw, what, own, packed=cfg.get("packed", False))
            own = power if what == "x0" else own
        print("  ok", what, flush=True)
    assert sw.sums_ok == (sw.exact and not expect_no_sums)
    sw.eng.close()
    kernels = sw.kernels
assert oracle_py.fp_flush_bits() == 0 and not V.host_flushes(), "the host flushes subnormals (who switched that on?)"
assert not oracle_py._refs, "this process loaded oracle/_ref"
print("CHILD OK", ",".join(sorted(kernels)))
