"""The cross-spectral maps (include/awpu_hip_csm.h) on the device.

1. Device spectra, C, q and all three kinds of plane equal the host rule (awpu_hip_csm_*_host) bit for bit, on the smallest shapes
   at which the kernels can go wrong: usable in {1, 2, 5 of a lut_stride of 8 (ragged, with gains), 64, 65 of 128} -- one mic, the
   map kernel's tail rows (usable not a multiple of its four rows in flight), more than one 16 x 16 tile of the accumulate kernel --,
   pixels in {1, 63, 64, 65, 130} (a wave is 64 pixels) and a slab handle, bins [0], [128], [3, 47, 128] and [0..7], both windows,
   n_blocks in {1, 3, 17} with a pitch greater than 256 n_blocks; 256 mics (144 KiB of LDS a workgroup) and 257 of 320 (32 pixels a
   workgroup); guard floats around every output stay intact; the host forms
   give the device forms' bits; a recording split over two calls gives one call's bits; EXACT and FAST handles give the same bits.
2. Value edges: subnormal and huge samples take the rule as written -- finite or infinite values bit for bit, NaN where the host
   has NaN.
3. Stream order: csm_samples_device and csm_map_device behind pending work on their stream (tests/stream_order.py).
4. The state refusals: FIR8, a band on the handle, a call during process_async, no table; bad requests; outputs left alone.
5. The scene: its Capon plane, swept on the device and passed to find_peaks_device, has its two sources.
6. Above 257 mics -- 544, 545 of 640, 1120, 1121 and 2048, where a workgroup maps 32, 16 and 8 pixels; the refusal at 2049 --:
   test_gpu_csm_large.py, with this file's Shape and helpers."""
import ctypes as C

import numpy as np
import pytest

import csm_util as CU
import stream_order as H
from test_gpu_stream_order import busy, check, scenes  # noqa: F401

pytestmark = pytest.mark.gpu

GUARD = 64
CANARY = np.float32(-3.0)
KINDS = (CU.CONVENTIONAL, CU.DIAGONAL_REMOVED, CU.CAPON)
# (bins, window, n_blocks): every bin set, both windows and every block count of the list above
SETTINGS = [([0], 0, 1), ([128], 1, 3), ([3, 47, 128], 1, 17), ([0, 1, 2, 3, 4, 5, 6, 7], 0, 3)]
BIG_SETTINGS = [([3, 47, 128], 1, 3), ([0], 0, 1)]  # ... of the two shapes with more than 64 KiB of LDS a workgroup
SLACK = 40  # floats between the last block of a stream and the next stream: pitch = 256 n_blocks + SLACK


class Shape:
    """A hand-made table -- offsets at both ends of the history, fractions 0, 1 and in between --, an active list and samples of
    `blocks` blocks.  invert=False (test_gpu_csm_large.py's lists above 512 mics, where csm_invert_host takes minutes): the Capon
    kind is given C itself in place of an inverse."""

    def __init__(self, pkg, name, n_streams, lut_stride, index, pixels, gains, seed, blocks=17, invert=True):
        rng = np.random.default_rng(seed)
        self.invert = invert
        self.pkg, self.name, self.S, self.stride, self.P = pkg, name, n_streams, lut_stride, pixels
        self.index = np.asarray(index, np.int32)
        self.U = len(self.index)
        self.off = rng.integers(0, 1024 - 256, (pixels, lut_stride)).astype(np.int32)
        self.frac = rng.random((pixels, lut_stride)).astype(np.float32)
        self.off.reshape(-1)[::7] = 0
        self.off.reshape(-1)[3::11] = 1024 - 257
        self.frac.reshape(-1)[::5] = 0.0
        self.frac.reshape(-1)[2::9] = 1.0
        self.gains = (0.5 + rng.random(n_streams)).astype(np.float32) if gains else None
        self.samples = (rng.standard_normal((n_streams, blocks * 256 + SLACK)) * 0.1).astype(np.float32)
        self._rules = {}

    def gain_list(self):
        return None if self.gains is None else self.gains[self.index]

    def engine(self, math=None, pixel_begin=0, pixel_count=0, **kw):
        pkg = self.pkg
        lo, hi = pixel_begin, pixel_begin + (pixel_count or self.P)
        eng = pkg.Engine(n_pixels=self.P, n_streams=self.S, lut_stride=self.stride, math=math, pixel_begin=pixel_begin, pixel_count=pixel_count, **kw)
        eng.set_delay_table(self.off[lo:hi], self.frac[lo:hi])
        eng.set_active_mics(self.index)
        if self.gains is not None:
            eng.set_mic_gains(self.gains)
        return eng

    def samples_of(self, n_blocks, samples=None):
        """[n_streams, 256 n_blocks + SLACK], contiguous: a pitch greater than the blocks."""
        return np.ascontiguousarray((self.samples if samples is None else samples)[:, :256 * n_blocks + SLACK])

    def rule(self, bins, window, n_blocks):
        """The host rule's answers (computed once per setting, left unchanged)."""
        key = (tuple(bins), window, n_blocks)
        if key not in self._rules:
            pkg, x = self.pkg, self.samples_of(n_blocks)
            out = {"spectra": pkg.csm_spectra_host(x, bins, window, index=self.index, gain=self.gain_list(), n_blocks=n_blocks)}
            out["C"], out["n"] = pkg.csm_accumulate_host(x, bins, window, index=self.index, gain=self.gain_list(), n_blocks=n_blocks)
            out["G"] = None if self.invert else out["C"]
            if self.invert and np.isfinite(out["C"]).all():
                try:
                    out["G"] = pkg.csm_invert_host(out["C"], out["n"], bins, loading=0.05)
                except pkg.AwpuError:
                    pass
            for kind in KINDS:
                Hm = out["G"] if kind == CU.CAPON else out["C"]
                if Hm is None or (kind == CU.DIAGONAL_REMOVED and self.U == 1):
                    continue
                out[kind] = pkg.csm_map_host(Hm, out["n"], self.off, self.frac, bins, window, kind, index=self.index, want=("map", "q"))
            for a in out.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            self._rules[key] = out
        return self._rules[key]


@pytest.fixture(scope="module")
def shapes(pkg):
    every_other = list(range(0, 128, 2)) + [127]  # 65 of 128
    made = [Shape(pkg, "one_mic", 8, 8, [3], 1, False, 1),
            Shape(pkg, "two_mics", 8, 8, [5, 2], 63, False, 2),
            Shape(pkg, "ragged5", 8, 8, [6, 1, 3, 0, 7], 65, True, 3),
            Shape(pkg, "sixty_four", 64, 64, list(range(64)), 64, False, 4),
            Shape(pkg, "sixty_five_of_128", 128, 128, every_other, 130, True, 5),
            Shape(pkg, "two_fifty_six", 256, 256, list(range(256)), 70, False, 6),
            Shape(pkg, "two_fifty_seven_of_320", 320, 320, [i for i in range(320) if i % 5 != 4] + [319], 40, True, 7)]
    return {sh.name: sh for sh in made}


def guarded(n, fill=CANARY):
    import torch

    return torch.full((n + 2 * GUARD,), float(fill), dtype=torch.float32, device="cuda")


def inner(raw, shape, what):
    host = raw.cpu().numpy()
    assert (host[:GUARD] == CANARY).all() and (host[-GUARD:] == CANARY).all(), f"{what}: guard overwritten"
    return host[GUARD:-GUARD].reshape(shape)


def device_samples(eng, x, n_blocks, bins, window, matrix=None, block_count=0, want_spectra=True, stream=0):
    """csm_samples_device of host samples -> (C, count, spectra); every buffer sits between guards, which must survive."""
    import torch

    U, K = eng._usable, len(bins)
    d_x = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_C = guarded(K * U * U * 2)
    d_C[GUARD:-GUARD] = torch.from_numpy(np.zeros(K * U * U * 2, np.float32) if matrix is None else np.ascontiguousarray(matrix).reshape(-1)).cuda()
    d_X = guarded(n_blocks * K * U * 2)
    torch.cuda.synchronize()
    count = eng.csm_samples_device(d_x.data_ptr(), x.shape[1], n_blocks, bins, d_C.data_ptr() + 4 * GUARD, window, block_count,
                                   d_X.data_ptr() + 4 * GUARD if want_spectra else 0, stream)
    eng.synchronize()
    return inner(d_C, (K, U, U, 2), "matrix"), count, inner(d_X, (n_blocks, K, U, 2), "spectra")


def device_map(eng, matrix, block_count, bins, window, kind, want=("map", "q"), stream=0):
    import torch

    K, P = len(bins), eng.pixel_count
    d_H = torch.from_numpy(np.array(matrix, np.float32)).cuda()
    raw = {name: guarded(K * P) for name in want}
    torch.cuda.synchronize()
    eng.csm_map_device(d_H.data_ptr(), block_count, bins, window, kind, stream=stream, **{f"d_{name}_ptr": raw[name].data_ptr() + 4 * GUARD for name in want})
    eng.synchronize()
    return {name: inner(raw[name], (K, P), name) for name in want}


def same_where_not_nan(got, want, where):
    """Bits wherever the host's value is finite or infinite; NaN exactly where the host has NaN."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, where
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (where, "NaN positions")
    assert np.array_equal(CU.bits(got)[~nan], CU.bits(want)[~nan]), where


# ------------------------------------------------------------------------------------------------ 1. the rule's bits

def check_against_host_rule(sh, settings):
    name = sh.name
    with sh.engine() as eng:
        before = eng.stats().kernel_variant
        for bins, window, n_blocks in settings:
            want = sh.rule(bins, window, n_blocks)
            x = sh.samples_of(n_blocks)
            Cm, count, X = device_samples(eng, x, n_blocks, bins, window)
            assert count == n_blocks == want["n"]
            assert CU.same_bits(X, want["spectra"]), (name, bins, "spectra")
            assert CU.same_bits(Cm, want["C"]), (name, bins, "C")
            # without the export, and through the host form: the same bits
            assert CU.same_bits(device_samples(eng, x, n_blocks, bins, window, want_spectra=False)[0], Cm)
            hostC, hcount, hostX = eng.csm_samples(x, bins, window, want_spectra=True)
            assert hcount == n_blocks and CU.same_bits(hostC, Cm) and CU.same_bits(hostX, X)
            for kind in KINDS:
                if kind not in want:
                    assert kind == CU.DIAGONAL_REMOVED and sh.U == 1
                    continue
                Hm = want["G"] if kind == CU.CAPON else want["C"]
                got = device_map(eng, Hm, n_blocks, bins, window, kind)
                assert CU.same_bits(got["q"], want[kind]["q"]), (name, bins, kind, "q")
                assert CU.same_bits(got["map"], want[kind]["map"]), (name, bins, kind, "map")
                for alone in ("map", "q"):
                    assert CU.same_bits(device_map(eng, Hm, n_blocks, bins, window, kind, want=(alone,))[alone], got[alone])
                host = eng.csm_map(Hm, n_blocks, bins, window, kind, want=("map", "q"))
                assert CU.same_bits(host["map"], got["map"]) and CU.same_bits(host["q"], got["q"])
        assert eng.stats().kernel_variant == before  # CSM calls leave it alone


@pytest.mark.parametrize("name", ["one_mic", "two_mics", "ragged5", "sixty_four", "sixty_five_of_128"])
def test_device_equals_the_host_rule(pkg, shapes, name):
    check_against_host_rule(shapes[name], SETTINGS)


@pytest.mark.parametrize("name", ["two_fifty_six", "two_fifty_seven_of_320"])
def test_device_equals_the_host_rule_where_the_map_kernel_changes_its_launch(pkg, shapes, name):
    """256 active mics: a workgroup's 64 steering vectors and its ring take 144 KiB of dynamic LDS, beyond the 64 KiB a launch gets
    without asking.  257 (of 320 streams, ragged, with gains): a workgroup maps 32 pixels, its lanes 32..63 go along with the last
    one and write nothing; 40 pixels leave a tail workgroup of 8.  70 pixels at 256 mics leave a tail of 6."""
    sh = shapes[name]
    ppw = 64 if sh.U <= 256 else 32
    assert (sh.U + 32) * ppw * 8 > 64 * 1024 and (sh.U + 32) * ppw * 8 <= 144 * 1024 < (sh.U + 32) * 2 * ppw * 8 and sh.P % ppw
    check_against_host_rule(sh, BIG_SETTINGS)


def test_a_split_recording_gives_one_calls_bits(pkg, shapes):
    sh = shapes["ragged5"]
    bins, window = [3, 47, 128], 1
    want = sh.rule(bins, window, 17)
    x = sh.samples_of(17)
    with sh.engine() as eng:
        first, n, _ = device_samples(eng, x, 6, bins, window, want_spectra=False)
        both, n, _ = device_samples(eng, np.ascontiguousarray(x[:, 6 * 256:]), 11, bins, window, matrix=first, block_count=n, want_spectra=False)
        assert n == 17 and CU.same_bits(both, want["C"])
        part, n = eng.csm_samples(x, bins, window, n_blocks=6)
        part, n = eng.csm_samples(np.ascontiguousarray(x[:, 6 * 256:]), bins, window, matrix=part, block_count=n, n_blocks=11)
        assert n == 17 and CU.same_bits(part, want["C"])


@pytest.mark.parametrize("name", ["ragged5", "sixty_five_of_128"])
def test_exact_and_fast_handles_give_the_same_bits(pkg, shapes, name):
    """The rule does not depend on cfg.math: an AWPU_MATH_F32_FAST handle (which has no LutEntry table of its own) maps as the
    exact handle does, and so does a handle whose active list was changed (the tables are rebuilt)."""
    sh = shapes[name]
    bins, window, n_blocks = SETTINGS[2]
    want = sh.rule(bins, window, n_blocks)
    for math in (pkg.MATH_F32_EXACT, pkg.MATH_F32_FAST):
        with sh.engine(math=math) as eng:
            for kind in KINDS:
                Hm = want["G"] if kind == CU.CAPON else want["C"]
                got = eng.csm_map(Hm, n_blocks, bins, window, kind, want=("map", "q"))
                assert CU.same_bits(got["map"], want[kind]["map"]) and CU.same_bits(got["q"], want[kind]["q"]), (math, kind)
            half = sh.index[::2]
            eng.set_active_mics(half)
            gl = None if sh.gains is None else sh.gains[half]
            Cm, n = pkg.csm_accumulate_host(sh.samples_of(3), bins, window, index=half, gain=gl, n_blocks=3)
            assert CU.same_bits(eng.csm_samples(sh.samples_of(3), bins, window, n_blocks=3)[0], Cm)
            ref = pkg.csm_map_host(Cm, n, sh.off, sh.frac, bins, window, index=half)["map"]
            assert CU.same_bits(eng.csm_map(Cm, n, bins, window)["map"], ref)


def test_a_slab_handle_maps_its_own_pixels(pkg, shapes):
    sh = shapes["sixty_five_of_128"]
    bins, window, n_blocks = SETTINGS[3]
    want = sh.rule(bins, window, n_blocks)
    lo, count = 32, 70
    with sh.engine(pixel_begin=lo, pixel_count=count) as eng:
        assert eng.pixel_count == count
        for kind in KINDS:
            Hm = want["G"] if kind == CU.CAPON else want["C"]
            got = device_map(eng, Hm, n_blocks, bins, window, kind)
            assert got["map"].shape == (len(bins), count)
            assert CU.same_bits(got["map"], want[kind]["map"][:, lo:lo + count]) and CU.same_bits(got["q"], want[kind]["q"][:, lo:lo + count]), kind


# ------------------------------------------------------------------------------------------------ 2. value edges

@pytest.mark.parametrize("scale_log2", [-140, -120, -72, 55, 58, 70])
def test_subnormal_and_huge_samples_take_the_rule_as_written(pkg, shapes, scale_log2):
    """Samples scaled into the subnormal range (subnormal spectra, C underflows to zero), to where C's entries are subnormal, to
    huge values, to where C is finite and q overflows to infinity, and to where C overflows and q becomes inf - inf: host and device
    agree bit for bit on every finite or infinite value and on where the NaNs are."""
    sh = shapes["ragged5"]
    bins, window, n_blocks = [3, 47, 128], 1, 3
    x = (sh.samples_of(n_blocks).astype(np.float64) * 2.0 ** scale_log2 * 10.0).astype(np.float32)
    if scale_log2 <= -120:
        assert (np.abs(x[x != 0]) < 2.0 ** -100).all()
    with np.errstate(all="ignore"), sh.engine() as eng:
        want_X = pkg.csm_spectra_host(x, bins, window, index=sh.index, gain=sh.gain_list(), n_blocks=n_blocks)
        want_C, n = pkg.csm_accumulate_host(x, bins, window, index=sh.index, gain=sh.gain_list(), n_blocks=n_blocks)
        Cm, count, X = device_samples(eng, x, n_blocks, bins, window)
        same_where_not_nan(X, want_X, "spectra")
        same_where_not_nan(Cm, want_C, "C")
        print(scale_log2, "largest |C|", np.nanmax(np.abs(want_C)), "inf in C", int(np.isinf(want_C).sum()), "nan in C", int(np.isnan(want_C).sum()))
        tiny = np.abs(want_C[want_C != 0])
        if scale_log2 == -72:  # (what the case is there for: every entry of C subnormal, none lost)
            assert tiny.size and (tiny < 2.0 ** -126).all()
        if scale_log2 == 70:
            assert np.isinf(want_C).any()
        for kind in (CU.CONVENTIONAL, CU.DIAGONAL_REMOVED):
            want = pkg.csm_map_host(want_C, n, sh.off, sh.frac, bins, window, kind, index=sh.index, want=("map", "q"))
            got = device_map(eng, want_C, n, bins, window, kind)
            print(kind, "inf in q", int(np.isinf(want["q"]).sum()), "nan in q", int(np.isnan(want["q"]).sum()))
            if scale_log2 == 58 and kind == CU.CONVENTIONAL:
                assert np.isfinite(want_C).all() and np.isinf(want["q"]).any()
            if scale_log2 == 70:
                assert np.isnan(want["q"]).any()
            same_where_not_nan(got["q"], want["q"], (kind, "q"))
            same_where_not_nan(got["map"], want["map"], (kind, "map"))


# ------------------------------------------------------------------------------------------------ 3. stream order

def test_csm_samples_device_behind_pending_work(pkg, scenes, busy):  # noqa: F811
    sc = scenes(16)
    bins, n_blocks = [3, 47, 128], 5
    rng = np.random.default_rng(8)
    matrices = tuple((rng.standard_normal((3, 64, 64, 2)) * s).astype(np.float32) for s in (1.0, 2.0))
    case = H.Case(sc.engine(), {"samples": sc.samples, "matrix": matrices}, {"spectra": ((n_blocks, 3, 64, 2), np.float32)},
                  lambda e, i, o, s: e.csm_samples_device(i["samples"], 256 * n_blocks, n_blocks, bins, i["matrix"], 1, 0, o["spectra"], s),
                  inout=("matrix",))
    got = check(case, busy)
    assert got["host"] == n_blocks and np.isfinite(got["spectra"]).all() and np.abs(got["spectra"]).max() > 0
    assert not CU.same_bits(got["matrix"], matrices[0])


def test_csm_map_device_behind_pending_work(pkg, scenes, busy):  # noqa: F811
    sc = scenes(16)
    bins = [3, 47, 128]
    matrices = tuple(pkg.csm_accumulate_host(x, bins, 1)[0] for x in sc.samples)
    for math_mode in ("exact", "fast"):
        case = H.Case(sc.engine(math_mode), {"matrix": matrices}, {"map": ((3, sc.P), np.float32), "q": ((3, sc.P), np.float32)},
                      lambda e, i, o, s: e.csm_map_device(i["matrix"], 5, bins, 1, CU.CONVENTIONAL, o["map"], o["q"], s))
        got = check(case, busy)
        want = pkg.csm_map_host(matrices[0], 5, sc.off, sc.frac, bins, 1, want=("map", "q"))
        assert CU.same_bits(got["map"], want["map"]) and CU.same_bits(got["q"], want["q"])


# ------------------------------------------------------------------------------------------------ 4. refusals

def test_handle_forms_refuse(pkg, shapes, scenes):  # noqa: F811
    """FIR8, a band on the handle, a device group and a call during process_async: AWPU_ERR_STATE; no table: AWPU_ERR_STATE; null buffers, a bad
    request, a pitch below the blocks, no output, diagonal removal with one mic: AWPU_ERR_INVALID.  The outputs, the matrix and the
    block count are left alone."""
    import torch

    B = pkg.binding
    sc = scenes(16)
    bins = [3, 47]
    d_x = torch.from_numpy(sc.samples[0]).cuda()
    d_C = torch.full((2 * 64 * 64 * 2,), float(CANARY), dtype=torch.float32, device="cuda")
    d_o = torch.full((2 * sc.P,), float(CANARY), dtype=torch.float32, device="cuda")
    host_C = np.full((2, 64, 64, 2), CANARY, np.float32)
    host_o = np.full((2, sc.P), CANARY, np.float32)

    def refused(eng, which=(0, 1, 2, 3), bins=bins, kind=CU.CONVENTIONAL, samples=True, matrix=True, out=True, pitch=1280, count=0, blocks=5):
        """The statuses of the calls `which`: 0 csm_samples_device, 1 csm_map_device, 2 csm_samples, 3 awpu_hip_csm_map."""
        c = B.csm_of(bins, 1, kind)
        calls = (lambda: eng.csm_samples_device(d_x.data_ptr() if samples else 0, pitch, 5, bins, d_C.data_ptr() if matrix else 0, 1, count),
                 lambda: eng.csm_map_device(d_C.data_ptr() if matrix else 0, blocks, bins, 1, kind, d_o.data_ptr() if out else 0),
                 lambda: eng.csm_samples(sc.samples[0][:, :pitch], bins, 1, matrix=host_C, block_count=count, n_blocks=5),
                 lambda: eng._lib.awpu_hip_csm_map(eng._h, B._f32(host_C) if matrix else None, blocks, C.byref(c), B._f32(host_o) if out else None, None))
        seen = []
        for k in which:
            try:
                rc = calls[k]()
                rc = rc if k == 3 else B.OK
            except pkg.AwpuError as e:
                rc = e.status
            seen.append(rc)
        return seen

    good = sc.engine()
    with good() as eng:
        assert refused(eng, bins=[47, 3]) == [B.ERR_INVALID] * 4
        assert refused(eng, bins=[3, 129]) == [B.ERR_INVALID] * 4
        assert refused(eng, (0, 1, 3), bins=list(range(9))) == [B.ERR_INVALID] * 3  # (the wrapper sizes csm_samples' matrix by n_bins)
        assert refused(eng, (1, 3), kind=3) == [B.ERR_INVALID] * 2
        assert refused(eng, (0, 1, 3), matrix=False) == [B.ERR_INVALID] * 3
        assert refused(eng, (0,), samples=False) == [B.ERR_INVALID]
        assert refused(eng, (1, 3), out=False) == [B.ERR_INVALID] * 2
        assert refused(eng, (0, 2), pitch=1279) == [B.ERR_INVALID] * 2
        assert refused(eng, (0, 2), count=-1) == [B.ERR_INVALID] * 2 and refused(eng, (0, 2), count=2 ** 31 - 3) == [B.ERR_INVALID] * 2
        assert refused(eng, (1, 3), blocks=0) == [B.ERR_INVALID] * 2
        eng.set_band(pkg.band_design(1000.0, 4000.0, 31))
        assert refused(eng) == [B.ERR_STATE] * 4
        eng.set_band(None)
        eng.process_async(sc.frames[0][:1])
        assert refused(eng) == [B.ERR_STATE] * 4
        eng.wait()
    with pkg.Engine(n_pixels=sc.P, n_streams=64, interp=B.INTERP_FIR8) as eng:
        eng.set_delay_table(sc.off, sc.frac)
        eng.set_active_mics(None)
        assert refused(eng) == [B.ERR_STATE] * 4
    with pkg.Engine(n_pixels=sc.P, n_streams=64, grid_columns=16, devices=[0, 0]) as eng:  # a device group
        eng.set_delay_table(sc.off, sc.frac)
        eng.set_active_mics(None)
        assert refused(eng) == [B.ERR_STATE] * 4
        # ... and the caller's block count stays as it was
        count, c = C.c_int32(7), B.csm_of(bins, 1)
        assert eng._lib.awpu_hip_csm_samples_device(eng._h, C.c_void_p(d_x.data_ptr()), 1280, 5, C.byref(c), C.c_void_p(d_C.data_ptr()),
                                                    C.cast(C.byref(count), B._i32p), None, None) == B.ERR_STATE
        assert eng._lib.awpu_hip_csm_samples(eng._h, B._f32(sc.samples[0]), 1280, 5, C.byref(c), B._f32(host_C), C.cast(C.byref(count), B._i32p),
                                             None) == B.ERR_STATE
        assert count.value == 7
    with pkg.Engine(n_pixels=sc.P, n_streams=64) as eng:  # no table, no mics
        assert refused(eng) == [B.ERR_STATE] * 4
    one = shapes["one_mic"]
    with one.engine() as eng:
        d_1 = torch.zeros(8, device="cuda")
        with pytest.raises(pkg.AwpuError) as ei:
            eng.csm_map_device(d_1.data_ptr(), 1, [3], 0, CU.DIAGONAL_REMOVED, d_o.data_ptr())
        assert ei.value.status == B.ERR_INVALID
    torch.cuda.synchronize()
    assert (d_C.cpu().numpy() == CANARY).all() and (d_o.cpu().numpy() == CANARY).all() and (host_C == CANARY).all() and (host_o == CANARY).all()


# ------------------------------------------------------------------------------------------------ 5. the scene

def test_the_scenes_capon_plane_has_its_two_sources(pkg):
    """csm_util's scene (tests/test_csm_cpu.py states it): accumulated and mapped on the device, the inverse from the host, the
    plane handed to find_peaks_device as it is."""
    import torch

    B = pkg.binding
    S = pkg.synthetic
    spec = S.WORKLOADS["c1"]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    x, _ = CU.scene_samples(pkg, spec, xyz)
    b = [CU.SCENE_BIN]
    with pkg.Engine(n_pixels=spec.n_pixels, n_streams=64, grid_columns=32) as eng:
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        Cm, n = eng.csm_samples(x, b, 1)
        assert n == CU.SCENE_BLOCKS
        G = pkg.csm_invert_host(Cm, n, b, loading=CU.SCENE_LOADING)
        d_G = torch.from_numpy(G).cuda()
        d_plane = torch.empty(1024, device="cuda")
        d_sources = torch.zeros(4 * 40, dtype=torch.uint8, device="cuda")
        d_count = torch.zeros(1, dtype=torch.int32, device="cuda")
        eng.csm_map_device(d_G.data_ptr(), n, b, 1, CU.CAPON, d_plane.data_ptr())
        eng.find_peaks_device(d_plane.data_ptr(), 1, 32, 32, d_sources.data_ptr(), d_count.data_ptr(), **CU.SCENE_FIND)
        eng.synchronize()
        conventional = eng.csm_map(Cm, n, b, 1, CU.CONVENTIONAL)["map"][0]
    count = int(d_count.cpu().numpy()[0])
    pixels = [int(p) for p in d_sources.cpu().numpy().view(B.SOURCE_DTYPE)["pixel"][:count]]
    print(count, pixels)
    assert count == 2
    for true in CU.scene_pixels(spec):
        assert any(abs(p // 32 - true // 32) <= 1 and abs(p % 32 - true % 32) <= 1 for p in pixels), (true, pixels)
    assert int(np.ravel(pkg.find_peaks(conventional, 32, 32, **CU.SCENE_FIND).count)[0]) == 1
    # the device's C is the host rule's
    assert CU.same_bits(Cm, pkg.csm_accumulate_host(x, b, 1)[0])
