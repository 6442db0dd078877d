"""Parity of the gfx950 sweep (through the C ABI) with the oracle, the reference-generated
golden vectors and size-independent properties.  Everything here needs a real MI355X."""
import importlib
import os
from pathlib import Path

import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
SWEEPS = ["sweep_c1", "sweep_c1_ragged", "sweep_c1_onemic", "sweep_headline", "sweep_c3"]
MATHS = ["exact", "fast"]


def math_id(pkg, name):
    return {"exact": pkg.MATH_F32_EXACT, "fast": pkg.MATH_F32_FAST}[name]


def run_engine(pkg, X, off, frac, index=None, math="fast", max_batch=None, **kw):
    X = np.asarray(X, np.float32)
    frames = X if X.ndim == 3 else X[None]
    eng = pkg.Engine(n_pixels=off.shape[0], n_streams=frames.shape[1], lut_stride=off.shape[1],
                     hist=frames.shape[2], math=math_id(pkg, math), max_batch=max_batch or frames.shape[0], **kw)
    with eng:
        eng.set_delay_table(off, frac)
        eng.set_active_mics(index)
        power = eng.process(frames)
        st = eng.stats()
    return (power if X.ndim == 3 else power[0]), st


def check_full_grid(oracle, got, frame, off, frac, what, index=None, fir_table=None):
    """The parity claim in the north star's wording, on EVERY pixel handed in: per-pixel power within 1e-5 relative of
    the reference's arithmetic (oracle.das_f32 / das_fir8_f32), no floor, no allowance: `ok` of util.parity_report is
    max_rel_unfloored <= 1e-5 and pixels_over_1e5 == 0 (round 4: the 3 x reference-noise allowance of round 3 is gone
    from here; it survives only as the named field `ok_within_reference_noise`, used by the one DC-bias test of the
    re-ordered fast sweep).  Oracle cost: 2-8 s per full 128x128 frame."""
    if fir_table is None:
        r32, r64 = oracle.das_f32(frame, off, frac, index), oracle.das_f64(frame, off, frac, index)
    else:
        r32, r64 = oracle.das_fir8_f32(frame, off, frac, fir_table, index), oracle.das_fir8_f64(frame, off, frac, fir_table, index)
    rep = util.parity_report(got, r32, r64)
    print(f"parity {what}: {rep}")
    assert rep["ok"] and rep["max_rel_unfloored"] <= util.POWER_RTOL and rep["pixels_over_1e5"] == 0, (what, rep)
    return rep


def test_native_library_is_loaded(pkg):
    """The GPU tests run the in-tree HIP library, not a fallback."""
    lib = pkg.binding.load()
    assert "libawpu_hip.so" in lib._name
    maps = Path("/proc/self/maps").read_text()
    assert "beamforming-lk_amd/libawpu_hip.so" in maps


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("name", SWEEPS)
def test_golden_vectors(pkg, name, math):
    """GPU power vs the power the reference's compiled delay() produced (tests/golden)."""
    g = np.load(GOLDEN / f"{name}.npz")
    ax, ay = g["arrays"]
    X = util.hash_frames(64 * int(ax) * int(ay), int(g["hist"]), seed=int(g["seed"]))[0]
    power, _ = run_engine(pkg, X, g["off"], g["frac"], g["index"], math=math)
    assert util.power_rel_err_unfloored(power, g["power"]) < util.POWER_RTOL


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("wl", ["c1", "c2"])
def test_full_grid_vs_oracle(pkg, oracle, wl, math):
    """BASELINE configs c1 (64 mics, 32x32) and c2 (256 mics, 64x64), plane wave + noise."""
    S = pkg.synthetic
    spec = S.WORKLOADS[wl]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    X = S.make_frames(xyz, 1, seed=1234)[0]
    power, st = run_engine(pkg, X, off, frac, math=math)
    want = oracle.das_f32(X, off, frac)
    assert util.power_rel_err_unfloored(power, want) < util.POWER_RTOL
    # against fp64 the GPU is in the same error class as the fp32 CPU restatement
    p64 = oracle.das_f64(X, off, frac)
    assert util.power_rel_err(power, p64) < max(3 * util.power_rel_err(want, p64), 5e-6)
    r, c = divmod(int(power.argmax()), spec.res)
    er, ec = S.source_pixel(spec)
    assert abs(r - er) <= 1 and abs(c - ec) <= 1
    assert st.usable == spec.n_mics and st.window == 256 + st.tau_max + 1
    assert st.alg_bytes_frame == S.algorithmic_bytes_per_frame(spec.n_mics, spec.n_pixels, st.window)


@pytest.mark.parametrize("math", MATHS)
def test_headline_rows_vs_oracle(pkg, oracle, math):
    """Headline shape (256 mics, 128x128): a slab of grid rows through the pixel-shard interface."""
    S = pkg.synthetic
    spec = S.WORKLOADS["headline"]
    xyz = S.geometry(spec)
    rows = (40, 6)
    off, frac = S.delay_table(spec, xyz, *rows)
    X = S.make_frames(xyz, 1, seed=77)[0]
    # n_pixels is the whole grid; the handle owns rows 40..45
    power = run_engine_shard(pkg, X, off, frac, spec.n_pixels, rows[0] * spec.res, math)
    want = oracle.das_f32(X, off, frac)
    assert util.power_rel_err_unfloored(power, want) < util.POWER_RTOL


def run_engine_shard(pkg, X, off, frac, n_pixels, pixel_begin, math="fast"):
    eng = pkg.Engine(n_pixels=n_pixels, n_streams=X.shape[0], lut_stride=off.shape[1], hist=X.shape[1],
                     math=math_id(pkg, math), pixel_begin=pixel_begin, pixel_count=off.shape[0])
    with eng:
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        return eng.process(X)


@pytest.mark.parametrize("math", MATHS)
def test_pixel_shards_tile_the_grid(pkg, oracle, math):
    """Multi-GPU decomposition: per-rank slabs concatenate to the single-handle result bit for bit."""
    S = pkg.synthetic
    spec = S.WORKLOADS["c1"]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    X = S.make_frames(xyz, 1, seed=5)[0]
    whole, _ = run_engine(pkg, X, off, frac, math=math)
    cuts = [0, 300, 301, 777, 1024]  # ragged, not multiples of any tile
    parts = [run_engine_shard(pkg, X, off[a:b], frac[a:b], spec.n_pixels, a, math) for a, b in zip(cuts, cuts[1:])]
    assert np.array_equal(np.concatenate(parts), whole)


@pytest.mark.parametrize("math", MATHS)
def test_batch_equals_single_frames(pkg, oracle, math):
    S = pkg.synthetic
    spec = S.WORKLOADS["c1"]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    off, frac = off[:200], frac[:200]
    frames = S.make_frames(xyz, 5, seed=8)
    batch, _ = run_engine(pkg, frames, off, frac, math=math)
    # the same frames in another order and another batch size: bit-identical per frame
    rev, _ = run_engine(pkg, frames[::-1][:4], off, frac, math=math, max_batch=7)
    assert np.array_equal(rev, batch[::-1][:4])
    for b in range(5):
        # a single-frame call may run another kernel shape (the epilogue sums in another order)
        single, _ = run_engine(pkg, frames[b], off, frac, math=math)
        assert util.power_rel_err(batch[b], single) < 2e-6
        assert util.power_rel_err_unfloored(batch[b], oracle.das_f32(frames[b], off, frac)) < util.POWER_RTOL


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("n_pix", [1, 3, 17, 63, 65])
def test_ragged_pixel_counts(pkg, oracle, math, n_pix):
    xyz = oracle.create_antenna()
    off, frac = oracle.compute_delay_lut(xyz, 12, 12)
    off, frac = off[5:5 + n_pix], frac[5:5 + n_pix]
    X = util.hash_frames(64, 1024, seed=n_pix)[0]
    power, _ = run_engine(pkg, X, off, frac, math=math)
    assert util.power_rel_err_unfloored(power, oracle.das_f32(X, off, frac)) < util.POWER_RTOL


@pytest.mark.parametrize("math", MATHS)
def test_active_mic_subsets(pkg, oracle, math):
    """antenna.index semantics (mimo.cpp:100-103,125-127): unsorted subset, table wider than streams used."""
    xyz = oracle.create_tiled_antenna(4, 1)
    off, frac = oracle.compute_delay_lut(xyz, 10, 10)
    X = util.hash_frames(256, 700, seed=31)[0]
    rng = np.random.default_rng(4)
    for usable in (1, 2, 63, 64, 65, 200, 256):
        index = rng.permutation(256)[:usable].astype(np.int32)
        power, st = run_engine(pkg, X, off, frac, index, math=math)
        assert st.usable == usable
        assert util.power_rel_err_unfloored(power, oracle.das_f32(X, off, frac, index)) < util.POWER_RTOL


@pytest.mark.parametrize("math", MATHS)
def test_extreme_offsets_and_fractions(pkg, oracle, math):
    """Offsets at both ends of the history and fractions 0 / 1-ulp: window edges are read correctly."""
    rng = np.random.default_rng(12)
    P, M, hist = 40, 64, 1024
    off = rng.integers(0, hist - 256, size=(P, M)).astype(np.int32)
    off[0, :] = 0
    off[1, :] = hist - 257
    off[2, ::2] = 0
    off[2, 1::2] = hist - 257
    frac = rng.uniform(0, 1, size=(P, M)).astype(np.float32)
    frac[3, :] = 0.0
    frac[4, :] = np.nextafter(np.float32(1.0), np.float32(0.0))
    X = util.hash_frames(M, hist, seed=77)[0]
    power, st = run_engine(pkg, X, off, frac, math=math)
    assert st.window == hist
    assert util.power_rel_err_unfloored(power, oracle.das_f32(X, off, frac)) < util.POWER_RTOL
    # the same with a ragged mic list and a history that is not a multiple of 4 (regression: the guarded
    # staging of the last, odd group of rows used to clip the unshifted copy to the shifted copy's length,
    # losing the newest sample for entries at the largest legal offset)
    hist = 777
    off = rng.integers(0, hist - 256, size=(P, M)).astype(np.int32)
    off[1, :] = hist - 257
    off[5, ::3] = hist - 257
    index = np.array([s for s in range(M) if s not in (7, 30, 55)], np.int32)
    frames = util.hash_frames(M, hist, seed=78, batch=3)
    for batch in (1, 3):
        power, st = run_engine(pkg, frames[:batch], off, frac, index=index, math=math)
        assert st.window == hist
        want = np.stack([oracle.das_f32(f, off, frac, index) for f in frames[:batch]])
        assert util.power_rel_err_unfloored(power, want) < util.POWER_RTOL, batch


@pytest.mark.parametrize("math", MATHS)
def test_linearity_and_scaling(pkg, math):
    """Size-independent properties on the full c2 shape: power(a*X) = a^2 power(X) exactly for a
    power of two, and a zero frame gives zero power."""
    S = pkg.synthetic
    spec = S.WORKLOADS["c2"]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    X = S.make_frames(xyz, 1, seed=2)[0]
    frames = np.stack([X, 4.0 * X, np.zeros_like(X)])
    power, _ = run_engine(pkg, frames, off, frac, math=math)
    assert np.array_equal(power[1], 16.0 * power[0])
    assert np.all(power[2] == 0.0)
    assert np.all(power[0] > 0.0)


def test_exact_mode_matches_oracle_to_rounding(pkg, oracle):
    """AWPU_MATH_F32_EXACT keeps delay.cpp:19-25's operation and mic order: only the epilogue's
    254-term sum order differs from the scalar restatement."""
    S = pkg.synthetic
    spec = S.WORKLOADS["c1"]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    X = S.make_frames(xyz, 1, seed=10)[0]
    power, _ = run_engine(pkg, X, off, frac, math="exact")
    want = oracle.das_f32(X, off, frac)
    assert np.abs(power / want - 1).max() < 1e-6


def test_error_paths(pkg, oracle):
    B = pkg.binding
    xyz = oracle.create_antenna()
    off, frac = oracle.compute_delay_lut(xyz, 4, 4)
    X = util.hash_frames(64, 1024, seed=1)
    eng = pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=16, max_batch=2)
    with eng:
        with pytest.raises(pkg.AwpuError) as ei:
            eng.process(X)
        assert ei.value.status == B.ERR_STATE
        eng.set_active_mics(None)
        bad = off.copy()
        bad[3, 5] = 1024 - 256  # reads signal[..+256] one past the history
        eng.set_delay_table(bad, frac)
        with pytest.raises(pkg.AwpuError) as ei:
            eng.process(X)
        assert ei.value.status == B.ERR_RANGE
        neg = off.copy()
        neg[0, 0] = -1
        eng.set_delay_table(neg, frac)
        with pytest.raises(pkg.AwpuError) as ei:
            eng.process(X)
        assert ei.value.status == B.ERR_RANGE
        with pytest.raises(pkg.AwpuError):
            eng.set_delay_table(off, frac + 2.0)
        with pytest.raises(pkg.AwpuError):
            eng.set_active_mics(np.array([64], np.int32))
        eng.set_delay_table(off, frac)
        with pytest.raises(pkg.AwpuError) as ei:
            eng.process(np.concatenate([X, X, X]))  # batch 3 > max_batch 2
        assert ei.value.status == B.ERR_INVALID
        ok = eng.process(X)
        assert util.power_rel_err_unfloored(ok[0], oracle.das_f32(X[0], off, frac)) < util.POWER_RTOL


def test_host_buffer_entry_split_in_two(pkg, oracle):
    """awpu_hip_process_async / awpu_hip_wait: the same bits as the synchronous call, one call in flight per handle,
    the caller's thread free in between (two handles overlap their work)."""
    S = pkg.synthetic
    spec = S.WORKLOADS["c1"]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    frames = S.make_frames(xyz, 4, seed=31)
    engines = [pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=spec.n_pixels, max_batch=4) for _ in range(2)]
    for eng in engines:
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
    want = engines[0].process(frames)
    engines[0].process_async(frames)
    engines[1].process_async(frames[::-1])  # both in flight
    with pytest.raises(pkg.AwpuError) as ei:
        engines[0].process_async(frames)
    assert ei.value.status == pkg.binding.ERR_STATE
    got1 = engines[1].wait()
    got0 = engines[0].wait()
    assert np.array_equal(got0, want) and np.array_equal(got1, want[::-1])
    assert engines[0].wait() is None  # nothing in flight: a no-op
    assert engines[0].stats().last_kernel_ms > 0
    for eng in engines:
        eng.close()


def test_device_pointer_entry_with_torch(pkg, oracle):
    """awpu_hip_process_device on torch-owned HBM buffers and a torch stream (the bench.py path)."""
    import torch

    S = pkg.synthetic
    spec = S.WORKLOADS["c1"]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    frames = S.make_frames(xyz, 3, seed=6)
    dev = torch.device("cuda:0")
    d_frames = torch.from_numpy(frames).to(dev)
    d_power = torch.zeros((3, spec.n_pixels), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()  # (torch fills on its own stream; the engine's streams do not wait for it)
    eng = pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=spec.n_pixels, max_batch=3)
    with eng:
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            eng.process_device(d_frames.data_ptr(), 3, d_power.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        host = eng.process(frames)
    got = d_power.cpu().numpy()
    assert np.array_equal(got, host)
    for b in range(3):
        assert util.power_rel_err_unfloored(got[b], oracle.das_f32(frames[b], off, frac)) < util.POWER_RTOL


FIR8_SWEEPS = ["sweep_c1_fir8", "sweep_c1_ragged_fir8", "sweep_headline_fir8", "sweep_c3_fir8"]


def measured_fir_table():
    """The weights the reference's compiled 8-tap delay() applies (its impulse responses, measured from
    oracle/_ref/libref_das_fir.so by tests/golden/make_golden.py): the table a caller would pass."""
    return np.load(GOLDEN / "delay_kat_fir8.npz")["impulse_response"]


def with_maths(values):
    """(value, math) for every value and both math modes; the FAST leg keeps the id it had when it was the only one."""
    return [pytest.param(v, m, id=v if m == "fast" else f"{v}-{m}") for v in values for m in MATHS]


@pytest.mark.parametrize("name,math", with_maths(FIR8_SWEEPS))
def test_fir8_golden_vectors(pkg, name, math):
    """AWPU_INTERP_FIR8 on the GPU vs the powers the reference's own non-AVX2 build produced (delay.cpp:31-40
    inside mimo.cpp:121-151): 64, 256 and 512 mics, a ragged mic list, clipped corner pixels; in the default mode
    (a multiply and an add per tap) and in AWPU_MATH_F32_FAST (one FMA per tap)."""
    g = np.load(GOLDEN / f"{name}.npz")
    ax, ay = g["arrays"]
    n = 64 * int(ax) * int(ay)
    X = util.hash_frames(n, int(g["hist"]), seed=int(g["seed"]))[0]
    eng = pkg.Engine(math=math_id(pkg, math), n_pixels=g["off"].shape[0], n_streams=n, hist=int(g["hist"]), interp=pkg.binding.INTERP_FIR8)
    with eng:
        eng.set_delay_table(g["off"], g["frac"])
        eng.set_active_mics(g["index"])
        eng.set_fir_table(measured_fir_table())
        power = eng.process(X)
    assert util.power_rel_err_unfloored(power, g["power"]) < util.POWER_RTOL


@pytest.mark.parametrize("name", FIR8_SWEEPS)
def test_fir8_golden_vectors_on_the_batch_kernel(pkg, name):
    """The same reference-produced powers through the kernel FIR8 BATCHES run (das_fir8_plane_kernel: four-plane
    frame-pair layout, taken once a launch has >= 256 workgroups): the golden's pixels repeated until the grid is
    that large, two frames (the golden's frame twice) -- every copy of a pixel, in both frames, must give the
    reference's power."""
    g = np.load(GOLDEN / f"{name}.npz")
    ax, ay = g["arrays"]
    n = 64 * int(ax) * int(ay)
    X = util.hash_frames(n, int(g["hist"]), seed=int(g["seed"]))[0]
    P = g["off"].shape[0]
    reps = -(-(256 * 64 + 1) // P)
    off, frac = np.tile(g["off"], (reps, 1)), np.tile(g["frac"], (reps, 1))
    with pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=P * reps, n_streams=n, hist=int(g["hist"]), interp=pkg.binding.INTERP_FIR8, max_batch=2) as eng:
        eng.set_delay_table(off, frac)
        eng.set_active_mics(g["index"])
        eng.set_fir_table(measured_fir_table())
        power = eng.process(np.stack([X, X]))
    want = np.tile(g["power"], reps)
    for b in range(2):
        assert util.power_rel_err_unfloored(power[b], want) < util.POWER_RTOL


@pytest.mark.parametrize("table_kind,math", with_maths(["synthetic", "reference"]))
def test_fir8_mode_vs_oracle(pkg, oracle, table_kind, math):
    """AWPU_INTERP_FIR8 (delay.cpp:31-40): GPU vs the restated FIR sweep, 64 and 256 mics, with a
    synthetic table and the reference's own (as measured from its compiled delay(), tests/golden), in both math modes."""
    table = util.synthetic_fir_table() if table_kind == "synthetic" else measured_fir_table()
    for arrays, res, usable in [((1, 1), 16, 64), ((4, 1), 8, 200)]:
        xyz = oracle.create_tiled_antenna(*arrays)
        off, frac = oracle.compute_delay_lut(xyz, res, res)
        n = xyz.shape[1]
        X = util.hash_frames(n, 1024, seed=50 + usable, batch=2)
        index = np.random.default_rng(usable).permutation(n)[:usable].astype(np.int32)
        eng = pkg.Engine(math=math_id(pkg, math), n_pixels=off.shape[0], n_streams=n, interp=pkg.binding.INTERP_FIR8, max_batch=2)
        with eng:
            eng.set_delay_table(off, frac)
            eng.set_active_mics(index)
            with pytest.raises(pkg.AwpuError) as ei:
                eng.process(X)
            assert ei.value.status == pkg.binding.ERR_STATE  # table not set yet
            eng.set_fir_table(table)
            power = eng.process(X)
        for b in range(2):
            want = oracle.das_fir8_f32(X[b], off, frac, table, index)
            assert util.power_rel_err_unfloored(power[b], want) < util.POWER_RTOL


def test_fir8_batched_frame_pair_shape(pkg, oracle):
    """AWPU_INTERP_FIR8 on a full grid with a batch: the frame-pair FIR8 sweep (das_fir8_plane_kernel).  One 8x8 array,
    128x128 grid, three frames (an odd batch: the last pair is half empty), a ragged mic list; every pixel against
    the restated FIR sweep with the reference's measured table, and whole frames against the single-frame calls
    (the exact-structure kernel: same taps in the same order, same bits before the epilogue)."""
    xyz = oracle.create_antenna()
    res = 128
    off, frac = oracle.compute_delay_lut(xyz, res, res)
    table = measured_fir_table()
    X = util.hash_frames(64, 1024, seed=91, batch=3)
    index = np.array([m for m in range(64) if m % 7 != 3], np.int32)
    with pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=res * res, interp=pkg.binding.INTERP_FIR8, max_batch=3) as eng:
        eng.set_delay_table(off, frac)
        eng.set_active_mics(index)
        eng.set_fir_table(table)
        batch = eng.process(X)
        single = np.stack([eng.process(X[b]) for b in range(3)])
    assert util.power_rel_err(batch, single) < 2e-6
    for b in range(3):
        check_full_grid(oracle, batch[b], X[b], off, frac, f"fir8 batch frame {b}", index=index, fir_table=table)


FIR8_DC_SWEEPS = ["sweep_c1_fir8_dc", "sweep_c1_ragged_fir8_dc", "sweep_headline_fir8_dc", "sweep_c3_fir8_dc"]
_fir8_dc_cases = {}


def fir8_dc_case(name):
    """(golden, frames [5, n, hist]) of a DC-biased FIR8 golden: hash frames + {0, 1e-4, 1e-3, 1e-2, 0.25}; made once per file."""
    if name not in _fir8_dc_cases:
        g = np.load(GOLDEN / f"{name}.npz")
        ax, ay = g["arrays"]
        X0 = util.hash_frames(64 * int(ax) * int(ay), int(g["hist"]), seed=int(g["seed"]))[0]
        frames = np.stack([(X0 + np.float32(dc)).astype(np.float32) for dc in g["offsets"]])
        frames.setflags(write=False)
        _fir8_dc_cases[name] = ({k: g[k] for k in g.files}, frames)
    return _fir8_dc_cases[name]


def fir8_engine(pkg, g, math, n_pixels=None, **kw):
    n = 64 * int(g["arrays"][0]) * int(g["arrays"][1])
    return pkg.Engine(n_pixels=n_pixels or g["off"].shape[0], n_streams=n, hist=int(g["hist"]), math=math, interp=pkg.binding.INTERP_FIR8, **kw)


def _fir8_sums_through_the_abi(pkg, g, frames, gains=None):
    """out [B, P, 256] of AWPU_MATH_F32_EXACT + AWPU_INTERP_FIR8 through awpu_hip_process_device_sums: the frames as one
    batch and one frame per call (the same handle), each into a buffer pre-filled with NaN."""
    import torch

    B, P = frames.shape[0], g["off"].shape[0]
    with fir8_engine(pkg, g, pkg.MATH_F32_EXACT, max_batch=B) as eng:
        eng.set_delay_table(g["off"], g["frac"])
        eng.set_active_mics(g["index"])
        eng.set_fir_table(measured_fir_table())
        eng.set_mic_gains(gains)
        d_X = torch.from_numpy(np.array(frames, np.float32)).cuda()
        d_P = torch.empty((2, B, P), dtype=torch.float32, device="cuda")
        d_S = torch.full((2, B, P, 256), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        eng.process_device_sums(d_X.data_ptr(), B, d_P[0].data_ptr(), d_S[0].data_ptr())
        for b in range(B):
            eng.process_device_sums(d_X[b].data_ptr(), 1, d_P[1, b].data_ptr(), d_S[1, b].data_ptr())
        eng.synchronize()
        assert pkg.binding.KERNEL_NAMES[eng.stats().kernel_variant] == "fir8"
        return d_S[0].cpu().numpy(), d_S[1].cpu().numpy()


@pytest.mark.parametrize("name", FIR8_DC_SWEEPS)
def test_fir8_exact_mode_sums_are_the_reference_bits(pkg, oracle, name):
    """out[0..255] of a pixel before the moving average, from das_fir8_kernel with the reference's rounding (EXACT + FIR8,
    awpu_hip_process_device_sums), against what the reference's non-AVX2 object code left in out[] on hash frames +
    {0, 1e-4, 1e-3, 1e-2, 0.25} (golden out_first / out_last): BIT-identical -- per tap a product and an add, taps 0..7, mics
    in index[] order -- with one, a few and many LDS chunks per pixel (64, 47 of 64, 256, 512 mics); every other pixel
    against the restatement, which tests/test_oracle_golden.py pins to the same object code.  A batch of five and one
    frame per call give the same bits.  The ragged file again with per-mic gains, against the restatement's out[] of the
    prescaled frames."""
    g, frames = fir8_dc_case(name)
    table = measured_fir_table()
    batch, single = _fir8_sums_through_the_abi(pkg, g, frames)
    assert not np.isnan(batch).any() and not np.isnan(single).any()
    for b in range(frames.shape[0]):
        assert np.array_equal(batch[b, :4], g["out_first"][b]), (name, b)
        assert np.array_equal(batch[b, -1:], g["out_last"][b]), (name, b)
        _, want = oracle.das_fir8_f32(frames[b], g["off"], g["frac"], table, g["index"], want_out=True)
        assert np.array_equal(batch[b], want), (name, b, np.argwhere(batch[b] != want)[:4])
    assert np.array_equal(single, batch)
    if name == "sweep_c1_ragged_fir8_dc":
        gains = np.random.default_rng(17).uniform(0.5, 2.0, 64).astype(np.float32)
        batch, single = _fir8_sums_through_the_abi(pkg, g, frames, gains=gains)
        assert not np.isnan(batch).any()
        for b in range(frames.shape[0]):
            _, want = oracle.das_fir8_f32(frames[b] * gains[:, None], g["off"], g["frac"], table, g["index"], want_out=True)
            assert np.array_equal(batch[b], want), (name, "gains", b)
        assert np.array_equal(single, batch)


def test_fir8_sums_are_refused_in_fast_mode(pkg):
    """AWPU_MATH_F32_FAST + FIR8 has an order of its own (an FMA per tap, or the plane kernel's): no out[] to export."""
    import torch

    g, frames = fir8_dc_case("sweep_c1_fir8_dc")
    P = g["off"].shape[0]
    with fir8_engine(pkg, g, pkg.MATH_F32_FAST) as eng:
        eng.set_delay_table(g["off"], g["frac"])
        eng.set_active_mics(g["index"])
        eng.set_fir_table(measured_fir_table())
        d_X = torch.from_numpy(frames[:1].copy()).cuda()
        d_P = torch.empty((1, P), dtype=torch.float32, device="cuda")
        d_S = torch.empty((1, P, 256), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(pkg.AwpuError) as ei:
            eng.process_device_sums(d_X.data_ptr(), 1, d_P.data_ptr(), d_S.data_ptr())
        assert ei.value.status == pkg.binding.ERR_STATE


@pytest.mark.parametrize("name", FIR8_DC_SWEEPS)
def test_fir8_dc_biased_goldens_default_mode_flat_1e5(pkg, name):
    """Engine(interp=FIR8) with the math left at the library's default, on the DC-biased FIR8 goldens: every pixel at every
    offset within 1e-5 of the powers the reference's non-AVX2 build produced, flat, no floor -- INTEGRATION.md's "within 1e-5
    of the reference on any input" for the 8-tap variant -- as a batch of five and one frame per call, which agree bit for
    bit.  (An FMA per tap instead of the reference's product and add misses this with a bias of 0.25: 1.30e-5 at 256 mics and
    1.42e-5 at 512, measured; with the reference's rounding at most 3.4e-7 at any offset.)"""
    g, frames = fir8_dc_case(name)
    with fir8_engine(pkg, g, None, max_batch=frames.shape[0]) as eng:
        eng.set_delay_table(g["off"], g["frac"])
        eng.set_active_mics(g["index"])
        eng.set_fir_table(measured_fir_table())
        batch = eng.process(frames)
        assert pkg.binding.KERNEL_NAMES[eng.stats().kernel_variant] == "fir8"
        single = np.stack([eng.process(frames[b]) for b in range(frames.shape[0])])
        assert pkg.binding.KERNEL_NAMES[eng.stats().kernel_variant] == "fir8"
    assert np.array_equal(single, batch)
    curve = {float(dc): util.power_rel_err_unfloored(batch[k], g["power"][k]) for k, dc in enumerate(g["offsets"])}
    print(f"parity_dc {name}: offset -> default mode max unfloored error vs the reference build: {curve}")
    for dc, err in curve.items():
        assert err <= util.POWER_RTOL, (name, dc, err)


@pytest.mark.parametrize("name", FIR8_DC_SWEEPS)
def test_fir8_dc_biased_goldens_fast_mode_recorded(pkg, oracle, name):
    """AWPU_MATH_F32_FAST + FIR8 on the same goldens through both of its kernels: das_fir8_kernel with an FMA per tap (the
    golden's pixels, a batch of five) and das_fir8_plane_kernel (the pixels tiled to 256 * 64 + 1, a batch of five: an odd
    last pair; every copy of a pixel must agree with the golden).  Zero-mean: 1e-5, strict.  Biased: FAST's order is its own,
    so only util.parity_report's named allowance is asserted -- max(1e-5, 3 x the reference's own distance to exact fp64 sums),
    computed from the reference -- and the error per offset PRINTED."""
    g, frames = fir8_dc_case(name)
    table = measured_fir_table()
    P, B = g["off"].shape[0], frames.shape[0]
    reps = -(-(256 * 64 + 1) // P)
    names = pkg.binding.KERNEL_NAMES
    with fir8_engine(pkg, g, pkg.MATH_F32_FAST, max_batch=B) as eng:
        eng.set_delay_table(g["off"], g["frac"])
        eng.set_active_mics(g["index"])
        eng.set_fir_table(table)
        small = eng.process(frames)
        assert names[eng.stats().kernel_variant] == "fir8"
    with fir8_engine(pkg, g, pkg.MATH_F32_FAST, n_pixels=P * reps, max_batch=B) as eng:
        eng.set_delay_table(np.tile(g["off"], (reps, 1)), np.tile(g["frac"], (reps, 1)))
        eng.set_active_mics(g["index"])
        eng.set_fir_table(table)
        planes = eng.process(frames)
        assert names[eng.stats().kernel_variant] == "fir8_planes"
    curve = {}
    for k, dc in enumerate(g["offsets"]):
        ref64 = oracle.das_fir8_f64(frames[k], g["off"], g["frac"], table, g["index"])
        reports = {"fir8": util.parity_report(small[k], g["power"][k], ref64),
                   "fir8_planes": util.parity_report(planes[k], np.tile(g["power"][k], reps), np.tile(ref64, reps))}
        curve[float(dc)] = {kern: (rep["max_rel_unfloored"], rep["noise_bound"]) for kern, rep in reports.items()}
        for kern, rep in reports.items():
            if dc == 0:
                assert rep["ok"], (name, kern, float(dc), rep)
            else:
                assert rep["ok_within_reference_noise"], (name, kern, float(dc), rep)
    print(f"parity_dc {name}: offset -> kernel -> (fast mode max unfloored error vs the reference build, bound): {curve}")


def test_device_heatmap_equals_populate_heatmap(pkg, oracle):
    """the display step on device buffers is byte-identical to the restated
    MIMOWorker::populateHeatmap (mimo.cpp:61-95), per frame, and accepts an external peak."""
    import torch

    S = pkg.synthetic
    spec = S.WORKLOADS["c1"]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    frames = S.make_frames(xyz, 3, seed=9)
    frames[2] *= 0.0  # an all-zero frame: max 0 -> 0/0 -> NaN, defined as level 0 (host, device and checker alike)
    dev = torch.device("cuda:0")
    with pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=spec.n_pixels, max_batch=3) as eng:
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        power = eng.process(frames)
        d_power = torch.from_numpy(power).to(dev)
        d_peak = torch.zeros(3, dtype=torch.float32, device=dev)
        d_pix = torch.zeros((3, spec.n_pixels), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()  # (torch fills on its own stream; the engine's streams do not wait for it)
        eng.heatmap_device(d_power.data_ptr(), spec.n_pixels, 3, d_peak.data_ptr(), d_pix.data_ptr())
        eng.synchronize()
        pix = d_pix.cpu().numpy()
        assert np.array_equal(d_peak.cpu().numpy(), power.max(axis=1))
        for b in range(2):
            assert np.array_equal(pix[b], oracle.heatmap_u8(power[b]))
            assert pix[b].max() == 255
        assert not power[2].any() and not pix[2].any()  # the all-zero frame: a black image, not garbage
        assert np.array_equal(pkg.binding.heatmap_u8(power[2]), pix[2])
        # externally supplied peak (what a rank does with the all-reduced maximum of all tiles)
        d_peak.fill_(float(2.0 * power[0].max()))
        torch.cuda.synchronize()
        eng.heatmap_device(d_power.data_ptr(), spec.n_pixels, 1, d_peak.data_ptr(), d_pix.data_ptr(), peak_given=True)
        eng.synchronize()
        want = np.clip(power[0].astype(np.float32) / np.float32(2.0 * power[0].max()) * 255.0, 0, 255).astype(np.uint8)
        assert np.array_equal(d_pix[0].cpu().numpy(), want)


def test_device_upscale_and_colour_table(pkg, oracle):
    """SURVEY 8f N2, second half: the display upscale of AWProcessingUnit::draw (aw_processing_unit.cpp:252)
    and the colour table of the GUI loop (main.cpp:345) on device images; bit-exact against the restated
    cv::resize arithmetic."""
    import torch

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(91)
    lut = torch.from_numpy(rng.integers(0, 256, (256, 3), dtype=np.uint8)).to(dev)
    with pkg.Engine(math=pkg.MATH_F32_FAST, n_streams=64, n_pixels=64, lut_stride=64) as eng:
        for (r, c, R, C_, batch) in [(16, 16, 64, 64, 3), (128, 128, 1024, 1024, 2), (12, 20, 50, 33, 1), (64, 64, 64, 64, 1)]:
            img = rng.integers(0, 256, (batch, r, c), dtype=np.uint8)
            d_img = torch.from_numpy(img).to(dev)
            d_out = torch.zeros((batch, R, C_), dtype=torch.uint8, device=dev)
            d_rgb = torch.zeros((batch, R, C_, 3), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()  # (torch fills on its own stream; the engine's streams do not wait for it)
            eng.upscale_device(d_img.data_ptr(), r, c, batch, d_out.data_ptr(), R, C_)
            eng.upscale_device(d_img.data_ptr(), r, c, batch, d_rgb.data_ptr(), R, C_, d_colormap_ptr=lut.data_ptr())
            eng.synchronize()
            for b in range(batch):
                want = oracle.resize_linear_u8(img[b], R, C_)
                assert np.array_equal(d_out[b].cpu().numpy(), want), (r, c, R, C_, b)
                assert np.array_equal(d_rgb[b].cpu().numpy(), lut.cpu().numpy()[want]), (r, c, R, C_, b)
        with pytest.raises(pkg.AwpuError):
            eng.upscale_device(d_img.data_ptr(), 64, 64, 1, d_out.data_ptr(), 32, 64)


def test_few_beam_das_for_trackers(pkg, oracle):
    """Particle::beam / Particle::das (particle.cpp:51-103) for a batch of steered directions
    in one launch.  Golden beams (made by the reference's delay()) bit-exact, powers to rounding; the
    same from a device snapshot and from the ingest ring."""
    import torch

    dev = torch.device("cuda:0")
    for name in ("beams_c1", "beams_c1_ragged"):
        g = np.load(GOLDEN / f"{name}.npz")
        X = util.hash_frames(64, 1024, seed=int(g["seed"]))[0]
        d_X = torch.from_numpy(X).to(dev)
        with pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=16) as eng:
            with pytest.raises(pkg.AwpuError) as ei:
                eng.beams(g["off"], g["frac"], d_X.data_ptr())
            assert ei.value.status == pkg.binding.ERR_STATE  # active mics not set
            eng.set_active_mics(g["index"])
            power, beams = eng.beams(g["off"], g["frac"], d_X.data_ptr())
            assert np.array_equal(beams, g["beams"])
            assert util.power_rel_err(power, g["power"]) < 2e-6
            p_only, none = eng.beams(g["off"][:3], g["frac"][:3], d_X.data_ptr(), want_beams=False)
            assert none is None and np.array_equal(p_only, power[:3])
            bad = g["off"].copy()
            bad[1, int(g["index"][0])] = 1024 - 256
            with pytest.raises(pkg.AwpuError) as ei:
                eng.beams(bad, g["frac"], d_X.data_ptr())
            assert ei.value.status == pkg.binding.ERR_RANGE
    # off the ingest ring: random int24 samples through the wire path, 100 random directions
    rng = np.random.default_rng(3)
    xyz = oracle.create_antenna()
    off, frac = pkg.steer_table(xyz, rng.uniform(0, 1.5, 100), rng.uniform(-np.pi, np.pi, 100))
    with pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=16) as eng:
        eng.set_active_mics(None)
        ring = np.zeros((64, 1024), np.float32)
        for b in range(5):
            stream = rng.integers(-(1 << 23), 1 << 23, (256, 256), dtype=np.int32)
            eng.ingest_block(make_datagrams(stream))
            ring = np.concatenate([ring[:, 256:], oracle.unpack_exposure(stream, 64)], axis=1)
        power, beams = eng.beams(off, frac)
        want_p, want_b = oracle.particle_beams(ring, off, frac)
        assert np.array_equal(beams, want_b)
        assert util.power_rel_err(power, want_p) < 2e-6


def test_device_calibration_equals_restated_loop(pkg, oracle):
    """AWProcessingUnit::calibrate (aw_processing_unit.cpp:102-212) with the mean squares
    computed on the device: same usable mics, bit-identical correction mask and median."""
    import torch

    dev = torch.device("cuda:0")
    X = util.hash_frames(128, 1024, seed=21, scale=2.0 ** -7)[0].copy()
    X[5] = 0.0            # dead
    X[17] *= 64.0         # far too loud
    X[64 + 9] *= 40.0     # second array: another loud one
    X[64 + 63] = 0.0
    d_X = torch.from_numpy(X).to(dev)
    with pkg.Engine(math=pkg.MATH_F32_FAST, n_streams=128, n_pixels=64, lut_stride=128) as eng:
        for array in range(2):
            index, corr, median = eng.calibrate_device(d_X.data_ptr(), array=array)
            want_index, want_corr, want_median = oracle.calibrate(X[64 * array: 64 * array + 64])
            assert np.array_equal(index, want_index) and index.size == 62
            assert np.array_equal(corr, want_corr) and median == want_median
        with pytest.raises(pkg.AwpuError):
            eng.calibrate_device(d_X.data_ptr(), array=2)
        with pytest.raises(pkg.AwpuError) as ei:
            eng.calibrate_ring()
        assert ei.value.status == pkg.binding.ERR_STATE


def test_mic_gains_equal_prescaled_frames(pkg, oracle):
    """The optional per-mic gain (the reference's unused power_correction_mask): a sweep with gains
    equals the oracle's sweep of frames scaled stream by stream, in every kernel shape."""
    S = pkg.synthetic
    spec = S.WORKLOADS["c1"]
    xyz = oracle.create_antenna()
    off, frac = oracle.compute_delay_lut(xyz, spec.res, spec.res)
    frames = S.make_frames(xyz, 4, seed=31)
    rng = np.random.default_rng(13)
    gains = rng.uniform(0.5, 2.0, 64).astype(np.float32)
    index = np.array([s for s in range(64) if s not in (3, 40)], np.int32)
    want = np.stack([oracle.das_f32(f * gains[:, None], off, frac, index) for f in frames])
    for math in (pkg.MATH_F32_EXACT, pkg.MATH_F32_FAST):
        with pkg.Engine(n_pixels=spec.n_pixels, math=math, max_batch=4) as eng:
            eng.set_delay_table(off, frac)
            eng.set_active_mics(index)
            eng.set_mic_gains(gains)
            for batch in (1, 4):  # single-frame and frame-pair shapes
                got = eng.process(frames[:batch])
                assert util.power_rel_err_unfloored(got, want[:batch]) <= util.POWER_RTOL, (math, batch)
            eng.set_mic_gains(None)  # off again = the reference
            plain = np.stack([oracle.das_f32(f, off, frac, index) for f in frames[:1]])
            assert util.power_rel_err_unfloored(eng.process(frames[:1]), plain) <= util.POWER_RTOL


def make_datagrams(stream_block, counter0=0, n_arrays=1):
    """256 wire datagrams (src/fpga/receiver.h:24-30: u16 frequency, u8 n_arrays, u8 version, u32 counter,
    i32 stream[256], packed) from stream_block[256 samples][256 channels] int32."""
    msg = np.zeros(256, dtype=np.dtype([("frequency", "<u2"), ("n_arrays", "u1"), ("version", "u1"),
                                        ("counter", "<u4"), ("stream", "<i4", (256,))]))
    assert msg.dtype.itemsize == 1032
    msg["frequency"] = 48828
    msg["n_arrays"] = n_arrays
    msg["version"] = 2
    msg["counter"] = counter0 + np.arange(256)
    msg["stream"] = stream_block
    return msg.tobytes()


def test_wire_ingest_and_ring_sweep(pkg, oracle):
    """Pipeline::receive_exposure (pipeline.cpp:260-297) + the stream ring on the device.
    Five blocks of raw datagrams go in -- the last two over a real UDP socket on loopback, as from
    the FPGA / udpreplay --; the ring snapshot must equal the restated unpacking bit for bit, and the
    sweep on it the oracle's."""
    import socket

    rng = np.random.default_rng(77)
    n = 64
    xyz = oracle.create_antenna()
    off, frac = oracle.compute_delay_lut(xyz, 12, 12)
    ring = np.zeros((n, 1024), np.float32)  # host model of the per-mic rings, oldest..newest after each roll
    rx = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    rx.bind(("127.0.0.1", 0))
    rx.settimeout(5.0)
    tx = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    with pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=off.shape[0], n_streams=n) as eng:
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        with pytest.raises(pkg.AwpuError):
            eng.process_ring()  # nothing ingested yet
        for b in range(5):
            stream = rng.integers(-(1 << 21), 1 << 21, size=(256, 256), dtype=np.int32)  # 24-bit samples
            wire = make_datagrams(stream, counter0=256 * b)
            if b >= 3:  # through the network stack, one datagram at a time like receive_message()
                got = bytearray()
                for i in range(256):
                    tx.sendto(wire[1032 * i:1032 * (i + 1)], rx.getsockname())
                    pkt = rx.recv(2048)
                    assert len(pkt) == 1032
                    got += pkt
                wire = bytes(got)
            eng.ingest_block(wire)
            block = oracle.unpack_exposure(stream, n)
            ring = np.concatenate([ring[:, 256:], block], axis=1)
            assert np.array_equal(eng.ring_snapshot(), ring), f"ring differs after block {b}"
        power = eng.process_ring()
        assert util.power_rel_err_unfloored(power, oracle.das_f32(ring, off, frac)) < util.POWER_RTOL
        # the ring path and the host-buffer path agree bit for bit on the same snapshot
        assert np.array_equal(power, eng.process(ring))
        # calibration straight off the ring (aw_processing_unit.cpp:102-212): random int24 noise is far
        # above the 1e-4 band, so what matters here is that all decisions equal the scalar loop's
        index, corr, median = eng.calibrate_ring()
        want_index, want_corr, want_median = oracle.calibrate(ring)
        assert np.array_equal(index, want_index) and np.array_equal(corr, want_corr) and median == want_median
    rx.close()
    tx.close()


def test_single_frames_on_the_headline_grid(pkg, oracle):
    """One frame per call on the full headline grid with the row length known -- the call MIMOWorker::update makes,
    and (from the ingest ring) the live path: the single-frame quad shape.  Host buffer, device ring and the
    batched call must agree with the oracle on every pixel (unfloored), and with each other to rounding."""
    S = pkg.synthetic
    spec = S.WORKLOADS["headline"]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    rng = np.random.default_rng(3)
    ring = np.zeros((spec.n_mics, 1024), np.float32)
    with pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=spec.n_pixels, n_streams=spec.n_mics, max_batch=2, grid_columns=spec.res) as eng:
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        for b in range(4):  # four blocks of 24-bit noise fill the ring
            stream = rng.integers(-(1 << 21), 1 << 21, size=(256, 256), dtype=np.int32)
            eng.ingest_block(make_datagrams(stream, counter0=256 * b, n_arrays=4))
            ring = np.concatenate([ring[:, 256:], oracle.unpack_exposure(stream, spec.n_mics)], axis=1)
        from_ring = eng.process_ring()
        from_host = eng.process(ring)
        batched = eng.process(np.stack([ring, 2.0 * ring]))
    assert np.array_equal(from_ring, from_host)  # same kernel, same bits, whichever way the frame came in
    assert util.power_rel_err(batched[0], from_host) < 5e-6 and np.array_equal(batched[1], 4.0 * batched[0])
    check_full_grid(oracle, from_host, ring, off, frac, "headline single frame (quad1 shape)")
    check_full_grid(oracle, batched[0], ring, off, frac, "headline pair of frames (quad shape)")


def test_reference_default_single_frames_run_the_resident_window_kernel(pkg, oracle):
    """The configuration the reference ships and runs live -- ONE 8x8 array, --mimo-res 100, one frame per
    MIMOWorker::update (src/main.cpp:38-41, worker.h:212-224): every mic's halves row fits the LDS at once, so the
    call runs das_quadh_stationary_kernel (the workgroup stages and filters the window itself: one launch, no pack
    pre-pass, no chunks).  Every pixel against the oracle, unfloored, for: a host frame, the same frame from the
    ingest ring (same kernel, other pitch: the same bits), a ragged mic list (51 of 64: padding mics), per-mic gains,
    a grid whose rows are no multiple of four and columns no multiple of 16 (90 x 70), and a call of two frames."""
    S = pkg.synthetic
    spec = S.WORKLOADS["ref_default"]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    names = pkg.binding.KERNEL_NAMES
    rng = np.random.default_rng(4)
    ring = np.zeros((64, 1024), np.float32)
    with pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=spec.n_pixels, n_streams=64, max_batch=2, grid_columns=spec.res) as eng:
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        for b in range(5):  # five blocks of 24-bit noise: the ring wraps once
            stream = rng.integers(-(1 << 21), 1 << 21, size=(256, 256), dtype=np.int32)
            eng.ingest_block(make_datagrams(stream, counter0=256 * b, n_arrays=1))
            ring = np.concatenate([ring[:, 256:], oracle.unpack_exposure(stream, 64)], axis=1)
        from_ring = eng.process_ring()
        assert names[eng.stats().kernel_variant] == "quadh_stationary"
        from_host = eng.process(ring)
        assert names[eng.stats().kernel_variant] == "quadh_stationary"
        assert np.array_equal(from_ring, from_host)
        check_full_grid(oracle, from_host, ring, off, frac, "reference default, one frame (resident-window kernel)")
        two = eng.process(np.stack([ring, 0.5 * ring]))
        check_full_grid(oracle, two[0], ring, off, frac, "reference default, first of two frames")
        assert util.power_rel_err_unfloored(two[1], 0.25 * two[0]) < 1e-6
        keep = np.sort(rng.choice(64, size=51, replace=False)).astype(np.int32)
        gains = rng.uniform(0.5, 2.0, 64).astype(np.float32)
        eng.set_active_mics(keep)
        eng.set_mic_gains(gains)
        ragged = eng.process(ring)
        assert names[eng.stats().kernel_variant] == "quadh_stationary"
        check_full_grid(oracle, ragged, ring * gains[:, None], off, frac, "reference default, 51 mics with gains", index=keep)
    X = S.make_frames(xyz, 1, seed=14)[0]
    off2, frac2 = pkg.build_delay_table(xyz, 90, 70, 120.0)
    with pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=90 * 70, n_streams=64, grid_columns=70) as eng:
        eng.set_delay_table(off2, frac2)
        eng.set_active_mics(None)
        odd = eng.process(X)
        assert names[eng.stats().kernel_variant] == "quadh_stationary"
    check_full_grid(oracle, odd, X, off2, frac2, "one array, 90 x 70 grid, fov 120")


def test_reference_order_mode_on_the_ingest_ring(pkg, oracle):
    """AWPU_MATH_F32_EXACT on the live path: frames read in place from the device ring (rows 2048 floats apart) through
    pack_pairs_kernel<false> and the reference-order kernels give the bits the host-buffer entry gives, and the oracle's powers;
    c2 geometry with the row length (one frame per call: das_exact_ndp_kernel on the halves form of the {next, d} layout) and without
    (das_exact_pair_kernel)."""
    S = pkg.synthetic
    spec = S.WORKLOADS["c2"]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    rng = np.random.default_rng(6)
    names = pkg.binding.KERNEL_NAMES
    forced = {"exact_quad": "exact_quad", "exact_pair": "exact_pair"}.get(os.environ.get("AWPU_SHAPE", ""))
    for cols, want in ((spec.res, forced or "exact_ndp"), (0, "exact_pair")):  # (one frame per call: the halves form of the {next, d} layout)
        ring = np.zeros((spec.n_mics, 1024), np.float32)
        with pkg.Engine(n_pixels=spec.n_pixels, n_streams=spec.n_mics, math=pkg.MATH_F32_EXACT, grid_columns=cols) as eng:
            eng.set_delay_table(off, frac)
            eng.set_active_mics(None)
            for b in range(5):
                stream = rng.integers(-(1 << 21), 1 << 21, size=(256, 256), dtype=np.int32)
                eng.ingest_block(make_datagrams(stream, counter0=256 * b, n_arrays=4))
                ring = np.concatenate([ring[:, 256:], oracle.unpack_exposure(stream, spec.n_mics)], axis=1)
            from_ring = eng.process_ring()
            assert names[eng.stats().kernel_variant] == want
            from_host = eng.process(ring)
        assert np.array_equal(from_ring, from_host)
        check_full_grid(oracle, from_ring, ring, off, frac, f"c2 off the ring, reference-order mode ({want})")


def test_two_handles_from_two_threads(pkg, oracle):
    """Several AWPUs in one process (the reference runs one per --port): two handles of different shapes used from two
    threads at the same time (ctypes drops the GIL during a call), first launches included -- the one-time kernel
    attribute set-up and the tuning knobs are process-wide.  Every result must equal the same handle's result alone."""
    import threading

    S = pkg.synthetic
    jobs = []
    for wl, batch, seed in (("c1", 6, 5), ("c2", 3, 6)):
        spec = S.WORKLOADS[wl]
        xyz = S.geometry(spec)
        off, frac = S.delay_table(spec, xyz)
        frames = util.hash_frames(spec.n_mics, 1024, seed=seed, batch=batch)
        jobs.append((spec, off, frac, frames, batch))
    results = [[], []]
    errors = []

    def work(k):
        try:
            spec, off, frac, frames, batch = jobs[k]
            with pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=spec.n_pixels, n_streams=spec.n_mics, max_batch=batch, grid_columns=spec.res) as eng:
                eng.set_delay_table(off, frac)
                eng.set_active_mics(None)
                for it in range(12):
                    results[k].append(eng.process(frames) if it % 2 == 0 else eng.process(frames[0])[None])
        except Exception as exc:  # noqa: BLE001
            errors.append(exc)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k in range(2):
        spec, off, frac, frames, batch = jobs[k]
        for it, got in enumerate(results[k]):
            ref = results[k][it % 2]
            assert np.array_equal(got, ref), (k, it)
        assert util.power_rel_err_unfloored(results[k][0][0], oracle.das_f32(frames[0], off, frac)) < util.POWER_RTOL
        assert util.power_rel_err_unfloored(results[k][1][0], oracle.das_f32(frames[0], off, frac)) < util.POWER_RTOL


def test_host_batches_upload_in_pieces(pkg, oracle):
    """awpu_hip_process uploads a batch of 64 frames or more in pieces beside the sweep (130 frames: pieces of 34, 34,
    34 and 28): every frame must come out as from the device-resident call on the whole batch, and as the oracle's."""
    import torch

    S = pkg.synthetic
    spec = S.WORKLOADS["c1"]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    frames = util.hash_frames(spec.n_mics, 1024, seed=77, batch=130)
    with pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=spec.n_pixels, n_streams=spec.n_mics, max_batch=130, grid_columns=spec.res) as eng:
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        host = eng.process(frames)
        assert eng.stats().last_kernel_ms > 0
        d_X = torch.from_numpy(frames).cuda()
        d_P = torch.zeros((130, spec.n_pixels), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        eng.process_device(d_X.data_ptr(), 130, d_P.data_ptr())
        eng.synchronize()
        again = eng.process(frames[:70])  # two pieces, an odd number of frame pairs in each
    assert util.power_rel_err(host, d_P.cpu().numpy()) < 2e-6
    assert np.array_equal(again, host[:70])
    for b in (0, 33, 34, 67, 101, 102, 129):
        assert util.power_rel_err_unfloored(host[b], oracle.das_f32(frames[b], off, frac)) < util.POWER_RTOL


def test_fir8_single_frames_on_the_headline_grid(pkg, oracle):
    """AWPU_INTERP_FIR8, one frame per call on the full headline grid: such a launch fills the chip, so it runs the
    batch kernel (das_fir8_plane_kernel) with the frame paired with itself.  From a host buffer, from the ingest
    ring (row pitch 2048) and as a member of a batch: the same powers to rounding, and the oracle's on every pixel."""
    S = pkg.synthetic
    spec = S.WORKLOADS["headline"]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    off = np.minimum(off, 1024 - 263).astype(np.int32)  # (the 8-tap variant reads 6 samples further than the table was made for)
    table = measured_fir_table()
    rng = np.random.default_rng(5)
    ring = np.zeros((spec.n_mics, 1024), np.float32)
    with pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=spec.n_pixels, n_streams=spec.n_mics, max_batch=3, grid_columns=spec.res,
                    interp=pkg.binding.INTERP_FIR8) as eng:
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        eng.set_fir_table(table)
        for b in range(4):
            stream = rng.integers(-(1 << 21), 1 << 21, size=(256, 256), dtype=np.int32)
            eng.ingest_block(make_datagrams(stream, counter0=256 * b, n_arrays=4))
            ring = np.concatenate([ring[:, 256:], oracle.unpack_exposure(stream, spec.n_mics)], axis=1)
        from_ring = eng.process_ring()
        from_host = eng.process(ring)
        batched = eng.process(np.stack([ring, 2.0 * ring, ring]))
    assert util.power_rel_err(from_ring, from_host) < 2e-6
    assert util.power_rel_err(batched[0], from_host) < 2e-6 and np.array_equal(batched[1], 4.0 * batched[0])
    assert util.power_rel_err(batched[2], from_host) < 2e-6  # the odd last frame of a batch
    check_full_grid(oracle, from_host, ring, off, frac, "headline FIR8 single frame", fir_table=table)
    check_full_grid(oracle, batched[2], ring, off, frac, "headline FIR8 odd last frame of a batch", fir_table=table)


@pytest.mark.parametrize("wl,batch", [("headline", 4), ("c3", 2)])
def test_full_size_properties(pkg, oracle, wl, batch):
    """BASELINE's full sizes (256 mics x 128x128, 512 mics x 128x128): EVERY pixel of the first and the last frame of
    the batch against the oracle, unfloored (the oracle takes 2.5 s / 5 s per whole frame here), with the row length
    given (quad shape) and without (pixel pairs), plus the size-independent properties:
      * frame 1 = 4 x frame 0  ->  power exactly 16 x (power-of-two scaling is exact in fp32)
      * the peak pixel looks at the plane-wave source."""
    S = pkg.synthetic
    spec = S.WORKLOADS[wl]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    frames = S.make_frames(xyz, batch, seed=3)
    frames[1] = 4.0 * frames[0]
    power, st = run_engine(pkg, frames, off, frac, grid_columns=spec.res)  # row length known: the quad shape where the
    assert st.usable == spec.n_mics                                        # table favours it, else vertical pixel pairs
    assert np.array_equal(power[1], 16.0 * power[0])
    plain, _ = run_engine(pkg, frames, off, frac)  # without the hint: consecutive pixels paired (another summation order)
    assert util.power_rel_err(plain, power) < 5e-6
    r, c = divmod(int(power[0].argmax()), spec.res)
    er, ec = S.source_pixel(spec)
    assert abs(r - er) <= 1 and abs(c - ec) <= 1
    for b in (0, batch - 1):
        check_full_grid(oracle, power[b], frames[b], off, frac, f"{wl} frame {b}, row length given")
        check_full_grid(oracle, plain[b], frames[b], off, frac, f"{wl} frame {b}, no row length")


def test_c4_rank_slab_of_eight(pkg, oracle):
    """BASELINE configs[3]/[4]: 512 mics x 256x256 sharded over 8 GPUs -- here the slab rank 5 would own
    (rows 160..191, 8192 pixels), a batch of 6 frames as one rank of a batched run would see them.
    Same size-independent properties as above plus the oracle on every pixel of the slab (unfloored); the second
    handle (rank 6's slab) shows that neighbouring slabs continue each other."""
    sharding = importlib.import_module("beamforming-lk_amd.sharding")
    S = pkg.synthetic
    spec = S.WORKLOADS["c4"]
    xyz = S.geometry(spec)
    frames = S.make_frames(xyz, 6, seed=9)
    frames[3] = -2.0 * frames[0]
    powers = []
    for rank in (5, 6):
        shard = sharding.shard_rows(spec.res, spec.res, 8, rank)
        assert (shard.row_count, shard.pixel_count) == (32, 8192)
        off, frac = S.delay_table(spec, xyz, shard.row_begin, shard.row_count)
        eng = pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=spec.n_pixels, n_streams=spec.n_mics, lut_stride=spec.n_mics, max_batch=6,
                         pixel_begin=shard.pixel_begin, pixel_count=shard.pixel_count, grid_columns=spec.res)
        with eng:
            eng.set_delay_table(off, frac)
            eng.set_active_mics(None)
            power = eng.process(frames)
        assert power.shape == (6, 8192)
        assert np.array_equal(power[3], 4.0 * power[0])
        for b in (0, 5):
            check_full_grid(oracle, power[b], frames[b], off, frac, f"c4 slab of rank {rank}, frame {b}")
        powers.append(power)
    # the last row of one slab and the first row of the next are neighbouring grid rows: smooth across the seam
    seam = np.abs(powers[0][0, -256:] - powers[1][0, :256]) / powers[0][0].max()
    assert seam.max() < 0.25


GROUP_CHILD = r"""
import importlib, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import util
pkg = importlib.import_module("beamforming-lk_amd")
S = pkg.synthetic
spec = S.WORKLOADS["c2"]
xyz = S.geometry(spec)
off, frac = S.delay_table(spec, xyz)
frames = S.make_frames(xyz, 6, seed=21)
import os
EXACT = os.environ.get("AWPU_SHAPE") == "noquad"
def run(devices, batch, **kw):
    with pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=spec.n_pixels, n_streams=spec.n_mics, max_batch=8, grid_columns=spec.res, devices=devices, **kw) as eng:
        eng.set_delay_table(off, frac); eng.set_active_mics(None)
        host = eng.process(frames[:batch])
        d_X = torch.from_numpy(frames[:batch]).cuda(); d_P = torch.zeros((batch, spec.n_pixels), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        for _ in range(3):  # three calls back to back: both fan-out buffers of every part get reused
            eng.process_device(d_X.data_ptr(), batch, d_P.data_ptr(), st.cuda_stream)
        st.synchronize(); eng.synchronize()
        dev = d_P.cpu().numpy()
        wire = util_wire()
        for b in range(4): eng.ingest_block(wire[b])
        ring = eng.process_ring(); snap = eng.ring_snapshot(); stats = eng.stats()
    return host, dev, ring, snap, stats
def util_wire():
    rng = np.random.default_rng(9); out = []
    for b in range(4):
        msg = np.zeros(256, dtype=np.dtype([("frequency", "<u2"), ("n_arrays", "u1"), ("version", "u1"), ("counter", "<u4"), ("stream", "<i4", (256,))]))
        msg["n_arrays"] = 4; msg["stream"] = rng.integers(-(1 << 21), 1 << 21, size=(256, 256), dtype=np.int32); out.append(msg.tobytes())
    return out
for batch in (1, 6):
    one = run(None, batch)
    for devices in ([0, 0], [0, 0, 0]):
        grp = run(devices, batch)
        for name, a, b in zip(("host", "device", "ring", "snapshot"), one[:4], grp[:4]):
            # the same bits where the slabs run the kernel shapes the whole grid runs (the shapes of round 1 do not
            # depend on the slab: AWPU_SHAPE=noquad); a small slab may pick another shape than the whole grid, and
            # the quad shapes differ from the others by rounding
            if EXACT or name == "snapshot":
                assert np.array_equal(a, b), (name, devices, batch)
            else:
                assert util.power_rel_err(b, a) < 5e-6, (name, devices, batch)
        assert grp[4].frames == one[4].frames and grp[4].usable == one[4].usable and grp[4].alg_flops_frame == one[4].alg_flops_frame
staged = os.environ.get("AWPU_GROUP_FORCE_COPY") == "2"
with pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=spec.n_pixels, n_streams=spec.n_mics, grid_columns=spec.res, devices=[0, 0, 0]) as eng:
    want = pkg.binding.PEER_HOST_STAGED if staged else pkg.binding.PEER_SAME_DEVICE
    assert eng.peer_status() == [want] * 3, eng.peer_status()
    assert "pinned host memory" not in eng.last_error()  # (equal ordinals have nothing to report; real pairs without peer access do)
with pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=spec.n_pixels, n_streams=spec.n_mics) as eng:
    assert eng.peer_status() == [pkg.binding.PEER_SAME_DEVICE]
# uneven slabs (64 rows over 3 devices = 22 + 21 + 21) and a group that owns only part of the grid
with pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=spec.n_pixels, n_streams=spec.n_mics, grid_columns=spec.res, devices=[0, 0], pixel_begin=10 * spec.res, pixel_count=7 * spec.res) as eng:
    eng.set_delay_table(off[10 * spec.res:17 * spec.res], frac[10 * spec.res:17 * spec.res]); eng.set_active_mics(None)
    assert util.power_rel_err(eng.process(frames[0]), run(None, 1)[0][0][10 * spec.res:17 * spec.res]) < (1e-12 if EXACT else 5e-6)
try:
    pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=4, devices=list(range(9)))
except pkg.AwpuError as e:
    assert e.status == pkg.binding.ERR_INVALID
else:
    raise SystemExit("9 devices accepted")
print("GROUP OK")
"""


@pytest.mark.parametrize("force_copy,quads", [("0", "noquad"), ("1", "noquad"), ("2", "noquad"), ("0", ""), ("1", ""), ("2", "")])
def test_device_group_equals_one_device(force_copy, quads):
    """awpu_hip_cfg.n_devices > 1 (the multi-GPU split under the C ABI): a handle that spreads the grid's rows over
    two / three engines -- here all on the one GPU of the box, the same code path with devices[k] equal -- gives
    the bits of the single-device handle through the host entry, the device-pointer entry (three calls back to
    back) and the ingest ring, for one frame and for a batch (quads="noquad": with the kernel shapes that do not depend
    on the slab; otherwise to rounding, a small slab may run another shape than the whole grid).  force_copy=1 makes
    every part take the copy path of the fan-out (2-D window copies, two buffers per part, events between the copy
    and the sweep streams) that a part on another GPU takes; force_copy=2 the path of a node WITHOUT peer access: the
    window goes down to pinned host memory once and up to every part, the tiles come back the same way
    (awpu_hip_group_peer_status then reports AWPU_PEER_HOST_STAGED for every device)."""
    import os, subprocess, sys
    env = dict(os.environ, AWPU_GROUP_FORCE_COPY=force_copy)
    if quads:
        env["AWPU_SHAPE"] = quads
    out = subprocess.run([sys.executable, "-c", GROUP_CHILD, str(Path(__file__).resolve().parent.parent)],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "GROUP OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]


GROUP_PACKED_CHILD = r"""
import importlib, os, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import util
pkg = importlib.import_module("beamforming-lk_amd")
B = pkg.binding
S = pkg.synthetic
spec = S.WORKLOADS["headline"]
xyz = S.geometry(spec)
off, frac = S.delay_table(spec, xyz)
frames = util.hash_frames(spec.n_mics, 1024, seed=31, batch=10)
MODE, KERNEL = (pkg.MATH_F32_FAST, "quad") if os.environ.get("TEST_MATH") == "fast" else (pkg.MATH_F32_EXACT, "exact_nd")
def run(devices, batch, index=None):
    with pkg.Engine(math=MODE, n_pixels=spec.n_pixels, n_streams=spec.n_mics, max_batch=10, grid_columns=spec.res, devices=devices) as eng:
        eng.set_delay_table(off, frac); eng.set_active_mics(index)
        d_X = torch.from_numpy(frames[:batch]).cuda(); d_P = torch.zeros((batch, spec.n_pixels), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        for _ in range(4):  # four calls back to back: both packed buffers, both receive buffers and their events get reused
            eng.process_device(d_X.data_ptr(), batch, d_P.data_ptr(), st.cuda_stream)
        st.synchronize(); eng.synchronize()
        stats = eng.stats()
        host = eng.process(frames[:batch])
    return d_P.cpu().numpy(), host, stats
one = run(None, 10)
assert B.KERNEL_NAMES[one[2].kernel_variant] == KERNEL
for devices in ([0, 0], [0, 0, 0, 0]):
    grp = run(devices, 10)
    assert grp[2].group_exchange == B.EXCHANGE_PACKED_PAIRS, grp[2].group_exchange
    assert grp[2].group_ranges == 32 // len(devices)  # 32 groups of four rows dealt round-robin
    assert np.array_equal(grp[0], one[0]), devices     # the same quads of the same packed samples through the same kernel: the same bits
    assert np.array_equal(grp[1], one[1]), devices     # (host entry: every part uploads the union window and sweeps on its own)
# a single frame, and a ragged mic list (usable % 4 != 0): raw windows travel, every part runs its whole sweep
grp1 = run([0, 0], 1)
assert grp1[2].group_exchange == B.EXCHANGE_WINDOWS
assert util.power_rel_err(grp1[0], run(None, 1)[0]) < 5e-6
keep = np.array([m for m in range(spec.n_mics) if m % 9 != 2], np.int32)
grp2 = run([0, 0, 0], 10, keep)
assert grp2[2].group_exchange == B.EXCHANGE_WINDOWS and grp2[2].group_ranges == 32 // 3 + 1
assert util.power_rel_err(grp2[0], run(None, 10, keep)[0]) < 5e-6
# the reference-order mode through a group, an ODD batch: the {next, d} rows travel (the last pair a frame with itself), every part
# runs das_exact_nd_kernel on its row groups -- the same quads in the same order as one device: the same bits
def run_exact(devices):
    with pkg.Engine(n_pixels=spec.n_pixels, n_streams=spec.n_mics, max_batch=3, grid_columns=spec.res, devices=devices, math=pkg.MATH_F32_EXACT) as eng:
        eng.set_delay_table(off, frac); eng.set_active_mics(None)
        d_X = torch.from_numpy(frames[:3]).cuda(); d_P = torch.zeros((3, spec.n_pixels), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        eng.process_device(d_X.data_ptr(), 3, d_P.data_ptr()); eng.synchronize()
        return d_P.cpu().numpy(), eng.stats()
e1, eg = run_exact(None), run_exact([0, 0, 0])
assert B.KERNEL_NAMES[e1[1].kernel_variant] == "exact_nd" and eg[1].group_exchange == B.EXCHANGE_PACKED_PAIRS
assert np.array_equal(e1[0], eg[0])
# one group handle re-targeted: the union window of the first table does not outlive it (a narrower second table gets its
# own, narrower union -- and the same bits as a fresh single-device handle on that table)
off_b = (off.max() + off.min() - off).astype(off.dtype); frac_b = np.ascontiguousarray(frac[::-1])
off_n = np.clip(off, off.min(), off.min() + 8).astype(off.dtype)
def sweep_tables(devices, tables):
    res = []
    with pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=spec.n_pixels, n_streams=spec.n_mics, max_batch=10, grid_columns=spec.res, devices=devices) as eng:
        eng.set_active_mics(None)
        d_X = torch.from_numpy(frames).cuda(); d_P = torch.zeros((10, spec.n_pixels), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for o, f in tables:
            eng.set_delay_table(o, f)
            eng.process_device(d_X.data_ptr(), 10, d_P.data_ptr()); eng.synchronize()
            st = eng.stats()
            res.append((d_P.cpu().numpy().copy(), st.window))
    return res
tables = [(off, frac), (off_b, frac_b), (off_n, frac), (off, frac)]
grp = sweep_tables([0, 0], tables)
for k, (o, f) in enumerate(tables):
    fresh = sweep_tables(None, [(o, f)])[0]
    assert np.array_equal(grp[k][0], fresh[0]), k
    assert grp[k][1] == fresh[1], (k, grp[k][1], fresh[1])
assert grp[2][1] < grp[0][1]   # the narrow table's window IS narrower
print("GROUP PACKED OK")
"""


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("force_copy", ["0", "1", "2"])
def test_device_group_exchanges_packed_frame_pairs(force_copy, math):
    """Round 4: the in-process device group on the exchange format of the one-process-per-GPU path.  A batch that the parts
    sweep with a frame-pair shape travels as PACKED frame pairs -- devices[0] runs the pack pass once, every other part gets
    one linear copy (force_copy=1: the peer-copy path; 2: through pinned host memory; 0: parts on devices[0] sweep the
    group's packed buffer in place) -- and the grid's rows are dealt to the parts in groups of four, round-robin.  The
    assembled heatmaps equal the single-device handle's BIT FOR BIT (the same quads of the same packed samples through the
    same kernel); single frames and mic lists that are no multiple of four fall back to raw windows, to rounding.
    Round 5: in BOTH math modes -- the reference's order (the default) exchanges the {next, d} rows das_exact_nd_kernel sweeps."""
    import os, subprocess, sys
    env = dict(os.environ, AWPU_GROUP_FORCE_COPY=force_copy, TEST_MATH=math)
    out = subprocess.run([sys.executable, "-c", GROUP_PACKED_CHILD, str(Path(__file__).resolve().parent.parent)],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "GROUP PACKED OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]


GROUP_TWO_DEVICES_CHILD = r"""
import importlib, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import util
pkg = importlib.import_module("beamforming-lk_amd")
S = pkg.synthetic
spec = S.WORKLOADS["c2"]
xyz = S.geometry(spec)
off, frac = S.delay_table(spec, xyz)
frames = S.make_frames(xyz, 6, seed=23)
def run(devices):
    with pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=spec.n_pixels, n_streams=spec.n_mics, max_batch=8, grid_columns=spec.res, devices=devices) as eng:
        eng.set_delay_table(off, frac); eng.set_active_mics(None)
        host = eng.process(frames)
        d_X = torch.from_numpy(frames).cuda(0); d_P = torch.zeros((6, spec.n_pixels), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        st = torch.cuda.Stream(device=0)
        for _ in range(4):  # four calls back to back: both staging buffers, both tile buffers and their events get reused
            eng.process_device(d_X.data_ptr(), 6, d_P.data_ptr(), st.cuda_stream)
        st.synchronize(); eng.synchronize()
        return host, d_P.cpu().numpy(), eng.peer_status(), eng.last_error()
one = run(None)
two = run([0, 1])
print("peer status", two[2], two[3])
for a, b in zip(one[:2], two[:2]):
    assert util.power_rel_err(b, a) < 5e-6
print("GROUP2 OK")
"""


@pytest.mark.parametrize("force_copy", ["0", "2"])
def test_device_group_on_two_distinct_devices(force_copy):
    """The device group on two DIFFERENT GPUs (skipped on a one-GPU box): direct peer copies (force_copy=0, where the node
    grants peer access) and the host-staged path (force_copy=2), whose events cross devices -- ev_tile_free[] is recorded on
    the caller's stream (devices[0]) and must have been created there (round-3 advisor finding: it was created on the
    part's device, which equal ordinals cannot show)."""
    import os, subprocess, sys
    import torch

    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    env = dict(os.environ, AWPU_GROUP_FORCE_COPY=force_copy)
    out = subprocess.run([sys.executable, "-c", GROUP_TWO_DEVICES_CHILD, str(Path(__file__).resolve().parent.parent)],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "GROUP2 OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]


def test_bf16_accumulator_mode(pkg, oracle):
    """AWPU_MATH_BF16_ACC (BASELINE configs[4], "bf16 vs fp32 accumulator"): the device keeps the running sums in
    bf16 exactly as the restatement does (same operations in the same order: the pre-epilogue sums are the same
    bits, the power agrees to the epilogue's summation order), and the distance to the fp32 result is the
    percent-level error the mode is known for -- reported, not gated to 1e-5."""
    S = pkg.synthetic
    spec = S.WORKLOADS["c1"]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    frames = S.make_frames(xyz, 2, seed=12)
    eng = pkg.Engine(n_pixels=spec.n_pixels, math=pkg.MATH_BF16_ACC, max_batch=2)
    with eng:
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        power = eng.process(frames)
    for b in range(2):
        assert util.power_rel_err(power[b], oracle.das_bf16acc(frames[b], off, frac)) < 2e-6
        err = util.power_rel_err(power[b], oracle.das_f32(frames[b], off, frac))
        assert 1e-4 < err < 1e-1, err
    with pytest.raises(pkg.AwpuError):  # the mode exists for the linear interpolation only
        pkg.Engine(n_pixels=16, math=pkg.MATH_BF16_ACC, interp=pkg.binding.INTERP_FIR8)


def test_c5_1024_frames_512_mics_rank_slab(pkg, oracle):
    """BASELINE configs[4] at its real size on one rank: 1024 frames in flight x 512 mics x the slab of a
    256x256 grid that one of 8 GPUs owns (32 rows, 8192 pixels) -- one call, 512 frame pairs.  The oracle checks
    every pixel of the first, a middle and the last frame (unfloored); frames that repeat give the same bits wherever
    they sit in the batch; the bf16-accumulator mode is run on the same call and its error recorded."""
    sharding = importlib.import_module("beamforming-lk_amd.sharding")
    S = pkg.synthetic
    spec = S.WORKLOADS["c4"]
    xyz = S.geometry(spec)
    shard = sharding.shard_rows(spec.res, spec.res, 8, 3)
    off, frac = S.delay_table(spec, xyz, shard.row_begin, shard.row_count)
    B = 1024
    distinct = np.concatenate([util.hash_frames(spec.n_mics, 1024, seed=70 + k, batch=16) for k in range(4)])  # 64 frames
    frames = np.empty((B, spec.n_mics, 1024), np.float32)  # 2.1 GB
    for k in range(B // 64):
        frames[64 * k:64 * (k + 1)] = distinct
    del distinct
    eng = pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=spec.n_pixels, n_streams=spec.n_mics, lut_stride=spec.n_mics, max_batch=B,
                     pixel_begin=shard.pixel_begin, pixel_count=shard.pixel_count, grid_columns=spec.res)
    with eng:
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        power = eng.process(frames)
        st = eng.stats()
    assert power.shape == (B, 8192) and st.usable == 512 and st.frames == B
    for b in (0, 511, 1023):
        check_full_grid(oracle, power[b], frames[b], off, frac, f"c5 slab, frame {b} of 1024")
    assert np.array_equal(power[64:128], power[:64]) and np.array_equal(power[960:], power[:64])
    # the same call with the bf16 accumulator (a slower kernel: 64 frames of the batch are enough)
    eng = pkg.Engine(n_pixels=spec.n_pixels, n_streams=spec.n_mics, lut_stride=spec.n_mics, max_batch=64,
                     math=pkg.MATH_BF16_ACC, pixel_begin=shard.pixel_begin, pixel_count=shard.pixel_count)
    with eng:
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        p16 = eng.process(frames[:64])
    err = util.power_rel_err(p16, power[:64])
    print(f"c5 bf16-accumulator max rel err vs the fp32 sweep: {err:.3e}")
    assert 1e-4 < err < 1e-1
    assert util.power_rel_err_unfloored(p16[63], oracle.das_bf16acc(frames[63], off, frac)) < 2e-6  # (its own checker, every pixel)


def test_1024_frames_in_flight(pkg, oracle):
    """BASELINE configs[4] batches 1024 frames per step: one call, 512 frame pairs (c1 geometry so that the
    oracle can check whole frames): first, last and two middle frames against the oracle, and repeated frames
    against each other."""
    S = pkg.synthetic
    spec = S.WORKLOADS["c1"]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    frames = np.tile(util.hash_frames(64, 1024, seed=40, batch=8), (128, 1, 1))  # 8 distinct frames, repeated
    assert frames.shape == (1024, 64, 1024)
    power, _ = run_engine(pkg, frames, off, frac)
    for b in (0, 511, 512, 1023):
        want = oracle.das_f32(frames[b], off, frac)
        assert util.power_rel_err_unfloored(power[b], want) < util.POWER_RTOL
    # frames repeat every 8: the same frame gives the same bits wherever it sits in the batch ...
    assert np.array_equal(power[8:16], power[:8]) and np.array_equal(power[1016:], power[:8])
    # ... and agrees with the small-batch call (a different kernel shape: other summation order)
    few, _ = run_engine(pkg, frames[:8], off, frac)
    assert util.power_rel_err(power[:8], few) < 2e-6


def test_live_block_equals_the_separate_steps(pkg, oracle):
    """awpu_hip_live_block = ingest_block + process_ring + populateHeatmap + cv::resize in one call: same
    power bits, same images as the separate entry points (and therefore as the restatements)."""
    import torch

    rng = np.random.default_rng(55)
    xyz = oracle.create_antenna()
    off, frac = oracle.compute_delay_lut(xyz, 16, 16)
    blocks = [make_datagrams(rng.integers(-(1 << 23), 1 << 23, (256, 256), dtype=np.int32), counter0=256 * b) for b in range(6)]
    lut = torch.from_numpy(rng.integers(0, 256, (256, 3), dtype=np.uint8)).to("cuda:0")
    with pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=256) as one, pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=256) as sep:
        for eng in (one, sep):
            eng.set_delay_table(off, frac)
            eng.set_active_mics(None)
        for b, wire in enumerate(blocks):
            power, image, big = one.live_block(wire, 16, 16, 64, 48)
            sep.ingest_block(wire)
            want_power = sep.process_ring()
            assert np.array_equal(power, want_power), b
            assert np.array_equal(image.ravel(), oracle.heatmap_u8(want_power)), b
            assert np.array_equal(big, oracle.resize_linear_u8(image, 64, 48)), b
        _, image, rgb = one.live_block(blocks[0], 16, 16, 32, 32, d_colormap_ptr=lut.data_ptr(), want_power=False)
        assert np.array_equal(rgb, lut.cpu().numpy()[oracle.resize_linear_u8(image, 32, 32)])
        with pytest.raises(pkg.AwpuError):
            one.live_block(blocks[0], 8, 16)  # rows x cols is not the grid


def test_live_block_replayed_as_a_graph(pkg, oracle):
    """A display loop keeps its buffers: the receive buffer is refilled in place and the images land in the same
    arrays block after block.  From the third such call on awpu_hip_live_block replays one captured HIP graph per
    ring position (eight of them) -- the copies in it must read the buffer's CURRENT contents, and a new delay table
    must retire the graphs.  24 blocks against the separate entry points, then a table change and 10 more."""
    rng = np.random.default_rng(56)
    xyz = oracle.create_antenna()
    off, frac = oracle.compute_delay_lut(xyz, 16, 16)
    off2, frac2 = oracle.compute_delay_lut(xyz, 16, 16, fov_deg=90.0)
    wire = np.zeros(256 * 1032, np.uint8)
    out = (np.zeros(256, np.float32), np.zeros((16, 16), np.uint8), np.zeros((40, 56), np.uint8))
    with pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=256) as one, pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=256) as sep:
        for eng in (one, sep):
            eng.set_delay_table(off, frac)
            eng.set_active_mics(None)
        for b in range(34):
            if b == 24:
                for eng in (one, sep):
                    eng.set_delay_table(off2, frac2)
            block = make_datagrams(rng.integers(-(1 << 23), 1 << 23, (256, 256), dtype=np.int32), counter0=256 * b)
            wire[:] = np.frombuffer(block, np.uint8)
            power, image, big = one.live_block(wire, 16, 16, 40, 56, out=out)
            assert power is out[0] and image is out[1] and big is out[2]
            sep.ingest_block(block)
            want_power = sep.process_ring()
            assert np.array_equal(power, want_power), b
            assert np.array_equal(image.ravel(), oracle.heatmap_u8(want_power)), b
            assert np.array_equal(big, oracle.resize_linear_u8(image, 40, 56)), b


@pytest.mark.parametrize("math", MATHS)
def test_packed_frames_split_the_sweep_at_its_pack_pass(pkg, oracle, math):
    """awpu_hip_pack_frames + awpu_hip_process_packed = awpu_hip_process_device, bit for bit: the multi-GPU exchange
    format (the ingest rank packs once, every rank sweeps the packed pairs as they arrive).  Quad shape (row length
    given), pair shape (not given), an odd batch; a handle created with a wider staging window than its table needs
    (cfg.window_begin/window_end: the union over all ranks' slabs) returns the same bits as one without.
    Round 5: the reference's order too -- the packed rows are then the {next, d} elements of das_exact_nd_kernel (which needs the
    grid's row length: without it the entry points say so and nothing is packed)."""
    import torch

    exact = math == "exact"

    S = pkg.synthetic
    spec = S.WORKLOADS["c2"]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    frames = S.make_frames(xyz, 11, seed=44)
    d_X = torch.from_numpy(frames).cuda()
    want0 = None
    for hint, window in ((spec.res, None), (0, None), (spec.res, (int(off.min()) - 20, int(off.max()) + 257 + 9))):
        for batch in (10, 11, 2):  # 5 and 6 frame pairs x 64 tiles fill the chip; a batch of 2 does not
            with pkg.Engine(math=math_id(pkg, math), n_pixels=spec.n_pixels, n_streams=spec.n_mics, max_batch=12, grid_columns=hint, window=window) as eng:
                eng.set_delay_table(off, frac)
                eng.set_active_mics(None)
                if exact and not hint:
                    with pytest.raises(pkg.AwpuError) as ei:
                        eng.packed_bytes(batch)
                    assert ei.value.status == pkg.binding.ERR_STATE
                    continue
                n = eng.packed_bytes(batch)
                assert n % 8 == 0 and n >= ((batch + 1) // 2) * spec.n_mics * 257 * 8
                d_pk = torch.zeros(n // 4, dtype=torch.float32, device="cuda")
                d_a = torch.zeros((batch, spec.n_pixels), dtype=torch.float32, device="cuda")
                d_b = torch.zeros_like(d_a)
                torch.cuda.synchronize()
                st = torch.cuda.Stream()
                eng.pack_frames(d_X.data_ptr(), batch, d_pk.data_ptr(), st.cuda_stream)
                eng.process_packed(d_pk.data_ptr(), batch, d_a.data_ptr(), st.cuda_stream)
                eng.process_device(d_X.data_ptr(), batch, d_b.data_ptr(), st.cuda_stream)
                st.synchronize()
                eng.synchronize()
            a, b = d_a.cpu().numpy(), d_b.cpu().numpy()
            if batch >= 10 or exact:  # process_device sweeps frame pairs itself: the same kernel on the same packed samples
                assert a.max() > 0 and np.array_equal(a, b), (hint, window, batch)
            else:            # process_device prefers a single-frame shape for so small a launch: equal to rounding (two
                # shapes, each within a few 1e-6 of the reference: 2.0e-6 apart on these frames)
                assert util.power_rel_err(a, b) < 4e-6, (hint, window, batch)
            if batch == 10 and hint:
                if want0 is None:
                    want0 = a
                    check_full_grid(oracle, a[0], frames[0], off, frac, f"c2 through pack_frames + process_packed ({math})")
                else:
                    assert np.array_equal(a, want0), "a wider staging window changed the bits"
    # a mic list that is not a multiple of four has no common packed layout: the caller is told, nothing is computed
    with pkg.Engine(math=math_id(pkg, math), n_pixels=spec.n_pixels, n_streams=spec.n_mics, max_batch=4, grid_columns=spec.res) as eng:
        eng.set_delay_table(off, frac)
        eng.set_active_mics(np.arange(253, dtype=np.int32))
        with pytest.raises(pkg.AwpuError) as ei:
            eng.packed_bytes(4)
        assert ei.value.status == pkg.binding.ERR_STATE
    with pytest.raises(pkg.AwpuError):
        pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=16, window=(900, 1000))  # narrower than one delay() read


def test_interleaved_row_groups_tile_the_headline_grid(pkg, oracle):
    """The N-GPU decomposition bench.py runs: row groups of four dealt round-robin over 8 ranks (every rank gets edge and
    centre rows alike), every rank staging the union window, rank 0 packing once and every rank sweeping the SAME
    packed buffer.  Here the 8 ranks run one after the other on one GPU: their tiles, put back where row_ranges says,
    equal the single-handle heatmap on every pixel to rounding, and the oracle's (unfloored)."""
    import torch

    sharding = importlib.import_module("beamforming-lk_amd.sharding")
    S = pkg.synthetic
    spec = S.WORKLOADS["headline"]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    frames = S.make_frames(xyz, 4, seed=61)
    whole, _ = run_engine(pkg, frames, off, frac, grid_columns=spec.res)
    window = (int(off.min()), int(off.max()) + 257)
    shards = sharding.all_shards(spec.res, spec.res, 8, interleaved=True)
    assert all(s.row_count == 16 and len(s.row_ranges) == 4 for s in shards) and shards[3].row_ranges[1] == (44, 4)
    d_X = torch.from_numpy(frames).cuda()
    d_pk, tiles = None, []
    for s in shards:
        o, f = S.delay_table_for(spec, xyz, s.row_ranges)
        rows = np.array(s.rows())
        assert np.array_equal(o, off.reshape(spec.res, spec.res, -1)[rows].reshape(-1, spec.n_mics))
        with pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=spec.n_pixels, n_streams=spec.n_mics, max_batch=4, pixel_begin=s.pixel_begin,
                        pixel_count=s.pixel_count, grid_columns=spec.res, window=window) as eng:
            eng.set_delay_table(o, f)
            eng.set_active_mics(None)
            if d_pk is None:  # "rank 0" packs; the others never see the raw frames
                d_pk = torch.zeros(eng.packed_bytes(4) // 4, dtype=torch.float32, device="cuda")
                eng.pack_frames(d_X.data_ptr(), 4, d_pk.data_ptr())
                eng.synchronize()
            d_P = torch.zeros((4, s.pixel_count), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            eng.process_packed(d_pk.data_ptr(), 4, d_P.data_ptr())
            eng.synchronize()
        tiles.append(d_P.cpu())
    full = sharding.assemble_tiles(tiles, shards).numpy()
    assert full.shape == whole.shape and util.power_rel_err(full, whole) < 5e-6
    check_full_grid(oracle, full[0], frames[0], off, frac, "headline assembled from 8 interleaved ranks")
    check_full_grid(oracle, full[3], frames[3], off, frac, "headline assembled from 8 interleaved ranks, frame 3")


def test_live_graphs_are_retired_when_their_buffers_move(pkg, oracle):
    """The captured live-block graphs bake in device pointers of the handle (power, display, upscale taps, FIR tables).
    Calls that free or reallocate one of them -- a batched awpu_hip_process on a max_batch > 1 handle (d_power grows), a
    live call with a larger upscale (d_display, d_taps), awpu_hip_upscale_u8_device with other dimensions (d_taps),
    awpu_hip_set_fir_table -- must retire the graphs: the display loop goes on, interleaved with all of them, and every
    block still equals the separate entry points."""
    import torch

    rng = np.random.default_rng(57)
    xyz = oracle.create_antenna()
    off, frac = oracle.compute_delay_lut(xyz, 16, 16)
    wire = np.zeros(256 * 1032, np.uint8)
    out_a = (np.zeros(256, np.float32), np.zeros((16, 16), np.uint8), np.zeros((40, 56), np.uint8))
    out_b = (np.zeros(256, np.float32), np.zeros((16, 16), np.uint8), np.zeros((96, 80), np.uint8))
    frames = util.hash_frames(64, 1024, seed=3, batch=4)
    d_pix = torch.zeros((16, 16), dtype=torch.uint8, device="cuda:0")
    d_up = torch.zeros((33, 47), dtype=torch.uint8, device="cuda:0")
    for interp in (pkg.binding.INTERP_LERP, pkg.binding.INTERP_FIR8):
        fir = interp == pkg.binding.INTERP_FIR8
        o = np.minimum(off, 1024 - 263).astype(np.int32) if fir else off
        with pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=256, max_batch=4, interp=interp) as one, pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=256, interp=interp) as sep:
            for eng in (one, sep):
                eng.set_delay_table(o, frac)
                eng.set_active_mics(None)
                if fir:
                    eng.set_fir_table(util.synthetic_fir_table())
            b = 0

            def live(out, rows_cols):
                nonlocal b
                block = make_datagrams(rng.integers(-(1 << 23), 1 << 23, (256, 256), dtype=np.int32), counter0=256 * b)
                wire[:] = np.frombuffer(block, np.uint8)
                power, image, big = one.live_block(wire, 16, 16, *rows_cols, out=out)
                sep.ingest_block(block)
                want = sep.process_ring()
                assert np.array_equal(power, want), b
                assert np.array_equal(image.ravel(), oracle.heatmap_u8(want)), b
                assert np.array_equal(big, oracle.resize_linear_u8(image, *rows_cols)), b
                b += 1

            for _ in range(5):
                live(out_a, (40, 56))           # warm, captured, replayed
            p4 = one.process(frames)             # (1) d_power grows from 256 to 4 x 256 floats
            assert p4.shape == (4, 256) and util.power_rel_err(p4[0], sep.process(frames[0])) < 2e-6
            for _ in range(5):
                live(out_a, (40, 56))           # the old key matches again: must not replay a stale graph
            for _ in range(4):
                live(out_b, (96, 80))           # (2) a larger display image and other taps
            for _ in range(4):
                live(out_a, (40, 56))           # back to the first shape: its graphs were retired with the buffers
            one.upscale_device(d_pix.data_ptr(), 16, 16, 1, d_up.data_ptr(), 33, 47)  # (3) the taps move again
            one.synchronize()
            for _ in range(4):
                live(out_a, (40, 56))
            if fir:
                for eng in (one, sep):          # (4) a new coefficient table: the plane entries are rebuilt
                    eng.set_fir_table(util.synthetic_fir_table()[::-1].copy())
                for _ in range(4):
                    live(out_a, (40, 56))


def test_calls_refused_while_an_async_call_is_in_flight(pkg, oracle):
    """awpu_hip_process, awpu_hip_calibrate_host and awpu_hip_live_block share the staging and power buffers of an
    awpu_hip_process_async that has not been waited for: AWPU_ERR_STATE until awpu_hip_wait, then they work."""
    xyz = oracle.create_antenna()
    off, frac = oracle.compute_delay_lut(xyz, 16, 16)
    frames = util.hash_frames(64, 1024, seed=5, batch=2)
    wire = make_datagrams(np.zeros((256, 256), np.int32))
    with pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=256, max_batch=2) as eng:
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        want = eng.process(frames)
        eng.process_async(frames)
        for call in (lambda: eng.process(frames), lambda: eng.calibrate_host(frames[0]), lambda: eng.live_block(wire, 16, 16),
                     lambda: eng.process_async(frames)):
            with pytest.raises(pkg.AwpuError) as ei:
                call()
            assert ei.value.status == pkg.binding.ERR_STATE
        assert np.array_equal(eng.wait(), want)
        assert np.array_equal(eng.process(frames), want)


DEBUG_CHILD = r"""
import importlib, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import util
pkg = importlib.import_module("beamforming-lk_amd")
S = pkg.synthetic
out = []
for wl, batch, hint in (("c2", 4, True), ("c2", 1, True), ("c2", 3, False), ("c2", 1, False), ("c1", 4, False)):
    spec = S.WORKLOADS[wl]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    frames = util.hash_frames(spec.n_mics, 1024, seed=31, batch=batch)
    with pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=spec.n_pixels, n_streams=spec.n_mics, max_batch=batch, grid_columns=spec.res if hint else 0) as eng:
        eng.set_delay_table(off, frac); eng.set_active_mics(None)
        out.append(eng.process(frames))
np.savez(sys.argv[2], *out)
"""


def test_timing_switches_are_not_in_the_shipping_library(tmp_path):
    """AWPU_FAST_DEBUG=1|2|4|8|64 (no refill DMA / no sweep / no tail pass / no chunk barrier / register staging) would
    give wrong heatmaps; the default build has them compiled out, so with the variable set every sweep shape returns
    the bits it returns without it."""
    import os, subprocess, sys
    outs = []
    for k, dbg in enumerate(("", "79")):  # 79 = 1 + 2 + 4 + 8 + 64
        env = dict(os.environ)
        env.pop("AWPU_FAST_DEBUG", None)
        if dbg:
            env["AWPU_FAST_DEBUG"] = dbg
        path = tmp_path / f"out{k}.npz"
        r = subprocess.run([sys.executable, "-c", DEBUG_CHILD, str(Path(__file__).resolve().parent.parent), str(path)],
                           env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        outs.append(np.load(path))
    assert outs[0].files == outs[1].files and len(outs[0].files) == 5
    for name in outs[0].files:
        assert outs[0][name].max() > 0 and np.array_equal(outs[0][name], outs[1][name]), name


@pytest.mark.parametrize("n_streams,usable,P", [(128, 128, 100), (256, 256, 4096), (256, 201, 333), (192, 64, 65)])
def test_ring_sweep_wider_arrays(pkg, oracle, n_streams, usable, P):
    """The device ring with 2..4 arrays on the wire (the datagram carries up to 256 sensors), ragged mic
    lists and grids on both sides of the kernel-shape thresholds, random tables that reach both ends of the
    history: snapshot bit-exact after every block (ring wrap-around included: 9 blocks), sweep within
    tolerance, second-array calibration equal to the scalar loop."""
    rng = np.random.default_rng(n_streams + P)
    off = rng.integers(0, 1024 - 256, size=(P, n_streams)).astype(np.int32)
    off[0, :] = 1024 - 257
    off[-1, :] = 0
    frac = rng.uniform(0, 1, size=(P, n_streams)).astype(np.float32)
    index = np.sort(rng.permutation(n_streams)[:usable]).astype(np.int32)
    ring = np.zeros((n_streams, 1024), np.float32)
    with pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=P, n_streams=n_streams) as eng:
        eng.set_delay_table(off, frac)
        eng.set_active_mics(index)
        for b in range(9):
            stream = rng.integers(-(1 << 23), 1 << 23, size=(256, 256), dtype=np.int32)
            eng.ingest_block(make_datagrams(stream, counter0=256 * b, n_arrays=n_streams // 64))
            ring = np.concatenate([ring[:, 256:], oracle.unpack_exposure(stream, n_streams)], axis=1)
            if b in (0, 3, 4, 8):
                assert np.array_equal(eng.ring_snapshot(), ring), b
                power = eng.process_ring()
                assert util.power_rel_err_unfloored(power, oracle.das_f32(ring, off, frac, index)) < util.POWER_RTOL, b
        got = eng.calibrate_ring(array=1)
        want = oracle.calibrate(ring[64:128])
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


def test_random_display_and_beam_shapes(pkg, oracle):
    """Randomised sizes through the neighbours of the sweep: device heatmap + upscale against the
    restatements for odd image shapes and batches, and few-beam sweeps with ragged mic lists, table strides
    wider than the stream count and offsets at both ends of the history."""
    import torch

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(808)
    with pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=64) as eng:
        for _ in range(12):
            r, c = int(rng.integers(1, 70)), int(rng.integers(1, 70))
            R, C_ = r + int(rng.integers(0, 200)), c + int(rng.integers(0, 200))
            batch = int(rng.integers(1, 5))
            power = rng.uniform(0, 1e-4, (batch, r * c)).astype(np.float32)
            power[0, rng.integers(0, r * c)] = 0.0
            d_power = torch.from_numpy(power).to(dev)
            d_peak = torch.zeros(batch, dtype=torch.float32, device=dev)
            d_pix = torch.zeros((batch, r * c), dtype=torch.uint8, device=dev)
            d_big = torch.zeros((batch, R, C_), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()  # (torch fills on its own stream; the engine's streams do not wait for it)
            eng.heatmap_device(d_power.data_ptr(), r * c, batch, d_peak.data_ptr(), d_pix.data_ptr())
            eng.upscale_device(d_pix.data_ptr(), r, c, batch, d_big.data_ptr(), R, C_)
            eng.synchronize()
            for b in range(batch):
                small = oracle.heatmap_u8(power[b])
                assert np.array_equal(d_pix[b].cpu().numpy(), small), (r, c, b)
                assert np.array_equal(d_big[b].cpu().numpy(), oracle.resize_linear_u8(small.reshape(r, c), R, C_)), (r, c, R, C_, b)
    for _ in range(8):
        n_streams = int(rng.choice([64, 128, 256]))
        stride = n_streams + int(rng.choice([0, 5]))
        hist = int(rng.choice([513, 800, 1024]))
        n_dir = int(rng.integers(1, 130))
        usable = int(rng.integers(1, n_streams + 1))
        off = rng.integers(0, hist - 256, size=(n_dir, stride)).astype(np.int32)
        off[0, :] = hist - 257
        frac = rng.uniform(0, 1, size=(n_dir, stride)).astype(np.float32)
        index = rng.permutation(n_streams)[:usable].astype(np.int32)
        X = util.hash_frames(n_streams, hist, seed=int(rng.integers(1, 1 << 30)))[0]
        d_X = torch.from_numpy(X).to(dev)
        with pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=4, n_streams=n_streams, lut_stride=stride, hist=hist) as eng:
            eng.set_active_mics(index)
            power, beams = eng.beams(off, frac, d_X.data_ptr())
        want_p, want_b = oracle.particle_beams(X, off, frac, index)
        assert np.array_equal(beams, want_b), (n_streams, hist, n_dir, usable)
        assert util.power_rel_err(power, want_p) < 2e-6


def test_bench_two_ranks_on_one_gpu_assemble_the_oracle_heatmap():
    """bench.py's N > 1 path end to end, rehearsed with two ranks on the one GPU of the box over gloo (BENCH_REHEARSAL=1:
    a logic check, not a measurement): row groups dealt round-robin, rank 0 packs on its side stream, the packed frame
    pairs travel, both ranks sweep them, the collective trial picks a schedule, and the heatmap assembled from the two
    tiles equals the oracle's on EVERY pixel, unfloored (BENCH_GATHER_CHECK=1)."""
    import json
    import os
    import subprocess
    import sys

    repo = Path(__file__).resolve().parent.parent
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "AWPU_UNDER_PROFILER")}  # (not under a profiler here)
    env.update(BENCH_REHEARSAL="1", BENCH_GATHER_CHECK="1")
    for exchange, schedule in (("packed", None), ("window", None), ("packed", "raw_scatter")):
        env["BENCH_EXCHANGE"] = exchange
        env.pop("BENCH_BCAST", None)
        if schedule:  # the schedule that spreads rank 0's pack pass over the ranks, pinned (over gloo it is slow, not wrong)
            env["BENCH_BCAST"] = schedule
        proc = subprocess.run([sys.executable, str(repo / "bench.py"), "--gpus", "2", "--workload", "c2", "--steps", "2", "--warmup", "1",
                               "--cpu-seconds", "0", "--full"], env=env, capture_output=True, text=True, timeout=600)
        assert proc.returncode == 0, proc.stderr[-3000:]
        lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, proc.stdout[-2000:]
        rec = json.loads(lines[0])
        assert rec["n_gpus"] == 2 and rec["scaling"] == "weak" and rec["config"]["frames_per_step"] == 256
        assert rec["parity"]["ok"] and rec["parity"]["pixels"] == 2048  # rank 0's share: 32 of the 64 rows
        assert ("packed frame pairs" in rec["config"]["sharding"]) == (exchange == "packed")
        assert "gather check: ok" in proc.stderr, proc.stderr[-3000:]
        if schedule:
            assert rec["config"]["frame_exchange"]["mode"] == schedule


def test_bench_plain_run_times_only_and_dumps_the_last_step(oracle, pkg, tmp_path):
    """A plain `bench.py` run times exactly --steps steps and prints the headline line without the --full legs; with
    --dump-outputs the powers of its last timed step are written as float32, and they are the oracle's powers of the
    run's seeded frames (frames b0 = 0 and 64 come from make_frames(seed + b0))."""
    import json
    import subprocess
    import sys

    repo = Path(__file__).resolve().parent.parent
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    proc = subprocess.run([sys.executable, str(repo / "bench.py"), "--gpus", "1", "--workload", "c2", "--steps", "3", "--warmup", "1",
                           "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr[-3000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, proc.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["metric"] == "heatmap frames/sec" and rec["unit"] == "frames/s" and rec["higher_is_better"] is True
    assert rec["dtype"] == "f32" and rec["steps"] == 3 and rec["warmup"] == 1 and rec["ms_per_step"] > 0
    assert not {"parity", "cpu_baseline", "single_frame", "workloads", "projected_scaling"} & set(rec)
    S = pkg.synthetic
    spec = S.WORKLOADS["c2"]
    power = np.load(tmp_path / "power.npy")
    assert power.dtype == np.float32 and power.shape == (128, spec.n_pixels)
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    for b in (0, 64):
        frame = S.make_frames(xyz, 1, seed=1234 + b)[0]
        rep = util.parity_report(power[b], oracle.das_f32(frame, off, frac))
        assert rep["ok"], rep


def test_dc_offset_frames_batched_sweep_is_closer_to_exact_than_the_reference(pkg, oracle):
    """Samples with a DC offset (an ADC bias the wire format does not remove): the reference sums 256 mics' worth of
    the offset into every out[i] and lets its moving-average stencil cancel it again -- in fp32 that cancellation costs
    it several digits (its distance to exact fp64 sums grows a hundredfold).  The batched FAST sweep applies the stencil
    to the samples first (docs/HISTORY.md 4.2g), so the offset never enters a sum: its result stays at fp32 precision of the
    exact one -- and is therefore NOT within 1e-5 of the reference's own fp32 result on such input: the strict `ok` is
    False here, and this is the one test that uses the named allowance `ok_within_reference_noise` (3 x the reference's
    own distance to exact).  AWPU_MATH_F32_EXACT is the mode that stays within 1e-5 of the reference on biased input
    (test_exact_mode_is_within_1e5_of_the_reference_on_dc_biased_full_grids)."""
    S = pkg.synthetic
    spec = S.WORKLOADS["c2"]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    frames = S.make_frames(xyz, 10, seed=71) + np.float32(0.25)
    power, _ = run_engine(pkg, frames, off, frac, grid_columns=spec.res)
    for b in (0, 9):
        r32, r64 = oracle.das_f32(frames[b], off, frac), oracle.das_f64(frames[b], off, frac)
        rep = util.parity_report(power[b], r32, r64)
        print(f"parity DC-offset frame {b}, fast mode: {rep}")
        assert rep["ok_within_reference_noise"], rep
        assert not rep["ok"]  # 150 x the north star's tolerance away from the REFERENCE: said, not hidden
        assert rep["ref_f32_vs_f64_unfloored"] > 1e-5  # the reference's own cancellation noise ...
        assert rep["gpu_vs_f64_unfloored"] < 0.2 * rep["ref_f32_vs_f64_unfloored"]  # ... which the pre-filtered sweep does not have


DC_SWEEPS = ["sweep_c1_dc", "sweep_headline_dc"]


@pytest.mark.parametrize("name", DC_SWEEPS)
def test_dc_biased_goldens_exact_mode_flat_1e5_fast_mode_recorded(pkg, name):
    """tests/golden/sweep_*_dc.npz: powers the reference's compiled delay() produced on hash frames + {1e-4, 1e-3, 1e-2,
    0.25}.  AWPU_MATH_F32_EXACT keeps delay.cpp:19-25's operation order and mimo.cpp:124-130's mic order and must be
    within 1e-5 of those powers, flat, on every pixel and offset -- one frame per call and as a batch of all four.  The
    re-ordered AWPU_MATH_F32_FAST sweep is run on the same input and its error per offset PRINTED (the curve bench.py
    reports as `parity_dc`); it is asserted only where it holds 1e-5 today (offsets up to 1e-3 of full scale)."""
    g = np.load(GOLDEN / f"{name}.npz")
    ax, ay = g["arrays"]
    X0 = util.hash_frames(64 * int(ax) * int(ay), int(g["hist"]), seed=int(g["seed"]))[0]
    frames = np.stack([(X0 + np.float32(dc)).astype(np.float32) for dc in g["offsets"]])
    exact_batch, _ = run_engine(pkg, frames, g["off"], g["frac"], g["index"], math="exact")
    fast_batch, _ = run_engine(pkg, frames, g["off"], g["frac"], g["index"], math="fast")
    curve = {}
    for k, dc in enumerate(g["offsets"]):
        exact_single, _ = run_engine(pkg, frames[k], g["off"], g["frac"], g["index"], math="exact")
        assert np.array_equal(exact_single, exact_batch[k])  # same order of the same operations whatever the batch
        e_exact = util.power_rel_err_unfloored(exact_batch[k], g["power"][k])
        e_fast = util.power_rel_err_unfloored(fast_batch[k], g["power"][k])
        curve[float(dc)] = (e_exact, e_fast)
        assert e_exact <= util.POWER_RTOL, (name, float(dc), e_exact)
        if dc <= 1e-3:
            assert e_fast <= util.POWER_RTOL, (name, float(dc), e_fast)
    print(f"parity_dc {name}: offset -> (exact, fast) max unfloored error vs the reference build: {curve}")


def _sums_through_the_abi(pkg, frames, off, frac, index=None, **kw):
    """(power [B, P], out [B, P, 256]) of AWPU_MATH_F32_EXACT through awpu_hip_process_device_sums."""
    import torch

    frames = np.ascontiguousarray(frames, np.float32)
    B, P = frames.shape[0], off.shape[0]
    with pkg.Engine(n_pixels=P, n_streams=frames.shape[1], lut_stride=off.shape[1], hist=frames.shape[2],
                    math=pkg.MATH_F32_EXACT, max_batch=B, **kw) as eng:
        eng.set_delay_table(off, frac)
        eng.set_active_mics(index)
        d_X = torch.from_numpy(frames).cuda()
        d_P = torch.empty((B, P), dtype=torch.float32, device="cuda")
        d_S = torch.full((B, P, 256), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        eng.process_device_sums(d_X.data_ptr(), B, d_P.data_ptr(), d_S.data_ptr())
        eng.synchronize()
        return d_P.cpu().numpy(), d_S.cpu().numpy()


@pytest.mark.parametrize("name", ["sweep_c1", "sweep_c1_ragged", "sweep_c1_onemic", "sweep_headline", "sweep_c3"] + DC_SWEEPS)
def test_exact_mode_pre_epilogue_sums_are_the_reference_bits(pkg, name):
    """out[0..255] of a pixel after the last mic and before the moving average, exported by the frame-pair
    reference-order kernel (awpu_hip_process_device_sums), against what the reference's compiled delay() left in out[]
    (golden out_first / out_last): BIT-identical -- the three operations of delay.cpp:19-25 in its order, mics in
    antenna.index[] order."""
    g = np.load(GOLDEN / f"{name}.npz")
    ax, ay = g["arrays"]
    X0 = util.hash_frames(64 * int(ax) * int(ay), int(g["hist"]), seed=int(g["seed"]))[0]
    if "offsets" in g.files:
        frames = np.stack([(X0 + np.float32(dc)).astype(np.float32) for dc in g["offsets"]])
        first, last = g["out_first"], g["out_last"]
    else:
        frames, first, last = X0[None], g["out_first"][None], g["out_last"][None]
    power, out = _sums_through_the_abi(pkg, frames, g["off"], g["frac"], g["index"])
    for b in range(frames.shape[0]):
        assert np.array_equal(out[b, :4], first[b]), (name, b)
        assert np.array_equal(out[b, -1:], last[b]), (name, b)
    assert not np.isnan(out).any()


@pytest.mark.parametrize("wl,cols,rows", [("c1", 0, 32), ("c1", 32, 32), ("c2", 64, 64), ("c2", 64, 30)])
def test_exact_mode_sums_equal_the_oracle_on_every_pixel(pkg, oracle, wl, cols, rows):
    """The same export against oracle_das_f32's out_dbg on EVERY pixel (plane wave + noise, three frames: an odd batch):
    consecutive pixel pairs (no row length: das_exact_pair_kernel) and, with the row length given, whichever of the two
    reference-order kernels the table's statistics pick (das_exact_quad_kernel where vertical neighbours coincide more; a
    grid of 30 rows: a last quad of two live pixels) -- bit-identical sums, powers within the sum-order noise of the 254-term
    epilogue."""
    S = pkg.synthetic
    spec = S.WORKLOADS[wl]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    off, frac = off[: rows * spec.res], frac[: rows * spec.res]
    frames = S.make_frames(xyz, 3, seed=91)
    power, out = _sums_through_the_abi(pkg, frames, off, frac, grid_columns=cols)
    for b in range(3):
        want_p, want_out = oracle.das_f32(frames[b], off, frac, want_out=True)
        assert np.array_equal(out[b], want_out), (b, np.argwhere(out[b] != want_out)[:4])
        assert util.power_rel_err_unfloored(power[b], want_p) < 3e-6


@pytest.mark.parametrize("case", ["ref_default", "ref_default_ragged_gains", "odd_grid", "c2", "c2_short", "c2_wide", "c2_ragged_gains", "c2_96", "c2_128x256", "c1"])
def test_exact_mode_single_frames_are_the_reference_bits(pkg, oracle, case):
    """One frame per call in the reference's order -- MIMOWorker::update's regime (worker.h:212-224, mimo.cpp:97-151) -- on the halves
    form of the {next, d} layout (das_exact_ndh_kernel): one array at the reference's default resolution with every mic resident
    (100 x 100, main.cpp:38-41; also a ragged mic list with gains, and an odd grid), four arrays chunked behind the pack pre-pass
    (64 x 64, 30 x 64 -- a last quad of two live pixels -- and 64 x 96 -- two rounds of workgroups --: one pixel per wave,
    das_exact_ndp_kernel, a ragged mic list with gains there too; 96 x 96: quads, das_exact_ndh_kernel<1, false>; 128 x 256: two quads
    per wave, das_exact_ndh_kernel<2, false>), and c1, whose
    table's quads do not share (batches go to das_exact_pair_kernel there, whose powers are reduced in another order: no bit-equality
    with the batch is asked of it).  The pre-epilogue sums equal oracle_das_f32's out[] bit for bit on EVERY
    pixel (DC-biased plane-wave frames), the powers are the bits the same frame gets inside a batch (das_exact_nd_kernel), and within
    1e-5 of the oracle on every pixel."""
    S = pkg.synthetic
    names = pkg.binding.KERNEL_NAMES
    index, gains, want_batch = None, None, "exact_nd"
    if case.startswith("c2"):
        spec = S.WORKLOADS["c2"]
        xyz = S.geometry(spec)
        off, frac = S.delay_table(spec, xyz)
        # (64 x 64 and 30 x 64: at most 16 pixels per CU -> one pixel per wave, das_exact_ndp_kernel)
        rows, cols, n_streams, want = (30 if case == "c2_short" else spec.res), spec.res, spec.n_mics, "exact_ndp"
        off, frac = off[: rows * cols], frac[: rows * cols]
        if case == "c2_wide":  # 16 quad rows x 96 columns: 384 tiles of 16 pixels = two rounds of workgroups
            rows, cols = 64, 96
            off, frac = pkg.build_delay_table(xyz, rows, cols, 180.0)
        if case == "c2_96":  # 576 tiles of 16 pixels would be a third round: quads
            rows, cols, want = 96, 96, "exact_ndh"
            off, frac = pkg.build_delay_table(xyz, rows, cols, 180.0)
        if case == "c2_128x256":  # 32 768 pixels: 256 tiles of TWO quads per wave (das_exact_ndh_kernel<2, false>)
            rows, cols, want = 128, 256, "exact_ndh"
            off, frac = pkg.build_delay_table(xyz, rows, cols, 180.0)
        if case == "c2_ragged_gains":  # 205 active mics (a last group of one live mic + three silent ones), gains on
            index = np.array([k for k in range(256) if k % 5 != 2], np.int32)
            gains = (0.5 + np.arange(256) / 256.0).astype(np.float32)
    elif case == "c1":
        spec = S.WORKLOADS["c1"]
        xyz = S.geometry(spec)
        off, frac = S.delay_table(spec, xyz)
        rows, cols, n_streams, want, want_batch = spec.res, spec.res, spec.n_mics, "exact_ndp", "exact_pair"
    else:
        xyz = pkg.create_antenna()
        rows = cols = 99 if case == "odd_grid" else 100  # (99: an odd grid, whose centre pixel looks straight ahead)
        off, frac = pkg.build_delay_table(xyz, rows, cols, 180.0)
        n_streams, want = 64, "exact_ndh_stationary"
        if case == "ref_default_ragged_gains":
            index = np.array([k for k in range(64) if k % 5 != 2], np.int32)
            gains = (0.5 + np.arange(64) / 64.0).astype(np.float32)
    frames = (S.make_frames(xyz, 3, seed=55) + np.float32(0.125)).astype(np.float32)
    P = rows * cols
    import torch

    with pkg.Engine(n_pixels=P, n_streams=n_streams, math=pkg.MATH_F32_EXACT, max_batch=3, grid_columns=cols) as eng:
        eng.set_delay_table(off, frac)
        eng.set_active_mics(index)
        if gains is not None:
            eng.set_mic_gains(gains)
        batch = eng.process(frames)
        assert names[eng.stats().kernel_variant] == want_batch
        d_X = torch.from_numpy(frames[1:2].copy()).cuda()
        d_P = torch.empty((1, P), dtype=torch.float32, device="cuda")
        d_S = torch.full((1, P, 256), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        eng.process_device_sums(d_X.data_ptr(), 1, d_P.data_ptr(), d_S.data_ptr())
        eng.synchronize()
        assert names[eng.stats().kernel_variant] == want
        single, sums = d_P.cpu().numpy()[0], d_S.cpu().numpy()[0]
    if want_batch == "exact_nd":
        assert np.array_equal(single, batch[1])  # a frame swept alone = the frame swept in a pair, bit for bit
    X = frames[1] * gains[:, None] if gains is not None else frames[1]
    want_p, want_out = oracle.das_f32(X, off, frac, index=index, want_out=True)
    assert np.array_equal(sums, want_out), np.argwhere(sums != want_out)[:4]
    check_full_grid(oracle, single, X, off, frac, f"{case}: one frame per call, reference order", index=index)


@pytest.mark.parametrize("math", ["exact", "fast"])
def test_one_frame_host_calls_equal_the_device_path(pkg, oracle, math):
    """awpu_hip_process on ONE pageable host frame -- the call MIMOWorker::update makes every block (mimo.cpp:100-103) -- at the
    reference's shipped shape, 70 calls in a row on changing frames: pinned staging, upload by a kernel, powers straight into pinned
    memory, the event bracket only on the first call and every 32nd, and (default mode) completion by the flag of the sweep's last
    workgroup instead of the stream's signal.  Every call must return the bits the device-pointer path returns for that frame (a
    result read before it was complete, or left over from the call before, would differ), and the oracle's powers."""
    import torch

    S = pkg.synthetic
    spec = S.WORKLOADS["ref_default"]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    frames = S.make_frames(xyz, 7, seed=99)
    frames *= (1.0 + np.arange(7, dtype=np.float32))[:, None, None]  # seven frames of different scale: powers differ by far more than an ulp
    math_id = pkg.MATH_F32_EXACT if math == "exact" else pkg.MATH_F32_FAST
    with pkg.Engine(n_pixels=spec.n_pixels, n_streams=64, math=math_id, max_batch=1, grid_columns=spec.res) as eng:
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        want = []
        for k in range(7):
            d_X = torch.from_numpy(frames[k:k + 1].copy()).cuda()
            d_P = torch.zeros((1, spec.n_pixels), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            eng.process_device(d_X.data_ptr(), 1, d_P.data_ptr())
            eng.synchronize()
            want.append(d_P.cpu().numpy()[0])
        for call in range(70):
            k = (3 * call) % 7
            got = eng.process(frames[k:k + 1])[0]
            assert np.array_equal(got, want[k]), (call, k, np.argwhere(got != want[k])[:4])
        assert eng.stats().last_kernel_ms > 0  # (the sampled bracket did time a call)
    check_full_grid(oracle, want[0], frames[0], off, frac, f"reference default, one frame per host call ({math})")


@pytest.mark.parametrize("wl,offset", [("c2", 0.25), ("c2", 1e-2), ("headline", 0.25)])
def test_exact_mode_is_within_1e5_of_the_reference_on_dc_biased_full_grids(pkg, oracle, wl, offset):
    """DC-biased plane-wave frames on FULL grids (beam nulls included), AWPU_MATH_F32_EXACT against the reference's
    arithmetic (oracle.das_f32: bit-identical pre-epilogue sums to the reference's object code): 1e-5 flat on every
    pixel, although the reference itself is ~1e-3 from exact sums here.  Batch of three (odd: the last pair is a frame
    with itself), row length given."""
    S = pkg.synthetic
    spec = S.WORKLOADS[wl]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    frames = S.make_frames(xyz, 3, seed=72) + np.float32(offset)
    power, _ = run_engine(pkg, frames, off, frac, math="exact", grid_columns=spec.res)
    for b in (0, 2):
        r32, r64 = oracle.das_f32(frames[b], off, frac), oracle.das_f64(frames[b], off, frac)
        rep = util.parity_report(power[b], r32, r64)
        print(f"parity DC-offset {offset} {wl} frame {b}, exact mode: {rep}")
        assert rep["ok"] and rep["max_rel_unfloored"] <= util.POWER_RTOL, rep


def test_packed_entry_points_refuse_what_they_cannot_sweep(pkg, oracle):
    """awpu_hip_packed_bytes / pack_frames / process_packed: argument and state errors come back as statuses, nothing
    is launched -- a batch beyond max_batch, no table yet, the exact-order and FIR8 modes, mic gains."""
    import torch

    S = pkg.synthetic
    spec = S.WORKLOADS["c1"]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    d = torch.zeros(1 << 20, dtype=torch.float32, device="cuda")
    B = pkg.binding
    with pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=spec.n_pixels, max_batch=4, grid_columns=spec.res) as eng:
        with pytest.raises(pkg.AwpuError) as ei:  # no table, no mic list yet
            eng.packed_bytes(2)
        assert ei.value.status == B.ERR_STATE
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        assert eng.packed_bytes(4) == 2 * 64 * eng.packed_bytes(2) // (1 * 64)  # two pairs = twice one pair
        with pytest.raises(pkg.AwpuError) as ei:
            eng.packed_bytes(5)  # beyond max_batch
        assert ei.value.status == B.ERR_INVALID
        with pytest.raises(pkg.AwpuError):
            eng.pack_frames(0, 2, d.data_ptr())
        with pytest.raises(pkg.AwpuError):
            eng.process_packed(d.data_ptr(), 2, 0)
        eng.set_mic_gains(np.full(64, 2.0, np.float32))
        with pytest.raises(pkg.AwpuError) as ei:  # gains are applied by the sweep's own pack pass, not by a shared one
            eng.packed_bytes(2)
        assert ei.value.status == B.ERR_STATE
        eng.set_mic_gains(None)
        assert eng.packed_bytes(2) > 0
    for kw in (dict(math=pkg.MATH_F32_EXACT), dict(math=pkg.MATH_F32_FAST, interp=B.INTERP_FIR8)):
        with pkg.Engine(n_pixels=spec.n_pixels, max_batch=4, **kw) as eng:
            eng.set_delay_table(np.minimum(off, 1024 - 263).astype(np.int32), frac)
            eng.set_active_mics(None)
            if "interp" in kw:
                eng.set_fir_table(util.synthetic_fir_table())
            with pytest.raises(pkg.AwpuError) as ei:
                eng.packed_bytes(2)
            assert ei.value.status == B.ERR_STATE


@pytest.mark.parametrize("res,fov", [(100, 180.0), (33, 180.0), (50, 90.0)])
def test_reference_cli_default_grid(pkg, oracle, res, fov):
    """The shape the reference ships: one 8x8 array, `--mimo-res 100`, `--fov 180` (src/main.cpp:38-41,53-56 ->
    MIMOWorker(pipeline, antennas[0], &running, 100, 100, fov), aw_processing_unit.cpp:74): rows and columns that are no
    multiple of the kernels' 4-row x 16-column tiles, an odd grid (whose centre pixel looks straight ahead: mimo.cpp:38-39
    divides by a norm of ~1e-17 there) and a narrower field of view.  One frame per call (MIMOWorker::update) and a batch
    of three, with the row length given and withheld: every pixel against the oracle, unfloored."""
    xyz = pkg.create_antenna()
    off, frac = pkg.build_delay_table(xyz, res, res, fov)
    assert off.shape == (res * res, 64) and off.min() >= 256 - 29 and off.max() <= 256
    frames = pkg.synthetic.make_frames(xyz, 3, seed=77)
    for cols in (res, 0):
        with pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=res * res, n_streams=64, max_batch=3, grid_columns=cols) as eng:
            eng.set_delay_table(off, frac)
            eng.set_active_mics(None)
            single = eng.process(frames[:1])[0]
            batch = eng.process(frames)
        check_full_grid(oracle, single, frames[0], off, frac, f"{res}x{res} fov {fov} single frame, grid_columns={cols}")
        check_full_grid(oracle, batch[2], frames[2], off, frac, f"{res}x{res} fov {fov} last of three, grid_columns={cols}")
        assert util.power_rel_err(batch[0], single) < 5e-6


@pytest.mark.parametrize("arrays,res,fov,rows", [((1, 1), 100, 180.0, None), ((1, 1), 33, 180.0, None), ((4, 1), 128, 180.0, None),
                                                 ((4, 2), 256, 180.0, (96, 40)), ((4, 2), 64, 90.0, None), ((3, 1), 50, 120.0, (7, 9))])
def test_device_table_builder_equals_the_host_builder(pkg, oracle, arrays, res, fov, rows):
    """awpu_hip_build_delay_table_device (MIMOWorker::computeDelayLUT with its pixels x mics part on the GPU)
    writes the bits awpu_hip_build_delay_table writes: the reference's own shape, an odd grid, the headline table, a slab
    of c4's rows, a narrower field of view, a mic count that is no multiple of the kernel's 256 threads."""
    xyz = pkg.create_tiled_antenna(*arrays) if arrays != (1, 1) else pkg.create_antenna()
    rb, rc = rows if rows else (0, res)
    off_h, frac_h = pkg.build_delay_table(xyz, res, res, fov, rb, rc)
    off_d, frac_d = pkg.build_delay_table_device(xyz, res, res, fov, rb, rc)
    assert off_d.shape == off_h.shape == (rc * res, xyz.shape[1])
    assert np.array_equal(off_d, off_h)
    assert np.array_equal(frac_d.view(np.uint32), frac_h.view(np.uint32))
    assert off_d.max() <= 256 and frac_d.min() >= 0.0 and frac_d.max() < 1.0
    assert (off_d == 256).any(axis=1).all()  # every pixel's nearest mic has delay 0 (antenna.cpp:93-96)
    # ... and both equal the ORACLE's restatement of computeDelayLUT (oracle/das_oracle.c, mimo.cpp:20-59), not only each other
    off_o, frac_o = oracle.compute_delay_lut(xyz, res, res, fov)
    sl = slice(rb * res, (rb + rc) * res)
    assert np.array_equal(off_d, off_o[sl])
    assert np.array_equal(frac_d.view(np.uint32), frac_o[sl].view(np.uint32))


@pytest.mark.parametrize("math", MATHS)
def test_one_ulp_of_tau_at_integer_entries(pkg, oracle, math):
    """The delay table is Eigen arithmetic in the reference (antenna.cpp:99-107: a 3x3 . 3xN float product and a minCoeff),
    built -march=native -Ofast, where Eigen may contract multiply-add pairs into FMAs: tau can differ from the restatement's
    (separate multiplies and adds) in its last bit, and that is unpinned (no Eigen in this image).  Where tau sits on an
    INTEGER the split of mimo.cpp:46-54 is discontinuous -- one ulp down turns (off, frac) = (o, 0) into (o + 1, 0.99999..)
    -- which is the case the round-3 verdict asked about.  Measured here on the c2 table with a tenth of its entries forced
    onto integers, those entries then moved one ulp up (no crossing) and one ulp down (every one crosses):
      * GIVEN THE SAME TABLE the device equals the reference's arithmetic within 1e-5 on every pixel for all three tables
        -- the parity claim is about the sweep, the table is its input (the drop-in keeps the reference's own
        computeDelayLUT and hands its bits to awpu_hip_set_delay_table: INTEGRATION.md);
      * crossing an integer moves the powers no more than the same ulp without a crossing: the lerp is continuous
        there (weight ~1 on X[o+1+i-1+...]: the same sample), the split's jump is harmless;
      * a one-ulp move of tau itself -- crossing or not -- DOES move deep-null pixels by more than 1e-5 unfloored
        (3e-5 here; 9e-5 with every entry moved by a random sign): a null's power is a small difference of large
        sums, it is that sensitive to its delays.  Printed, bounded at 3e-4, and the reason the last bit of
        awpu_hip_build_delay_table (the optional Eigen-free builder) stays 'unpinned' in DESIGN.md 2."""
    S = pkg.synthetic
    spec = S.WORKLOADS["c2"]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    X = S.make_frames(xyz, 1, seed=33)[0]
    tau = (256 - off).astype(np.float32) + frac  # exact: the split's two halves add back to the float they came from

    def split(t):  # mimo.cpp:46-54
        whole = np.trunc(t.astype(np.float64))
        return (256 - whole).astype(np.int32), (t.astype(np.float64) - whole).astype(np.float32)

    assert all(np.array_equal(a, b) for a, b in zip(split(tau), (off, frac)))
    rng = np.random.default_rng(5)
    pick = rng.random(tau.shape) < 0.1
    t0 = np.where(pick, np.maximum(np.rint(tau), 1.0).astype(np.float32), tau)
    tables = {"integer": split(t0),
              "ulp up": split(np.where(pick, np.nextafter(t0, np.float32(np.inf)), t0)),
              "ulp down": split(np.where(pick, np.nextafter(t0, np.float32(-np.inf)), t0))}
    assert np.array_equal(tables["ulp up"][0], tables["integer"][0])  # no crossing upwards ...
    assert int((tables["ulp down"][0] != tables["integer"][0]).sum()) == int(pick.sum())  # ... every picked entry crosses downwards
    ref = {k: oracle.das_f32(X, o, f) for k, (o, f) in tables.items()}
    for k, (o, f) in tables.items():  # the sweep's parity, given the table
        got, _ = run_engine(pkg, X, o, f, math=math, grid_columns=spec.res)
        assert util.power_rel_err_unfloored(got, ref[k]) <= util.POWER_RTOL, k
    e_up = util.power_rel_err_unfloored(ref["ulp up"], ref["integer"])
    e_down = util.power_rel_err_unfloored(ref["ulp down"], ref["integer"])
    sign = rng.random(tau.shape) < 0.5
    t_rand = np.maximum(np.where(sign, np.nextafter(tau, np.float32(np.inf)), np.nextafter(tau, np.float32(-np.inf))), np.float32(0.0))
    e_rand = util.power_rel_err_unfloored(oracle.das_f32(X, *split(t_rand)), oracle.das_f32(X, off, frac))
    e_rand_floored = util.power_rel_err(oracle.das_f32(X, *split(t_rand)), oracle.das_f32(X, off, frac))
    print(f"one ulp of tau, c2, unfloored power movement: {int(pick.sum())} integer entries up {e_up:.2e}, down (all crossing) {e_down:.2e}; "
          f"every entry by a random sign {e_rand:.2e} (floored metric {e_rand_floored:.2e})")
    assert e_down < 1.5 * e_up + 1e-6  # the crossing adds nothing to what the ulp itself does
    assert max(e_up, e_down, e_rand) < 3e-4


@pytest.mark.parametrize("arrays,res,batch", [((4, 1), 128, 3), ((4, 2), 66, 8), ((4, 1), 100, 5)])
def test_fir8_vertical_quads_share_samples_bit_for_bit(pkg, oracle, arrays, res, batch):
    """The FIR8 batch kernel with the grid's row length given sweeps four vertically adjacent pixels mic by mic and reuses
    the samples between pixels whose integer delays coincide (sweep_fir8_planes_shared); without the hint it sweeps four
    consecutive pixels one after the other.  Per pixel the items and the taps run in the same order either way: the powers
    are the same bits -- on a full grid, on grids whose rows are no multiple of four and columns no multiple of 16 (batches
    large enough for the plane kernel: 256 workgroups), on a ragged mic list with per-mic gains, odd batches included -- and
    match the restated FIR sweep on every pixel."""
    xyz = pkg.create_tiled_antenna(*arrays)
    n = xyz.shape[1]
    off, frac = pkg.build_delay_table(xyz, res, res)
    table = measured_fir_table()
    X = util.hash_frames(n, 1024, seed=17 + res, batch=batch)
    index = np.array([m for m in range(n) if m % 11 != 5], np.int32)
    gains = (1.0 + 0.25 * np.sin(np.arange(n))).astype(np.float32)
    out = {}
    for cols in (res, 0):
        with pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=res * res, n_streams=n, interp=pkg.binding.INTERP_FIR8, max_batch=batch, grid_columns=cols) as eng:
            eng.set_delay_table(off, frac)
            eng.set_active_mics(index)
            eng.set_fir_table(table)
            plain = eng.process(X)
            eng.set_mic_gains(gains)
            gained = eng.process(X)
        out[cols] = (plain, gained)
    assert np.array_equal(out[res][0], out[0][0]) and np.array_equal(out[res][1], out[0][1])
    for b in (0, batch - 1):
        check_full_grid(oracle, out[res][0][b], X[b], off, frac, f"fir8 shared {res}x{res} frame {b}", index=index, fir_table=table)
    scaled = X * gains[None, :, None]
    check_full_grid(oracle, out[res][1][0], scaled[0], off, frac, f"fir8 shared {res}x{res} with gains", index=index, fir_table=table)


def test_pack_frames_in_slices_equals_one_pass(pkg, oracle):
    """What sharding.RawScatterExchange relies on: awpu_hip_pack_frames on a slice of the batch, written to that slice's
    slot of the packed buffer, gives the bytes one pass over the whole batch writes there -- and the sweep on the buffer
    assembled from slices gives the same powers."""
    import torch

    S = pkg.synthetic
    spec = S.WORKLOADS["c2"]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    B, parts = 16, 4
    frames = S.make_frames(xyz, B, seed=5)
    dev = torch.device("cuda", 0)
    d_frames = torch.from_numpy(frames).to(dev)
    with pkg.Engine(math=pkg.MATH_F32_FAST, n_pixels=spec.n_pixels, n_streams=spec.n_mics, max_batch=B, grid_columns=spec.res) as eng:
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        n = eng.packed_bytes(B) // 4
        whole = torch.zeros((B // 2, n // (B // 2)), dtype=torch.float32, device=dev)
        pieces = torch.zeros_like(whole)
        stream = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        eng.pack_frames(d_frames.data_ptr(), B, whole.data_ptr(), stream.cuda_stream)
        per = B // parts
        for r in (2, 0, 3, 1):  # any order
            eng.pack_frames(d_frames[r * per:(r + 1) * per].data_ptr(), per, pieces[r * per // 2:(r + 1) * per // 2].data_ptr(), stream.cuda_stream)
        p_whole = torch.zeros((B, spec.n_pixels), dtype=torch.float32, device=dev)
        p_pieces = torch.zeros_like(p_whole)
        eng.process_packed(whole.data_ptr(), B, p_whole.data_ptr(), stream.cuda_stream)
        eng.process_packed(pieces.data_ptr(), B, p_pieces.data_ptr(), stream.cuda_stream)
        torch.cuda.synchronize()
    assert torch.equal(whole, pieces)
    assert torch.equal(p_whole, p_pieces)
    check_full_grid(oracle, p_pieces[B - 1].cpu().numpy(), frames[B - 1], off, frac, "c2, packed in four slices, last frame")
