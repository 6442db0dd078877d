"""Sample values at the edges of float32 through every sweep kernel: exact powers of two times the usual hash frames down to all-subnormal
and up to overflowing squares, signed zeros, and infinities / NaN in a few samples (value_edges.py defines the tiers;
test_value_edges_cpu.py checks that they are what they claim).  The default mode must give the IEEE restatement's pre-epilogue sums bit
for bit on all of them -- gradual underflow included: a kernel, a build flag or a kernel descriptor that flushes subnormals fails here
and nowhere else -- and powers within the flat 1e-5 (exactly 0 and +inf where the restatement says so).  Two tiers put subnormal,
non-zero powers through the epilogue: at `dusk` the division by 256 * usable rounds into the subnormal range (powers within the flat
1e-5 still), at `dim` every square is subnormal (powers within one unit of 2^-149, derived in gpu_value_edges_check.py, and none 0):
a flushing square, a flushing add tree or a reciprocal-multiply in place of the division fails there.  AWPU_MATH_F32_FAST must be
exactly invariant under powers of two, and within one unit of 2^-149 of its own scaled powers at those two tiers.  In both modes a
bad frame must stay inside its own slot of a batch.

One child process per forced AWPU_SHAPE (the library reads it once per process; gpu_value_edges_check.py); the child compares with the
oracle itself and reports the kernel the handle ran, which must be the one the case is about."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu

GRID = ["x0", "small", "big", "top", "dusk", "dim", "under", "sub", "zeros", "nonfinite", "isolation"]  # batch 3: zeros holds both kinds
SINGLE = ["x0", "small", "big", "top", "dusk", "dim", "under", "sub", "zeros", "zero_row", "nonfinite"]
FAST = ["x0", "small", "big", "top", "dusk", "dim", "under", "sub", "isolation"]

# id: AWPU_SHAPE (None: the dispatch rule), case of value_edges.CASES, math, interpolation, checks, the kernel that must have run, extras
CASES = {
    # ---- the default mode: sums and powers against the oracle
    # (the round-1 verification kernel exports no pre-epilogue sums -- awpu_hip_process_device_sums answers ERR_STATE, asserted --: its powers)
    "exact_verify": ("exact_verify", "grid37", "exact", "lerp", GRID, "exact_verify", {"no_sums": True}),
    "exact_pair": ("exact_pair", "grid37", "exact", "lerp", GRID, "exact_pair", {}),
    "exact_quad": ("exact_quad", "grid37", "exact", "lerp", GRID, "exact_quad", {}),
    "exact_nd1": ("exact_nd1", "grid37", "exact", "lerp", GRID, "exact_nd", {}),
    "exact_nd2": ("exact_nd2", "grid37", "exact", "lerp", GRID + ["gains"], "exact_nd", {}),
    "exact_nd2_packed": ("exact_nd2", "grid36", "exact", "lerp", GRID[:-1], "exact_nd", {"packed": True}),  # pack_frames + process_packed
    "exact_ndh_stationary": (None, "one_array_100", "exact", "lerp", SINGLE + ["gains"], "exact_ndh_stationary", {}),
    "exact_ndh": (None, "four_arrays_96", "exact", "lerp", SINGLE, "exact_ndh", {}),
    "exact_ndp": (None, "c2_64", "exact", "lerp", SINGLE, "exact_ndp", {}),
    "exact_fir8": (None, "grid37", "exact", "fir8", GRID, "fir8", {}),  # the reference's rounding: a multiply and an add per tap
    # ---- AWPU_MATH_F32_FAST: scale invariance against the kernel's own X0 result, exact zeros, +inf, isolation
    "fast_quad": ("quad", "grid37", "fast", "lerp", FAST, "quad", {}),
    "fast_pair_vertical": ("pair_vertical", "grid37", "fast", "lerp", FAST, "pair", {}),
    "fast_pair_horizontal": ("pair_horizontal", "grid37", "fast", "lerp", FAST, "pair", {}),
    "fast_stationary": ("stationary", "grid37", "fast", "lerp", FAST, "pair_stationary", {}),
    "fast_quadh": ("quadh", "grid37", "fast", "lerp", FAST, "quadh_stationary", {}),  # 37 mics' halves rows fit the LDS: the resident form
    "fast_quadh_chunked": ("quadh_chunked", "grid37", "fast", "lerp", FAST, "quadh", {}),
    "fast_single_db": ("single_db", "grid37", "fast", "lerp", FAST, "single_db", {}),
    "fast_single_small": ("single_small", "grid37", "fast", "lerp", FAST, "single_small", {}),
    "fast_fir8_planes": ("fir8_planes", "grid37", "fast", "fir8", FAST, "fir8_planes", {}),
    "fast_fir8": (None, "grid37", "fast", "fir8", FAST, "fir8", {}),
    # ---- awpu_hip_beams on the dusk, dim, under and sub tiers
    "beams": (None, None, None, None, ["beams"], "beams", {}),
}


@pytest.mark.parametrize("name", list(CASES))
def test_value_edges(name):
    shape, case, math, interp, checks, kernel, extras = CASES[name]
    cfg = dict(case=case, math=math, interp=interp, checks=checks, **extras)
    env = {k: v for k, v in os.environ.items() if k != "AWPU_SHAPE"}
    if shape:
        env["AWPU_SHAPE"] = shape
    proc = subprocess.run([sys.executable, str(REPO / "tests" / "gpu_value_edges_check.py"), json.dumps(cfg)], env=env, capture_output=True,
                          text=True, timeout=300)
    print(proc.stdout[-3000:])
    assert proc.returncode == 0 and "CHILD OK" in proc.stdout, proc.stdout[-2000:] + proc.stderr[-3000:]
    ran = proc.stdout.split("CHILD OK")[1].split()[0]
    assert ran == kernel, (name, ran, kernel)  # one kernel, the one this case is about: no case silently runs another
