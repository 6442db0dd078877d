"""A census of the dispatch rule (csrc/awpu_sweep.cpp: choose_shape / launch, and sweep_packed): which kernel serves which call."""
import functools
import importlib
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"


@functools.lru_cache(maxsize=None)
def tables(mics, rows, cols):
    """(off, frac) of a rows x cols grid over one 8x8 array (64 mics) or the four arrays of the c2 / headline geometry (256)."""
    pkg = importlib.import_module("beamforming-lk_amd")
    xyz = pkg.create_antenna() if mics == 64 else pkg.synthetic.geometry(pkg.synthetic.WORKLOADS["c2"])
    return pkg.build_delay_table(xyz, rows, cols, 180.0)


# (id, math, interp, mics, rows, cols, grid_columns given, batch, entry point, expected KERNEL_NAMES entry)
# The expected names were recorded by running this list on the commit BEFORE the sweep layer moved into awpu_sweep.cpp, on an
# MI355X (256 CUs); they are that commit's answers, not this code's (the run's output: profiles/r11_sweep_refactor_rate.txt).
CASES = [
    ("exact_small_grid_one_frame", "exact", "lerp", 64, 16, 16, True, 1, "process", "exact_ndp"),
    ("exact_small_grid_batch", "exact", "lerp", 64, 16, 16, True, 3, "process", "exact_pair"),
    ("exact_one_array_one_frame", "exact", "lerp", 64, 100, 100, True, 1, "process", "exact_ndh_stationary"),
    ("exact_one_array_batch", "exact", "lerp", 64, 100, 100, True, 2, "process", "exact_nd"),
    ("exact_no_row_length", "exact", "lerp", 64, 100, 100, False, 1, "process", "exact_pair"),
    ("exact_c2_one_frame", "exact", "lerp", 256, 64, 64, True, 1, "process", "exact_ndp"),
    ("exact_four_arrays_96_one_frame", "exact", "lerp", 256, 96, 96, True, 1, "process", "exact_ndh"),
    ("exact_one_array_ring", "exact", "lerp", 64, 100, 100, True, 1, "ring", "exact_ndh_stationary"),
    ("exact_fir8", "exact", "fir8", 64, 16, 16, False, 1, "process", "fir8"),
    ("bf16", "bf16", "lerp", 64, 16, 16, False, 1, "process", "exact_verify"),
    ("fast_one_array_one_frame", "fast", "lerp", 64, 100, 100, True, 1, "process", "quadh_stationary"),
    ("fast_one_array_batch", "fast", "lerp", 64, 100, 100, True, 4, "process", "quad"),
    ("fast_one_array_batch_no_row_length", "fast", "lerp", 64, 100, 100, False, 4, "process", "pair_stationary"),
    ("fast_one_array_one_frame_no_row_length", "fast", "lerp", 64, 100, 100, False, 1, "process", "single_small"),
    ("fast_small_grid_one_frame", "fast", "lerp", 64, 16, 16, True, 1, "process", "exact_ndp"),
    ("fast_four_arrays_one_frame", "fast", "lerp", 256, 100, 100, True, 1, "process", "quadh"),
    ("fast_four_arrays_batch_no_row_length", "fast", "lerp", 256, 128, 128, False, 4, "process", "pair"),
    ("fast_fir8_headline_batch", "fast", "fir8", 256, 128, 128, False, 4, "process", "fir8_planes"),
    ("fast_fir8_small_grid", "fast", "fir8", 256, 16, 16, False, 1, "process", "fir8"),
    ("exact_packed", "exact", "lerp", 64, 100, 100, True, 2, "packed", "exact_nd"),
    ("fast_packed", "fast", "lerp", 64, 100, 100, True, 4, "packed", "quad"),
    ("fast_c2_batch_no_row_length", "fast", "lerp", 256, 64, 64, False, 4, "process", "single_db"),
    ("fast_one_array_ring", "fast", "lerp", 64, 100, 100, True, 1, "ring", "quadh_stationary"),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_dispatch_census(pkg, case):
    """One call per branch of the dispatch rule that a small shape reaches without a forced shape: the kernel the handle reports
    (Stats.kernel_variant) is the one the rule chose before the sweep layer had a file of its own.  Only the variant is read, so the
    frames are zeros.  The thresholds count workgroups against the device's compute units: the names hold on an MI355X (256 CUs).
    `packed` = process_packed(pack_frames(x)) (usable % 4 == 0, no gains); `ring` = four ingested blocks, then process_ring."""
    name, math, interp, mics, rows, cols, columns_given, batch, entry, want = case
    B = pkg.binding
    off, frac = tables(mics, rows, cols)
    P = rows * cols
    with pkg.Engine(n_pixels=P, n_streams=mics, math={"exact": pkg.MATH_F32_EXACT, "fast": pkg.MATH_F32_FAST, "bf16": pkg.MATH_BF16_ACC}[math],
                    interp=B.INTERP_FIR8 if interp == "fir8" else B.INTERP_LERP, max_batch=batch,
                    grid_columns=cols if columns_given else 0) as eng:
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        if interp == "fir8":
            eng.set_fir_table(np.load(GOLDEN / "delay_kat_fir8.npz")["impulse_response"])
        if entry == "process":
            eng.process(np.zeros((batch, mics, 1024), np.float32))
        elif entry == "ring":
            from test_gpu_parity import make_datagrams

            for b in range(4):
                eng.ingest_block(make_datagrams(np.zeros((256, 256), np.int32), counter0=256 * b, n_arrays=mics // 64))
            eng.process_ring()
        else:
            import torch

            d_x = torch.zeros((batch, mics, 1024), dtype=torch.float32, device="cuda")
            d_packed = torch.zeros(eng.packed_bytes(batch) // 4, dtype=torch.float32, device="cuda")
            d_power = torch.empty((batch, P), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            eng.pack_frames(d_x.data_ptr(), batch, d_packed.data_ptr())
            eng.process_packed(d_packed.data_ptr(), batch, d_power.data_ptr())
            eng.synchronize()
        got = B.KERNEL_NAMES[eng.stats().kernel_variant]
    print(f"census {name}: {got}")
    assert got == want, (name, got, want)
