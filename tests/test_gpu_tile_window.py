"""das_exact_nd_kernel stages, of every mic's packed row, only the window the item's tile reads (csrc/nd_tile_window.h): wave w copies
row w of a chunk from the row's start on, and the table's LDS addresses count from that start.  The cases are the smallest at which
that staging can go wrong, on c2's geometry (build_delay_table), with both shapes of the kernel forced (AWPU_SHAPE=exact_nd2: the octet
block; exact_nd1: one quad per wave).  References: the CPU oracle's pre-epilogue sums (bit for bit, every frame and pixel) and the
powers of AWPU_SHAPE=exact_verify, which stages nothing this way.  The library reads AWPU_SHAPE once per process: every shape runs in
a child process, which compares its sums with the oracle itself and leaves its powers for the parent."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import util

REPO = Path(__file__).resolve().parent.parent

CHILD = r"""
import importlib, json, sys
import numpy as np
import torch
cfg = json.loads(sys.argv[2])
sys.path.insert(0, sys.argv[1])
pkg = importlib.import_module("beamforming-lk_amd")
from oracle import oracle_py
S = pkg.synthetic
xyz = S.geometry(S.WORKLOADS["c2"])
rows, cols, B = cfg["rows"], cfg["cols"], cfg["batch"]
off, frac = pkg.binding.build_delay_table(xyz, rows, cols, 180.0)
P = off.shape[0]
index = np.sort(np.random.default_rng(7).choice(xyz.shape[1], cfg["mics"], replace=False)).astype(np.int32)
lo, hi = int(off[:, index].min()), int(off[:, index].max())
window = (lo - cfg["widen"], hi + 257 + cfg["widen"]) if cfg["widen"] else None
frames = S.make_frames(xyz, B, seed=cfg["seed"])
with pkg.Engine(n_pixels=P, n_streams=frames.shape[1], lut_stride=off.shape[1], hist=frames.shape[2], math=pkg.MATH_F32_EXACT,
                max_batch=B, grid_columns=cols, window=window) as eng:
    eng.set_delay_table(off, frac)
    eng.set_active_mics(index)
    d_X = torch.from_numpy(frames).cuda()
    d_P = torch.empty((B, P), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    if cfg["sums"]:
        d_S = torch.full((B, P, 256), float("nan"), dtype=torch.float32, device="cuda")
        eng.process_device_sums(d_X.data_ptr(), B, d_P.data_ptr(), d_S.data_ptr())
        eng.synchronize()
        variant = pkg.binding.KERNEL_NAMES[eng.stats().kernel_variant]
        sums = d_S.cpu().numpy()
        for b in range(B):
            _, want = oracle_py.das_f32(frames[b], off, frac, index=index, want_out=True)
            assert np.array_equal(sums[b].view(np.uint32), want.view(np.uint32)), ("sums", b, np.argwhere(sums[b] != want)[:4].tolist())
    else:
        eng.process_device(d_X.data_ptr(), B, d_P.data_ptr())
        eng.synchronize()
        variant = pkg.binding.KERNEL_NAMES[eng.stats().kernel_variant]
    power = d_P.cpu().numpy()
    if cfg["packed"]:  # the same frames through the packed-exchange entry points: the same bits
        d_K = torch.empty(eng.packed_bytes(B) // 4, dtype=torch.float32, device="cuda")
        d_Q = torch.full((B, P), float("nan"), dtype=torch.float32, device="cuda")
        eng.pack_frames(d_X.data_ptr(), B, d_K.data_ptr())
        eng.process_packed(d_K.data_ptr(), B, d_Q.data_ptr())
        eng.synchronize()
        assert pkg.binding.KERNEL_NAMES[eng.stats().kernel_variant] == variant
        assert np.array_equal(d_Q.cpu().numpy().view(np.uint32), power.view(np.uint32)), "packed frames: other powers"
    if cfg["alone"]:  # the last frame of an odd batch (a pair with itself) swept alone: the same bits
        d_A = torch.empty((1, P), dtype=torch.float32, device="cuda")
        eng.process_device(d_X[B - 1].data_ptr(), 1, d_A.data_ptr())
        eng.synchronize()
        assert np.array_equal(d_A.cpu().numpy().view(np.uint32)[0], power.view(np.uint32)[B - 1]), "a frame alone: other powers"
    np.save(cfg["out"], power)
    print("CHILD OK", variant)
"""

# name: rows, cols, batch, active mics (picked from c2's 256), samples the window is widened by at either end, packed entry points too
CASES = {
    # three tiles across (the last one partial) and three down: starts differ in both directions; 37 mics: a ragged list, padded to 40,
    # chunks of 12 + 12 + 12 + 4 (so coarse a grid spreads a tile's delays over 69 samples: twelve rows fit, four waves copy none); batch 59: the last pair is a frame with itself, and 30 pairs x 9 (nd2) tiles = 270 items are more than the
    # chip's 256 persistent workgroups, so some take a second item, on another tile (the refill of the NEXT item's first chunk)
    "ragged_three_by_three": (24, 40, 59, 37, 0, False),
    # a window wider than the table's own (the packed-exchange staging: ranks stage the union of their slabs' windows): starts no
    # longer begin at 0; 36 mics (the packed entry points take whole groups of four): three chunks of 12
    "wider_window_packed": (24, 40, 5, 36, 8, True),
    # one tile, one chunk of four rows (twelve waves copy nothing), rows that are not a whole number of 1 KiB pieces: the lane mask
    "one_tile_four_mics": (8, 16, 2, 4, 0, False),
}


def _run(shape, case, tmp_path, sums=True):
    rows, cols, batch, mics, widen, packed = CASES[case]
    out = str(tmp_path / f"{shape}.npy")
    cfg = dict(rows=rows, cols=cols, batch=batch, mics=mics, widen=widen, packed=packed and sums, sums=sums, alone=sums and batch % 2 == 1, seed=4321, out=out)
    env = dict(os.environ, AWPU_SHAPE=shape)
    proc = subprocess.run([sys.executable, "-c", CHILD, str(REPO), json.dumps(cfg)], env=env, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0 and "CHILD OK" in proc.stdout, proc.stdout[-2000:] + proc.stderr[-3000:]
    return np.load(out), proc.stdout.split("CHILD OK")[1].split()[0]


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_tile_window_staging_gives_the_oracle_sums(case, tmp_path):
    """Both shapes of the kernel: every pre-epilogue sum is the oracle's bits (asserted in the child), the two shapes' powers are equal
    bit for bit -- also through the packed entry points, and for a frame swept alone --, and they agree with exact_verify's within the
    sum-order noise of the 254-term epilogue (3e-6, the bound of the exact-mode sums tests)."""
    p2, v2 = _run("exact_nd2", case, tmp_path)
    p1, v1 = _run("exact_nd1", case, tmp_path)
    assert v1 == v2 == "exact_nd", (v1, v2)
    assert np.array_equal(p1.view(np.uint32), p2.view(np.uint32)), case
    pv, vv = _run("exact_verify", case, tmp_path, sums=False)
    assert vv == "exact_verify", vv
    for b in range(p2.shape[0]):
        assert util.power_rel_err_unfloored(p2[b], pv[b]) < 3e-6, (case, b)


def test_the_cases_are_what_they_claim(pkg):
    """(no device) the tile windows are narrower than the rows, the mic counts chunk as the cases say, and the one-tile case's rows are
    no whole number of 1 KiB pieces."""
    want_chunks = {"ragged_three_by_three": [12, 12, 12, 4], "wider_window_packed": [12, 12, 12], "one_tile_four_mics": [4]}
    S = pkg.synthetic
    xyz = S.geometry(S.WORKLOADS["c2"])
    for case, (rows, cols, batch, mics, widen, packed) in CASES.items():
        off, _ = pkg.binding.build_delay_table(xyz, rows, cols, 180.0)
        index = np.sort(np.random.default_rng(7).choice(xyz.shape[1], mics, replace=False))
        o = off[:, index].reshape(rows, cols, mics)
        wq = int(o.max() - o.min()) + 256 + 2 * widen
        spread = 0
        for r0 in range(0, rows, 8):
            for c0 in range(0, cols, 16):
                t = o[r0:r0 + 8, c0:c0 + 16].reshape(-1, mics)
                spread = max(spread, int((t.max(axis=0) - t.min(axis=0)).max()))
        wq_tile = min(wq, 256 + spread)
        assert wq_tile < wq or case == "one_tile_four_mics", (case, wq, wq_tile)  # (a single tile spans the table's whole window)
        pad = (mics + 3) & ~3
        chunk = min(16, (78 * 1024 // (wq_tile * 16)) & ~3, pad)
        assert [min(chunk, pad - c) for c in range(0, pad, chunk)] == want_chunks[case], (case, wq_tile, chunk)
        if case == "one_tile_four_mics":
            assert (wq_tile * 16) % 1024 != 0, wq_tile
