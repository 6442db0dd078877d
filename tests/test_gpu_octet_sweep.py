"""das_exact_nd_kernel<2> sweeps a wave's two quads as one octet (eight rows of a column, each distinct LDS address read once per
mic).  Its pre-epilogue sums must be the bits of the one-quad-per-wave kernel (AWPU_SHAPE=exact_nd1), which the reference-bits
tests pin.  The library reads AWPU_SHAPE once per process, so every shape runs in a child process; the sums (up to 8 GiB at the
c5 slab) stay on the device and are compared through per-frame digests of their uint32 bits, the powers in full."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent

CHILD = r"""
import importlib, json, sys
import numpy as np
import torch
cfg = json.loads(sys.argv[2])
sys.path.insert(0, sys.argv[1])
pkg = importlib.import_module("beamforming-lk_amd")
S = pkg.synthetic
spec = S.WORKLOADS[cfg["workload"]]
res = cfg.get("res") or spec.res
xyz = S.geometry(spec)
off, frac = pkg.binding.build_delay_table(xyz, res, res, spec.fov, cfg["row_begin"], cfg["row_count"])
P, B = off.shape[0], cfg["batch"]
index = None
if cfg.get("mics"):
    index = np.sort(np.random.default_rng(7).choice(xyz.shape[1], cfg["mics"], replace=False)).astype(np.int32)
distinct = S.make_frames(xyz, min(B, 16), seed=cfg["seed"])
with pkg.Engine(n_pixels=P, n_streams=distinct.shape[1], lut_stride=off.shape[1], hist=distinct.shape[2],
                math=pkg.MATH_F32_EXACT, max_batch=B, grid_columns=res) as eng:
    eng.set_delay_table(off, frac)
    eng.set_active_mics(index)
    d_X = torch.from_numpy(distinct).cuda().repeat(((B + distinct.shape[0] - 1) // distinct.shape[0], 1, 1))[:B].contiguous()
    d_P = torch.empty((B, P), dtype=torch.float32, device="cuda")
    d_S = torch.full((B, P, 256), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.process_device_sums(d_X.data_ptr(), B, d_P.data_ptr(), d_S.data_ptr())
    eng.synchronize()
    variant = pkg.binding.KERNEL_NAMES[eng.stats().kernel_variant]
    assert not torch.isnan(d_S).any().item(), "sums left unwritten"
    gen = torch.Generator(device="cuda").manual_seed(99)
    w = torch.randint(-2 ** 62, 2 ** 62, (2, P * 256), generator=gen, device="cuda", dtype=torch.int64)
    digest = []
    for b0 in range(0, B, 16):  # per frame: two weighted sums of the 32-bit patterns (int64, wrapping)
        v = d_S[b0:b0 + 16].view(torch.int32).reshape(-1, P * 256).to(torch.int64)
        digest.append(torch.stack([(v * w[0]).sum(dim=1), (v * w[1]).sum(dim=1)], dim=1))
    np.save(cfg["out"] + "_digest.npy", torch.cat(digest).cpu().numpy())
    np.save(cfg["out"] + "_power.npy", d_P.cpu().numpy())
    print("CHILD OK", variant)
"""

CASES = {
    # name: (workload, res (0 = the workload's), row_begin, row_count (None = all), batch, active mics (0 = all))
    "headline_b128": ("headline", 0, 0, None, 128, 0),
    "c3_slab": ("c3", 0, 48, 16, 24, 0),
    "c4_slab": ("c4", 0, 96, 32, 16, 0),
    "c5_slab_b1024": ("c4", 0, 0, 32, 1024, 0),
    "headline_ragged_mics": ("headline", 0, 0, None, 5, 203),
    # 32x32 over the 512-mic aperture: most octets see 5..8 distinct addresses per mic (every run path of the block)
    "coarse_grid_many_steps": ("c4", 32, 0, None, 6, 0),
}


def _run(shape, case, tmp_path):
    workload, res, row_begin, row_count, batch, mics = CASES[case]
    out = str(tmp_path / shape)
    cfg = dict(workload=workload, res=res, row_begin=row_begin, row_count=row_count, batch=batch, mics=mics, seed=321, out=out)
    env = dict(os.environ, AWPU_SHAPE=shape)
    proc = subprocess.run([sys.executable, "-c", CHILD, str(REPO), json.dumps(cfg)], env=env, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0 and "CHILD OK" in proc.stdout, proc.stdout[-2000:] + proc.stderr[-3000:]
    assert "CHILD OK exact_nd" in proc.stdout, proc.stdout[-500:]
    return np.load(out + "_digest.npy"), np.load(out + "_power.npy")


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_octet_sweep_sums_are_the_one_quad_bits(case, tmp_path):
    """AWPU_SHAPE=exact_nd2 (the octet block) against exact_nd1 (one quad per wave): every pre-epilogue sum bit-equal, and so
    every power."""
    d1, p1 = _run("exact_nd1", case, tmp_path)
    d2, p2 = _run("exact_nd2", case, tmp_path)
    assert d1.shape == d2.shape and np.array_equal(d1, d2), (case, np.flatnonzero((d1 != d2).any(axis=1))[:10])
    assert np.array_equal(p1.view(np.uint32), p2.view(np.uint32)), case
