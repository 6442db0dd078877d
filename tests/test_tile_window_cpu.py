"""The planner of das_exact_nd_kernel's tile windows (csrc/nd_tile_window.h), with no device: a workgroup stages, of every mic's
packed row, only the window its tile's pixels read.  tests/host/nd_tile_window_check.cpp (g++) runs the planner on a workload's
delay table and checks every (tile pixel, mic) against the window; here: the row length and the chunk it plans."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
IMAGE_BYTES = 78 * 1024  # kFastLdsBytes (csrc/das_kernels.h)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("tile_window") / "nd_tile_window_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{REPO / 'beamforming-lk_amd' / 'csrc'}",
                    str(REPO / "tests" / "host" / "nd_tile_window_check.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True)
    return exe


def _plan(checker, tmp_path, off, res, index=None, image_bytes=IMAGE_BYTES):
    index = np.arange(off.shape[1], dtype=np.int32) if index is None else index
    lo, hi = int(off[:, index].min()), int(off[:, index].max())
    wq = hi - lo + 256  # prepare(): window = hi - lo + 256 + 1 samples, one element less
    path = tmp_path / "table.bin"
    with open(path, "wb") as f:
        np.array([off.shape[0] // res, res, off.shape[1], len(index), lo, wq, image_bytes], np.int32).tofile(f)
        np.ascontiguousarray(off, np.int32).tofile(f)
        np.ascontiguousarray(index, np.int32).tofile(f)
    out = subprocess.run([str(checker), str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("ok"), out.stdout + out.stderr
    fields = dict(kv.split("=") for kv in out.stdout.split()[:-1])
    return wq, int(fields["wq_tile"]), int(fields["chunk"]), int(fields["max_spread"])


@pytest.mark.parametrize("workload, want_wq_tile", [("headline", 279), ("c3", 282)])
def test_tile_windows_of_the_batch_workloads(pkg, checker, tmp_path, workload, want_wq_tile):
    """Every pixel of every tile reads inside [start, start + wq_tile) of every mic's row; the LDS row is 279 elements at the headline
    (of 347) and 282 at c3, and sixteen rows -- one per wave -- make a chunk."""
    S = pkg.synthetic
    spec = S.WORKLOADS[workload]
    off, _ = S.delay_table(spec)
    wq, wq_tile, chunk, spread = _plan(checker, tmp_path, off, spec.res)
    assert wq_tile == want_wq_tile == 256 + spread and wq_tile < wq, (wq, wq_tile, spread)
    assert chunk == 16


def test_a_table_whose_tiles_span_the_window_keeps_whole_rows(checker, tmp_path):
    """Random delays: some tile reads both ends of a mic's window, so rows are staged whole from element 0 (the staging before tile
    windows, through the same code); a ragged mic list pads its slots with start 0."""
    rng = np.random.default_rng(5)
    off = rng.integers(100, 400, size=(24 * 40, 64), dtype=np.int32)
    index = np.sort(rng.choice(64, 37, replace=False)).astype(np.int32)
    wq, wq_tile, chunk, spread = _plan(checker, tmp_path, off, 40, index)
    assert wq_tile == wq == 256 + spread
    assert chunk == (IMAGE_BYTES // (wq * 16)) & ~3
