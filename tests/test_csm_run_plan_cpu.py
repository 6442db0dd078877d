"""The arithmetic of a cross-spectral run (csrc/csm_run_plan.h), with no device: tests/host/csm_run_plan_check.cpp (g++, the header
alone) holds the scratch totals recorded from the library before the run's layout became this header and compares; it checks that
the regions are disjoint, in order, on multiples of 4 floats and empty where nobody asked; it walks the chunks of every recording of
1 to 600 blocks by brute force (they tile the blocks, none is longer than 256, every shown frame comes once, in order and in its
block's chunk, no chunk shows more than a piece, a chunk cut short ends behind its last frame); and it checks every frame's window
in the spectra store for every carry.  A program of its own under ASan and UBSan."""
import subprocess
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent


def test_the_run_plan_keeps_the_recorded_totals_and_its_properties(tmp_path):
    exe = tmp_path / "csm_run_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{REPO / 'beamforming-lk_amd' / 'csrc'}", str(REPO / "tests" / "host" / "csm_run_plan_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "csm run plan: ok", out.stdout + out.stderr
