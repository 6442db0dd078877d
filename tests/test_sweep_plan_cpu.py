"""The planners of the sweep kernels' LDS images (csrc/sweep_plan.h), with no device: which layouts fit, how many mics a chunk holds,
what the table rows are padded to.  tests/host/sweep_plan_check.cpp (g++) holds the plans recorded from the library before the
planners became a host-only header and compares; it also checks that every planner names its own layout and that the one XCD
pair-group rule gives the FIR8 plane launch what its launcher used to compute itself."""
import subprocess
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent


def test_planners_give_the_recorded_plans(tmp_path):
    exe = tmp_path / "sweep_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{REPO / 'beamforming-lk_amd' / 'csrc'}",
                    str(REPO / "tests" / "host" / "sweep_plan_check.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
