"""Build recipe for libawpu_hip.so (gfx950 only, in-tree): the one place that knows what the library is built from and how.

hipcc cross-compiles without a GPU, so this runs on a machine without one and on the GPU
box alike.  The library is written next to this file and is git-ignored.
`make lib` and the CMake target run this file as a script (--out).
"""
from __future__ import annotations

import os
import shutil
import subprocess
from pathlib import Path

PKG_DIR = Path(__file__).resolve().parent
REPO = PKG_DIR.parent
CSRC = PKG_DIR / "csrc"
LIB_PATH = PKG_DIR / "libawpu_hip.so"

# every source of csrc/ is compiled, the device files first; every header of csrc/ and include/ makes the library stale.  (Nothing
# depends on the order: no object at namespace scope of a host file has a constructor that reads another file's -- the
# thread_local error string of awpu_hip.cpp and env()'s function-local static are made at first use)
SOURCES = sorted(CSRC.glob("*.hip")) + sorted(CSRC.glob("*.cpp"))
# das_fast_trip.inc -- the hand-scheduled inner loops of das_fast.hip -- is GENERATED at build time by tools/gen_trip_asm.py
# (not tracked: ~19 000 lines of asm text whose source is the generator)
GENERATOR = REPO / "tools" / "gen_trip_asm.py"
TRIP_INC = CSRC / "das_fast_trip.inc"
HEADERS = sorted(CSRC.glob("*.h")) + sorted((REPO / "include").glob("*.h")) + [GENERATOR]


def hipcc_path() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and Path(cand).exists():
            return cand
    raise RuntimeError("hipcc not found: libawpu_hip.so cannot be built (there is no CPU fallback)")


def hipcc_command(out: Path, extra_flags: tuple = ()) -> list:
    """The one compile command: every source into the shared library `out`, with `extra_flags` in front of the sources."""
    return [
        hipcc_path(),
        "--offload-arch=gfx950",
        "-O3",
        "-std=c++17",
        "-fPIC",
        "-shared",
        "-Wall",
        "-Wno-unused-result",
        "-Werror=inline-asm",  # e.g. a reserved register on a hand-written block's clobber list: undefined behaviour, not a warning
        "-x", "hip",
        f"-I{REPO / 'include'}",
        f"-I{CSRC}",
        *os.environ.get("AWPU_EXTRA_HIPCC_FLAGS", "").split(),  # tuning builds (e.g. -DAWPU_QUAD_VARIANTS)
        *extra_flags,
        *[str(s) for s in SOURCES],
        "-o", str(out),
    ]


def stale(lib: Path = LIB_PATH) -> bool:
    if not lib.exists():
        return True
    built = lib.stat().st_mtime
    return any(p.stat().st_mtime > built for p in SOURCES + HEADERS)


def build_library(force: bool = False, verbose: bool = False, out: Path = LIB_PATH) -> Path:
    """Compile the HIP kernels and the C ABI into beamforming-lk_amd/libawpu_hip.so (or `out`)."""
    if not force and not stale(out):
        return out
    # several ranks of one job may get here at once (torch.distributed.run starts them together): one builds,
    # the others wait for the lock and then find the library fresh
    import fcntl

    with open(PKG_DIR / ".build.lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not force and not stale(out):
            return out
        return _compile(verbose, force, out)


def generate_blocks(force: bool = False) -> Path:
    """Write csrc/das_fast_trip.inc with the generator's defaults (its tuning variables are for tuning builds, by hand)."""
    if not force and TRIP_INC.exists() and TRIP_INC.stat().st_mtime >= GENERATOR.stat().st_mtime:
        return TRIP_INC
    import sys

    env = {k: v for k, v in os.environ.items()
           if not k.startswith(("QUAD", "TRIP_", "PAIR_DEPTH", "FIR_PRIO", "BLOCK_END_PRIO", "ND_"))}  # a shipping build: the defaults
    proc = subprocess.run([sys.executable, str(GENERATOR)], capture_output=True, text=True, env=env)
    if proc.returncode != 0 or not TRIP_INC.exists():
        raise RuntimeError(f"tools/gen_trip_asm.py failed ({proc.returncode}):\n{proc.stdout}\n{proc.stderr}")
    return TRIP_INC


def _compile(verbose: bool, force: bool = False, out: Path = LIB_PATH) -> Path:
    generate_blocks(force)
    tmp = out.with_name(f"{out.name}.tmp{os.getpid()}")
    cmd = hipcc_command(tmp)
    if verbose:
        print(" ".join(cmd))
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        tmp.unlink(missing_ok=True)
        raise RuntimeError(f"hipcc failed ({proc.returncode}):\n{proc.stdout}\n{proc.stderr}")
    if verbose and proc.stderr.strip():
        print(proc.stderr)
    os.replace(tmp, out)  # a process that is loading the old file keeps its mapping
    return out


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", type=Path, help="build into this file, and only if it is older than a source or header (make lib, CMake); "
                                             "without it: the in-tree library, rebuilt whatever its age")
    args = ap.parse_args()
    print(build_library(verbose=True, out=args.out.resolve()) if args.out else build_library(force=True, verbose=True))
