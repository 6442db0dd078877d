#!/bin/bash
# a tuning/timing variant of the library into tools/ab/<name>.so: the generator's environment variables (QUAD1_NOBRANCH=1 ...)
# and AWPU_EXTRA_HIPCC_FLAGS apply; the tracked build's generated include is restored afterwards.
# usage: [GENERATOR VARS] tools/build_variant.sh <name>
set -euo pipefail
cd "$(dirname "$0")/.."
name=$1
mkdir -p tools/ab
python tools/gen_trip_asm.py > /dev/null
# the shipping build's own command (_build.hipcc_command: its sources and flags, AWPU_EXTRA_HIPCC_FLAGS among them), so that a variant is the whole library
python -c 'import subprocess, sys; sys.path.insert(0, "beamforming-lk_amd"); import _build; subprocess.run(_build.hipcc_command(sys.argv[1]), check=True)' tools/ab/$name.so
env -i PATH="$PATH" HOME="$HOME" python tools/gen_trip_asm.py > /dev/null   # back to the defaults
touch -r beamforming-lk_amd/libawpu_hip.so beamforming-lk_amd/csrc/das_fast_trip.inc 2>/dev/null || true
echo "built tools/ab/$name.so"
