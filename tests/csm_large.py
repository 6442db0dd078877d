"""The mic lists at which the cross-spectral kernels change their launch shape above 257 mics, for test_gpu_csm_large.py (the device
against the host rule) and test_csm_large_cpu.py (the host rule against fp64): test_gpu_csm's Shape with two sample blocks, made
once per name and left unchanged.  A plain helper, not a conftest."""
from __future__ import annotations

LDS_BYTES = 144 * 1024  # csm_kernels.h: kCsmMapLdsBytes
BINS, WINDOW, N_BLOCKS = [47], 1, 2  # the one setting every list runs: Hann, two blocks, pitch 256 * 2 + 40

# 545 of 640 streams: every seventh stream left out, and the last one kept
RAGGED_545 = [i for i in range(635) if i % 7 != 3] + [639]

# name -> (n_streams, active list, pixels, gains, seed, pixels a workgroup of the map kernel takes)
LISTS = {"544": (544, list(range(544)), 40, False, 21, 32),
         "545_of_640": (640, RAGGED_545, 21, True, 22, 16),
         "1120": (1120, list(range(1120)), 21, False, 23, 16),
         "1121": (1121, list(range(1121)), 11, False, 24, 8),
         "2048": (2048, list(range(2048)), 11, False, 25, 8)}

_made = {}


def map_lds_bytes(usable, ppw):
    """csm_map_lds_bytes of csm_kernels.h: the steering vectors [usable][ppw] and the ring [2][16][ppw], 8 bytes each."""
    return (usable + 32) * ppw * 8


def pixels_per_workgroup(usable):
    """csm_map_pixels_per_wave of csm_kernels.h, restated: 64, or the largest halving of it that fits the LDS; 0 above 2048 mics."""
    if usable > 2048:
        return 0
    return next((ppw for ppw in (64, 32, 16, 8) if map_lds_bytes(usable, ppw) <= LDS_BYTES), 0)


def shape(pkg, name):
    """The list's Shape: its inverse is taken (csm_invert_host, loading 0.05) up to 545 mics only -- at 2048 it takes minutes."""
    if name not in _made:
        from test_gpu_csm import Shape

        n_streams, index, pixels, gains, seed, _ = LISTS[name]
        _made[name] = Shape(pkg, name, n_streams, n_streams, index, pixels, gains, seed, blocks=N_BLOCKS, invert=len(index) <= 545)
    return _made[name]
