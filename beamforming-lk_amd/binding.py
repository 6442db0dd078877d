"""ctypes binding of libawpu_hip.so (include/awpu_hip.h).

Plumbing only: it loads the in-tree HIP library and forwards to the C ABI.  There is no
Python or CPU implementation of the sweep behind it -- if the library cannot be built or
loaded, importing a compute entry point raises.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
import os
from typing import Optional

import numpy as np

from . import _build

N_SAMPLES = 256
HIST = 1024
ELEMENTS = 64
DATAGRAM_BYTES = 1032  # sizeof(message), src/fpga/receiver.h:24-30

INTERP_LERP, INTERP_FIR8 = 0, 1
MATH_F32_EXACT, MATH_F32_FAST, MATH_BF16_ACC = 0, 1, 2

OK, ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_STATE, ERR_RANGE, ERR_NOMEM = 0, -1, -2, -3, -4, -5, -6


class Cfg(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32),
        ("device", C.c_int32),
        ("n_streams", C.c_int32),
        ("hist", C.c_int32),
        ("n_pixels", C.c_int32),
        ("lut_stride", C.c_int32),
        ("interp", C.c_int32),
        ("math", C.c_int32),
        ("max_batch", C.c_int32),
        ("pixel_begin", C.c_int32),
        ("pixel_count", C.c_int32),
        ("grid_columns", C.c_int32),
        ("n_devices", C.c_int32),
        ("devices", C.c_int32 * 8),
        ("window_begin", C.c_int32),
        ("window_end", C.c_int32),
        ("reserved", C.c_int32 * 1),
    ]


class Stats(C.Structure):
    _fields_ = [
        ("frames", C.c_uint64),
        ("launches", C.c_uint64),
        ("last_kernel_ms", C.c_double),
        ("total_kernel_ms", C.c_double),
        ("alg_bytes_frame", C.c_uint64),
        ("alg_flops_frame", C.c_uint64),
        ("tau_max", C.c_int32),
        ("window", C.c_int32),
        ("usable", C.c_int32),
        ("kernel_variant", C.c_int32),
        ("group_exchange", C.c_int32),
        ("group_ranges", C.c_int32),
    ]


class AwpuError(RuntimeError):
    def __init__(self, status: int, where: str, detail: str):
        self.status = status
        super().__init__(f"{where}: status {status} ({detail})")


PEER_SAME_DEVICE, PEER_DIRECT, PEER_HOST_STAGED = 0, 1, 2
EXCHANGE_NONE, EXCHANGE_WINDOWS, EXCHANGE_PACKED_PAIRS = 0, 1, 2  # Stats.group_exchange
# awpu_kernel_id (include/awpu_hip.h): Stats.kernel_variant after a launch
KERNEL_NAMES = ("none", "quad", "pair", "pair_stationary", "quadh", "quadh_stationary", "single_db", "single_small", "fir8_planes",
                "fir8", "exact_pair", "exact_verify", "tuning", "exact_quad", "exact_nd", "exact_ndh", "exact_ndh_stationary", "exact_ndp",
                "cohere", "tones")

_lib: Optional[C.CDLL] = None

_f32p = C.POINTER(C.c_float)
_i32p = C.POINTER(C.c_int32)
_u8p = C.POINTER(C.c_uint8)

_SIGNATURES = {
    "awpu_hip_default_cfg": (None, [C.POINTER(Cfg)]),
    "awpu_hip_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(Cfg)]),
    "awpu_hip_destroy": (C.c_int, [C.c_void_p]),
    "awpu_hip_set_delay_table": (C.c_int, [C.c_void_p, _i32p, _f32p]),
    "awpu_hip_set_active_mics": (C.c_int, [C.c_void_p, _i32p, C.c_int32]),
    "awpu_hip_set_fir_table": (C.c_int, [C.c_void_p, _f32p]),
    "awpu_hip_process": (C.c_int, [C.c_void_p, _f32p, C.c_int32, _f32p]),
    "awpu_hip_process_async": (C.c_int, [C.c_void_p, _f32p, C.c_int32, _f32p]),
    "awpu_hip_wait": (C.c_int, [C.c_void_p]),
    "awpu_hip_process_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "awpu_hip_process_device_sums": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "awpu_hip_synchronize": (C.c_int, [C.c_void_p]),
    "awpu_hip_packed_bytes": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_uint64)]),
    "awpu_hip_pack_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "awpu_hip_process_packed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "awpu_hip_ingest_block": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "awpu_hip_process_ring": (C.c_int, [C.c_void_p, _f32p]),
    "awpu_hip_ring_snapshot": (C.c_int, [C.c_void_p, _f32p]),
    "awpu_hip_heatmap_u8": (C.c_int, [_f32p, C.c_int32, _u8p]),
    "awpu_hip_live_block": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, _f32p, C.c_int32, C.c_int32, _u8p, C.c_int32,
                                      C.c_int32, C.c_void_p, _u8p]),
    "awpu_hip_steer_table": (C.c_int, [_f32p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int32,
                                       _i32p, _f32p]),
    "awpu_hip_beams": (C.c_int, [C.c_void_p, C.c_void_p, _i32p, _f32p, C.c_int32, _f32p, _f32p]),
    "awpu_hip_set_mic_gains": (C.c_int, [C.c_void_p, _f32p]),
    "awpu_hip_calibrate_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_float, _i32p, _f32p,
                                            C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_void_p]),
    "awpu_hip_calibrate_ring": (C.c_int, [C.c_void_p, C.c_int32, C.c_float, _i32p, _f32p, C.POINTER(C.c_float),
                                          C.POINTER(C.c_int32)]),
    "awpu_hip_calibrate_host": (C.c_int, [C.c_void_p, _f32p, C.c_int32, C.c_float, _i32p, _f32p, C.POINTER(C.c_float),
                                          C.POINTER(C.c_int32)]),
    "awpu_hip_last_error_of": (C.c_char_p, [C.c_void_p]),
    "awpu_hip_upscale_u8_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                             C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "awpu_hip_resize_linear_u8": (C.c_int, [_u8p, C.c_int32, C.c_int32, _u8p, C.c_int32, C.c_int32]),
    "awpu_hip_heatmap_u8_device": (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "awpu_hip_create_antenna": (C.c_int, [C.c_int32, C.c_int32, C.c_float, _f32p]),
    "awpu_hip_create_tiled_antenna": (C.c_int, [C.c_int32, C.c_int32, C.c_float, _f32p]),
    "awpu_hip_steering_delays": (C.c_int, [_f32p, C.c_int32, C.c_double, C.c_double, _f32p]),
    "awpu_hip_build_delay_table": (
        C.c_int,
        [_f32p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int32, _i32p, _f32p],
    ),
    "awpu_hip_build_delay_table_device": (
        C.c_int,
        [C.c_int32, _f32p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int32, _i32p, _f32p],
    ),
    "awpu_hip_get_stats": (C.c_int, [C.c_void_p, C.POINTER(Stats)]),
    "awpu_hip_group_peer_status": (C.c_int, [C.c_void_p, _i32p, C.c_int32]),
    "awpu_hip_strerror": (C.c_char_p, [C.c_int]),
    "awpu_hip_last_error": (C.c_char_p, []),
    "awpu_hip_abi_version": (C.c_int, []),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)


class Particle(C.Structure):
    """awpu_particle_t (include/awpu_hip_track.h)."""
    _fields_ = [
        ("theta", C.c_double),
        ("phi", C.c_double),
        ("spread", C.c_double),
        ("rate", C.c_double),
        ("steps", C.c_int32),
        ("error", C.c_float),
        ("grad_theta", C.c_double),
        ("grad_phi", C.c_double),
        ("radius", C.c_double),
        ("power", C.c_float * 4),
    ]


# particle tracking: the entry points of include/awpu_hip_track.h (EXPORTED_SYMBOLS is awpu_hip.h's set)
_TRACK_SIGNATURES = {
    "awpu_hip_set_antenna": (C.c_int, [C.c_void_p, _f32p, C.c_int32]),
    "awpu_hip_steer_table_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int32, _i32p,
                                              _f32p]),
    "awpu_hip_track": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Particle), C.c_int32, C.c_double, C.c_double,
                                 C.POINTER(C.c_double), _f32p]),
}
TRACK_SYMBOLS = tuple(_TRACK_SIGNATURES)

# runs of consecutive blocks: the entry points of include/awpu_hip_blocks.h
_BLOCK_SIGNATURES = {
    "awpu_hip_process_blocks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, _f32p]),
    "awpu_hip_process_samples": (C.c_int, [C.c_void_p, _f32p, C.c_int64, C.c_int32, _f32p]),
    "awpu_hip_process_samples_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
}
BLOCK_SYMBOLS = tuple(_BLOCK_SIGNATURES)

# listening to such runs: the entry points of include/awpu_hip_listen.h
_LISTEN_TAIL = [C.c_int32, C.POINTER(Particle), C.c_int32, C.c_double, C.c_double]  # n_blocks, listeners, n, theta_limit, reference
_LISTEN_SIGNATURES = {
    "awpu_hip_listen_blocks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, *_LISTEN_TAIL, _f32p, C.c_int64, C.POINTER(Particle), _f32p]),
    "awpu_hip_listen_samples": (C.c_int, [C.c_void_p, _f32p, C.c_int64, *_LISTEN_TAIL, _f32p, C.c_int64, C.POINTER(Particle), _f32p]),
    "awpu_hip_listen_samples_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, *_LISTEN_TAIL, C.c_void_p, C.c_int64, C.c_void_p,
                                                 C.c_void_p, C.c_void_p]),
}
LISTEN_SYMBOLS = tuple(_LISTEN_SIGNATURES)



class Watch(C.Structure):
    """awpu_watch_t (include/awpu_hip_watch.h)."""
    _fields_ = [
        ("first", C.c_int32),
        ("every", C.c_int32),
        ("rows", C.c_int32),
        ("cols", C.c_int32),
        ("out_rows", C.c_int32),
        ("out_cols", C.c_int32),
        ("flip", C.c_int32),
        ("d_colormap", C.c_void_p),
    ]


# watching such runs: the entry points of include/awpu_hip_watch.h
_WATCH_TAIL = [C.c_int32, C.POINTER(Watch)]  # n_blocks, w
_WATCH_SIGNATURES = {
    "awpu_hip_watch_count": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _i32p, _i32p]),
    "awpu_hip_watch_blocks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, *_WATCH_TAIL, _u8p, _u8p, _f32p]),
    "awpu_hip_watch_samples": (C.c_int, [C.c_void_p, _f32p, C.c_int64, *_WATCH_TAIL, _u8p, _u8p, _f32p]),
    "awpu_hip_watch_samples_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, *_WATCH_TAIL, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p]),
}
WATCH_SYMBOLS = tuple(_WATCH_SIGNATURES)

FIND_MAX_RADIUS, FIND_MAX_SOURCES, FIND_MAX_PIXELS = 8, 32, 262144


class Find(C.Structure):
    """awpu_find_t (include/awpu_hip_find.h)."""
    _fields_ = [
        ("rows", C.c_int32),
        ("cols", C.c_int32),
        ("radius", C.c_int32),
        ("max_sources", C.c_int32),
        ("min_power", C.c_float),
        ("min_ratio", C.c_float),
        ("fov_deg", C.c_float),
    ]


class Source(C.Structure):
    """awpu_source_t (include/awpu_hip_find.h)."""
    _fields_ = [
        ("pixel", C.c_int32),
        ("power", C.c_float),
        ("row", C.c_double),
        ("col", C.c_double),
        ("theta", C.c_double),
        ("phi", C.c_double),
    ]


# finding sources: the entry points of include/awpu_hip_find.h
_FIND_TAIL = [C.POINTER(Find), C.c_void_p, C.c_void_p]  # f, sources, count
_FIND_SIGNATURES = {
    "awpu_hip_find_peaks": (C.c_int, [_f32p, C.c_int32, *_FIND_TAIL]),
    "awpu_hip_find_peaks_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, *_FIND_TAIL, C.c_void_p]),
    "awpu_hip_find_blocks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, *_WATCH_TAIL, *_FIND_TAIL, _f32p]),
    "awpu_hip_find_samples": (C.c_int, [C.c_void_p, _f32p, C.c_int64, *_WATCH_TAIL, *_FIND_TAIL, _f32p]),
    "awpu_hip_find_samples_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, *_WATCH_TAIL, *_FIND_TAIL, C.c_void_p, C.c_void_p]),
}
FIND_SYMBOLS = tuple(_FIND_SIGNATURES)

# band-limited heatmaps: the entry points of include/awpu_hip_band.h
BAND_MAX_TAPS = 128
_BAND_SIGNATURES = {
    "awpu_hip_band_filter": (C.c_int, [_f32p, C.c_int32, C.c_int64, C.c_int32, _f32p, C.c_int32, _f32p]),
    "awpu_hip_band_design": (C.c_int, [C.c_double, C.c_double, C.c_double, C.c_int32, _f32p]),
    "awpu_hip_set_band": (C.c_int, [C.c_void_p, _f32p, C.c_int32]),
}
BAND_SYMBOLS = tuple(_BAND_SIGNATURES)

# spectral heatmaps: the entry points of include/awpu_hip_spectral.h
SPECTRAL_MAX_BANDS = 4
SPECTRAL_SCALE_COMMON, SPECTRAL_SCALE_PER_BAND = 0, 1


class Spectral(C.Structure):
    """awpu_spectral_t (include/awpu_hip_spectral.h)."""
    _fields_ = [
        ("n_bands", C.c_int32),
        ("taps", C.c_int32 * SPECTRAL_MAX_BANDS),
        ("coef", _f32p * SPECTRAL_MAX_BANDS),
        ("channel", C.c_int32 * 3),
        ("scale", C.c_int32),
    ]


_SPECTRAL_TAIL = [*_WATCH_TAIL, C.POINTER(Spectral)]  # n_blocks, w, sp
_SPECTRAL_SIGNATURES = {
    "awpu_hip_spectral_compose": (C.c_int, [_f32p, C.c_int64, C.c_int32, C.c_int32, _i32p, C.c_int32, _u8p, _u8p]),
    "awpu_hip_process_bands": (C.c_int, [C.c_void_p, _f32p, C.c_int32, C.POINTER(Spectral), _f32p]),
    "awpu_hip_process_bands_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(Spectral), C.c_void_p, C.c_void_p]),
    "awpu_hip_spectral_blocks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, *_SPECTRAL_TAIL, _u8p, _u8p, _u8p, _f32p]),
    "awpu_hip_spectral_samples": (C.c_int, [C.c_void_p, _f32p, C.c_int64, *_SPECTRAL_TAIL, _u8p, _u8p, _u8p, _f32p]),
    "awpu_hip_spectral_samples_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, *_SPECTRAL_TAIL, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_void_p]),
}
SPECTRAL_SYMBOLS = tuple(_SPECTRAL_SIGNATURES)

RANGE_MAX_CANDIDATES = 64


class Range(C.Structure):
    """awpu_range_t (include/awpu_hip_focus.h)."""
    _fields_ = [
        ("index", C.c_int32),
        ("power", C.c_float),
        ("distance", C.c_double),
    ]


# focus and range: the entry points of include/awpu_hip_focus.h
_f64p = C.POINTER(C.c_double)
_LOCATE_TAIL = [*_WATCH_TAIL, *_FIND_TAIL]  # n_blocks, w, f, sources, count
_FOCUS_SIGNATURES = {
    "awpu_hip_focus_delays": (C.c_int, [_f32p, C.c_int32, C.c_double, C.c_double, C.c_double, _f32p]),
    "awpu_hip_focus_steer_table": (C.c_int, [_f32p, C.c_int32, _f64p, _f64p, _f64p, C.c_int32, _i32p, _f32p]),
    "awpu_hip_build_focus_table": (C.c_int, [_f32p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_double, C.c_int32, C.c_int32, _i32p, _f32p]),
    "awpu_hip_build_focus_table_device": (C.c_int, [C.c_int32, _f32p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_double, C.c_int32,
                                                    C.c_int32, _i32p, _f32p]),
    "awpu_hip_range": (C.c_int, [C.c_void_p, C.c_void_p, _f64p, _f64p, C.c_int32, _f64p, C.c_int32, _f32p, C.c_void_p]),
    "awpu_hip_range_pick": (C.c_int, [_f32p, C.c_int32, _f64p, C.c_int32, C.c_void_p]),
    "awpu_hip_locate_blocks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, *_LOCATE_TAIL, _f32p, _f64p, C.c_int32, C.c_void_p, _f32p]),
    "awpu_hip_locate_samples": (C.c_int, [C.c_void_p, _f32p, C.c_int64, *_LOCATE_TAIL, _f32p, _f64p, C.c_int32, C.c_void_p, _f32p]),
    "awpu_hip_locate_samples_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, *_LOCATE_TAIL, C.c_void_p, _f64p, C.c_int32, C.c_void_p,
                                                 C.c_void_p, C.c_void_p]),
}
FOCUS_SYMBOLS = tuple(_FOCUS_SIGNATURES)

# exposure: the entry points of include/awpu_hip_expose.h
EXPOSE_MEAN, EXPOSE_PEAK = 0, 1


class Expose(C.Structure):
    """awpu_expose_t (include/awpu_hip_expose.h)."""
    _fields_ = [
        ("length", C.c_int32),
        ("mode", C.c_int32),
    ]


_EXPOSE_TAIL = [*_WATCH_TAIL, C.POINTER(Expose), C.POINTER(Find)]  # n_blocks, w, e, f
_EXPOSE_SIGNATURES = {
    "awpu_hip_expose_count": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _i32p, _i32p, _i32p, _i32p, _i32p]),
    "awpu_hip_expose_rows": (C.c_int, [_f32p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Expose), _f32p, _f32p]),
    "awpu_hip_expose_rows_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Expose), C.c_void_p,
                                              C.c_void_p, C.c_void_p]),
    "awpu_hip_expose_blocks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, *_EXPOSE_TAIL, _f32p, _u8p, _u8p, _f32p, C.c_void_p, C.c_void_p]),
    "awpu_hip_expose_samples": (C.c_int, [C.c_void_p, _f32p, C.c_int64, *_EXPOSE_TAIL, _f32p, _u8p, _u8p, _f32p, C.c_void_p, C.c_void_p]),
    "awpu_hip_expose_samples_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, *_EXPOSE_TAIL, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]),
}
EXPOSE_SYMBOLS = tuple(_EXPOSE_SIGNATURES)

# coherence heatmaps: the entry points of include/awpu_hip_cohere.h
COHERE_WEIGHTED, COHERE_FACTOR = 0, 1


class Cohere(C.Structure):
    """awpu_cohere_t (include/awpu_hip_cohere.h)."""
    _fields_ = [
        ("show", C.c_int32),
    ]


_COHERE_TAIL = [*_WATCH_TAIL, C.POINTER(Cohere), C.POINTER(Find)]  # n_blocks, w, co, f
_COHERE_SIGNATURES = {
    "awpu_hip_cohere_host": (C.c_int, [_f32p, C.c_int32, C.c_int32, C.c_int32, _i32p, _f32p, C.c_int32, C.c_int32, _i32p, C.c_int32, _f32p,
                                       _f32p, _f32p, _f32p, _f32p, _f32p]),
    "awpu_hip_cohere": (C.c_int, [C.c_void_p, _f32p, C.c_int32, _f32p, _f32p, _f32p]),
    "awpu_hip_cohere_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "awpu_hip_cohere_device_sums": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p]),
    "awpu_hip_cohere_blocks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, *_COHERE_TAIL, _u8p, _u8p, _f32p, C.c_void_p, C.c_void_p]),
    "awpu_hip_cohere_samples": (C.c_int, [C.c_void_p, _f32p, C.c_int64, *_COHERE_TAIL, _u8p, _u8p, _f32p, C.c_void_p, C.c_void_p]),
    "awpu_hip_cohere_samples_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, *_COHERE_TAIL, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p]),
}
COHERE_SYMBOLS = tuple(_COHERE_SIGNATURES)

# peeling sources: the entry points of include/awpu_hip_peel.h
PEEL_MAX_STEPS, PEEL_MAX_MICS = 32, 256
PEEL_MAP, PEEL_CLEAN, PEEL_RESIDUAL = 0, 1, 2  # what a peel run shows


class Peel(C.Structure):
    """awpu_peel_t (include/awpu_hip_peel.h)."""
    _fields_ = [
        ("steps", C.c_int32),
        ("gain", C.c_float),
        ("stop_ratio", C.c_float),
    ]


# numpy view of awpu_peel_step_t: what peel_host and Engine.peel return, `steps` records per frame (unused: pixel -1)
PEEL_STEP_DTYPE = np.dtype([("pixel", "<i4"), ("before", "<f4"), ("removed", "<f4")])
assert PEEL_STEP_DTYPE.itemsize == 12 and C.sizeof(Peel) == 12

_PEEL_TABLE = [C.c_int32, C.c_int32, _i32p, _f32p, C.c_int32, C.c_int32, _i32p, C.c_int32]  # n_streams, hist, off, frac, lut_stride, n_pixels, index, usable
_PEEL_TAIL = [*_WATCH_TAIL, C.POINTER(Peel), C.c_int32, C.POINTER(Find)]  # n_blocks, w, pe, show, f
_PEEL_SIGNATURES = {
    "awpu_hip_peel_beam_length": (C.c_int32, _PEEL_TABLE),
    "awpu_hip_peel_step_host": (C.c_int, [_f32p, C.c_int32, *_PEEL_TABLE, _f32p, _i32p, C.c_float, _f32p]),
    "awpu_hip_peel_host": (C.c_int, [_f32p, C.c_int32, *_PEEL_TABLE, _f32p, C.POINTER(Peel), C.c_void_p, _f32p, _f32p, _f32p, _f32p]),
    "awpu_hip_peel_step_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    "awpu_hip_peel": (C.c_int, [C.c_void_p, _f32p, C.c_int32, C.POINTER(Peel), C.c_void_p, _f32p, _f32p, _f32p, _f32p]),
    "awpu_hip_peel_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(Peel), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "awpu_hip_peel_blocks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, *_PEEL_TAIL, _u8p, _u8p, _f32p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "awpu_hip_peel_samples": (C.c_int, [C.c_void_p, _f32p, C.c_int64, *_PEEL_TAIL, _u8p, _u8p, _f32p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "awpu_hip_peel_samples_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, *_PEEL_TAIL, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p]),
}
PEEL_SYMBOLS = tuple(_PEEL_SIGNATURES)

# tone maps: the entry points of include/awpu_hip_tones.h
TONES_BINS = 129
TONES_RECT, TONES_HANN = 0, 1
TONES_SHOW_PITCH = -1


class Tones(C.Structure):
    """awpu_tones_t (include/awpu_hip_tones.h)."""
    _fields_ = [
        ("window", C.c_int32),
        ("n_groups", C.c_int32),
        ("edge", C.c_int32 * (TONES_BINS + 1)),
    ]


assert C.sizeof(Tones) == 528

_TONES_TAIL = [*_WATCH_TAIL, C.POINTER(Tones), C.c_int32, C.POINTER(Find)]  # n_blocks, w, t, show, f
_TONES_SIGNATURES = {
    "awpu_hip_tones_window": (C.c_int, [C.c_int32, _f32p]),
    "awpu_hip_tones_twiddles": (C.c_int, [_f32p]),
    "awpu_hip_tones_linear": (C.c_int, [C.c_float, C.c_float, C.c_int32, C.c_float, C.POINTER(Tones)]),
    "awpu_hip_tones_host": (C.c_int, [_f32p, C.c_int32, C.c_int32, C.c_int32, _i32p, _f32p, C.c_int32, C.c_int32, _i32p, C.c_int32, _f32p,
                                      C.POINTER(Tones), _f32p, _i32p, _f32p, _f32p]),
    "awpu_hip_tones": (C.c_int, [C.c_void_p, _f32p, C.c_int32, C.POINTER(Tones), _f32p, _i32p]),
    "awpu_hip_tones_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(Tones), C.c_void_p, C.c_void_p, C.c_void_p]),
    "awpu_hip_tones_device_bins": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(Tones), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p]),
    "awpu_hip_tones_blocks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, *_TONES_TAIL, _u8p, _u8p, _f32p, C.c_void_p, C.c_void_p]),
    "awpu_hip_tones_samples": (C.c_int, [C.c_void_p, _f32p, C.c_int64, *_TONES_TAIL, _u8p, _u8p, _f32p, C.c_void_p, C.c_void_p]),
    "awpu_hip_tones_samples_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, *_TONES_TAIL, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p]),
}
TONES_SYMBOLS = tuple(_TONES_SIGNATURES)

# cross-spectral maps: the entry points of include/awpu_hip_csm.h
CSM_MAX_BINS = 8
CSM_CONVENTIONAL, CSM_DIAGONAL_REMOVED, CSM_CAPON = 0, 1, 2


class Csm(C.Structure):
    """awpu_csm_t (include/awpu_hip_csm.h)."""
    _fields_ = [
        ("window", C.c_int32),
        ("n_bins", C.c_int32),
        ("bin", C.c_int32 * CSM_MAX_BINS),
        ("kind", C.c_int32),
        ("loading", C.c_float),
    ]


assert C.sizeof(Csm) == 48

_CSM_MICS = [_i32p, C.c_int32]  # index, usable
_CSM_SAMPLES = [_f32p, C.c_int64, C.c_int32, C.c_int32, *_CSM_MICS, _f32p, C.POINTER(Csm)]  # samples, pitch, n_streams, n_blocks, .., gain, c
_CSM_TABLE = [_i32p, _f32p, C.c_int32, C.c_int32, *_CSM_MICS, C.POINTER(Csm)]  # off, frac, lut_stride, n_pixels, .., c
_CSM_SIGNATURES = {
    "awpu_hip_csm_spectra_host": (C.c_int, [*_CSM_SAMPLES, _f32p]),
    "awpu_hip_csm_accumulate_host": (C.c_int, [*_CSM_SAMPLES, _f32p, _i32p]),
    "awpu_hip_csm_steer_host": (C.c_int, [*_CSM_TABLE, _f32p]),
    "awpu_hip_csm_map_host": (C.c_int, [_f32p, C.c_int32, *_CSM_TABLE, _f32p, _f32p]),
    "awpu_hip_csm_invert_host": (C.c_int, [_f32p, C.c_int32, C.c_int32, C.POINTER(Csm), _f32p]),
    "awpu_hip_csm_samples": (C.c_int, [C.c_void_p, _f32p, C.c_int64, C.c_int32, C.POINTER(Csm), _f32p, _i32p, _f32p]),
    "awpu_hip_csm_samples_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(Csm), C.c_void_p, _i32p, C.c_void_p,
                                              C.c_void_p]),
    "awpu_hip_csm_map": (C.c_int, [C.c_void_p, _f32p, C.c_int32, C.POINTER(Csm), _f32p, _f32p]),
    "awpu_hip_csm_map_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(Csm), C.c_void_p, C.c_void_p, C.c_void_p]),
}
CSM_SYMBOLS = tuple(_CSM_SIGNATURES)

# the loaded inverse with a written arithmetic (step 6a): the entry points of include/awpu_hip_csm_invert.h
CSM_INVERT_MAX_MICS = 512
_CSM_INVERT_SIGNATURES = {
    "awpu_hip_csm_invert_rule_host": (C.c_int, [_f32p, C.c_int32, C.c_int32, C.POINTER(Csm), _f32p, _i32p]),
    "awpu_hip_csm_invert": (C.c_int, [C.c_void_p, _f32p, C.c_int32, C.POINTER(Csm), _f32p]),
    "awpu_hip_csm_invert_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(Csm), C.c_void_p, C.c_void_p, C.c_void_p]),
}
CSM_INVERT_SYMBOLS = tuple(_CSM_INVERT_SIGNATURES)

# cross-spectral runs: the entry points of include/awpu_hip_csm_watch.h
CSM_SHOW_SUM = -1
CSM_MAX_LENGTH = 1024
# w, c, length, show, f, carry, carried, then image, big_image, power, sources, count, planes, solved
_CSM_WATCH_HOST = [C.POINTER(Watch), C.POINTER(Csm), C.c_int32, C.c_int32, C.POINTER(Find), _f32p, _i32p, _u8p, _u8p, _f32p, C.c_void_p,
                   C.c_void_p, _f32p, _i32p]
_CSM_WATCH_SIGNATURES = {
    "awpu_hip_csm_watch_blocks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, *_CSM_WATCH_HOST]),
    "awpu_hip_csm_watch_samples": (C.c_int, [C.c_void_p, _f32p, C.c_int64, C.c_int32, *_CSM_WATCH_HOST]),
    "awpu_hip_csm_watch_samples_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(Watch), C.POINTER(Csm), C.c_int32,
                                                    C.c_int32, C.POINTER(Find), C.c_void_p, _i32p, *([C.c_void_p] * 8)]),
}
CSM_WATCH_SYMBOLS = tuple(_CSM_WATCH_SIGNATURES)

# CLEAN-SC (step 7): the entry points of include/awpu_hip_csm_clean.h
CSM_CLEAN_MAX_STEPS = 32


class CsmClean(C.Structure):
    """awpu_csm_clean_t (include/awpu_hip_csm_clean.h)."""
    _fields_ = [
        ("steps", C.c_int32),
        ("gain", C.c_float),
        ("stop_ratio", C.c_float),
    ]


# numpy view of awpu_csm_clean_step_t: `steps` records per bin (unused: pixel -1)
CSM_CLEAN_STEP_DTYPE = np.dtype([("pixel", "<i4"), ("before", "<f4"), ("removed", "<f4")])
assert CSM_CLEAN_STEP_DTYPE.itemsize == 12 and C.sizeof(CsmClean) == 12

CSM_CLEAN_MAP, CSM_CLEAN_CLEAN, CSM_CLEAN_RESIDUAL = 0, 1, 2  # what a CLEAN-SC run shows
# w, c, length, show, f, carry, carried, cl, what, then image, big_image, power, sources, count, planes, steps
_CSM_CLEAN_RUN_HOST = [C.POINTER(Watch), C.POINTER(Csm), C.c_int32, C.c_int32, C.POINTER(Find), _f32p, _i32p, C.POINTER(CsmClean), C.c_int32,
                       _u8p, _u8p, _f32p, C.c_void_p, C.c_void_p, _f32p, C.c_void_p]
_CSM_CLEAN_SIGNATURES = {
    "awpu_hip_csm_clean_step_host": (C.c_int, [_f32p, _i32p, C.c_float, *_CSM_TABLE, _f32p, _f32p]),
    "awpu_hip_csm_clean_host": (C.c_int, [_f32p, C.c_int32, *_CSM_TABLE, C.POINTER(CsmClean), C.c_void_p, _f32p, _f32p, _f32p, _f32p]),
    "awpu_hip_csm_clean_step_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Csm), C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "awpu_hip_csm_clean": (C.c_int, [C.c_void_p, _f32p, C.c_int32, C.POINTER(Csm), C.POINTER(CsmClean), C.c_void_p, _f32p, _f32p, _f32p, _f32p]),
    "awpu_hip_csm_clean_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(Csm), C.POINTER(CsmClean), *([C.c_void_p] * 6)]),
    "awpu_hip_csm_clean_blocks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, *_CSM_CLEAN_RUN_HOST]),
    "awpu_hip_csm_clean_samples": (C.c_int, [C.c_void_p, _f32p, C.c_int64, C.c_int32, *_CSM_CLEAN_RUN_HOST]),
    "awpu_hip_csm_clean_samples_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(Watch), C.POINTER(Csm), C.c_int32,
                                                    C.c_int32, C.POINTER(Find), C.c_void_p, _i32p, C.POINTER(CsmClean), C.c_int32,
                                                    *([C.c_void_p] * 8)]),
}
CSM_CLEAN_SYMBOLS = tuple(_CSM_CLEAN_SIGNATURES)

# the eigendecomposition and the subspace maps (step 8): the entry points of include/awpu_hip_csm_eig.h
CSM_EIG_MUSIC, CSM_EIG_FUNCTIONAL = 0, 1
CSM_EIG_MAX_MICS, CSM_EIG_MAX_SWEEPS, CSM_EIG_MAX_ROOT = 256, 32, 6


class CsmEig(C.Structure):
    """awpu_csm_eig_t (include/awpu_hip_csm_eig.h)."""
    _fields_ = [
        ("kind", C.c_int32),
        ("n_sources", C.c_int32),
        ("root", C.c_int32),
        ("reserved", C.c_int32),
    ]


assert C.sizeof(CsmEig) == 16

_CSM_EIG_SIGNATURES = {
    "awpu_hip_csm_eig_host": (C.c_int, [_f32p, C.c_int32, C.c_int32, C.POINTER(Csm), _f32p, _f32p, _i32p, _i32p]),
    "awpu_hip_csm_eig_weigh_host": (C.c_int, [_f32p, _f32p, C.c_int32, C.POINTER(Csm), C.POINTER(CsmEig), _f32p]),
    "awpu_hip_csm_eig_map_host": (C.c_int, [_f32p, _i32p, *_CSM_TABLE, C.POINTER(CsmEig), _f32p]),
    "awpu_hip_csm_eig": (C.c_int, [C.c_void_p, _f32p, C.c_int32, C.POINTER(Csm), _f32p, _f32p, _i32p, _i32p]),
    "awpu_hip_csm_eig_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(Csm), *([C.c_void_p] * 5)]),
    "awpu_hip_csm_eig_weigh_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Csm), C.POINTER(CsmEig), C.c_void_p, C.c_void_p]),
    "awpu_hip_csm_eig_map": (C.c_int, [C.c_void_p, _f32p, C.c_int32, C.POINTER(Csm), C.POINTER(CsmEig), _f32p, _f32p, _i32p]),
    "awpu_hip_csm_eig_map_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(Csm), C.POINTER(CsmEig), *([C.c_void_p] * 4)]),
}
CSM_EIG_SYMBOLS = tuple(_CSM_EIG_SIGNATURES)

# every table above, one per public header: what load() sets the types of
_ALL_SIGNATURES = (_SIGNATURES, _TRACK_SIGNATURES, _BLOCK_SIGNATURES, _LISTEN_SIGNATURES, _WATCH_SIGNATURES, _FIND_SIGNATURES, _BAND_SIGNATURES,
                   _FOCUS_SIGNATURES, _SPECTRAL_SIGNATURES, _EXPOSE_SIGNATURES, _COHERE_SIGNATURES, _PEEL_SIGNATURES,
                   _TONES_SIGNATURES, _CSM_SIGNATURES, _CSM_INVERT_SIGNATURES, _CSM_WATCH_SIGNATURES, _CSM_CLEAN_SIGNATURES)
# ... and the tables of later headers, which load() walks behind those
_LATER_SIGNATURES = (_CSM_EIG_SIGNATURES,)

# numpy view of awpu_range_t: what range_pick, Engine.range and Engine.locate_* return (unused entries: index -1)
RANGE_DTYPE = np.dtype([("index", "<i4"), ("power", "<f4"), ("distance", "<f8")], align=True)
assert RANGE_DTYPE.itemsize == C.sizeof(Range) == 16

# numpy view of awpu_source_t: what find_peaks and Engine.find_* return, max_sources records per frame
SOURCE_DTYPE = np.dtype([("pixel", "<i4"), ("power", "<f4"), ("row", "<f8"), ("col", "<f8"), ("theta", "<f8"), ("phi", "<f8")], align=True)
assert SOURCE_DTYPE.itemsize == C.sizeof(Source) == 40

# numpy view of awpu_particle_t: what Engine.track returns, one record per particle
PARTICLE_DTYPE = np.dtype([("theta", "<f8"), ("phi", "<f8"), ("spread", "<f8"), ("rate", "<f8"), ("steps", "<i4"),
                           ("error", "<f4"), ("grad_theta", "<f8"), ("grad_phi", "<f8"), ("radius", "<f8"),
                           ("power", "<f4", (4,))], align=True)
assert PARTICLE_DTYPE.itemsize == C.sizeof(Particle) == 80


def load(build: bool = True) -> C.CDLL:
    """Load (building first if stale) the in-tree libawpu_hip.so."""
    global _lib
    if _lib is not None:
        return _lib
    # AWPU_NO_BUILD=1: never start a compiler from this process (set by the profiling scripts: under rocprofv3
    # a child process inherits the profiler's preloaded library, see tools/pmc.sh)
    if os.environ.get("AWPU_NO_BUILD") == "1":
        build = False
    path = _build.build_library() if build else _build.LIB_PATH
    # PyTorch-ROCm wheels bundle their own libamdhip64.so.7; a process that uses both torch and
    # this library must run on ONE HIP runtime, and the first one loaded wins the SONAME.  Load
    # torch's first when torch is installed, so that libawpu_hip.so binds to the same runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not path.exists():
        raise RuntimeError(f"{path} is missing and there is no CPU fallback")
    lib = C.CDLL(str(path))
    for table in _ALL_SIGNATURES + _LATER_SIGNATURES:
        for name, (res, args) in table.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
    _lib = lib
    return lib


@contextlib.contextmanager
def loaded_library(lib: C.CDLL):
    """Within the block load() hands out `lib` -- a variant build whose entry points the caller has typed -- in place of this
    build's; an Engine keeps the library it was created with, so one made in the block stays on `lib` after it."""
    global _lib
    mine, _lib = load(), lib
    try:
        yield lib
    finally:
        _lib = mine


def _check(status: int, where: str) -> None:
    if status != OK:
        lib = load()
        detail = lib.awpu_hip_strerror(status).decode()
        last = lib.awpu_hip_last_error().decode()
        raise AwpuError(status, where, f"{detail}; {last}" if last else detail)


def _f32(a: np.ndarray):
    # (the buffer protocol is 5 x cheaper than ndarray.ctypes -- 0.7 against 3.5 us per argument on the build host -- and the one-frame
    # call is ~45 us in all; read-only or empty arrays take the general path)
    try:
        return C.byref(C.c_float.from_buffer(a))
    except (TypeError, ValueError):
        return a.ctypes.data_as(_f32p)


def _i32(a: np.ndarray):
    return a.ctypes.data_as(_i32p)


def _f64_vector(x) -> np.ndarray:
    """A scalar or sequence as the contiguous 1-D float64 array the calls take angles and distances as."""
    return np.ascontiguousarray(np.atleast_1d(x), np.float64)


def _ref(struct):
    """An optional structure as a call's argument: by reference, or a null pointer for None (a run without `find`)."""
    return None if struct is None else C.byref(struct)


def _dev(*pointers):
    """Device addresses (integers; 0 = not given) and a stream as the void pointers a call takes."""
    return [C.c_void_p(p) for p in pointers]


def _wire_blocks(wire, stride: int):
    """(the bytes of wire datagrams `stride` bytes apart, how many blocks of 256 they are)."""
    buf = np.frombuffer(wire, dtype=np.uint8)
    if stride < DATAGRAM_BYTES or buf.size % (256 * stride) or buf.size == 0:
        raise ValueError(f"wire must be a whole number of blocks of 256 datagrams {stride} bytes apart")
    return buf, buf.size // (256 * stride)


def _find_struct(rows: int, cols: int, find: Optional[dict]) -> Optional[Find]:
    """find_peaks' keywords as the awpu_find_t of a run on a rows x cols grid; None (no find request) stays None."""
    if find is None:
        return None
    return Find(rows, cols, find.get("radius", 2), find.get("max_sources", 4), find.get("min_power", 0.0), find.get("min_ratio", 0.0),
                find.get("fov_deg", 180.0))


def _watch_struct(rows: int, cols: int, first: int, every: int, out_rows: int = 0, out_cols: int = 0, d_colormap_ptr: int = 0,
                  flip: bool = False) -> Watch:
    """The display keywords of a run's method as its awpu_watch_t: the run helpers take them as **shown and hand them on here."""
    return Watch(first, every, rows, cols, out_rows, out_cols, int(flip), C.c_void_p(d_colormap_ptr))


def _out_ptr(a: Optional[np.ndarray], ctype=None):
    """An output array as a call's argument: one that is wanted is never a null pointer, not even with no frame to write."""
    if a is None:
        return None
    return C.c_void_p(a.ctypes.data or 16) if ctype is None else C.cast(C.c_void_p(a.ctypes.data or 16), ctype)


# ----------------------------------------------------------------------------- geometry


def create_antenna(columns: int = 8, rows: int = 8, distance: float = 0.02) -> np.ndarray:
    """create_antenna, src/geometry/antenna.cpp:60-87 -> xyz[3, rows*columns]."""
    xyz = np.empty((3, rows * columns), np.float32)
    _check(load().awpu_hip_create_antenna(columns, rows, distance, _f32(xyz)), "create_antenna")
    return xyz


def create_tiled_antenna(arrays_x: int, arrays_y: int, distance: float = 0.02) -> np.ndarray:
    xyz = np.empty((3, 64 * arrays_x * arrays_y), np.float32)
    _check(load().awpu_hip_create_tiled_antenna(arrays_x, arrays_y, distance, _f32(xyz)),
           "create_tiled_antenna")
    return xyz


def steering_delays(xyz: np.ndarray, theta: float, phi: float) -> np.ndarray:
    """steering_vector_spherical, src/geometry/antenna.cpp:126-129."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    tau = np.empty(xyz.shape[1], np.float32)
    _check(load().awpu_hip_steering_delays(_f32(xyz), xyz.shape[1], theta, phi, _f32(tau)),
           "steering_delays")
    return tau


def build_delay_table(xyz: np.ndarray, rows: int, columns: int, fov_deg: float = 180.0,
                      row_begin: int = 0, row_count: Optional[int] = None):
    """MIMOWorker::computeDelayLUT, src/dsp/mimo.cpp:20-59 -> (off, frac) [row_count*columns, n]."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    n = xyz.shape[1]
    row_count = rows - row_begin if row_count is None else row_count
    off = np.empty((row_count * columns, n), np.int32)
    frac = np.empty((row_count * columns, n), np.float32)
    _check(load().awpu_hip_build_delay_table(_f32(xyz), n, rows, columns, fov_deg, row_begin,
                                             row_count, _i32(off), _f32(frac)), "build_delay_table")
    return off, frac


def build_delay_table_device(xyz: np.ndarray, rows: int, columns: int, fov_deg: float = 180.0,
                             row_begin: int = 0, row_count: Optional[int] = None, device: int = 0):
    """The same table, its rows x columns x n part computed on HIP device `device` (bit-identical to build_delay_table)."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    n = xyz.shape[1]
    row_count = rows - row_begin if row_count is None else row_count
    off = np.empty((row_count * columns, n), np.int32)
    frac = np.empty((row_count * columns, n), np.float32)
    _check(load().awpu_hip_build_delay_table_device(device, _f32(xyz), n, rows, columns, fov_deg, row_begin,
                                                    row_count, _i32(off), _f32(frac)), "build_delay_table_device")
    return off, frac


def steer_table(xyz: np.ndarray, theta, phi):
    """Particle::steer (src/dsp/particle.cpp:37-49) for a batch of directions -> (off, frac) [n_dir, n]."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    theta = _f64_vector(theta)
    phi = _f64_vector(phi)
    if theta.shape != phi.shape or theta.ndim != 1:
        raise ValueError("theta and phi must be 1-D and alike")
    n = xyz.shape[1]
    off = np.empty((theta.size, n), np.int32)
    frac = np.empty((theta.size, n), np.float32)
    dp = C.POINTER(C.c_double)
    _check(load().awpu_hip_steer_table(_f32(xyz), n, theta.ctypes.data_as(dp), phi.ctypes.data_as(dp), theta.size,
                                       _i32(off), _f32(frac)), "steer_table")
    return off, frac


def focus_delays(xyz: np.ndarray, theta: float, phi: float, distance: float) -> np.ndarray:
    """The delays [n] (samples, minimum 0) that focus the elements xyz on the point `distance` metres along (theta, phi): the rule
    of include/awpu_hip_focus.h (awpu_hip_focus_delays); distance inf = steering_delays, bit for bit."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    tau = np.empty(xyz.shape[1], np.float32)
    _check(load().awpu_hip_focus_delays(_f32(xyz), xyz.shape[1], theta, phi, distance, _f32(tau)), "awpu_hip_focus_delays")
    return tau


def focus_steer_table(xyz: np.ndarray, theta, phi, distance):
    """steer_table with a focus distance per direction (scalars broadcast) -> (off, frac) [n_dir, n] (awpu_hip_focus_steer_table)."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    theta, phi, distance = np.broadcast_arrays(np.atleast_1d(np.asarray(theta, np.float64)), np.atleast_1d(np.asarray(phi, np.float64)),
                                               np.atleast_1d(np.asarray(distance, np.float64)))
    if theta.ndim != 1:
        raise ValueError("theta, phi and distance must be 1-D and alike")
    theta, phi, distance = (np.ascontiguousarray(a) for a in (theta, phi, distance))
    n = xyz.shape[1]
    off = np.empty((theta.size, n), np.int32)
    frac = np.empty((theta.size, n), np.float32)
    _check(load().awpu_hip_focus_steer_table(_f32(xyz), n, theta.ctypes.data_as(_f64p), phi.ctypes.data_as(_f64p),
                                             distance.ctypes.data_as(_f64p), theta.size, _i32(off), _f32(frac)), "awpu_hip_focus_steer_table")
    return off, frac


def build_focus_table(xyz: np.ndarray, rows: int, columns: int, distance: float, fov_deg: float = 180.0, row_begin: int = 0,
                      row_count: Optional[int] = None):
    """build_delay_table with every pixel focused `distance` metres along its direction -> (off, frac) [row_count*columns, n]
    (awpu_hip_build_focus_table); Engine.set_delay_table takes it as it is."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    n = xyz.shape[1]
    row_count = rows - row_begin if row_count is None else row_count
    off = np.empty((max(row_count, 0) * columns, n), np.int32)
    frac = np.empty((max(row_count, 0) * columns, n), np.float32)
    _check(load().awpu_hip_build_focus_table(_f32(xyz), n, rows, columns, fov_deg, distance, row_begin, row_count, _i32(off), _f32(frac)),
           "awpu_hip_build_focus_table")
    return off, frac


def build_focus_table_device(xyz: np.ndarray, rows: int, columns: int, distance: float, fov_deg: float = 180.0, row_begin: int = 0,
                             row_count: Optional[int] = None, device: int = 0):
    """The same table, its rows x columns x n part computed on HIP device `device` (bit-identical to build_focus_table)."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    n = xyz.shape[1]
    row_count = rows - row_begin if row_count is None else row_count
    off = np.empty((max(row_count, 0) * columns, n), np.int32)
    frac = np.empty((max(row_count, 0) * columns, n), np.float32)
    _check(load().awpu_hip_build_focus_table_device(device, _f32(xyz), n, rows, columns, fov_deg, distance, row_begin, row_count,
                                                    _i32(off), _f32(frac)), "awpu_hip_build_focus_table_device")
    return off, frac


def range_candidates(lo: float, hi: float, n: int) -> np.ndarray:
    """n candidate distances from lo to hi metres (hi may be inf), uniform in 1 / d: where range_pick's refinement is exact for a
    peak that is a parabola in 1 / d."""
    with np.errstate(divide="ignore"):
        return 1.0 / np.linspace(1.0 / lo, 1.0 / hi, int(n))


def range_pick(power: np.ndarray, distance) -> np.ndarray:
    """Which candidate distance wins for every row of power [n_src, n_dist], refined between the candidates -> RANGE_DTYPE records
    [n_src] (awpu_hip_range_pick: the rule of include/awpu_hip_focus.h as executable C)."""
    power = np.ascontiguousarray(power, np.float32)
    distance = _f64_vector(distance)
    power = power.reshape(-1, max(distance.size, 1))
    best = np.zeros(len(power), RANGE_DTYPE)
    _check(load().awpu_hip_range_pick(_f32(power), len(power), distance.ctypes.data_as(_f64p), distance.size,
                                      best.ctypes.data_as(C.c_void_p)), "awpu_hip_range_pick")
    return best


def resize_linear_u8(pix: np.ndarray, out_rows: int, out_cols: int) -> np.ndarray:
    """cv::resize(..., INTER_LINEAR) of AWProcessingUnit::draw, src/aw_processing_unit/aw_processing_unit.cpp:252
    (8-bit single channel, upscaling only), on the host."""
    pix = np.ascontiguousarray(pix, np.uint8)
    if pix.ndim != 2:
        raise ValueError("pix must be [rows][cols]")
    out = np.empty((out_rows, out_cols), np.uint8)
    _check(load().awpu_hip_resize_linear_u8(pix.ctypes.data_as(_u8p), pix.shape[0], pix.shape[1],
                                            out.ctypes.data_as(_u8p), out_rows, out_cols), "resize_linear_u8")
    return out


def heatmap_u8(power: np.ndarray) -> np.ndarray:
    """MIMOWorker::populateHeatmap (USE_DB 0), src/dsp/mimo.cpp:61-95."""
    power = np.ascontiguousarray(power, np.float32)
    pix = np.empty(power.shape, np.uint8)
    _check(load().awpu_hip_heatmap_u8(_f32(power), power.size, pix.ctypes.data_as(_u8p)), "heatmap_u8")
    return pix


# ------------------------------------------------------------------------------- engine


class TrackResult:
    """What Engine.track hands back: the particles after the call and the call's reference power / beams."""

    def __init__(self, particles: np.ndarray, reference: float, beams: Optional[np.ndarray]):
        self.particles = particles
        self.reference = reference
        self.beams = beams

    def __getattr__(self, name):
        if name in PARTICLE_DTYPE.names:
            return self.particles[name]
        raise AttributeError(name)

    def __len__(self):
        return self.particles.size


class ListenResult:
    """What Engine.listen_* hand back: .audio [n, 256 * n_blocks] (a row = a listener's channel at 48 828 Hz), .listeners
    (PARTICLE_DTYPE records after the run: pass them as `theta` to the next call to carry the trackers on), .trail
    [n_blocks, n] records or None, .power [n_blocks, pixels] or None; .theta, .phi, ... are the listeners' fields."""

    def __init__(self, audio, listeners: np.ndarray, trail, power):
        self.audio = audio
        self.listeners = listeners
        self.trail = trail
        self.power = power

    def __getattr__(self, name):
        if name in PARTICLE_DTYPE.names:
            return self.listeners[name]
        raise AttributeError(name)

    def __len__(self):
        return self.listeners.size


class WatchResult:
    """What Engine.watch_* hand back: .image [n_frames, rows, cols] uint8 or None, .big [n_frames, out_rows, out_cols] (x 3 with a
    colour table) or None, .power [n_frames, pixels] or None, and .next_first: the `first` of the call that continues the
    recording.  Frame j shows block first + j * every of the call."""

    def __init__(self, image, big, power, next_first: int):
        self.image = image
        self.big = big
        self.power = power
        self.next_first = next_first

    def __len__(self):
        return next(len(a) for a in (self.image, self.big, self.power) if a is not None)


def watch_count(n_blocks: int, first: int, every: int):
    """(frames a call of n_blocks blocks shows, the `first` of the call that continues it) (awpu_hip_watch_count)."""
    n, nxt = C.c_int32(0), C.c_int32(0)
    _check(load().awpu_hip_watch_count(n_blocks, first, every, C.byref(n), C.byref(nxt)), "awpu_hip_watch_count")
    return int(n.value), int(nxt.value)


class FindResult:
    """What find_peaks and Engine.find_* hand back: .sources [n_frames, max_sources] SOURCE_DTYPE records (unused entries:
    pixel -1), .count [n_frames], .power [n_frames, pixels] or None, .next_first (the run forms: the `first` of the call that
    continues the recording); .pixel, .row, .col, .theta, .phi are the records' fields.  Frame j of a run form is block first +
    j * every of the call."""

    def __init__(self, sources: np.ndarray, count: np.ndarray, power=None, next_first: int = 0):
        self.sources = sources
        self.count = count
        self.power = power
        self.next_first = next_first

    def __getattr__(self, name):
        if name in SOURCE_DTYPE.names:
            return self.sources[name]
        raise AttributeError(name)

    def __len__(self):
        return len(self.count)


class LocateResult(FindResult):
    """What Engine.locate_* hand back: a FindResult plus .ranges [n_frames, max_sources] RANGE_DTYPE records (unused entries:
    index -1) and .range_power [n_frames, max_sources, n_dist] or None; .distance is the records' field."""

    def __init__(self, sources, count, power, next_first, ranges, range_power):
        super().__init__(sources, count, power, next_first)
        self.ranges = ranges
        self.range_power = range_power

    def __getattr__(self, name):
        if name == "distance":
            return self.ranges["distance"]
        return super().__getattr__(name)


def find_peaks(power: np.ndarray, rows: int, cols: int, radius: int = 2, max_sources: int = 4, min_power: float = 0.0,
               min_ratio: float = 0.0, fov_deg: float = 180.0) -> FindResult:
    """The strongest peaks of power rows [n_frames, rows * cols] (or one row) on the host: the rule of include/awpu_hip_find.h
    as executable C (awpu_hip_find_peaks)."""
    power = np.ascontiguousarray(power, np.float32).reshape(-1, rows * cols)
    f = Find(rows, cols, radius, max_sources, min_power, min_ratio, fov_deg)
    sources = np.empty((len(power), max(max_sources, 0)), SOURCE_DTYPE)
    count = np.empty(len(power), np.int32)
    _check(load().awpu_hip_find_peaks(_f32(power), len(power), C.byref(f), sources.ctypes.data_as(C.c_void_p),
                                      count.ctypes.data_as(C.c_void_p)), "awpu_hip_find_peaks")
    return FindResult(sources, count)


class ExposeResult:
    """What Engine.expose_* hand back: .image, .big, .power as a WatchResult has them -- of the exposed frames --, .sources and
    .count as a FindResult has them or None, .next_first (the `first` of the call that continues the recording) and .carry: the
    open window's row [pixels], to be passed as `carry` to that call.  Frame j is exposed over the `length` blocks that end with
    block first + j * every of the call."""

    def __init__(self, image, big, power, sources, count, next_first: int, carry):
        self.image = image
        self.big = big
        self.power = power
        self.sources = sources
        self.count = count
        self.next_first = next_first
        self.carry = carry

    def __getattr__(self, name):
        if name in SOURCE_DTYPE.names and self.__dict__.get("sources") is not None:
            return self.sources[name]
        raise AttributeError(name)

    def __len__(self):
        return next(len(a) for a in (self.image, self.big, self.power, self.count) if a is not None)


def expose_count(n_blocks: int, first: int, every: int, length: int):
    """(n_frames, next_first, carry_in, carry_out, n_swept) of a call of n_blocks blocks exposed over `length` blocks a frame
    (awpu_hip_expose_count)."""
    out = [C.c_int32(0) for _ in range(5)]
    _check(load().awpu_hip_expose_count(n_blocks, first, every, length, *[C.byref(v) for v in out]), "awpu_hip_expose_count")
    return tuple(int(v.value) for v in out)


def expose_rows(power: np.ndarray, first: int, every: int, length: int, mode: int = EXPOSE_MEAN, carry: Optional[np.ndarray] = None):
    """The rule of include/awpu_hip_expose.h as executable C (awpu_hip_expose_rows): power [n_blocks, n_pixels], every block's row
    -> (frames [n_frames, n_pixels], next_first).  `carry` [n_pixels] float32 is the open window: read where the first window began
    before these rows, written in place where the last one ends behind them; it may be None where neither is the case."""
    power = np.ascontiguousarray(power, np.float32)
    if power.ndim != 2 or power.size == 0:
        raise ValueError("power must be [n_blocks, n_pixels]")
    if carry is not None and (carry.dtype != np.float32 or carry.shape != (power.shape[1],) or not carry.flags.c_contiguous):
        raise ValueError("carry must be a contiguous float32 array [n_pixels]")
    e = Expose(length, mode)
    n_frames, next_first = watch_count(len(power), first, every) if every >= 1 and first >= 0 else (0, 0)
    frames = np.empty((n_frames, power.shape[1]), np.float32)
    _check(load().awpu_hip_expose_rows(_f32(power), len(power), power.shape[1], first, every, C.byref(e),
                                       None if carry is None else _f32(carry), C.cast(C.c_void_p(frames.ctypes.data or 16), _f32p)),
           "awpu_hip_expose_rows")
    return frames, next_first


def cohere_host(frames: np.ndarray, off: np.ndarray, frac: np.ndarray, index=None, gain=None, want_sums: bool = False):
    """The rule of include/awpu_hip_cohere.h as executable C (awpu_hip_cohere_host): frames [batch, n_streams, hist] (or one
    frame), off / frac [n_pixels, lut_stride], index = the active stream ids (default: all of the table's), gain [usable] in
    their order or None.  -> (power, coherence, weighted) [batch, n_pixels], with want_sums also (sums, energy) [batch, n_pixels,
    256]: out[] and e[] of every pixel; one frame in, rows without the batch axis out."""
    frames = np.ascontiguousarray(frames, np.float32)
    single = frames.ndim == 2
    if single:
        frames = frames[None]
    off = np.ascontiguousarray(off, np.int32)
    frac = np.ascontiguousarray(frac, np.float32)
    if frames.ndim != 3 or off.ndim != 2 or off.shape != frac.shape:
        raise ValueError("frames must be [batch, n_streams, hist], off and frac [n_pixels, lut_stride]")
    index = np.arange(off.shape[1], dtype=np.int32) if index is None else np.ascontiguousarray(index, np.int32)
    if gain is not None:
        gain = np.ascontiguousarray(gain, np.float32)
        if gain.shape != index.shape:
            raise ValueError("gain must be [usable], in the active list's order")
    batch, n_pixels = frames.shape[0], off.shape[0]
    maps = [np.empty((batch, n_pixels), np.float32) for _ in range(3)]
    wide = [np.empty((batch, n_pixels, 256), np.float32) for _ in range(2)] if want_sums else [None, None]
    _check(load().awpu_hip_cohere_host(_f32(frames), batch, frames.shape[1], frames.shape[2], _i32(off), _f32(frac), off.shape[1], n_pixels,
                                       _i32(index), len(index), None if gain is None else _f32(gain), *[_f32(m) for m in maps],
                                       *[None if m is None else _f32(m) for m in wide]), "awpu_hip_cohere_host")
    out = maps + wide if want_sums else maps
    return tuple(m[0] for m in out) if single else tuple(out)


def tones_window(window: int = TONES_RECT) -> np.ndarray:
    """The window table [256] of the rule of include/awpu_hip_tones.h (awpu_hip_tones_window)."""
    w = np.empty(256, np.float32)
    _check(load().awpu_hip_tones_window(int(window), _f32(w)), "awpu_hip_tones_window")
    return w


def tones_twiddles() -> np.ndarray:
    """The twiddle table [128, 2] of the rule: (cos, -sin) of 2 pi k / 256 (awpu_hip_tones_twiddles)."""
    t = np.empty((128, 2), np.float32)
    _check(load().awpu_hip_tones_twiddles(_f32(t)), "awpu_hip_tones_twiddles")
    return t


def tones_linear(lo_hz: float, hi_hz: float, n_groups: int = 1, window: int = TONES_RECT, sample_rate: float = 48828.125) -> Tones:
    """A Tones whose n_groups groups deal out the bins with centres in [lo_hz, hi_hz) as equally as possible (awpu_hip_tones_linear)."""
    t = Tones()
    t.window = int(window)
    _check(load().awpu_hip_tones_linear(float(lo_hz), float(hi_hz), int(n_groups), float(sample_rate), C.byref(t)), "awpu_hip_tones_linear")
    return t


def tones_of(groups, window: int = TONES_RECT, sample_rate: float = 48828.125) -> Tones:
    """A Tones from a Tones (returned as it is), a list or array of edges (n_groups + 1 ascending bins) or a tuple
    (lo_hz, hi_hz, n_groups) for tones_linear.  The edges are not judged here: the library refuses a bad request."""
    if isinstance(groups, Tones):
        return groups
    if isinstance(groups, tuple) and len(groups) == 3:
        return tones_linear(groups[0], groups[1], groups[2], window, sample_rate)
    edges = [int(e) for e in groups]
    if not 2 <= len(edges) <= TONES_BINS + 1:
        raise ValueError("edges are n_groups + 1 bins, n_groups in [1, 129]")
    t = Tones()
    t.window, t.n_groups = int(window), len(edges) - 1
    for g, e in enumerate(edges):
        t.edge[g] = e
    return t


def tones_from_text(text: str, sample_rate: float = 48828.125) -> Tones:
    """'LO:HI[:hann]' (Hz; the rectangular window unless 'hann' is given), as the tools' --tone and --pitch take it -> a Tones with
    the one group of bins whose centres lie in [LO, HI)."""
    parts = text.split(":")
    if len(parts) not in (2, 3) or (len(parts) == 3 and parts[2] != "hann"):
        raise ValueError(f"tone '{text}': LO:HI or LO:HI:hann, in Hz")
    lo, hi = float(parts[0]), float(parts[1])
    if not 0.0 <= lo < hi:
        raise ValueError(f"tone '{text}': 0 <= LO < HI")
    try:
        return tones_linear(lo, hi, 1, TONES_HANN if len(parts) == 3 else TONES_RECT, sample_rate)
    except AwpuError:
        raise ValueError(f"tone '{text}': no bin of {sample_rate / 256:.1f} Hz has its centre in that range") from None


def tones_edges(t: Tones) -> np.ndarray:
    """edge[0 .. n_groups] of a Tones."""
    return np.array(t.edge[:t.n_groups + 1], np.int32)


def tones_host(frames: np.ndarray, off: np.ndarray, frac: np.ndarray, groups, window: int = TONES_RECT, index=None, gain=None,
               want=("tone", "pitch")):
    """The rule of include/awpu_hip_tones.h as executable C (awpu_hip_tones_host): frames, off, frac, index and gain as cohere_host
    takes them, groups as tones_of does.  -> a dict of the outputs named in `want`: "tone" [batch, n_groups, n_pixels], "pitch"
    [batch, n_pixels] int32, "bins" [batch, n_pixels, 129], "spectrum" [batch, n_pixels, 129, 2]; one frame in, arrays without
    the batch axis out."""
    t = tones_of(groups, window)
    frames = np.ascontiguousarray(frames, np.float32)
    single = frames.ndim == 2
    if single:
        frames = frames[None]
    off = np.ascontiguousarray(off, np.int32)
    frac = np.ascontiguousarray(frac, np.float32)
    if frames.ndim != 3 or off.ndim != 2 or off.shape != frac.shape:
        raise ValueError("frames must be [batch, n_streams, hist], off and frac [n_pixels, lut_stride]")
    index = np.arange(off.shape[1], dtype=np.int32) if index is None else np.ascontiguousarray(index, np.int32)
    if gain is not None:
        gain = np.ascontiguousarray(gain, np.float32)
        if gain.shape != index.shape:
            raise ValueError("gain must be [usable], in the active list's order")
    batch, n_pixels = frames.shape[0], off.shape[0]
    shapes = {"tone": ((batch, max(t.n_groups, 0), n_pixels), np.float32), "pitch": ((batch, n_pixels), np.int32),
              "bins": ((batch, n_pixels, TONES_BINS), np.float32), "spectrum": ((batch, n_pixels, TONES_BINS, 2), np.float32)}
    if not want or any(name not in shapes for name in want):
        raise ValueError(f"want names some of {tuple(shapes)}")
    out = {name: np.empty(*shapes[name]) for name in shapes if name in want}
    ptr = lambda name: _out_ptr(out.get(name), _i32p if name == "pitch" else _f32p)
    _check(load().awpu_hip_tones_host(_f32(frames), batch, frames.shape[1], frames.shape[2], _i32(off), _f32(frac), off.shape[1], n_pixels,
                                      _i32(index), len(index), None if gain is None else _f32(gain), C.byref(t), ptr("tone"), ptr("pitch"),
                                      ptr("bins"), ptr("spectrum")), "awpu_hip_tones_host")
    return {name: a[0] for name, a in out.items()} if single else out


def csm_of(bins, window: int = TONES_RECT, kind: int = CSM_CONVENTIONAL, loading: float = 0.0) -> Csm:
    """The Csm of a list of bins (or a Csm, passed through).  Nothing is judged here: the library refuses a bad request."""
    if isinstance(bins, Csm):
        return bins
    c = Csm()
    bins = [int(b) for b in np.atleast_1d(bins)]
    c.window, c.n_bins, c.kind, c.loading = int(window), len(bins), int(kind), float(loading)
    for i, b in enumerate(bins[:CSM_MAX_BINS]):
        c.bin[i] = b
    return c


def _csm_samples(samples, index, gain, n_blocks):
    """(samples [n_streams, pitch] as contiguous floats, index, gain or None, n_blocks) as the csm host calls take them."""
    samples = np.ascontiguousarray(samples, np.float32)
    if samples.ndim != 2:
        raise ValueError("samples must be [n_streams, pitch]")
    index = np.arange(samples.shape[0], dtype=np.int32) if index is None else np.ascontiguousarray(index, np.int32)
    if gain is not None:
        gain = np.ascontiguousarray(gain, np.float32)
        if gain.shape != index.shape:
            raise ValueError("gain must be [usable], in the active list's order")
    return samples, index, gain, samples.shape[1] // 256 if n_blocks is None else int(n_blocks)


def _csm_table(off, frac, index):
    off = np.ascontiguousarray(off, np.int32)
    frac = np.ascontiguousarray(frac, np.float32)
    if off.ndim != 2 or off.shape != frac.shape:
        raise ValueError("off and frac must be [n_pixels, lut_stride]")
    index = np.arange(off.shape[1], dtype=np.int32) if index is None else np.ascontiguousarray(index, np.int32)
    return off, frac, index


def csm_spectra_host(samples: np.ndarray, bins, window: int = TONES_RECT, index=None, gain=None, n_blocks: Optional[int] = None) -> np.ndarray:
    """Step 1 of the rule of include/awpu_hip_csm.h (awpu_hip_csm_spectra_host): samples [n_streams, pitch], the first n_blocks
    blocks of 256 (default: all whole ones) -> spectra [n_blocks, n_bins, usable, 2]."""
    c = csm_of(bins, window)
    samples, index, gain, n_blocks = _csm_samples(samples, index, gain, n_blocks)
    out = np.empty((max(n_blocks, 0), max(c.n_bins, 0), len(index), 2), np.float32)
    _check(load().awpu_hip_csm_spectra_host(_f32(samples), samples.shape[1], samples.shape[0], n_blocks, _i32(index), len(index),
                                            None if gain is None else _f32(gain), C.byref(c), _out_ptr(out, _f32p)), "awpu_hip_csm_spectra_host")
    return out


def csm_accumulate_host(samples: np.ndarray, bins, window: int = TONES_RECT, index=None, gain=None, matrix: Optional[np.ndarray] = None,
                        block_count: int = 0, n_blocks: Optional[int] = None):
    """Steps 1 and 2 (awpu_hip_csm_accumulate_host): adds the blocks of samples [n_streams, pitch] into `matrix`
    [n_bins, usable, usable, 2] (default: a new one of zeros; one given is added into in place) -> (matrix, block_count + n_blocks)."""
    c = csm_of(bins, window)
    samples, index, gain, n_blocks = _csm_samples(samples, index, gain, n_blocks)
    shape = (max(c.n_bins, 0), len(index), len(index), 2)
    if matrix is None:
        matrix = np.zeros(shape, np.float32)
    if matrix.dtype != np.float32 or matrix.shape != shape or not matrix.flags.c_contiguous:
        raise ValueError(f"matrix must be contiguous float32 {shape}")
    count = C.c_int32(block_count)
    _check(load().awpu_hip_csm_accumulate_host(_f32(samples), samples.shape[1], samples.shape[0], n_blocks, _i32(index), len(index),
                                               None if gain is None else _f32(gain), C.byref(c), _out_ptr(matrix, _f32p),
                                               C.cast(C.byref(count), _i32p)), "awpu_hip_csm_accumulate_host")
    return matrix, count.value


def csm_steer_host(off: np.ndarray, frac: np.ndarray, bins, index=None) -> np.ndarray:
    """Step 3 (awpu_hip_csm_steer_host): off, frac [n_pixels, lut_stride] -> steer [n_pixels, n_bins, usable, 2]."""
    c = csm_of(bins)
    off, frac, index = _csm_table(off, frac, index)
    out = np.empty((off.shape[0], max(c.n_bins, 0), len(index), 2), np.float32)
    _check(load().awpu_hip_csm_steer_host(_i32(off), _f32(frac), off.shape[1], off.shape[0], _i32(index), len(index), C.byref(c),
                                          _out_ptr(out, _f32p)), "awpu_hip_csm_steer_host")
    return out


def csm_map_host(matrix: np.ndarray, block_count: int, off: np.ndarray, frac: np.ndarray, bins, window: int = TONES_RECT,
                 kind: int = CSM_CONVENTIONAL, index=None, want=("map",)):
    """Steps 3 to 5 (awpu_hip_csm_map_host) of matrix [n_bins, usable, usable, 2] -- C with its block count, or for CSM_CAPON the
    inverse csm_invert_host made -> a dict of the outputs named in `want`: "map" and "q", each [n_bins, n_pixels]."""
    c = csm_of(bins, window, kind)
    off, frac, index = _csm_table(off, frac, index)
    matrix = np.ascontiguousarray(matrix, np.float32)
    if matrix.shape != (max(c.n_bins, 0), len(index), len(index), 2):
        raise ValueError("matrix must be [n_bins, usable, usable, 2]")
    if not want or any(name not in ("map", "q") for name in want):
        raise ValueError("want names some of ('map', 'q')")
    out = {name: np.empty((max(c.n_bins, 0), off.shape[0]), np.float32) for name in ("map", "q") if name in want}
    _check(load().awpu_hip_csm_map_host(_f32(matrix), int(block_count), _i32(off), _f32(frac), off.shape[1], off.shape[0], _i32(index), len(index),
                                        C.byref(c), _out_ptr(out.get("map"), _f32p), _out_ptr(out.get("q"), _f32p)), "awpu_hip_csm_map_host")
    return out


def csm_invert_host(matrix: np.ndarray, block_count: int, bins, loading: float = 1e-3) -> np.ndarray:
    """Step 6 (awpu_hip_csm_invert_host): the loaded inverse [n_bins, usable, usable, 2] of matrix with its block count, what
    csm_map_host and Engine.csm_map take with kind=CSM_CAPON."""
    c = csm_of(bins, TONES_RECT, CSM_CAPON, loading)
    matrix = np.ascontiguousarray(matrix, np.float32)
    if matrix.ndim != 4 or matrix.shape[0] != max(c.n_bins, 0) or matrix.shape[1] != matrix.shape[2] or matrix.shape[3] != 2:
        raise ValueError("matrix must be [n_bins, usable, usable, 2]")
    out = np.empty_like(matrix)
    _check(load().awpu_hip_csm_invert_host(_f32(matrix), int(block_count), matrix.shape[1], C.byref(c), _out_ptr(out, _f32p)),
           "awpu_hip_csm_invert_host")
    return out


def _csm_square(matrix, c) -> np.ndarray:
    matrix = np.ascontiguousarray(matrix, np.float32)
    if matrix.ndim != 4 or matrix.shape[0] != max(c.n_bins, 0) or matrix.shape[1] != matrix.shape[2] or matrix.shape[3] != 2:
        raise ValueError("matrix must be [n_bins, usable, usable, 2]")
    return matrix


def csm_invert_rule_host(matrix: np.ndarray, block_count: int, bins, loading: float = 1e-3):
    """Step 6a (awpu_hip_csm_invert_rule_host): the loaded inverse by the written arithmetic, what Engine.csm_invert_device gives
    bit for bit -> (inverse [n_bins, usable, usable, 2], solved [n_bins] int32).  An unsolved bin is +0 with solved 0, no error."""
    c = csm_of(bins, TONES_RECT, CSM_CAPON, loading)
    matrix = _csm_square(matrix, c)
    out = np.empty_like(matrix)
    solved = np.empty(max(c.n_bins, 0), np.int32)
    _check(load().awpu_hip_csm_invert_rule_host(_f32(matrix), int(block_count), matrix.shape[1], C.byref(c), _out_ptr(out, _f32p),
                                                _out_ptr(solved, _i32p)), "awpu_hip_csm_invert_rule_host")
    return out, solved


def csm_eig_of(kind, n_sources: int = 0, root: int = 0) -> CsmEig:
    """The CsmEig of a subspace map (or a CsmEig, passed through): CSM_EIG_MUSIC with the signal subspace's dimension, or
    CSM_EIG_FUNCTIONAL with the exponent 2 ** root.  Nothing is judged here: the library refuses a bad request."""
    if isinstance(kind, CsmEig):
        return kind
    return CsmEig(int(kind), int(n_sources), int(root), 0)


def csm_eig_host(matrix: np.ndarray, block_count: int, bins):
    """Step 8a (awpu_hip_csm_eig_host): the eigendecomposition of matrix [n_bins, usable, usable, 2] with its block count by the
    written arithmetic, what Engine.csm_eig_device gives bit for bit -> (values [n_bins, usable] descending, vectors
    [n_bins, usable, usable, 2] with vectors[k, r] the eigenvector of values[k, r], solved [n_bins] int32, sweeps [n_bins] int32).
    An unsolved bin is +0 with solved 0, no error."""
    c = csm_of(bins)
    matrix = _csm_square(matrix, c)
    K, U = max(c.n_bins, 0), matrix.shape[1]
    values, vectors = np.empty((K, U), np.float32), np.empty_like(matrix)
    solved, sweeps = np.empty(K, np.int32), np.empty(K, np.int32)
    _check(load().awpu_hip_csm_eig_host(_f32(matrix), int(block_count), U, C.byref(c), _out_ptr(values, _f32p), _out_ptr(vectors, _f32p),
                                        _out_ptr(solved, _i32p), _out_ptr(sweeps, _i32p)), "awpu_hip_csm_eig_host")
    return values, vectors, solved, sweeps


def csm_eig_weigh_host(values: np.ndarray, vectors: np.ndarray, bins, kind: int = CSM_EIG_MUSIC, n_sources: int = 0, root: int = 0) -> np.ndarray:
    """Step 8b (awpu_hip_csm_eig_weigh_host): the weighed matrix H [n_bins, usable, usable, 2] of csm_eig_host's values and
    vectors: the noise subspace's projector (CSM_EIG_MUSIC) or C ** (1 / 2 ** root) (CSM_EIG_FUNCTIONAL)."""
    c, e = csm_of(bins), csm_eig_of(kind, n_sources, root)
    vectors = _csm_square(vectors, c)
    values = np.ascontiguousarray(values, np.float32)
    if values.shape != vectors.shape[:2]:
        raise ValueError("values must be [n_bins, usable]")
    out = np.empty_like(vectors)
    _check(load().awpu_hip_csm_eig_weigh_host(_f32(values), _f32(vectors), vectors.shape[1], C.byref(c), C.byref(e), _out_ptr(out, _f32p)),
           "awpu_hip_csm_eig_weigh_host")
    return out


def csm_eig_map_host(weighed: np.ndarray, solved, off: np.ndarray, frac: np.ndarray, bins, kind: int = CSM_EIG_MUSIC, n_sources: int = 0,
                     root: int = 0, window: int = TONES_RECT, index=None) -> np.ndarray:
    """Step 8c (awpu_hip_csm_eig_map_host): the subspace map [n_bins, n_pixels] of csm_eig_weigh_host's matrix; solved [n_bins]
    (an unsolved bin is a +0 plane) or None."""
    c, e = csm_of(bins, window), csm_eig_of(kind, n_sources, root)
    off, frac, index = _csm_table(off, frac, index)
    weighed = np.ascontiguousarray(weighed, np.float32)
    if weighed.shape != (max(c.n_bins, 0), len(index), len(index), 2):
        raise ValueError("weighed must be [n_bins, usable, usable, 2]")
    if solved is not None:
        solved = np.ascontiguousarray(solved, np.int32)
        if solved.shape != (max(c.n_bins, 0),):
            raise ValueError("solved must be [n_bins]")
    out = np.empty((max(c.n_bins, 0), off.shape[0]), np.float32)
    _check(load().awpu_hip_csm_eig_map_host(_f32(weighed), None if solved is None else _i32(solved), _i32(off), _f32(frac), off.shape[1],
                                            off.shape[0], _i32(index), len(index), C.byref(c), C.byref(e), _out_ptr(out, _f32p)),
           "awpu_hip_csm_eig_map_host")
    return out


_CSM_CLEAN_OUTPUTS = ("steps", "clean", "residual", "map", "residual_matrix")


def _csm_clean_outputs(want, n_bins: int, steps: int, pixels: int, usable: int) -> dict:
    """The arrays a CLEAN-SC loop writes, those named in `want`."""
    if not want or any(name not in _CSM_CLEAN_OUTPUTS for name in want):
        raise ValueError(f"want names some of {_CSM_CLEAN_OUTPUTS}")
    shapes = {"steps": ((n_bins, steps), CSM_CLEAN_STEP_DTYPE), "clean": ((n_bins, pixels), np.float32), "residual": ((n_bins, pixels), np.float32),
              "map": ((n_bins, pixels), np.float32), "residual_matrix": ((n_bins, usable, usable, 2), np.float32)}
    return {name: np.empty(*shapes[name]) for name in _CSM_CLEAN_OUTPUTS if name in want}


def csm_clean_step_host(matrix: np.ndarray, pixel, off: np.ndarray, frac: np.ndarray, bins, gain: float = 1.0, window: int = TONES_RECT,
                        kind: int = CSM_CONVENTIONAL, index=None, want=("component", "qs")):
    """One CLEAN-SC step (step 7 of include/awpu_hip_csm.h; awpu_hip_csm_clean_step_host) of matrix [n_bins, usable, usable, 2] at
    pixel [n_bins] (-1: the bin is left alone) -> (the updated matrix -- a copy --, a dict of the outputs in `want`: "component"
    [n_bins, usable, 2] and "qs" [n_bins])."""
    c = csm_of(bins, window, kind)
    off, frac, index = _csm_table(off, frac, index)
    matrix = np.array(matrix, np.float32, order="C")
    if matrix.shape != (max(c.n_bins, 0), len(index), len(index), 2):
        raise ValueError("matrix must be [n_bins, usable, usable, 2]")
    pixel = np.ascontiguousarray(pixel, np.int32)
    if pixel.shape != (max(c.n_bins, 0),):
        raise ValueError("pixel must be [n_bins]")
    if any(name not in ("component", "qs") for name in want):
        raise ValueError("want names some of ('component', 'qs')")
    shapes = {"component": (max(c.n_bins, 0), len(index), 2), "qs": (max(c.n_bins, 0),)}
    out = {name: np.empty(shapes[name], np.float32) for name in ("component", "qs") if name in want}
    _check(load().awpu_hip_csm_clean_step_host(_out_ptr(matrix, _f32p), _i32(pixel), float(gain), _i32(off), _f32(frac), off.shape[1], off.shape[0],
                                               _i32(index), len(index), C.byref(c), _out_ptr(out.get("component"), _f32p),
                                               _out_ptr(out.get("qs"), _f32p)), "awpu_hip_csm_clean_step_host")
    return matrix, out


def csm_clean_host(matrix: np.ndarray, block_count: int, off: np.ndarray, frac: np.ndarray, bins, steps: int, gain: float = 1.0,
                   stop_ratio: float = 0.0, window: int = TONES_RECT, kind: int = CSM_CONVENTIONAL, index=None,
                   want=("steps", "clean", "residual", "map")):
    """The CLEAN-SC loop (awpu_hip_csm_clean_host) of matrix [n_bins, usable, usable, 2] with its block count -> a dict of the
    outputs in `want`: "steps" [n_bins, steps] (CSM_CLEAN_STEP_DTYPE; unused: pixel -1), "clean", "residual", "map"
    [n_bins, n_pixels] and "residual_matrix" [n_bins, usable, usable, 2]."""
    c, cl = csm_of(bins, window, kind), CsmClean(int(steps), float(gain), float(stop_ratio))
    off, frac, index = _csm_table(off, frac, index)
    matrix = np.ascontiguousarray(matrix, np.float32)
    if matrix.shape != (max(c.n_bins, 0), len(index), len(index), 2):
        raise ValueError("matrix must be [n_bins, usable, usable, 2]")
    out = _csm_clean_outputs(want, max(c.n_bins, 0), max(int(steps), 0), off.shape[0], len(index))
    _check(load().awpu_hip_csm_clean_host(_f32(matrix), int(block_count), _i32(off), _f32(frac), off.shape[1], off.shape[0], _i32(index), len(index),
                                          C.byref(c), C.byref(cl), _out_ptr(out.get("steps")),
                                          *(_out_ptr(out.get(name), _f32p) for name in ("clean", "residual", "map", "residual_matrix"))),
           "awpu_hip_csm_clean_host")
    return out


class CsmWatchResult:
    """What Engine.csm_watch_blocks / csm_watch_samples hand back: .image, .big, .power as a WatchResult has them -- of the shown
    row --, .sources and .count as a FindResult has them (None without `find`), .planes [n_frames, n_bins, pixels] and .solved
    [n_frames, n_bins] (None unless asked for), .next_first, and .carry / .carried for the call that continues the run."""

    def __init__(self, image, big, power, sources, count, planes, solved, next_first: int, carry, carried: int):
        self.image, self.big, self.power, self.sources, self.count = image, big, power, sources, count
        self.planes, self.solved, self.next_first, self.carry, self.carried = planes, solved, next_first, carry, carried

    def __len__(self):
        return len(next(a for a in (self.image, self.big, self.power, self.count, self.planes, self.solved) if a is not None))


class CsmCleanRunResult:
    """What Engine.csm_clean_blocks / csm_clean_samples hand back: .image, .big, .power as a WatchResult has them -- of the shown
    row --, .sources and .count as a FindResult has them (None without `find`), .planes [n_frames, n_bins, pixels] (the map, clean
    or residual rows; None unless asked for), .steps [n_frames, n_bins, steps] CSM_CLEAN_STEP_DTYPE records, .next_first, and
    .carry / .carried for the call that continues the run."""

    def __init__(self, image, big, power, sources, count, planes, steps, next_first: int, carry, carried: int):
        self.image, self.big, self.power, self.sources, self.count = image, big, power, sources, count
        self.planes, self.steps, self.next_first, self.carry, self.carried = planes, steps, next_first, carry, carried

    def __len__(self):
        return len(self.steps)


def csm_clean_from_text(text: str):
    """'STEPS[:GAIN[:STOP]]' (gain 1 and stop ratio 0 unless given), as the tools' --csm-clean takes it -> (steps, gain, stop_ratio)."""
    parts = text.split(":")
    if not 1 <= len(parts) <= 3:
        raise ValueError(f"csm clean '{text}': STEPS[:GAIN[:STOP]]")
    steps, gain, stop = int(parts[0]), float(parts[1]) if len(parts) > 1 else 1.0, float(parts[2]) if len(parts) > 2 else 0.0
    if not 1 <= steps <= CSM_CLEAN_MAX_STEPS or not 0.0 < gain <= 1.0 or not 0.0 <= stop < 1.0:
        raise ValueError(f"csm clean '{text}': STEPS in [1, {CSM_CLEAN_MAX_STEPS}], GAIN in (0, 1], STOP in [0, 1)")
    return steps, gain, stop


def csm_clean_source_records(steps: np.ndarray, rows: int, cols: int, max_sources: int, fov_deg: float = 180.0):
    """The steps of a CLEAN-SC run's frames [n_frames, n_bins, steps] as find results, as peel_source_records gives a peel run's: a
    frame's sources are its steps merged per pixel over steps and bins, strongest first -> (sources [n_frames, max_sources]
    SOURCE_DTYPE records, count [n_frames])."""
    steps = np.asarray(steps)
    return peel_source_records(steps.reshape(len(steps), -1), rows, cols, max_sources, fov_deg)


def csm_from_text(text: str, sample_rate: float = 48828.125):
    """'LO:HI[:hann]' (Hz; the rectangular window unless 'hann' is given), as the tools' --csm takes it -> (bins, window): the
    transform bins whose centres lie in [LO, HI).  More than CSM_MAX_BINS of them is a ValueError that names the limit."""
    parts = text.split(":")
    if len(parts) not in (2, 3) or (len(parts) == 3 and parts[2] != "hann"):
        raise ValueError(f"csm '{text}': LO:HI or LO:HI:hann, in Hz")
    lo, hi = float(parts[0]), float(parts[1])
    if not 0.0 <= lo < hi:
        raise ValueError(f"csm '{text}': 0 <= LO < HI")
    step = sample_rate / 256
    bins = [k for k in range(129) if lo <= k * step < hi]
    if not bins:
        raise ValueError(f"csm '{text}': no bin of {step:.1f} Hz has its centre in that range")
    if len(bins) > CSM_MAX_BINS:
        raise ValueError(f"csm '{text}': {len(bins)} bins of {step:.1f} Hz have their centres in that range; a cross-spectral map takes at most {CSM_MAX_BINS}")
    return bins, TONES_HANN if len(parts) == 3 else TONES_RECT


def csm_kind_from_text(text: str):
    """'conventional', 'diagonal-removed' or 'capon[:LOADING]' (1e-2 unless given), as the tools' --csm-kind takes it -> (kind, loading)."""
    name, _, loading = text.partition(":")
    kinds = {"conventional": CSM_CONVENTIONAL, "diagonal-removed": CSM_DIAGONAL_REMOVED, "capon": CSM_CAPON}
    if name not in kinds or (loading and name != "capon"):
        raise ValueError(f"csm kind '{text}': conventional, diagonal-removed or capon[:LOADING]")
    value = float(loading) if loading else 1e-2
    if not 0.0 <= value < float("inf"):
        raise ValueError(f"csm kind '{text}': LOADING is finite and not negative")
    return kinds[name], value


class TonesResult:
    """What Engine.tones_blocks / tones_samples hand back: .image, .big, .power as a WatchResult has them -- of the shown group's
    plane or, with show=TONES_SHOW_PITCH, of the pitch row --, .sources and .count as a FindResult has them (None without `find`),
    .next_first for the call that continues the run."""

    def __init__(self, image, big, power, sources, count, next_first: int):
        self.image, self.big, self.power, self.sources, self.count, self.next_first = image, big, power, sources, count, next_first

    def __len__(self):
        return len(next(a for a in (self.image, self.big, self.power, self.count) if a is not None))


class PeelResult:
    """What peel_host and Engine.peel hand back: .steps [batch, steps] records of PEEL_STEP_DTYPE (unused: pixel -1), .clean,
    .residual, .map [batch, n_pixels], .frames the residual frames [batch, n_streams, hist] or None."""

    def __init__(self, steps, clean, residual, map, frames):  # noqa: A002 (the header's name)
        self.steps, self.clean, self.residual, self.map, self.frames = steps, clean, residual, map, frames


def peel_source_records(steps: np.ndarray, rows: int, cols: int, max_sources: int, fov_deg: float = 180.0):
    """The steps of a peel run's frames [n_frames, steps] as find results: -> (sources [n_frames, max_sources] SOURCE_DTYPE records,
    count [n_frames]).  A frame's sources are its steps merged per pixel (peel_sources: the clean map's entries), strongest
    first; row and col are the pixel's own (a step has no sub-pixel refinement), theta and phi its direction on the table's
    sine-space grid, as awpu_hip_find.h gives them."""
    steps = np.asarray(steps)
    sources = np.zeros((len(steps), max_sources), SOURCE_DTYPE)
    sources["pixel"] = -1
    count = np.zeros(len(steps), np.int32)
    sep_r, sep_c = (np.sin(np.float64(np.float32(fov_deg)) * (np.pi / 180.0) / 2.0) / (n / 2.0) for n in (rows, cols))
    for j, frame in enumerate(steps):
        merged = peel_sources(frame)[:max_sources]
        count[j] = len(merged)
        for k, (pixel, power) in enumerate(merged):
            r, c = divmod(int(pixel), cols)
            y = r * sep_r - rows * sep_r / 2.0 + sep_r / 2.0
            x = c * sep_c - cols * sep_c / 2.0 + sep_c / 2.0
            sources[j, k] = (pixel, power, r, c, np.arcsin(min(np.hypot(x, y), 1.0)), 0.0 if x == 0.0 and y == 0.0 else np.arctan2(y, x))
    return sources, count


class PeelRunResult:
    """What Engine.peel_blocks / peel_samples hand back: .image, .big, .power as a WatchResult has them -- of the map (or, by
    `show`, the clean or the residual) rows --, .steps [n_frames, steps] PEEL_STEP_DTYPE records, .sources and .count as a
    FindResult has them (None without `find`), .next_first for the call that continues the run."""

    def __init__(self, image, big, power, steps, sources, count, next_first: int):
        self.image, self.big, self.power, self.steps, self.sources, self.count, self.next_first = image, big, power, steps, sources, count, next_first

    def __len__(self):
        return len(self.steps)


def _peel_table(frames, off, frac, index, gain):
    frames = np.ascontiguousarray(frames, np.float32)
    off = np.ascontiguousarray(off, np.int32)
    frac = np.ascontiguousarray(frac, np.float32)
    if frames.ndim != 3 or off.ndim != 2 or off.shape != frac.shape:
        raise ValueError("frames must be [batch, n_streams, hist], off and frac [n_pixels, lut_stride]")
    index = np.arange(off.shape[1], dtype=np.int32) if index is None else np.ascontiguousarray(index, np.int32)
    if gain is not None:
        gain = np.ascontiguousarray(gain, np.float32)
        if gain.shape != index.shape:
            raise ValueError("gain must be [usable], in the active list's order")
    table = (frames.shape[1], frames.shape[2], _i32(off), _f32(frac), off.shape[1], off.shape[0], _i32(index), len(index))
    return frames, table, None if gain is None else _f32(gain), (off, frac, index, gain)  # (the arrays: kept alive by the caller)


def peel_beam_length(n_streams: int, hist: int, off: np.ndarray, frac: np.ndarray, index=None) -> int:
    """258 + 2 E: the samples of a peel step's beam for this table at these mics (awpu_hip_peel_beam_length)."""
    _, table, _, _keep = _peel_table(np.zeros((1, n_streams, hist), np.float32), off, frac, index, None)
    n = load().awpu_hip_peel_beam_length(*table)
    if n < 0:
        _check(n, "awpu_hip_peel_beam_length")
    return n


def peel_step_host(frames: np.ndarray, off: np.ndarray, frac: np.ndarray, pixel, loop_gain: float = 1.0, index=None, gain=None):
    """One peel step as executable C (awpu_hip_peel_step_host): frames [batch, n_streams, hist], pixel [batch] (-1 = leave the
    frame alone).  -> (residual frames, beams [batch, 258 + 2 E]); `frames` itself is not written."""
    frames, table, g, _keep = _peel_table(frames, off, frac, index, gain)
    frames = frames.copy()
    pixel = np.ascontiguousarray(pixel, np.int32)
    if pixel.shape != (frames.shape[0],):
        raise ValueError("pixel must be [batch]")
    n = load().awpu_hip_peel_beam_length(*table)
    beams = np.empty((frames.shape[0], max(n, 1)), np.float32)
    _check(load().awpu_hip_peel_step_host(_f32(frames), frames.shape[0], *table, g, _i32(pixel), loop_gain, _f32(beams)), "awpu_hip_peel_step_host")
    return frames, beams


def peel_host(frames: np.ndarray, off: np.ndarray, frac: np.ndarray, steps: int, gain_loop: float = 1.0, stop_ratio: float = 0.0, index=None,
              gain=None, want_frames: bool = True) -> PeelResult:
    """The peel loop as executable C (awpu_hip_peel_host): frames [batch, n_streams, hist], the table off / frac [n_pixels,
    lut_stride], index = the active stream ids (default: all of the table's), gain [usable] in their order or None."""
    frames, table, g, _keep = _peel_table(frames, off, frac, index, gain)
    batch, n_pixels = frames.shape[0], table[5]
    pe = Peel(steps, gain_loop, stop_ratio)
    rec = np.empty((batch, max(steps, 0)), PEEL_STEP_DTYPE)
    maps = [np.empty((batch, n_pixels), np.float32) for _ in range(3)]
    left = np.empty_like(frames) if want_frames else None
    _check(load().awpu_hip_peel_host(_f32(frames), batch, *table, g, C.byref(pe), C.c_void_p(rec.ctypes.data or 16), *[_f32(m) for m in maps],
                                     None if left is None else _f32(left)), "awpu_hip_peel_host")
    return PeelResult(rec, *maps, left)


def peel_sources(steps: np.ndarray) -> np.ndarray:
    """The steps of one frame merged per pixel: records (pixel, power) -- the `removed` of the steps at a pixel, added in step
    order, which is clean[pixel] --, strongest first."""
    merged = {}
    for s in np.asarray(steps).reshape(-1):
        if s["pixel"] >= 0:
            merged[int(s["pixel"])] = np.float32(merged.get(int(s["pixel"]), np.float32(0)) + s["removed"])
    out = np.array(sorted(merged.items(), key=lambda kv: (-kv[1], kv[0])), dtype=[("pixel", "<i4"), ("power", "<f4")])
    return out


class CohereResult:
    """What Engine.cohere_blocks / cohere_samples hand back: .image, .big, .power as a WatchResult has them -- of the weighted
    (or, with show=COHERE_FACTOR, the coherence) rows --, .sources and .count as a FindResult has them (None without `find`),
    .next_first for the call that continues the run."""

    def __init__(self, image, big, power, sources, count, next_first: int):
        self.image, self.big, self.power, self.sources, self.count, self.next_first = image, big, power, sources, count, next_first

    def __len__(self):
        return len(next(a for a in (self.image, self.big, self.power, self.count) if a is not None))


def band_design(lo_hz: float, hi_hz: float, taps: int = 63, sample_rate: float = 48828.125) -> np.ndarray:
    """Coefficients [taps] of a linear-phase band lo_hz .. hi_hz by the window method (awpu_hip_band_design: what fir1 does by
    default); taps odd in [3, 127], lo_hz = 0 a low-pass, hi_hz = sample_rate / 2 a high-pass."""
    c = np.empty(max(int(taps), 1), np.float32)
    _check(load().awpu_hip_band_design(float(lo_hz), float(hi_hz), float(sample_rate), int(taps), _f32(c)), "awpu_hip_band_design")
    return c


def band_from_text(text: str, sample_rate: float = 48828.125) -> np.ndarray:
    """'LO:HI[:TAPS]' (Hz; 63 taps unless given), as the tools' --band takes it -> band_design's coefficients."""
    parts = text.split(":")
    if len(parts) not in (2, 3):
        raise ValueError(f"band '{text}': LO:HI or LO:HI:TAPS, in Hz")
    return band_design(float(parts[0]), float(parts[1]), int(parts[2]) if len(parts) == 3 else 63, sample_rate)


def band_filter(samples: np.ndarray, coeffs: np.ndarray) -> np.ndarray:
    """Every row of `samples` [..., n] through the band's rule on the host (awpu_hip_band_filter): what a handle with these
    coefficients sweeps in place of `samples`, bit for bit."""
    x = np.ascontiguousarray(samples, np.float32)
    c = np.ascontiguousarray(coeffs, np.float32).reshape(-1)
    y = np.empty_like(x)
    n = x.shape[-1] if x.ndim else 0
    _check(load().awpu_hip_band_filter(_f32(x), x.size // n if n else 0, n, n, _f32(c), c.size, _f32(y)), "awpu_hip_band_filter")
    return y


def spectral_of(bands, channel=None, scale: int = SPECTRAL_SCALE_COMMON):
    """(awpu_spectral_t, what keeps its coefficients alive) of `bands`, a sequence of coefficient arrays (band_design's, say);
    channel None: byte c shows band c where there is one.  Nothing is judged here: the library refuses a bad set."""
    if channel is None:
        channel = [c if c < len(bands) else -1 for c in range(3)]
    coeffs = [np.ascontiguousarray(c, np.float32).reshape(-1) for c in bands]
    sp = Spectral()
    sp.n_bands = len(coeffs)
    for b, c in enumerate(coeffs[:SPECTRAL_MAX_BANDS]):
        sp.taps[b] = c.size
        sp.coef[b] = c.ctypes.data_as(_f32p)
    sp.channel[:] = [int(c) for c in channel]
    sp.scale = int(scale)
    return sp, coeffs


def spectral_compose(power: np.ndarray, channel=(0, 1, 2), scale: int = SPECTRAL_SCALE_COMMON):
    """One frame's band powers [n_bands, n] -> (image [n, 3] uint8, dominant [n] uint8): the display rule of the spectral runs on
    the host (awpu_hip_spectral_compose).  Byte c of a pixel shows band channel[c] (-1: 0), scaled by one maximum over the shown
    bands (SPECTRAL_SCALE_COMMON) or by each band's own (SPECTRAL_SCALE_PER_BAND); dominant names the strongest band of all."""
    power = np.ascontiguousarray(power, np.float32)
    if power.ndim != 2:
        raise ValueError("power must be [n_bands, n]")
    n_bands, n = power.shape
    image, dominant = np.empty((n, 3), np.uint8), np.empty(n, np.uint8)
    ch = np.asarray(channel, np.int32).reshape(3)
    _check(load().awpu_hip_spectral_compose(_f32(power), n, n_bands, n, _i32(ch), int(scale), image.ctypes.data_as(_u8p),
                                            dominant.ctypes.data_as(_u8p)), "awpu_hip_spectral_compose")
    return image, dominant


class SpectralResult:
    """What Engine.spectral_* hand back: .image [n_frames, rows, cols, 3] uint8 or None, .big [n_frames, out_rows, out_cols, 3] or
    None, .dominant [n_frames, rows, cols] or None, .power [n_bands, n_frames, pixels] or None, and .next_first: the `first` of the
    call that continues the recording.  Frame j shows block first + j * every of the call."""

    def __init__(self, image, big, dominant, power, next_first: int):
        self.image = image
        self.big = big
        self.dominant = dominant
        self.power = power
        self.next_first = next_first

    def __len__(self):
        return next(a.shape[1] if a is self.power else len(a) for a in (self.image, self.big, self.dominant, self.power) if a is not None)


def _particles(theta, phi, spread, rate, steps, where: str) -> np.ndarray:
    """PARTICLE_DTYPE records from per-particle values (scalars broadcast), or a copy of such records passed as `theta`."""
    if isinstance(theta, np.ndarray) and theta.dtype == PARTICLE_DTYPE:
        return np.ascontiguousarray(theta).reshape(-1).copy()
    theta = np.atleast_1d(np.asarray(theta, np.float64))
    n = max(theta.size, np.size(phi), np.size(spread), np.size(rate), np.size(steps))
    parts = np.zeros(n, PARTICLE_DTYPE)
    parts["theta"], parts["phi"] = np.broadcast_to(theta, n), np.broadcast_to(np.asarray(phi, np.float64), n)
    parts["spread"], parts["rate"] = np.broadcast_to(np.asarray(spread, np.float64), n), np.broadcast_to(np.asarray(rate, np.float64), n)
    steps = np.broadcast_to(np.asarray(steps, np.int64), n)
    if steps.size and (steps.min() < 0 or steps.max() > 4096):  # (before the int32 field could wrap it into range)
        raise AwpuError(ERR_INVALID, where, "steps outside [0, 4096]")
    parts["steps"] = steps
    return parts


class Engine:
    """One awpu_hip handle = one MIMO worker's sweep state on one GPU (src/dsp/mimo.h:74-91)."""

    def __init__(self, n_pixels: int, n_streams: int = ELEMENTS, lut_stride: Optional[int] = None,
                 hist: int = HIST, math: Optional[int] = None, interp: int = INTERP_LERP,
                 max_batch: int = 1, device: int = 0, pixel_begin: int = 0, pixel_count: int = 0,
                 grid_columns: int = 0, devices=None, window=None):
        lib = load()
        cfg = Cfg()
        lib.awpu_hip_default_cfg(C.byref(cfg))
        cfg.device = device
        if devices is not None:  # a device group: the pixels are spread over these GPUs (include/awpu_hip.h)
            cfg.n_devices = len(devices)
            for i, d in enumerate(devices[:8]):  # (more than AWPU_MAX_DEVICES: the library refuses the count)
                cfg.devices[i] = d
            cfg.device = devices[0]
        cfg.grid_columns = grid_columns
        cfg.n_streams = n_streams
        cfg.hist = hist
        cfg.n_pixels = n_pixels
        cfg.lut_stride = n_streams if lut_stride is None else lut_stride
        cfg.interp = interp
        if math is not None:  # None: the library's default (awpu_hip_default_cfg: AWPU_MATH_F32_EXACT, the reference's arithmetic)
            cfg.math = math
        cfg.max_batch = max_batch
        cfg.pixel_begin = pixel_begin
        cfg.pixel_count = pixel_count
        if window is not None:  # (begin, end): history samples staged per stream, the union over the ranks' slabs
            cfg.window_begin, cfg.window_end = int(window[0]), int(window[1])
        self._h = C.c_void_p()
        _check(lib.awpu_hip_create(C.byref(self._h), C.byref(cfg)), "awpu_hip_create")
        self.cfg = cfg
        self.pixel_count = pixel_count or n_pixels
        self._lib = lib

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.awpu_hip_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_delay_table(self, off: np.ndarray, frac: np.ndarray) -> None:
        off = np.ascontiguousarray(off, np.int32)
        frac = np.ascontiguousarray(frac, np.float32)
        want = (self.pixel_count, self.cfg.lut_stride)
        if off.shape != want or frac.shape != want:
            raise ValueError(f"delay tables must be {want}, got {off.shape} / {frac.shape}")
        _check(self._lib.awpu_hip_set_delay_table(self._h, _i32(off), _f32(frac)), "set_delay_table")

    def set_active_mics(self, index: Optional[np.ndarray] = None, usable: Optional[int] = None) -> None:
        if index is None:
            n = self.cfg.n_streams if usable is None else usable
            _check(self._lib.awpu_hip_set_active_mics(self._h, None, n), "set_active_mics")
        else:
            index = np.ascontiguousarray(index, np.int32)
            n = index.size
            _check(self._lib.awpu_hip_set_active_mics(self._h, _i32(index), index.size),
                   "set_active_mics")
        self._usable = int(n)

    @property
    def usable(self) -> int:
        """How many mics are active: what the cross-spectral calls size their matrices by (all streams until set_active_mics)."""
        return getattr(self, "_usable", self.cfg.n_streams)

    def ingest_block(self, datagrams) -> None:
        """One block of 256 wire datagrams (bytes-like, 256 x 1032 B; src/fpga/receiver.h:24-30)."""
        buf = np.frombuffer(datagrams, dtype=np.uint8)
        if buf.size != 256 * DATAGRAM_BYTES:
            raise ValueError("a block is 256 datagrams of 1032 bytes")
        _check(self._lib.awpu_hip_ingest_block(self._h, buf.ctypes.data_as(C.c_void_p), DATAGRAM_BYTES), "ingest_block")

    def process_ring(self) -> np.ndarray:
        power = np.empty(self.pixel_count, np.float32)
        _check(self._lib.awpu_hip_process_ring(self._h, _f32(power)), "process_ring")
        return power

    def ring_snapshot(self) -> np.ndarray:
        frames = np.empty((self.cfg.n_streams, HIST), np.float32)
        _check(self._lib.awpu_hip_ring_snapshot(self._h, _f32(frames)), "ring_snapshot")
        return frames

    def _sample_blocks(self, samples):
        """(unpacked samples [n_streams, N] as contiguous floats, how many blocks of 256 they are)."""
        samples = np.ascontiguousarray(samples, np.float32)
        if samples.ndim != 2 or samples.shape[0] != self.cfg.n_streams or samples.shape[1] % 256 or samples.shape[1] == 0:
            raise ValueError(f"samples must be [{self.cfg.n_streams}, N] with N a positive multiple of 256")
        return samples, samples.shape[1] // 256

    def _wire_run(self, where: str, wire, stride: int):
        """A run on wire datagrams as its helper takes it: (entry point `where` with the handle, the bytes and their stride in
        place, where, n_blocks)."""
        buf, n_blocks = _wire_blocks(wire, stride)
        return functools.partial(getattr(self._lib, where), self._h, buf.ctypes.data_as(C.c_void_p), stride), where, n_blocks

    def _sample_run(self, where: str, samples):
        """The same on unpacked samples: the floats and their pitch in place."""
        samples, n_blocks = self._sample_blocks(samples)
        return functools.partial(getattr(self._lib, where), self._h, _f32(samples), samples.shape[1]), where, n_blocks

    def _device_run(self, where: str, d_samples_ptr: int, pitch: int, n_blocks: int, w: Watch, *rest) -> int:
        """A run on device pointers: entry point `where` on samples [n_streams, pitch], with `rest` behind n_blocks and w, in the
        order of its prototype -> next_first."""
        _check(getattr(self._lib, where)(self._h, C.c_void_p(d_samples_ptr), pitch, n_blocks, C.byref(w), *rest), where)
        return watch_count(n_blocks, w.first, w.every)[1]

    @staticmethod
    def _shown_frames(n_blocks: int, *, first: int, every: int, **shown):
        """(n_frames, next_first, the awpu_watch_t) of a run of n_blocks blocks with these display keywords (_watch_struct's)."""
        n_frames, next_first = watch_count(n_blocks, first, every)
        return n_frames, next_first, _watch_struct(first=first, every=every, **shown)

    def _shown_outputs(self, n_frames, w: Watch, want_image, want_power, f: Optional[Find] = None, new=lambda shape, dtype, name: np.empty(shape, dtype)):
        """What a run shows of its n_frames frames: the arrays (image, big, power, sources, count), each or None, and their
        pointers as the C calls take them; new(shape, dtype, name) allocates one."""
        image = new((n_frames, w.rows, w.cols), np.uint8, "image") if want_image else None
        big = None
        if w.out_rows:
            big = new((n_frames, w.out_rows, w.out_cols, 3) if w.d_colormap else (n_frames, w.out_rows, w.out_cols), np.uint8, "big")
        power = new((n_frames, self.pixel_count), np.float32, "power") if want_power else None
        sources = None if f is None else np.empty((n_frames, max(f.max_sources, 0)), SOURCE_DTYPE)
        count = None if f is None else np.empty(n_frames, np.int32)
        return (image, big, power, sources, count), (_out_ptr(image, _u8p), _out_ptr(big, _u8p), _out_ptr(power, _f32p), _out_ptr(sources),
                                                    _out_ptr(count))

    def process_blocks(self, wire, stride: int = DATAGRAM_BYTES) -> np.ndarray:
        """A run of consecutive blocks of wire datagrams (bytes-like, n_blocks x 256 datagrams `stride` bytes apart) ->
        power [n_blocks, pixels]: row k = process_ring() after k + 1 ingest_block() calls, and the ring is left there
        (awpu_hip_process_blocks)."""
        call, where, n_blocks = self._wire_run("awpu_hip_process_blocks", wire, stride)
        power = np.empty((n_blocks, self.pixel_count), np.float32)
        _check(call(n_blocks, _f32(power)), where)
        return power

    def process_samples(self, samples: np.ndarray) -> np.ndarray:
        """The same from unpacked samples [n_streams, N] (N a multiple of 256, oldest first) -> power [N // 256, pixels]
        (awpu_hip_process_samples)."""
        call, where, n_blocks = self._sample_run("awpu_hip_process_samples", samples)
        power = np.empty((n_blocks, self.pixel_count), np.float32)
        _check(call(n_blocks, _f32(power)), where)
        return power

    def process_samples_device(self, d_samples_ptr: int, pitch: int, n_blocks: int, d_power_ptr: int, stream: int = 0) -> None:
        """The same on device pointers (samples [n_streams, pitch], power [n_blocks, pixels]) on `stream`; asynchronous."""
        _check(self._lib.awpu_hip_process_samples_device(self._h, C.c_void_p(d_samples_ptr), pitch, n_blocks, *_dev(d_power_ptr, stream)),
               "awpu_hip_process_samples_device")

    def _listen(self, run, *, particles, theta_limit, reference, want_trail, want_power) -> ListenResult:
        call, where, n_blocks = run
        parts = _particles(*particles, where)
        n = parts.size
        audio = np.empty((n, 256 * n_blocks), np.float32)
        trail = np.zeros((n_blocks, n), PARTICLE_DTYPE) if want_trail else None
        power = np.empty((n_blocks, self.pixel_count), np.float32) if want_power else None
        pp = C.POINTER(Particle)
        _check(call(n_blocks, parts.ctypes.data_as(pp), n, float(theta_limit), -1.0 if reference is None else float(reference),
                    _f32(audio), audio.shape[1], trail.ctypes.data_as(pp) if want_trail else None, _f32(power) if want_power else None),
               where)
        return ListenResult(audio, parts, trail, power)

    def listen_blocks(self, wire, theta, phi, spread, rate, steps, theta_limit: float, reference: Optional[float] = None,
                      stride: int = DATAGRAM_BYTES, want_trail: bool = True, want_power: bool = False) -> ListenResult:
        """Listen to a run of consecutive blocks of wire datagrams (as process_blocks takes them): per block, listener l takes
        steps[l] gradient steps (0 = a fixed, steered listener) and its delayed-and-summed signal at where it then points is
        256 samples of its audio row; the ring is left where the run ends (awpu_hip_listen_blocks).  theta/phi/spread/rate/steps
        are per listener (scalars broadcast), or `theta` is the .listeners of an earlier result (the rest then None);
        reference None = from each block's own snapshot, as MISOWorker does.  -> ListenResult."""
        return self._listen(self._wire_run("awpu_hip_listen_blocks", wire, stride), particles=(theta, phi, spread, rate, steps),
                            theta_limit=theta_limit, reference=reference, want_trail=want_trail, want_power=want_power)

    def listen_samples(self, samples: np.ndarray, theta, phi, spread, rate, steps, theta_limit: float,
                       reference: Optional[float] = None, want_trail: bool = True, want_power: bool = False) -> ListenResult:
        """The same from unpacked samples [n_streams, N] (N a multiple of 256, oldest first) (awpu_hip_listen_samples)."""
        return self._listen(self._sample_run("awpu_hip_listen_samples", samples), particles=(theta, phi, spread, rate, steps),
                            theta_limit=theta_limit, reference=reference, want_trail=want_trail, want_power=want_power)

    def listen_samples_device(self, d_samples_ptr: int, pitch: int, n_blocks: int, theta, phi, spread, rate, steps, theta_limit: float,
                              d_audio_ptr: int, audio_pitch: int, reference: Optional[float] = None, d_trail_ptr: int = 0,
                              d_power_ptr: int = 0, stream: int = 0) -> np.ndarray:
        """The same on device pointers (samples [n_streams, pitch], audio [n, audio_pitch], trail [n_blocks, n] records or 0,
        power [n_blocks, pixels] or 0) on `stream`; returns the listeners after the run (PARTICLE_DTYPE records), for which it
        waits (awpu_hip_listen_samples_device)."""
        parts = _particles(theta, phi, spread, rate, steps, "awpu_hip_listen_samples_device")
        _check(self._lib.awpu_hip_listen_samples_device(
            self._h, C.c_void_p(d_samples_ptr), pitch, n_blocks, parts.ctypes.data_as(C.POINTER(Particle)), parts.size,
            float(theta_limit), -1.0 if reference is None else float(reference), C.c_void_p(d_audio_ptr), audio_pitch,
            *_dev(d_trail_ptr, d_power_ptr, stream)), "awpu_hip_listen_samples_device")
        return parts

    def _watch(self, run, *, want_image, want_power, out, **shown) -> WatchResult:
        call, where, n_blocks = run
        n_frames, next_first, w = self._shown_frames(n_blocks, **shown)

        def array(shape, dtype, old):  # the earlier result's array where it has room (its first n_frames rows), else a new one
            if isinstance(old, np.ndarray) and old.dtype == dtype and old.shape[1:] == shape[1:] and old.flags.c_contiguous:
                base = old if old.base is None else old.base
                if isinstance(base, np.ndarray) and base.dtype == dtype and base.shape[1:] == shape[1:] and len(base) >= shape[0]:
                    return base[: shape[0]]
            return np.empty(shape, dtype)

        shown, ptrs = self._shown_outputs(n_frames, w, want_image, want_power,
                                          new=lambda shape, dtype, name: array(shape, dtype, getattr(out, name, None)))
        _check(call(n_blocks, C.byref(w), *ptrs[:3]), where)
        return WatchResult(*shown[:3], next_first)

    def watch_blocks(self, wire, rows: int, cols: int, first: int = 0, every: int = 1, out_rows: int = 0, out_cols: int = 0,
                     d_colormap_ptr: int = 0, flip: bool = False, stride: int = DATAGRAM_BYTES, want_image: bool = True,
                     want_power: bool = False, out: Optional[WatchResult] = None) -> WatchResult:
        """Watch a run of consecutive blocks of wire datagrams (as process_blocks takes them): every block is appended to the
        ring, blocks first, first + every, ... are swept and shown -- the compact image [rows, cols], with out_rows / out_cols the
        large one (upscaled, through the [256, 3] device colour table when d_colormap_ptr, mirrored when flip), on request the
        powers (awpu_hip_watch_blocks).  -> WatchResult; pass its .next_first as `first` of the call that continues the run, and
        the result itself as `out` when its arrays may be written again (a writer that is done with a chunk's frames: 3 MiB per
        1024 x 1024 colour frame are then not allocated and paged in anew for every call)."""
        return self._watch(self._wire_run("awpu_hip_watch_blocks", wire, stride), rows=rows, cols=cols, first=first, every=every,
                           out_rows=out_rows, out_cols=out_cols, d_colormap_ptr=d_colormap_ptr, flip=flip, want_image=want_image,
                           want_power=want_power, out=out)

    def watch_samples(self, samples: np.ndarray, rows: int, cols: int, first: int = 0, every: int = 1, out_rows: int = 0,
                      out_cols: int = 0, d_colormap_ptr: int = 0, flip: bool = False, want_image: bool = True,
                      want_power: bool = False, out: Optional[WatchResult] = None) -> WatchResult:
        """The same from unpacked samples [n_streams, N] (N a multiple of 256, oldest first) (awpu_hip_watch_samples)."""
        return self._watch(self._sample_run("awpu_hip_watch_samples", samples), rows=rows, cols=cols, first=first, every=every,
                           out_rows=out_rows, out_cols=out_cols, d_colormap_ptr=d_colormap_ptr, flip=flip, want_image=want_image,
                           want_power=want_power, out=out)

    def watch_samples_device(self, d_samples_ptr: int, pitch: int, n_blocks: int, rows: int, cols: int, first: int = 0, every: int = 1,
                             d_image_ptr: int = 0, d_big_ptr: int = 0, d_power_ptr: int = 0, out_rows: int = 0, out_cols: int = 0,
                             d_colormap_ptr: int = 0, flip: bool = False, stream: int = 0) -> int:
        """The same on device pointers (samples [n_streams, pitch]; image [n_frames, rows * cols], big [n_frames, out_rows,
        out_cols (, 3)], power [n_frames, pixels], each or 0) on `stream`; asynchronous.  -> next_first
        (awpu_hip_watch_samples_device)."""
        w = _watch_struct(rows=rows, cols=cols, first=first, every=every, out_rows=out_rows, out_cols=out_cols, d_colormap_ptr=d_colormap_ptr,
                          flip=flip)
        return self._device_run("awpu_hip_watch_samples_device", d_samples_ptr, pitch, n_blocks, w,
                                *_dev(d_image_ptr, d_big_ptr, d_power_ptr, stream))

    def process_bands(self, frames: np.ndarray, bands) -> np.ndarray:
        """frames [batch, n_streams, hist] through every band of `bands` (a sequence of up to four coefficient arrays) from one
        upload and one pre-pass -> power [n_bands, batch, pixels]; power[b] is process() with set_band(bands[b]), bit for bit
        (awpu_hip_process_bands)."""
        frames = np.ascontiguousarray(frames, np.float32)
        if frames.ndim != 3 or frames.shape[1:] != (self.cfg.n_streams, self.cfg.hist):
            raise ValueError(f"frames must be [batch, {self.cfg.n_streams}, {self.cfg.hist}]")
        sp, _keep = spectral_of(bands)
        power = np.empty((max(sp.n_bands, 1), frames.shape[0], self.pixel_count), np.float32)
        _check(self._lib.awpu_hip_process_bands(self._h, _f32(frames), frames.shape[0], C.byref(sp), _f32(power)), "awpu_hip_process_bands")
        return power

    def process_bands_device(self, d_frames_ptr: int, batch: int, bands, d_power_ptr: int, stream: int = 0) -> None:
        """The same on device pointers (frames [batch, n_streams, hist], power [n_bands, batch, pixels]) on `stream`; asynchronous
        (awpu_hip_process_bands_device)."""
        sp, _keep = spectral_of(bands)
        _check(self._lib.awpu_hip_process_bands_device(self._h, C.c_void_p(d_frames_ptr), batch, C.byref(sp), *_dev(d_power_ptr, stream)),
               "awpu_hip_process_bands_device")

    def _spectral(self, run, *, bands, channel, scale, want_image, want_dominant, want_power, **shown) -> SpectralResult:
        call, where, n_blocks = run
        n_frames, next_first, w = self._shown_frames(n_blocks, **shown)
        sp, _keep = spectral_of(bands, channel, scale)
        image = np.empty((n_frames, w.rows, w.cols, 3), np.uint8) if want_image else None
        big = np.empty((n_frames, w.out_rows, w.out_cols, 3), np.uint8) if w.out_rows else None
        dominant = np.empty((n_frames, w.rows, w.cols), np.uint8) if want_dominant else None
        power = np.empty((max(sp.n_bands, 1), n_frames, self.pixel_count), np.float32) if want_power else None
        _check(call(n_blocks, C.byref(w), C.byref(sp), _out_ptr(image, _u8p), _out_ptr(big, _u8p), _out_ptr(dominant, _u8p),
                    _out_ptr(power, _f32p)), where)
        return SpectralResult(image, big, dominant, power, next_first)

    def spectral_blocks(self, wire, rows: int, cols: int, bands, channel=None, scale: int = SPECTRAL_SCALE_COMMON, first: int = 0,
                        every: int = 1, out_rows: int = 0, out_cols: int = 0, flip: bool = False, stride: int = DATAGRAM_BYTES,
                        want_image: bool = True, want_dominant: bool = True, want_power: bool = False) -> SpectralResult:
        """Watch a run of wire datagrams (as watch_blocks takes them) in up to four bands at once: every block is appended to the
        ring, blocks first, first + every, ... are filtered by every band of `bands` in one pre-pass and swept once per band; byte c
        of a pixel of .image shows band channel[c] (None: band c where there is one; spectral_compose), .big is that image upscaled (and mirrored when flip),
        .dominant the strongest band of every pixel, .power every band's powers (awpu_hip_spectral_blocks).  -> SpectralResult."""
        return self._spectral(self._wire_run("awpu_hip_spectral_blocks", wire, stride), bands=bands, channel=channel, scale=scale,
                              rows=rows, cols=cols, first=first, every=every, out_rows=out_rows, out_cols=out_cols, flip=flip,
                              want_image=want_image, want_dominant=want_dominant, want_power=want_power)

    def spectral_samples(self, samples: np.ndarray, rows: int, cols: int, bands, channel=None, scale: int = SPECTRAL_SCALE_COMMON,
                         first: int = 0, every: int = 1, out_rows: int = 0, out_cols: int = 0, flip: bool = False, want_image: bool = True,
                         want_dominant: bool = True, want_power: bool = False) -> SpectralResult:
        """The same from unpacked samples [n_streams, N] (N a multiple of 256, oldest first) (awpu_hip_spectral_samples)."""
        return self._spectral(self._sample_run("awpu_hip_spectral_samples", samples), bands=bands, channel=channel, scale=scale,
                              rows=rows, cols=cols, first=first, every=every, out_rows=out_rows, out_cols=out_cols, flip=flip,
                              want_image=want_image, want_dominant=want_dominant, want_power=want_power)

    def spectral_samples_device(self, d_samples_ptr: int, pitch: int, n_blocks: int, rows: int, cols: int, bands, channel=None,
                                scale: int = SPECTRAL_SCALE_COMMON, first: int = 0, every: int = 1, d_image_ptr: int = 0, d_big_ptr: int = 0,
                                d_dominant_ptr: int = 0, d_power_ptr: int = 0, out_rows: int = 0, out_cols: int = 0, flip: bool = False,
                                stream: int = 0) -> int:
        """The same on device pointers (samples [n_streams, pitch]; image [n_frames, rows * cols, 3], big [n_frames, out_rows, out_cols,
        3], dominant [n_frames, rows * cols], power [n_bands, n_frames, pixels], each or 0) on `stream`; asynchronous.  -> next_first
        (awpu_hip_spectral_samples_device)."""
        w = _watch_struct(rows=rows, cols=cols, first=first, every=every, out_rows=out_rows, out_cols=out_cols, flip=flip)
        sp, _keep = spectral_of(bands, channel, scale)
        return self._device_run("awpu_hip_spectral_samples_device", d_samples_ptr, pitch, n_blocks, w, C.byref(sp),
                                *_dev(d_image_ptr, d_big_ptr, d_dominant_ptr, d_power_ptr, stream))

    def find_peaks_device(self, d_power_ptr: int, n_frames: int, rows: int, cols: int, d_sources_ptr: int, d_count_ptr: int,
                          radius: int = 2, max_sources: int = 4, min_power: float = 0.0, min_ratio: float = 0.0, fov_deg: float = 180.0,
                          stream: int = 0) -> None:
        """find_peaks on device pointers (power [n_frames, rows * cols] floats, sources [n_frames, max_sources] records of 40
        bytes, count [n_frames] int32) on `stream`; asynchronous (awpu_hip_find_peaks_device)."""
        f = Find(rows, cols, radius, max_sources, min_power, min_ratio, fov_deg)
        _check(self._lib.awpu_hip_find_peaks_device(self._h, C.c_void_p(d_power_ptr), n_frames, C.byref(f),
                                                    *_dev(d_sources_ptr, d_count_ptr, stream)), "awpu_hip_find_peaks_device")

    def _find(self, run, *, find, want_power, **shown) -> FindResult:
        call, where, n_blocks = run
        n_frames, next_first, w = self._shown_frames(n_blocks, **shown)
        f = _find_struct(w.rows, w.cols, find)
        sources = np.empty((n_frames, max(f.max_sources, 0)), SOURCE_DTYPE)
        count = np.empty(n_frames, np.int32)
        power = np.empty((n_frames, self.pixel_count), np.float32) if want_power else None
        _check(call(n_blocks, C.byref(w), C.byref(f), _out_ptr(sources), _out_ptr(count), _out_ptr(power, _f32p)), where)
        return FindResult(sources, count, power, next_first)

    def find_blocks(self, wire, rows: int, cols: int, first: int = 0, every: int = 1, stride: int = DATAGRAM_BYTES,
                    want_power: bool = False, **find) -> FindResult:
        """The sources in a run of consecutive blocks of wire datagrams (as watch_blocks takes them): every block is appended to
        the ring, blocks first, first + every, ... are swept and their strongest peaks found on the device; find_peaks'
        keywords (radius, max_sources, min_power, min_ratio, fov_deg) say what a source is (awpu_hip_find_blocks).  -> FindResult;
        pass its .next_first as `first` of the call that continues the run."""
        return self._find(self._wire_run("awpu_hip_find_blocks", wire, stride), rows=rows, cols=cols, first=first, every=every, find=find,
                          want_power=want_power)

    def find_samples(self, samples: np.ndarray, rows: int, cols: int, first: int = 0, every: int = 1, want_power: bool = False,
                     **find) -> FindResult:
        """The same from unpacked samples [n_streams, N] (N a multiple of 256, oldest first) (awpu_hip_find_samples)."""
        return self._find(self._sample_run("awpu_hip_find_samples", samples), rows=rows, cols=cols, first=first, every=every, find=find,
                          want_power=want_power)

    def find_samples_device(self, d_samples_ptr: int, pitch: int, n_blocks: int, rows: int, cols: int, d_sources_ptr: int,
                            d_count_ptr: int, first: int = 0, every: int = 1, d_power_ptr: int = 0, stream: int = 0, **find) -> int:
        """The same on device pointers (samples [n_streams, pitch]; sources [n_frames, max_sources] records of 40 bytes, count
        [n_frames] int32, power [n_frames, pixels] or 0) on `stream`; asynchronous.  -> next_first
        (awpu_hip_find_samples_device)."""
        w = _watch_struct(rows=rows, cols=cols, first=first, every=every)
        return self._device_run("awpu_hip_find_samples_device", d_samples_ptr, pitch, n_blocks, w, C.byref(_find_struct(rows, cols, find)),
                                *_dev(d_sources_ptr, d_count_ptr, d_power_ptr, stream))

    def expose_rows_device(self, d_power_ptr: int, n_blocks: int, n_pixels: int, first: int, every: int, length: int, d_frames_ptr: int,
                           mode: int = EXPOSE_MEAN, d_carry_ptr: int = 0, stream: int = 0) -> int:
        """expose_rows on device pointers (power [n_blocks, n_pixels], frames [n_frames, n_pixels], carry [n_pixels] or 0) on
        `stream`; asynchronous.  -> next_first (awpu_hip_expose_rows_device)."""
        e = Expose(length, mode)
        _check(self._lib.awpu_hip_expose_rows_device(self._h, C.c_void_p(d_power_ptr), n_blocks, n_pixels, first, every, C.byref(e),
                                                     *_dev(d_carry_ptr, d_frames_ptr, stream)), "awpu_hip_expose_rows_device")
        return watch_count(n_blocks, first, every)[1]

    def _expose(self, run, *, length, mode, carry, want_image, want_power, find, **shown) -> ExposeResult:
        call, where, n_blocks = run
        n_frames, next_first, w = self._shown_frames(n_blocks, **shown)
        e = Expose(length, mode)
        if carry is None:  # a recording's first call: silence before it
            carry = np.zeros(self.pixel_count, np.float32)
        elif carry.dtype != np.float32 or carry.shape != (self.pixel_count,) or not carry.flags.c_contiguous:
            raise ValueError("carry must be a contiguous float32 array [pixels]")
        f = _find_struct(w.rows, w.cols, find)
        arrays, ptrs = self._shown_outputs(n_frames, w, want_image, want_power, f)
        _check(call(n_blocks, C.byref(w), C.byref(e), _ref(f), _f32(carry), *ptrs), where)
        return ExposeResult(*arrays, next_first, carry)

    def expose_blocks(self, wire, rows: int, cols: int, length: int, first: Optional[int] = None, every: Optional[int] = None,
                      mode: int = EXPOSE_MEAN, carry: Optional[np.ndarray] = None, out_rows: int = 0, out_cols: int = 0,
                      d_colormap_ptr: int = 0, flip: bool = False, stride: int = DATAGRAM_BYTES, want_image: bool = True,
                      want_power: bool = False, find: Optional[dict] = None) -> ExposeResult:
        """Watch a run of consecutive blocks of wire datagrams (as watch_blocks takes them) with every frame exposed over the
        `length` blocks that end with its shown block: their mean power row, or with mode=EXPOSE_PEAK their per-pixel maximum
        (awpu_hip_expose_blocks).  every defaults to length and first to length - 1: back-to-back windows from the recording's
        first block on.  `find` (a dict of find_peaks' keywords, {} for the defaults) also finds the sources of every exposed
        frame.  -> ExposeResult; pass its .next_first as `first` and its .carry as `carry` to the call that continues the run
        (carry is written in place)."""
        return self._expose(self._wire_run("awpu_hip_expose_blocks", wire, stride), length=length, mode=mode, carry=carry, rows=rows, cols=cols,
                            first=length - 1 if first is None else first, every=length if every is None else every, out_rows=out_rows,
                            out_cols=out_cols, d_colormap_ptr=d_colormap_ptr, flip=flip, want_image=want_image, want_power=want_power, find=find)

    def expose_samples(self, samples: np.ndarray, rows: int, cols: int, length: int, first: Optional[int] = None,
                       every: Optional[int] = None, mode: int = EXPOSE_MEAN, carry: Optional[np.ndarray] = None, out_rows: int = 0,
                       out_cols: int = 0, d_colormap_ptr: int = 0, flip: bool = False, want_image: bool = True, want_power: bool = False,
                       find: Optional[dict] = None) -> ExposeResult:
        """The same from unpacked samples [n_streams, N] (N a multiple of 256, oldest first) (awpu_hip_expose_samples)."""
        return self._expose(self._sample_run("awpu_hip_expose_samples", samples), length=length, mode=mode, carry=carry, rows=rows, cols=cols,
                            first=length - 1 if first is None else first, every=length if every is None else every, out_rows=out_rows,
                            out_cols=out_cols, d_colormap_ptr=d_colormap_ptr, flip=flip, want_image=want_image, want_power=want_power, find=find)

    def expose_samples_device(self, d_samples_ptr: int, pitch: int, n_blocks: int, rows: int, cols: int, length: int, first: int,
                              every: int, mode: int = EXPOSE_MEAN, d_carry_ptr: int = 0, d_image_ptr: int = 0, d_big_ptr: int = 0,
                              d_power_ptr: int = 0, d_sources_ptr: int = 0, d_count_ptr: int = 0, out_rows: int = 0, out_cols: int = 0,
                              d_colormap_ptr: int = 0, flip: bool = False, stream: int = 0, find: Optional[dict] = None) -> int:
        """The same on device pointers (samples [n_streams, pitch]; carry [pixels]; image, big, power as watch_samples_device
        takes them, sources and count as find_samples_device does, each or 0) on `stream`; asynchronous.  -> next_first
        (awpu_hip_expose_samples_device)."""
        w = _watch_struct(rows=rows, cols=cols, first=first, every=every, out_rows=out_rows, out_cols=out_cols, d_colormap_ptr=d_colormap_ptr,
                          flip=flip)
        return self._device_run("awpu_hip_expose_samples_device", d_samples_ptr, pitch, n_blocks, w, C.byref(Expose(length, mode)),
                                _ref(_find_struct(rows, cols, find)),
                                *_dev(d_carry_ptr, d_image_ptr, d_big_ptr, d_power_ptr, d_sources_ptr, d_count_ptr, stream))

    def cohere(self, frames: np.ndarray, want=("power", "coherence", "weighted")):
        """The coherence sweep of host frames [batch, n_streams, hist] (or one frame): -> a dict of the maps in `want`, each
        [batch, pixels] (awpu_hip_cohere): "power" the delay-and-sum power, "coherence" the coherence factor in [0, 1],
        "weighted" their product.  The handle's gains and band apply."""
        frames = np.ascontiguousarray(frames, np.float32)
        single = frames.ndim == 2
        if single:
            frames = frames[None]
        if frames.shape[1:] != (self.cfg.n_streams, self.cfg.hist):
            raise ValueError(f"frames must be [batch, {self.cfg.n_streams}, {self.cfg.hist}]")
        names = ("power", "coherence", "weighted")
        if not want or any(name not in names for name in want):
            raise ValueError(f"want names some of {names}")
        maps = {name: np.empty((frames.shape[0], self.pixel_count), np.float32) for name in names if name in want}
        _check(self._lib.awpu_hip_cohere(self._h, _f32(frames), frames.shape[0], *[_f32(maps[name]) if name in maps else None for name in names]),
               "awpu_hip_cohere")
        return {name: m[0] for name, m in maps.items()} if single else maps

    def cohere_device(self, d_frames_ptr: int, batch: int, d_power_ptr: int = 0, d_coherence_ptr: int = 0, d_weighted_ptr: int = 0,
                      stream: int = 0) -> None:
        """The same on device pointers (frames [batch, n_streams, hist]; each map [batch, pixels] or 0) on `stream`; asynchronous
        (awpu_hip_cohere_device)."""
        _check(self._lib.awpu_hip_cohere_device(self._h, C.c_void_p(d_frames_ptr), batch,
                                                *_dev(d_power_ptr, d_coherence_ptr, d_weighted_ptr, stream)), "awpu_hip_cohere_device")

    def cohere_device_sums(self, d_frames_ptr: int, batch: int, d_sums_ptr: int = 0, d_energy_ptr: int = 0, d_power_ptr: int = 0,
                           d_coherence_ptr: int = 0, d_weighted_ptr: int = 0, stream: int = 0) -> None:
        """cohere_device plus every pixel's out[0..255] and e[0..255] into d_sums / d_energy [batch, pixels, 256], each or 0
        (awpu_hip_cohere_device_sums): the rule's bits."""
        _check(self._lib.awpu_hip_cohere_device_sums(self._h, C.c_void_p(d_frames_ptr), batch,
                                                     *_dev(d_power_ptr, d_coherence_ptr, d_weighted_ptr, d_sums_ptr, d_energy_ptr, stream)),
               "awpu_hip_cohere_device_sums")

    def peel(self, frames: np.ndarray, steps: int, gain: float = 1.0, stop_ratio: float = 0.0, want_frames: bool = False) -> "PeelResult":
        """Peel the sources of host frames [batch, n_streams, hist] (or one frame) (awpu_hip_peel): `steps` rounds of sweep, pick
        the strongest pixel, subtract its beam from every active mic.  -> a PeelResult: .steps [batch, steps] (PEEL_STEP_DTYPE),
        .clean, .residual, .map [batch, pixels], and with want_frames .frames, the residual frames.  The handle's gains apply."""
        frames = np.ascontiguousarray(frames, np.float32)
        single = frames.ndim == 2
        if single:
            frames = frames[None]
        if frames.shape[1:] != (self.cfg.n_streams, self.cfg.hist):
            raise ValueError(f"frames must be [batch, {self.cfg.n_streams}, {self.cfg.hist}]")
        batch = frames.shape[0]
        pe = Peel(steps, gain, stop_ratio)
        rec = np.empty((batch, max(steps, 0)), PEEL_STEP_DTYPE)
        maps = [np.empty((batch, self.pixel_count), np.float32) for _ in range(3)]
        left = np.empty_like(frames) if want_frames else None
        _check(self._lib.awpu_hip_peel(self._h, _f32(frames), batch, C.byref(pe), C.c_void_p(rec.ctypes.data or 16), *[_f32(m) for m in maps],
                                       None if left is None else _f32(left)), "awpu_hip_peel")
        out = [rec, *maps, left]
        return PeelResult(*[m[0] if single and m is not None else m for m in out])

    def peel_device(self, d_frames_ptr: int, batch: int, steps: int, gain: float = 1.0, stop_ratio: float = 0.0, d_steps_ptr: int = 0,
                    d_clean_ptr: int = 0, d_residual_ptr: int = 0, d_map_ptr: int = 0, d_residual_frames_ptr: int = 0, stream: int = 0) -> None:
        """The same on device pointers (frames [batch, n_streams, hist], not written; steps [batch, steps] records of 12 bytes;
        each map [batch, pixels]; the residual frames; each output or 0) on `stream`; asynchronous, with no wait inside the loop
        (awpu_hip_peel_device)."""
        pe = Peel(steps, gain, stop_ratio)
        _check(self._lib.awpu_hip_peel_device(self._h, C.c_void_p(d_frames_ptr), batch, C.byref(pe),
                                              *_dev(d_steps_ptr, d_clean_ptr, d_residual_ptr, d_map_ptr, d_residual_frames_ptr, stream)),
               "awpu_hip_peel_device")

    def peel_step_device(self, d_frames_ptr: int, batch: int, d_pixel_ptr: int, gain: float = 1.0, d_beams_ptr: int = 0, stream: int = 0) -> None:
        """One step, in place, on device pointers: frames [batch, n_streams, hist]; pixel [batch] int32, -1 = leave the frame alone;
        beams [batch, peel_beam_length] or 0 (awpu_hip_peel_step_device).  Asynchronous on `stream`."""
        _check(self._lib.awpu_hip_peel_step_device(self._h, C.c_void_p(d_frames_ptr), batch, C.c_void_p(d_pixel_ptr), gain, C.c_void_p(d_beams_ptr),
                                                   C.c_void_p(stream)), "awpu_hip_peel_step_device")

    def _peel_run(self, run, *, steps, gain, stop_ratio, show, want_image, want_power, find, **shown) -> PeelRunResult:
        call, where, n_blocks = run
        n_frames, next_first, w = self._shown_frames(n_blocks, **shown)
        pe = Peel(steps, gain, stop_ratio)
        f = _find_struct(w.rows, w.cols, find)
        (image, big, power, sources, count), ptrs = self._shown_outputs(n_frames, w, want_image, want_power, f)
        rec = np.empty((n_frames, max(steps, 0)), PEEL_STEP_DTYPE)
        _check(call(n_blocks, C.byref(w), C.byref(pe), show, _ref(f), *ptrs[:3], _out_ptr(rec), *ptrs[3:]), where)
        return PeelRunResult(image, big, power, rec, sources, count, next_first)

    def peel_blocks(self, wire, rows: int, cols: int, steps: int, gain: float = 1.0, stop_ratio: float = 0.0, first: int = 0, every: int = 1,
                    show: int = PEEL_MAP, out_rows: int = 0, out_cols: int = 0, d_colormap_ptr: int = 0, flip: bool = False,
                    stride: int = DATAGRAM_BYTES, want_image: bool = True, want_power: bool = False, find: Optional[dict] = None) -> PeelRunResult:
        """Watch a run of consecutive blocks of wire datagrams (as watch_blocks takes them) with every shown snapshot peeled
        (awpu_hip_peel_blocks): the frame is its map row, or by `show` its clean or residual row.  `find` (a dict of find_peaks'
        keywords, {} for the defaults) also finds the sources of every frame.  -> PeelRunResult."""
        return self._peel_run(self._wire_run("awpu_hip_peel_blocks", wire, stride), steps=steps, gain=gain, stop_ratio=stop_ratio, show=show,
                              rows=rows, cols=cols, first=first, every=every, out_rows=out_rows, out_cols=out_cols,
                              d_colormap_ptr=d_colormap_ptr, flip=flip, want_image=want_image, want_power=want_power, find=find)

    def peel_samples(self, samples: np.ndarray, rows: int, cols: int, steps: int, gain: float = 1.0, stop_ratio: float = 0.0, first: int = 0,
                     every: int = 1, show: int = PEEL_MAP, out_rows: int = 0, out_cols: int = 0, d_colormap_ptr: int = 0, flip: bool = False,
                     want_image: bool = True, want_power: bool = False, find: Optional[dict] = None) -> PeelRunResult:
        """The same from unpacked samples [n_streams, N] (N a multiple of 256, oldest first) (awpu_hip_peel_samples)."""
        return self._peel_run(self._sample_run("awpu_hip_peel_samples", samples), steps=steps, gain=gain, stop_ratio=stop_ratio, show=show,
                              rows=rows, cols=cols, first=first, every=every, out_rows=out_rows, out_cols=out_cols,
                              d_colormap_ptr=d_colormap_ptr, flip=flip, want_image=want_image, want_power=want_power, find=find)

    def peel_samples_device(self, d_samples_ptr: int, pitch: int, n_blocks: int, rows: int, cols: int, steps: int, gain: float = 1.0,
                            stop_ratio: float = 0.0, first: int = 0, every: int = 1, show: int = PEEL_MAP, d_image_ptr: int = 0, d_big_ptr: int = 0,
                            d_power_ptr: int = 0, d_steps_ptr: int = 0, d_sources_ptr: int = 0, d_count_ptr: int = 0, out_rows: int = 0,
                            out_cols: int = 0, d_colormap_ptr: int = 0, flip: bool = False, stream: int = 0, find: Optional[dict] = None) -> int:
        """The same on device pointers (samples [n_streams, pitch]; image, big, power as watch_samples_device takes them, steps
        [n_frames, steps] records of 12 bytes, sources and count as find_samples_device does, each or 0) on `stream`; asynchronous.
        -> next_first (awpu_hip_peel_samples_device)."""
        w = _watch_struct(rows=rows, cols=cols, first=first, every=every, out_rows=out_rows, out_cols=out_cols, d_colormap_ptr=d_colormap_ptr,
                          flip=flip)
        return self._device_run("awpu_hip_peel_samples_device", d_samples_ptr, pitch, n_blocks, w, C.byref(Peel(steps, gain, stop_ratio)), show,
                                _ref(_find_struct(rows, cols, find)),
                                *_dev(d_image_ptr, d_big_ptr, d_power_ptr, d_steps_ptr, d_sources_ptr, d_count_ptr, stream))

    def _cohere_run(self, run, *, show, want_image, want_power, find, **shown) -> CohereResult:
        call, where, n_blocks = run
        n_frames, next_first, w = self._shown_frames(n_blocks, **shown)
        co = Cohere(show)
        f = _find_struct(w.rows, w.cols, find)
        arrays, ptrs = self._shown_outputs(n_frames, w, want_image, want_power, f)
        _check(call(n_blocks, C.byref(w), C.byref(co), _ref(f), *ptrs), where)
        return CohereResult(*arrays, next_first)

    def cohere_blocks(self, wire, rows: int, cols: int, first: int = 0, every: int = 1, show: int = COHERE_WEIGHTED, out_rows: int = 0,
                      out_cols: int = 0, d_colormap_ptr: int = 0, flip: bool = False, stride: int = DATAGRAM_BYTES, want_image: bool = True,
                      want_power: bool = False, find: Optional[dict] = None) -> CohereResult:
        """Watch a run of consecutive blocks of wire datagrams (as watch_blocks takes them) through the coherence sweep: every
        shown frame is its coherence-weighted row, or with show=COHERE_FACTOR its coherence row (awpu_hip_cohere_blocks).  `find`
        (a dict of find_peaks' keywords, {} for the defaults) also finds the sources of every frame.  -> CohereResult; pass its
        .next_first as `first` of the call that continues the run."""
        return self._cohere_run(self._wire_run("awpu_hip_cohere_blocks", wire, stride), show=show, rows=rows, cols=cols, first=first, every=every,
                                out_rows=out_rows, out_cols=out_cols, d_colormap_ptr=d_colormap_ptr, flip=flip, want_image=want_image,
                                want_power=want_power, find=find)

    def cohere_samples(self, samples: np.ndarray, rows: int, cols: int, first: int = 0, every: int = 1, show: int = COHERE_WEIGHTED,
                       out_rows: int = 0, out_cols: int = 0, d_colormap_ptr: int = 0, flip: bool = False, want_image: bool = True,
                       want_power: bool = False, find: Optional[dict] = None) -> CohereResult:
        """The same from unpacked samples [n_streams, N] (N a multiple of 256, oldest first) (awpu_hip_cohere_samples)."""
        return self._cohere_run(self._sample_run("awpu_hip_cohere_samples", samples), show=show, rows=rows, cols=cols, first=first, every=every,
                                out_rows=out_rows, out_cols=out_cols, d_colormap_ptr=d_colormap_ptr, flip=flip, want_image=want_image,
                                want_power=want_power, find=find)

    def cohere_samples_device(self, d_samples_ptr: int, pitch: int, n_blocks: int, rows: int, cols: int, first: int = 0, every: int = 1,
                              show: int = COHERE_WEIGHTED, d_image_ptr: int = 0, d_big_ptr: int = 0, d_power_ptr: int = 0,
                              d_sources_ptr: int = 0, d_count_ptr: int = 0, out_rows: int = 0, out_cols: int = 0, d_colormap_ptr: int = 0,
                              flip: bool = False, stream: int = 0, find: Optional[dict] = None) -> int:
        """The same on device pointers (samples [n_streams, pitch]; image, big, power as watch_samples_device takes them, sources
        and count as find_samples_device does, each or 0) on `stream`; asynchronous.  -> next_first
        (awpu_hip_cohere_samples_device)."""
        w = _watch_struct(rows=rows, cols=cols, first=first, every=every, out_rows=out_rows, out_cols=out_cols, d_colormap_ptr=d_colormap_ptr,
                          flip=flip)
        return self._device_run("awpu_hip_cohere_samples_device", d_samples_ptr, pitch, n_blocks, w, C.byref(Cohere(show)),
                                _ref(_find_struct(rows, cols, find)), *_dev(d_image_ptr, d_big_ptr, d_power_ptr, d_sources_ptr, d_count_ptr, stream))

    def tones(self, frames: np.ndarray, groups, window: int = TONES_RECT, want=("tone", "pitch")):
        """The tone sweep of host frames [batch, n_streams, hist] (or one frame), groups as tones_of takes them: -> a dict of the
        outputs in `want`: "tone" [batch, n_groups, pixels], "pitch" [batch, pixels] int32 (awpu_hip_tones).  The handle's gains
        and band apply."""
        t = tones_of(groups, window)
        frames = np.ascontiguousarray(frames, np.float32)
        single = frames.ndim == 2
        if single:
            frames = frames[None]
        if frames.shape[1:] != (self.cfg.n_streams, self.cfg.hist):
            raise ValueError(f"frames must be [batch, {self.cfg.n_streams}, {self.cfg.hist}]")
        if not want or any(name not in ("tone", "pitch") for name in want):
            raise ValueError("want names some of ('tone', 'pitch')")
        out = {}
        if "tone" in want:
            out["tone"] = np.empty((frames.shape[0], max(t.n_groups, 0), self.pixel_count), np.float32)
        if "pitch" in want:
            out["pitch"] = np.empty((frames.shape[0], self.pixel_count), np.int32)
        _check(self._lib.awpu_hip_tones(self._h, _f32(frames), frames.shape[0], C.byref(t), _out_ptr(out.get("tone"), _f32p),
                                        _out_ptr(out.get("pitch"), _i32p)), "awpu_hip_tones")
        return {name: a[0] for name, a in out.items()} if single else out

    def tones_device(self, d_frames_ptr: int, batch: int, groups, window: int = TONES_RECT, d_tone_ptr: int = 0, d_pitch_ptr: int = 0,
                     stream: int = 0) -> None:
        """The same on device pointers (frames [batch, n_streams, hist]; tone [batch, n_groups, pixels], pitch [batch, pixels] int32,
        each or 0) on `stream`; asynchronous (awpu_hip_tones_device)."""
        t = tones_of(groups, window)
        _check(self._lib.awpu_hip_tones_device(self._h, C.c_void_p(d_frames_ptr), batch, C.byref(t), *_dev(d_tone_ptr, d_pitch_ptr, stream)),
               "awpu_hip_tones_device")

    def tones_device_bins(self, d_frames_ptr: int, batch: int, groups, window: int = TONES_RECT, d_bins_ptr: int = 0, d_spectrum_ptr: int = 0,
                          d_tone_ptr: int = 0, d_pitch_ptr: int = 0, stream: int = 0) -> None:
        """tones_device plus every pixel's bins [batch, pixels, 129] and spectrum [batch, pixels, 129, 2] into d_bins / d_spectrum,
        each or 0 (awpu_hip_tones_device_bins): the rule's bits."""
        t = tones_of(groups, window)
        _check(self._lib.awpu_hip_tones_device_bins(self._h, C.c_void_p(d_frames_ptr), batch, C.byref(t),
                                                    *_dev(d_tone_ptr, d_pitch_ptr, d_bins_ptr, d_spectrum_ptr, stream)), "awpu_hip_tones_device_bins")

    def _tones_run(self, run, *, groups, window, show, want_image, want_power, find, **shown) -> TonesResult:
        call, where, n_blocks = run
        n_frames, next_first, w = self._shown_frames(n_blocks, **shown)
        t = tones_of(groups, window)
        f = _find_struct(w.rows, w.cols, find)
        arrays, ptrs = self._shown_outputs(n_frames, w, want_image, want_power, f)
        _check(call(n_blocks, C.byref(w), C.byref(t), show, _ref(f), *ptrs), where)
        return TonesResult(*arrays, next_first)

    def tones_blocks(self, wire, rows: int, cols: int, groups, window: int = TONES_RECT, show: int = 0, first: int = 0, every: int = 1,
                     out_rows: int = 0, out_cols: int = 0, d_colormap_ptr: int = 0, flip: bool = False, stride: int = DATAGRAM_BYTES,
                     want_image: bool = True, want_power: bool = False, find: Optional[dict] = None) -> TonesResult:
        """Watch a run of consecutive blocks of wire datagrams (as watch_blocks takes them) through the tone sweep: every shown
        frame is the plane of group `show`, or with show=TONES_SHOW_PITCH the pitch row (awpu_hip_tones_blocks).  `find` (a dict
        of find_peaks' keywords, {} for the defaults) also finds the sources of every frame.  -> TonesResult; pass its .next_first
        as `first` of the call that continues the run."""
        return self._tones_run(self._wire_run("awpu_hip_tones_blocks", wire, stride), groups=groups, window=window, show=show, rows=rows, cols=cols,
                               first=first, every=every, out_rows=out_rows, out_cols=out_cols, d_colormap_ptr=d_colormap_ptr, flip=flip,
                               want_image=want_image, want_power=want_power, find=find)

    def tones_samples(self, samples: np.ndarray, rows: int, cols: int, groups, window: int = TONES_RECT, show: int = 0, first: int = 0,
                      every: int = 1, out_rows: int = 0, out_cols: int = 0, d_colormap_ptr: int = 0, flip: bool = False,
                      want_image: bool = True, want_power: bool = False, find: Optional[dict] = None) -> TonesResult:
        """The same from unpacked samples [n_streams, N] (N a multiple of 256, oldest first) (awpu_hip_tones_samples)."""
        return self._tones_run(self._sample_run("awpu_hip_tones_samples", samples), groups=groups, window=window, show=show, rows=rows, cols=cols,
                               first=first, every=every, out_rows=out_rows, out_cols=out_cols, d_colormap_ptr=d_colormap_ptr, flip=flip,
                               want_image=want_image, want_power=want_power, find=find)

    def tones_samples_device(self, d_samples_ptr: int, pitch: int, n_blocks: int, rows: int, cols: int, groups, window: int = TONES_RECT,
                             show: int = 0, first: int = 0, every: int = 1, d_image_ptr: int = 0, d_big_ptr: int = 0, d_power_ptr: int = 0,
                             d_sources_ptr: int = 0, d_count_ptr: int = 0, out_rows: int = 0, out_cols: int = 0, d_colormap_ptr: int = 0,
                             flip: bool = False, stream: int = 0, find: Optional[dict] = None) -> int:
        """The same on device pointers (samples [n_streams, pitch]; image, big, power as watch_samples_device takes them, sources
        and count as find_samples_device does, each or 0) on `stream`; asynchronous.  -> next_first
        (awpu_hip_tones_samples_device)."""
        w = _watch_struct(rows=rows, cols=cols, first=first, every=every, out_rows=out_rows, out_cols=out_cols, d_colormap_ptr=d_colormap_ptr,
                          flip=flip)
        return self._device_run("awpu_hip_tones_samples_device", d_samples_ptr, pitch, n_blocks, w, C.byref(tones_of(groups, window)), show,
                                _ref(_find_struct(rows, cols, find)), *_dev(d_image_ptr, d_big_ptr, d_power_ptr, d_sources_ptr, d_count_ptr, stream))

    def _csm_window(self, c: Csm, n_frames: int, *, length, carry, carried, want_planes):
        """What the two cross-spectral runs carry from call to call and may hand out: (carry [length - 1, n_bins, usable, 2] -- the
        caller's, copied, or zeros --, how many of its blocks are held as the C int the call updates, planes [n_frames, n_bins,
        pixels] or None)."""
        shape = (max(int(length) - 1, 0), max(c.n_bins, 0), self.usable, 2)
        carry = np.zeros(shape, np.float32) if carry is None else np.ascontiguousarray(carry, np.float32).copy()
        if carry.shape != shape:
            raise ValueError(f"carry must be {shape}")
        planes = np.empty((n_frames, max(c.n_bins, 0), self.pixel_count), np.float32) if want_planes else None
        return carry, C.c_int32(int(carried)), planes

    def _csm_watch(self, run, *, bins, window, kind, loading, length, show, carry, carried, want_image, want_power, want_planes, want_solved,
                   find, **shown) -> CsmWatchResult:
        call, where, n_blocks = run
        n_frames, next_first, w = self._shown_frames(n_blocks, **shown)
        c = csm_of(bins, window, kind, loading)
        f = _find_struct(w.rows, w.cols, find)
        carry, held, planes = self._csm_window(c, n_frames, length=length, carry=carry, carried=carried, want_planes=want_planes)
        arrays, ptrs = self._shown_outputs(n_frames, w, want_image, want_power, f)
        solved = np.empty((n_frames, max(c.n_bins, 0)), np.int32) if want_solved else None
        _check(call(n_blocks, C.byref(w), C.byref(c), int(length), int(show), _ref(f), _out_ptr(carry, _f32p),
                    C.cast(C.byref(held), _i32p), *ptrs, _out_ptr(planes, _f32p), _out_ptr(solved, _i32p)), where)
        return CsmWatchResult(*arrays, planes, solved, next_first, carry, held.value)

    def csm_watch_blocks(self, wire, rows: int, cols: int, bins, window: int = TONES_RECT, kind: int = CSM_CONVENTIONAL, loading: float = 1e-3,
                         length: int = 64, show: int = CSM_SHOW_SUM, first: int = 0, every: int = 1, carry=None, carried: int = 0,
                         out_rows: int = 0, out_cols: int = 0, d_colormap_ptr: int = 0, flip: bool = False, stride: int = DATAGRAM_BYTES,
                         want_image: bool = True, want_power: bool = False, want_planes: bool = False, want_solved: bool = False,
                         find: Optional[dict] = None) -> CsmWatchResult:
        """Watch a run of consecutive blocks of wire datagrams (as watch_blocks takes them) through the cross-spectral maps
        (awpu_hip_csm_watch_blocks): every shown frame is the map of the `length` blocks that end with it -- the plane of bin index
        `show`, or with CSM_SHOW_SUM the planes added up --, conventional, diagonal-removed or Capon's.  `find` also finds the
        sources of every frame.  -> CsmWatchResult; pass its .next_first, .carry and .carried to the call that continues the run."""
        return self._csm_watch(self._wire_run("awpu_hip_csm_watch_blocks", wire, stride), bins=bins, window=window, kind=kind, loading=loading,
                               length=length, show=show, carry=carry, carried=carried, rows=rows, cols=cols, first=first, every=every,
                               out_rows=out_rows, out_cols=out_cols, d_colormap_ptr=d_colormap_ptr, flip=flip, want_image=want_image,
                               want_power=want_power, want_planes=want_planes, want_solved=want_solved, find=find)

    def csm_watch_samples(self, samples: np.ndarray, rows: int, cols: int, bins, window: int = TONES_RECT, kind: int = CSM_CONVENTIONAL,
                          loading: float = 1e-3, length: int = 64, show: int = CSM_SHOW_SUM, first: int = 0, every: int = 1, carry=None,
                          carried: int = 0, out_rows: int = 0, out_cols: int = 0, d_colormap_ptr: int = 0, flip: bool = False,
                          want_image: bool = True, want_power: bool = False, want_planes: bool = False, want_solved: bool = False,
                          find: Optional[dict] = None) -> CsmWatchResult:
        """The same from unpacked samples [n_streams, N] (N a multiple of 256, oldest first) (awpu_hip_csm_watch_samples)."""
        return self._csm_watch(self._sample_run("awpu_hip_csm_watch_samples", samples), bins=bins, window=window, kind=kind, loading=loading,
                               length=length, show=show, carry=carry, carried=carried, rows=rows, cols=cols, first=first, every=every,
                               out_rows=out_rows, out_cols=out_cols, d_colormap_ptr=d_colormap_ptr, flip=flip, want_image=want_image,
                               want_power=want_power, want_planes=want_planes, want_solved=want_solved, find=find)

    def csm_watch_samples_device(self, d_samples_ptr: int, pitch: int, n_blocks: int, rows: int, cols: int, bins, window: int = TONES_RECT,
                                 kind: int = CSM_CONVENTIONAL, loading: float = 1e-3, length: int = 64, show: int = CSM_SHOW_SUM,
                                 first: int = 0, every: int = 1, d_carry_ptr: int = 0, carried: int = 0, d_image_ptr: int = 0,
                                 d_big_ptr: int = 0, d_power_ptr: int = 0, d_sources_ptr: int = 0, d_count_ptr: int = 0,
                                 d_planes_ptr: int = 0, d_solved_ptr: int = 0, out_rows: int = 0, out_cols: int = 0, d_colormap_ptr: int = 0,
                                 flip: bool = False, stream: int = 0, find: Optional[dict] = None):
        """The same on device pointers (samples [n_streams, pitch]; carry [length - 1, n_bins, usable, 2]; image, big, power, sources
        and count as tones_samples_device takes them; planes [n_frames, n_bins, pixels] and solved [n_frames, n_bins], each or 0) on
        `stream`; asynchronous.  -> (next_first, carried) for the call that continues the run
        (awpu_hip_csm_watch_samples_device)."""
        w = _watch_struct(rows=rows, cols=cols, first=first, every=every, out_rows=out_rows, out_cols=out_cols, d_colormap_ptr=d_colormap_ptr,
                          flip=flip)
        c, held = csm_of(bins, window, kind, loading), C.c_int32(int(carried))
        next_first = self._device_run("awpu_hip_csm_watch_samples_device", d_samples_ptr, pitch, n_blocks, w, C.byref(c), int(length), int(show),
                                      _ref(_find_struct(rows, cols, find)), C.c_void_p(d_carry_ptr), C.cast(C.byref(held), _i32p),
                                      *_dev(d_image_ptr, d_big_ptr, d_power_ptr, d_sources_ptr, d_count_ptr, d_planes_ptr, d_solved_ptr, stream))
        return next_first, held.value

    def _csm_clean_run(self, run, *, bins, steps, gain, stop_ratio, what, window, length, show, carry, carried, want_image, want_power,
                       want_planes, find, **shown) -> CsmCleanRunResult:
        call, where, n_blocks = run
        n_frames, next_first, w = self._shown_frames(n_blocks, **shown)
        c, cl = csm_of(bins, window), CsmClean(int(steps), float(gain), float(stop_ratio))
        f = _find_struct(w.rows, w.cols, find)
        carry, held, planes = self._csm_window(c, n_frames, length=length, carry=carry, carried=carried, want_planes=want_planes)
        arrays, ptrs = self._shown_outputs(n_frames, w, want_image, want_power, f)
        rec = np.empty((n_frames, max(c.n_bins, 0), max(int(steps), 0)), CSM_CLEAN_STEP_DTYPE)
        _check(call(n_blocks, C.byref(w), C.byref(c), int(length), int(show), _ref(f), _out_ptr(carry, _f32p),
                    C.cast(C.byref(held), _i32p), C.byref(cl), int(what), *ptrs, _out_ptr(planes, _f32p), _out_ptr(rec)), where)
        return CsmCleanRunResult(*arrays, planes, rec, next_first, carry, held.value)

    def csm_clean_blocks(self, wire, rows: int, cols: int, bins, steps: int, gain: float = 1.0, stop_ratio: float = 0.0,
                         what: int = CSM_CLEAN_MAP, window: int = TONES_RECT, length: int = 64, show: int = CSM_SHOW_SUM, first: int = 0,
                         every: int = 1, carry=None, carried: int = 0, out_rows: int = 0, out_cols: int = 0, d_colormap_ptr: int = 0,
                         flip: bool = False, stride: int = DATAGRAM_BYTES, want_image: bool = True, want_power: bool = False,
                         want_planes: bool = False, find: Optional[dict] = None) -> CsmCleanRunResult:
        """Watch a run of consecutive blocks of wire datagrams through CLEAN-SC (awpu_hip_csm_clean_blocks): every shown frame is
        csm_clean of the matrix of the `length` blocks that end with it -- its map (CSM_CLEAN_MAP), clean (CSM_CLEAN_CLEAN) or
        residual (CSM_CLEAN_RESIDUAL) rows, of which the plane of bin index `show` or with CSM_SHOW_SUM their sum is shown.
        -> CsmCleanRunResult; pass its .next_first, .carry and .carried to the call that continues the run."""
        return self._csm_clean_run(self._wire_run("awpu_hip_csm_clean_blocks", wire, stride), bins=bins, steps=steps, gain=gain, stop_ratio=stop_ratio,
                                   what=what, window=window, length=length, show=show, carry=carry, carried=carried, rows=rows, cols=cols,
                                   first=first, every=every, out_rows=out_rows, out_cols=out_cols, d_colormap_ptr=d_colormap_ptr, flip=flip,
                                   want_image=want_image, want_power=want_power, want_planes=want_planes, find=find)

    def csm_clean_samples(self, samples: np.ndarray, rows: int, cols: int, bins, steps: int, gain: float = 1.0, stop_ratio: float = 0.0,
                          what: int = CSM_CLEAN_MAP, window: int = TONES_RECT, length: int = 64, show: int = CSM_SHOW_SUM, first: int = 0,
                          every: int = 1, carry=None, carried: int = 0, out_rows: int = 0, out_cols: int = 0, d_colormap_ptr: int = 0,
                          flip: bool = False, want_image: bool = True, want_power: bool = False, want_planes: bool = False,
                          find: Optional[dict] = None) -> CsmCleanRunResult:
        """The same from unpacked samples [n_streams, N] (N a multiple of 256, oldest first) (awpu_hip_csm_clean_samples)."""
        return self._csm_clean_run(self._sample_run("awpu_hip_csm_clean_samples", samples), bins=bins, steps=steps, gain=gain, stop_ratio=stop_ratio,
                                   what=what, window=window, length=length, show=show, carry=carry, carried=carried, rows=rows, cols=cols,
                                   first=first, every=every, out_rows=out_rows, out_cols=out_cols, d_colormap_ptr=d_colormap_ptr, flip=flip,
                                   want_image=want_image, want_power=want_power, want_planes=want_planes, find=find)

    def csm_clean_samples_device(self, d_samples_ptr: int, pitch: int, n_blocks: int, rows: int, cols: int, bins, steps: int, gain: float = 1.0,
                                 stop_ratio: float = 0.0, what: int = CSM_CLEAN_MAP, window: int = TONES_RECT, length: int = 64,
                                 show: int = CSM_SHOW_SUM, first: int = 0, every: int = 1, d_carry_ptr: int = 0, carried: int = 0,
                                 d_image_ptr: int = 0, d_big_ptr: int = 0, d_power_ptr: int = 0, d_sources_ptr: int = 0, d_count_ptr: int = 0,
                                 d_planes_ptr: int = 0, d_steps_ptr: int = 0, out_rows: int = 0, out_cols: int = 0, d_colormap_ptr: int = 0,
                                 flip: bool = False, stream: int = 0, find: Optional[dict] = None):
        """The same on device pointers (as csm_watch_samples_device takes them; steps [n_frames, n_bins, steps] records or 0) on
        `stream`; asynchronous.  -> (next_first, carried) for the call that continues the run (awpu_hip_csm_clean_samples_device)."""
        w = _watch_struct(rows=rows, cols=cols, first=first, every=every, out_rows=out_rows, out_cols=out_cols, d_colormap_ptr=d_colormap_ptr,
                          flip=flip)
        c, cl, held = csm_of(bins, window), CsmClean(int(steps), float(gain), float(stop_ratio)), C.c_int32(int(carried))
        next_first = self._device_run("awpu_hip_csm_clean_samples_device", d_samples_ptr, pitch, n_blocks, w, C.byref(c), int(length), int(show),
                                      _ref(_find_struct(rows, cols, find)), C.c_void_p(d_carry_ptr), C.cast(C.byref(held), _i32p), C.byref(cl),
                                      int(what),
                                      *_dev(d_image_ptr, d_big_ptr, d_power_ptr, d_sources_ptr, d_count_ptr, d_planes_ptr, d_steps_ptr, stream))
        return next_first, held.value

    def csm_samples(self, samples: np.ndarray, bins, window: int = TONES_RECT, matrix: Optional[np.ndarray] = None, block_count: int = 0,
                    n_blocks: Optional[int] = None, want_spectra: bool = False):
        """Steps 1 and 2 of include/awpu_hip_csm.h on the device (awpu_hip_csm_samples): the blocks of host samples [n_streams, pitch]
        (the first n_blocks, default all whole ones) of the handle's active mics, with its gains, added into `matrix`
        [n_bins, usable, usable, 2] (default: a new one of zeros) -> (matrix, block_count + n_blocks), and with want_spectra the
        blocks' spectra [n_blocks, n_bins, usable, 2] as a third item."""
        c = csm_of(bins, window)
        samples = np.ascontiguousarray(samples, np.float32)
        if samples.ndim != 2 or samples.shape[0] != self.cfg.n_streams:
            raise ValueError(f"samples must be [{self.cfg.n_streams}, pitch]")
        n_blocks = samples.shape[1] // 256 if n_blocks is None else int(n_blocks)
        usable = self.usable
        shape = (max(c.n_bins, 0), usable, usable, 2)
        if matrix is None:
            matrix = np.zeros(shape, np.float32)
        if matrix.dtype != np.float32 or matrix.shape != shape or not matrix.flags.c_contiguous:
            raise ValueError(f"matrix must be contiguous float32 {shape}")
        spectra = np.empty((max(n_blocks, 0), shape[0], usable, 2), np.float32) if want_spectra else None
        count = C.c_int32(block_count)
        _check(self._lib.awpu_hip_csm_samples(self._h, _f32(samples), samples.shape[1], n_blocks, C.byref(c), _out_ptr(matrix, _f32p),
                                              C.cast(C.byref(count), _i32p), _out_ptr(spectra, _f32p)), "awpu_hip_csm_samples")
        return (matrix, count.value, spectra) if want_spectra else (matrix, count.value)

    def csm_samples_device(self, d_samples_ptr: int, pitch: int, n_blocks: int, bins, d_matrix_ptr: int, window: int = TONES_RECT,
                           block_count: int = 0, d_spectra_ptr: int = 0, stream: int = 0) -> int:
        """The same on device pointers (samples [n_streams, pitch], matrix [n_bins, usable, usable, 2] added into, spectra
        [n_blocks, n_bins, usable, 2] or 0) on `stream`; asynchronous -> block_count + n_blocks (awpu_hip_csm_samples_device)."""
        c = csm_of(bins, window)
        count = C.c_int32(block_count)
        _check(self._lib.awpu_hip_csm_samples_device(self._h, C.c_void_p(d_samples_ptr), pitch, n_blocks, C.byref(c), C.c_void_p(d_matrix_ptr),
                                                     C.cast(C.byref(count), _i32p), *_dev(d_spectra_ptr, stream)), "awpu_hip_csm_samples_device")
        return count.value

    def csm_map(self, matrix: np.ndarray, block_count: int, bins, window: int = TONES_RECT, kind: int = CSM_CONVENTIONAL, want=("map",)):
        """Steps 3 to 5 on the device with the handle's table and active mics (awpu_hip_csm_map): matrix [n_bins, usable, usable, 2]
        as csm_map_host takes it -> a dict of the outputs in `want`: "map" and "q", each [n_bins, pixels]."""
        c = csm_of(bins, window, kind)
        matrix = np.ascontiguousarray(matrix, np.float32)
        usable = self.usable
        if matrix.shape != (max(c.n_bins, 0), usable, usable, 2):
            raise ValueError(f"matrix must be [{max(c.n_bins, 0)}, {usable}, {usable}, 2]")
        if not want or any(name not in ("map", "q") for name in want):
            raise ValueError("want names some of ('map', 'q')")
        out = {name: np.empty((max(c.n_bins, 0), self.pixel_count), np.float32) for name in ("map", "q") if name in want}
        _check(self._lib.awpu_hip_csm_map(self._h, _f32(matrix), int(block_count), C.byref(c), _out_ptr(out.get("map"), _f32p),
                                          _out_ptr(out.get("q"), _f32p)), "awpu_hip_csm_map")
        return out

    def csm_invert(self, matrix: np.ndarray, block_count: int, bins, loading: float = 1e-3) -> np.ndarray:
        """Step 6a on the device (awpu_hip_csm_invert): the loaded inverse [n_bins, usable, usable, 2] of a host matrix, the bits
        of csm_invert_rule_host.  An unsolved bin raises AwpuError (ERR_RANGE)."""
        c = csm_of(bins, TONES_RECT, CSM_CAPON, loading)
        matrix = _csm_square(matrix, c)
        usable = self.usable
        if matrix.shape[1] != usable:
            raise ValueError(f"matrix must be [n_bins, {usable}, {usable}, 2]")
        out = np.empty_like(matrix)
        _check(self._lib.awpu_hip_csm_invert(self._h, _f32(matrix), int(block_count), C.byref(c), _out_ptr(out, _f32p)), "awpu_hip_csm_invert")
        return out

    def csm_invert_device(self, d_matrix_ptr: int, block_count: int, bins, d_inverse_ptr: int, loading: float = 1e-3, d_solved_ptr: int = 0,
                          stream: int = 0) -> None:
        """The same on device pointers (d_solved [n_bins] int32 or 0) on `stream`; asynchronous, and an unsolved bin is +0 with
        solved 0, no error (awpu_hip_csm_invert_device)."""
        c = csm_of(bins, TONES_RECT, CSM_CAPON, loading)
        _check(self._lib.awpu_hip_csm_invert_device(self._h, C.c_void_p(d_matrix_ptr), int(block_count), C.byref(c),
                                                    *_dev(d_inverse_ptr, d_solved_ptr, stream)), "awpu_hip_csm_invert_device")

    def csm_map_device(self, d_matrix_ptr: int, block_count: int, bins, window: int = TONES_RECT, kind: int = CSM_CONVENTIONAL,
                       d_map_ptr: int = 0, d_q_ptr: int = 0, stream: int = 0) -> None:
        """The same on device pointers (map and q [n_bins, pixels], each or 0) on `stream`; asynchronous (awpu_hip_csm_map_device)."""
        c = csm_of(bins, window, kind)
        _check(self._lib.awpu_hip_csm_map_device(self._h, C.c_void_p(d_matrix_ptr), int(block_count), C.byref(c), *_dev(d_map_ptr, d_q_ptr, stream)),
               "awpu_hip_csm_map_device")

    def csm_eig(self, matrix: np.ndarray, block_count: int, bins):
        """Step 8a on the device (awpu_hip_csm_eig): the eigendecomposition of a host matrix [n_bins, usable, usable, 2], the bits of
        csm_eig_host -> (values, vectors, solved, sweeps) as csm_eig_host returns them."""
        c = csm_of(bins)
        matrix = _csm_square(matrix, c)
        K, U = max(c.n_bins, 0), self.usable
        if matrix.shape[1] != U:
            raise ValueError(f"matrix must be [n_bins, {U}, {U}, 2]")
        values, vectors = np.empty((K, U), np.float32), np.empty_like(matrix)
        solved, sweeps = np.empty(K, np.int32), np.empty(K, np.int32)
        _check(self._lib.awpu_hip_csm_eig(self._h, _f32(matrix), int(block_count), C.byref(c), _out_ptr(values, _f32p), _out_ptr(vectors, _f32p),
                                          _out_ptr(solved, _i32p), _out_ptr(sweeps, _i32p)), "awpu_hip_csm_eig")
        return values, vectors, solved, sweeps

    def csm_eig_device(self, d_matrix_ptr: int, block_count: int, bins, d_values_ptr: int, d_vectors_ptr: int, d_solved_ptr: int = 0,
                       d_sweeps_ptr: int = 0, stream: int = 0) -> None:
        """The same on device pointers (values [n_bins, usable], vectors [n_bins, usable, usable, 2]; solved and sweeps [n_bins]
        int32, each or 0) on `stream`; asynchronous (awpu_hip_csm_eig_device)."""
        c = csm_of(bins)
        _check(self._lib.awpu_hip_csm_eig_device(self._h, C.c_void_p(d_matrix_ptr), int(block_count), C.byref(c),
                                                 *_dev(d_values_ptr, d_vectors_ptr, d_solved_ptr, d_sweeps_ptr, stream)), "awpu_hip_csm_eig_device")

    def csm_eig_weigh_device(self, d_values_ptr: int, d_vectors_ptr: int, bins, d_weighed_ptr: int, kind: int = CSM_EIG_MUSIC, n_sources: int = 0,
                             root: int = 0, stream: int = 0) -> None:
        """Step 8b on device pointers (weighed [n_bins, usable, usable, 2]) on `stream`; asynchronous, the bits of
        csm_eig_weigh_host (awpu_hip_csm_eig_weigh_device)."""
        c, e = csm_of(bins), csm_eig_of(kind, n_sources, root)
        _check(self._lib.awpu_hip_csm_eig_weigh_device(self._h, C.c_void_p(d_values_ptr), C.c_void_p(d_vectors_ptr), C.byref(c), C.byref(e),
                                                       *_dev(d_weighed_ptr, stream)), "awpu_hip_csm_eig_weigh_device")

    def csm_eig_map(self, matrix: np.ndarray, block_count: int, bins, kind: int = CSM_EIG_MUSIC, n_sources: int = 0, root: int = 0,
                    window: int = TONES_RECT, want=("map",)):
        """Steps 8a to 8c on the device with the handle's table and active mics (awpu_hip_csm_eig_map): the MUSIC or functional map
        of a host matrix [n_bins, usable, usable, 2] with its block count -> a dict of the outputs in `want`: "map" [n_bins, pixels]
        (always computed), "values" [n_bins, usable] and "solved" [n_bins] int32."""
        c, e = csm_of(bins, window), csm_eig_of(kind, n_sources, root)
        matrix = np.ascontiguousarray(matrix, np.float32)
        K, U = max(c.n_bins, 0), self.usable
        if matrix.shape != (K, U, U, 2):
            raise ValueError(f"matrix must be [{K}, {U}, {U}, 2]")
        if not want or any(name not in ("map", "values", "solved") for name in want):
            raise ValueError("want names some of ('map', 'values', 'solved')")
        out = {"map": np.empty((K, self.pixel_count), np.float32)}
        if "values" in want:
            out["values"] = np.empty((K, U), np.float32)
        if "solved" in want:
            out["solved"] = np.empty(K, np.int32)
        _check(self._lib.awpu_hip_csm_eig_map(self._h, _f32(matrix), int(block_count), C.byref(c), C.byref(e), _out_ptr(out["map"], _f32p),
                                              _out_ptr(out.get("values"), _f32p), _out_ptr(out.get("solved"), _i32p)), "awpu_hip_csm_eig_map")
        return {name: out[name] for name in ("map", "values", "solved") if name in want}

    def csm_eig_map_device(self, d_matrix_ptr: int, block_count: int, bins, d_map_ptr: int, kind: int = CSM_EIG_MUSIC, n_sources: int = 0,
                           root: int = 0, window: int = TONES_RECT, d_values_ptr: int = 0, d_solved_ptr: int = 0, stream: int = 0) -> None:
        """The same on device pointers (map [n_bins, pixels]; values [n_bins, usable] and solved [n_bins] int32, each or 0) on
        `stream`; asynchronous (awpu_hip_csm_eig_map_device)."""
        c, e = csm_of(bins, window), csm_eig_of(kind, n_sources, root)
        _check(self._lib.awpu_hip_csm_eig_map_device(self._h, C.c_void_p(d_matrix_ptr), int(block_count), C.byref(c), C.byref(e),
                                                     *_dev(d_map_ptr, d_values_ptr, d_solved_ptr, stream)), "awpu_hip_csm_eig_map_device")

    def csm_clean(self, matrix: np.ndarray, block_count: int, bins, steps: int, gain: float = 1.0, stop_ratio: float = 0.0,
                  window: int = TONES_RECT, kind: int = CSM_CONVENTIONAL, want=("steps", "clean", "residual", "map")):
        """CLEAN-SC on the device with the handle's table and active mics (awpu_hip_csm_clean): matrix [n_bins, usable, usable, 2]
        as csm_clean_host takes it -> a dict of the outputs in `want`: "steps" [n_bins, steps] (CSM_CLEAN_STEP_DTYPE), "clean",
        "residual", "map" [n_bins, pixels] and "residual_matrix" [n_bins, usable, usable, 2]."""
        c, cl = csm_of(bins, window, kind), CsmClean(int(steps), float(gain), float(stop_ratio))
        matrix = np.ascontiguousarray(matrix, np.float32)
        usable = self.usable
        if matrix.shape != (max(c.n_bins, 0), usable, usable, 2):
            raise ValueError(f"matrix must be [{max(c.n_bins, 0)}, {usable}, {usable}, 2]")
        out = _csm_clean_outputs(want, max(c.n_bins, 0), max(int(steps), 0), self.pixel_count, usable)
        _check(self._lib.awpu_hip_csm_clean(self._h, _f32(matrix), int(block_count), C.byref(c), C.byref(cl), _out_ptr(out.get("steps")),
                                            *(_out_ptr(out.get(name), _f32p) for name in ("clean", "residual", "map", "residual_matrix"))),
               "awpu_hip_csm_clean")
        return out

    def csm_clean_device(self, d_matrix_ptr: int, block_count: int, bins, steps: int, gain: float = 1.0, stop_ratio: float = 0.0,
                         window: int = TONES_RECT, kind: int = CSM_CONVENTIONAL, d_steps_ptr: int = 0, d_clean_ptr: int = 0, d_residual_ptr: int = 0,
                         d_map_ptr: int = 0, d_residual_matrix_ptr: int = 0, stream: int = 0) -> None:
        """The same on device pointers (each output or 0, not all) on `stream`; asynchronous: the picks, the stop tests and the
        records stay on the device (awpu_hip_csm_clean_device).  d_matrix is not written."""
        c, cl = csm_of(bins, window, kind), CsmClean(int(steps), float(gain), float(stop_ratio))
        _check(self._lib.awpu_hip_csm_clean_device(self._h, C.c_void_p(d_matrix_ptr), int(block_count), C.byref(c), C.byref(cl),
                                                   *_dev(d_steps_ptr, d_clean_ptr, d_residual_ptr, d_map_ptr, d_residual_matrix_ptr, stream)),
               "awpu_hip_csm_clean_device")

    def csm_clean_step_device(self, d_matrix_ptr: int, d_pixel_ptr: int, bins, gain: float = 1.0, window: int = TONES_RECT,
                              kind: int = CSM_CONVENTIONAL, d_component_ptr: int = 0, d_qs_ptr: int = 0, stream: int = 0) -> None:
        """One CLEAN-SC step of d_matrix [n_bins, usable, usable, 2], in place, at the pixels d_pixel [n_bins] int32 holds (outside
        the table: the bin is skipped); d_component [n_bins, usable, 2] and d_qs [n_bins], each or 0; asynchronous
        (awpu_hip_csm_clean_step_device)."""
        c = csm_of(bins, window, kind)
        _check(self._lib.awpu_hip_csm_clean_step_device(self._h, *_dev(d_matrix_ptr, d_pixel_ptr), C.byref(c), float(gain),
                                                        *_dev(d_component_ptr, d_qs_ptr, stream)), "awpu_hip_csm_clean_step_device")

    def range(self, theta, phi, distance, d_frame_ptr: int = 0):
        """The beam power of every direction (theta[k], phi[k]) focused at every candidate distance[j] (metres, inf = a plane wave),
        in one launch on raw samples; d_frame_ptr 0 = the ingest ring's snapshot -> (power [n_src, n_dist], best [n_src]
        RANGE_DTYPE records = range_pick(power)) (awpu_hip_range)."""
        theta = _f64_vector(theta)
        phi = _f64_vector(phi)
        distance = _f64_vector(distance)
        if theta.shape != phi.shape or theta.ndim != 1 or distance.ndim != 1:
            raise ValueError("theta and phi must be 1-D and alike, distance 1-D")
        power = np.empty((theta.size, distance.size), np.float32)
        best = np.zeros(theta.size, RANGE_DTYPE)
        _check(self._lib.awpu_hip_range(self._h, C.c_void_p(d_frame_ptr), theta.ctypes.data_as(_f64p), phi.ctypes.data_as(_f64p), theta.size,
                                        distance.ctypes.data_as(_f64p), distance.size, _f32(power) if power.size else None,
                                        best.ctypes.data_as(C.c_void_p)), "awpu_hip_range")
        return power, best

    def _locate(self, run, *, distance, find, want_power, want_range_power, **shown) -> LocateResult:
        call, where, n_blocks = run
        n_frames, next_first, w = self._shown_frames(n_blocks, **shown)
        f = _find_struct(w.rows, w.cols, find)
        distance = _f64_vector(distance)
        ms = max(f.max_sources, 0)
        sources = np.empty((n_frames, ms), SOURCE_DTYPE)
        count = np.empty(n_frames, np.int32)
        power = np.empty((n_frames, self.pixel_count), np.float32) if want_power else None
        ranges = np.empty((n_frames, ms), RANGE_DTYPE)
        range_power = np.empty((n_frames, ms, distance.size), np.float32) if want_range_power else None
        _check(call(n_blocks, C.byref(w), C.byref(f), _out_ptr(sources), _out_ptr(count), _out_ptr(power, _f32p),
                    distance.ctypes.data_as(_f64p), distance.size, _out_ptr(ranges), _out_ptr(range_power, _f32p)), where)
        return LocateResult(sources, count, power, next_first, ranges, range_power)

    def locate_blocks(self, wire, rows: int, cols: int, distance, first: int = 0, every: int = 1, stride: int = DATAGRAM_BYTES,
                      want_power: bool = False, want_range_power: bool = False, **find) -> LocateResult:
        """find_blocks, and for every source it reports the beam power at that direction focused at every candidate `distance`
        (metres, inf = a plane wave), swept on the block's raw snapshot while it is on the device, and the distance at which it
        peaks (awpu_hip_locate_blocks).  Needs set_antenna.  -> LocateResult."""
        return self._locate(self._wire_run("awpu_hip_locate_blocks", wire, stride), distance=distance, rows=rows, cols=cols, first=first,
                            every=every, find=find, want_power=want_power, want_range_power=want_range_power)

    def locate_samples(self, samples: np.ndarray, rows: int, cols: int, distance, first: int = 0, every: int = 1, want_power: bool = False,
                       want_range_power: bool = False, **find) -> LocateResult:
        """The same from unpacked samples [n_streams, N] (N a multiple of 256, oldest first) (awpu_hip_locate_samples)."""
        return self._locate(self._sample_run("awpu_hip_locate_samples", samples), distance=distance, rows=rows, cols=cols, first=first,
                            every=every, find=find, want_power=want_power, want_range_power=want_range_power)

    def locate_samples_device(self, d_samples_ptr: int, pitch: int, n_blocks: int, rows: int, cols: int, distance, d_sources_ptr: int,
                              d_count_ptr: int, d_ranges_ptr: int, first: int = 0, every: int = 1, d_power_ptr: int = 0,
                              d_range_power_ptr: int = 0, stream: int = 0, **find) -> int:
        """The same on device pointers (as find_samples_device takes them; ranges [n_frames, max_sources] records of 16 bytes,
        range_power [n_frames, max_sources, n_dist] floats or 0) on `stream`; asynchronous.  -> next_first
        (awpu_hip_locate_samples_device)."""
        w = _watch_struct(rows=rows, cols=cols, first=first, every=every)
        distance = _f64_vector(distance)
        return self._device_run("awpu_hip_locate_samples_device", d_samples_ptr, pitch, n_blocks, w, C.byref(_find_struct(rows, cols, find)),
                                *_dev(d_sources_ptr, d_count_ptr, d_power_ptr), distance.ctypes.data_as(_f64p), distance.size,
                                *_dev(d_ranges_ptr, d_range_power_ptr, stream))

    def set_fir_table(self, coeffs: np.ndarray) -> None:
        """The caller's [101, 8] coefficient table of the FIR variant (src/dsp/filter.h:10-112)."""
        coeffs = np.ascontiguousarray(coeffs, np.float32)
        if coeffs.shape != (101, 8):
            raise ValueError("FIR table must be [101, 8]")
        _check(self._lib.awpu_hip_set_fir_table(self._h, _f32(coeffs)), "set_fir_table")

    def process(self, frames: np.ndarray) -> np.ndarray:
        """frames [batch, n_streams, hist] (or one frame [n_streams, hist]) -> power [batch, pixels]."""
        frames = np.ascontiguousarray(frames, np.float32)
        single = frames.ndim == 2
        if single:
            frames = frames[None]
        if frames.shape[1:] != (self.cfg.n_streams, self.cfg.hist):
            raise ValueError(f"frames must be [batch, {self.cfg.n_streams}, {self.cfg.hist}]")
        power = np.empty((frames.shape[0], self.pixel_count), np.float32)
        _check(self._lib.awpu_hip_process(self._h, _f32(frames), frames.shape[0], _f32(power)),
               "awpu_hip_process")
        return power[0] if single else power

    def process_async(self, frames: np.ndarray):
        """awpu_hip_process_async: enqueue upload + sweep + read-back and return; wait() hands out the power.
        The arrays are kept alive (and must not be touched) until wait() returns."""
        frames = np.ascontiguousarray(frames, np.float32)
        if frames.ndim != 3 or frames.shape[1:] != (self.cfg.n_streams, self.cfg.hist):
            raise ValueError(f"frames must be [batch, {self.cfg.n_streams}, {self.cfg.hist}]")
        power = np.empty((frames.shape[0], self.pixel_count), np.float32)
        _check(self._lib.awpu_hip_process_async(self._h, _f32(frames), frames.shape[0], _f32(power)), "awpu_hip_process_async")
        self._pending = (frames, power)

    def wait(self) -> Optional[np.ndarray]:
        _check(self._lib.awpu_hip_wait(self._h), "awpu_hip_wait")
        pending, self._pending = getattr(self, "_pending", None), None
        return pending[1] if pending else None

    def process_device(self, d_frames_ptr: int, batch: int, d_power_ptr: int, stream: int = 0) -> None:
        """Asynchronous sweep on device pointers (e.g. torch tensors' data_ptr()) on `stream`."""
        _check(self._lib.awpu_hip_process_device(self._h, C.c_void_p(d_frames_ptr), batch, *_dev(d_power_ptr, stream)), "awpu_hip_process_device")

    def process_device_sums(self, d_frames_ptr: int, batch: int, d_power_ptr: int, d_sums_ptr: int, stream: int = 0) -> None:
        """process_device plus every pixel's out[0..255] before the epilogue into d_sums [batch, pixels, 256]
        (awpu_hip_process_device_sums: MATH_F32_EXACT only, either interpolation; bit-identical to the reference's out[])."""
        _check(self._lib.awpu_hip_process_device_sums(self._h, C.c_void_p(d_frames_ptr), batch, *_dev(d_power_ptr, d_sums_ptr, stream)),
               "awpu_hip_process_device_sums")

    def packed_bytes(self, batch: int) -> int:
        """Bytes of the packed frame-pair buffer for `batch` frames (awpu_hip_packed_bytes); raises AwpuError with
        status ERR_STATE when this handle's sweep does not take packed frames."""
        n = C.c_uint64(0)
        _check(self._lib.awpu_hip_packed_bytes(self._h, batch, C.byref(n)), "awpu_hip_packed_bytes")
        return int(n.value)

    def pack_frames(self, d_frames_ptr: int, batch: int, d_packed_ptr: int, stream: int = 0) -> None:
        """The sweep's pack pass on its own (the ingest rank of a multi-GPU job): frames -> packed pairs, on `stream`."""
        _check(self._lib.awpu_hip_pack_frames(self._h, C.c_void_p(d_frames_ptr), batch, *_dev(d_packed_ptr, stream)), "awpu_hip_pack_frames")

    def process_packed(self, d_packed_ptr: int, batch: int, d_power_ptr: int, stream: int = 0) -> None:
        """The sweep on packed frame pairs as they arrive from the ingest rank, on `stream`; asynchronous."""
        _check(self._lib.awpu_hip_process_packed(self._h, C.c_void_p(d_packed_ptr), batch, *_dev(d_power_ptr, stream)), "awpu_hip_process_packed")

    def heatmap_device(self, d_power_ptr: int, n: int, batch: int, d_peak_ptr: int, d_pix_ptr: int,
                       peak_given: bool = False, stream: int = 0) -> None:
        """populateHeatmap (src/dsp/mimo.cpp:61-95) on device buffers, asynchronous on `stream`."""
        _check(self._lib.awpu_hip_heatmap_u8_device(self._h, C.c_void_p(d_power_ptr), n, batch,
                                                    C.c_void_p(d_peak_ptr), int(peak_given), C.c_void_p(d_pix_ptr),
                                                    C.c_void_p(stream)), "awpu_hip_heatmap_u8_device")

    def beams(self, off: np.ndarray, frac: np.ndarray, d_frame_ptr: int = 0, want_beams: bool = True):
        """Particle::beam / Particle::das (src/dsp/particle.cpp:51-103) for off/frac [n_dir, lut_stride];
        d_frame_ptr 0 = the ingest ring's snapshot -> (power [n_dir], beams [n_dir, 256] or None)."""
        off = np.ascontiguousarray(off, np.int32)
        frac = np.ascontiguousarray(frac, np.float32)
        if off.ndim != 2 or off.shape[1] != self.cfg.lut_stride or frac.shape != off.shape:
            raise ValueError("off/frac must be [n_dir, lut_stride]")
        n = off.shape[0]
        power = np.empty(n, np.float32)
        out = np.empty((n, 256), np.float32) if want_beams else None
        _check(self._lib.awpu_hip_beams(self._h, C.c_void_p(d_frame_ptr), _i32(off), _f32(frac), n, _f32(power),
                                        _f32(out) if want_beams else None), "awpu_hip_beams")
        return power, out

    def set_antenna(self, xyz: np.ndarray) -> None:
        """The element positions xyz [3, n] (stream ids, n <= lut_stride) the particles steer with (awpu_hip_set_antenna)."""
        xyz = np.ascontiguousarray(xyz, np.float32)
        if xyz.ndim != 2 or xyz.shape[0] != 3:
            raise ValueError("xyz must be [3, n]")
        _check(self._lib.awpu_hip_set_antenna(self._h, _f32(xyz), xyz.shape[1]), "awpu_hip_set_antenna")
        self._antenna_n = xyz.shape[1]

    def steer_table_device(self, theta, phi):
        """steer_table for the handle's antenna, computed on the device -> (off, frac) [n_dir, n]."""
        theta = _f64_vector(theta)
        phi = _f64_vector(phi)
        if theta.shape != phi.shape or theta.ndim != 1:
            raise ValueError("theta and phi must be 1-D and alike")
        # (the row length is the n of the last set_antenna call through this Engine: set the antenna here, not through the
        # C entry point on the same handle)
        n = getattr(self, "_antenna_n", 0)
        if not n:
            raise AwpuError(ERR_STATE, "steer_table_device", "antenna not set (Engine.set_antenna)")
        off = np.empty((theta.size, n), np.int32)
        frac = np.empty((theta.size, n), np.float32)
        dp = C.POINTER(C.c_double)
        _check(self._lib.awpu_hip_steer_table_device(self._h, theta.ctypes.data_as(dp), phi.ctypes.data_as(dp), theta.size,
                                                     _i32(off), _f32(frac)), "awpu_hip_steer_table_device")
        return off, frac

    def track(self, theta, phi, spread, rate, steps, theta_limit: float, reference: Optional[float] = None,
              d_frame_ptr: int = 0, want_beams: bool = False):
        """awpu_hip_track: every particle k advanced by steps[k] gradient steps in one launch.  theta/phi/spread/rate/steps are
        per particle (scalars broadcast); reference None = computed on the device; d_frame_ptr 0 = the ingest ring.
        -> TrackResult: .particles (PARTICLE_DTYPE records after the call), .theta, .phi, .error, .grad_theta,
        .grad_phi, .radius, .power [n, 4], .reference, .beams [n, 256] or None."""
        parts = _particles(theta, phi, spread, rate, steps, "awpu_hip_track")
        n = parts.size
        used = C.c_double(0.0)
        beams = np.empty((n, 256), np.float32) if want_beams else None
        _check(self._lib.awpu_hip_track(self._h, C.c_void_p(d_frame_ptr), parts.ctypes.data_as(C.POINTER(Particle)), n,
                                        float(theta_limit), -1.0 if reference is None else float(reference), C.byref(used),
                                        _f32(beams) if want_beams else None), "awpu_hip_track")
        return TrackResult(parts, float(used.value), beams)

    def live_block(self, wire, rows: int, cols: int, out_rows: int = 0, out_cols: int = 0,
                   d_colormap_ptr: int = 0, want_power: bool = True, out=None):
        """Block in, images out (awpu_hip_live_block): ingest 256 raw datagrams, sweep the new snapshot, 8-bit
        heatmap, optional upscale -> (power or None, image [rows, cols], big image or None).  `wire`: bytes or a
        contiguous uint8 array (a receive buffer that is refilled in place); `out` = (power, image, big) arrays of an
        earlier call to write into again (a display loop keeps its buffers: the library then replays one HIP graph
        per ring position instead of enqueuing the steps one by one)."""
        if len(wire) != 256 * 1032:
            raise ValueError("wire must be 256 datagrams of 1032 bytes")
        if isinstance(wire, np.ndarray):
            if wire.dtype != np.uint8 or not wire.flags.c_contiguous:
                raise ValueError("wire array must be contiguous uint8")
            wire = wire.ctypes.data_as(C.c_void_p)
        if out is not None:
            power, image, big = out
        else:
            power = np.empty(self.cfg.n_pixels, np.float32) if want_power else None
            image = np.empty((rows, cols), np.uint8)
            big = None
            if out_rows:
                big = np.empty((out_rows, out_cols, 3) if d_colormap_ptr else (out_rows, out_cols), np.uint8)
        want_power = power is not None
        _check(self._lib.awpu_hip_live_block(self._h, wire, 1032, _f32(power) if want_power else None, rows, cols,
                                             image.ctypes.data_as(_u8p), out_rows, out_cols, C.c_void_p(d_colormap_ptr),
                                             big.ctypes.data_as(_u8p) if big is not None else None), "awpu_hip_live_block")
        return power, image, big

    def set_mic_gains(self, gains: Optional[np.ndarray]) -> None:
        """Optional per-mic gain (the reference's unused power_correction_mask, aw_processing_unit.cpp:190-200);
        gains [n_streams] by stream id, None = off."""
        if gains is None:
            _check(self._lib.awpu_hip_set_mic_gains(self._h, None), "set_mic_gains")
            return
        gains = np.ascontiguousarray(gains, np.float32)
        if gains.shape != (self.cfg.n_streams,):
            raise ValueError("gains must be [n_streams]")
        _check(self._lib.awpu_hip_set_mic_gains(self._h, _f32(gains)), "set_mic_gains")

    def set_band(self, coeffs: Optional[np.ndarray]) -> None:
        """The handle's band (awpu_hip_set_band): FIR coefficients [taps <= 128] every sweep's input goes through first, e.g.
        band_design(6375, 9000); None = off.  Heatmaps, images and sources follow it; beams, tracking and audio do not."""
        if coeffs is None:
            _check(self._lib.awpu_hip_set_band(self._h, None, 0), "awpu_hip_set_band")
            return
        c = np.ascontiguousarray(coeffs, np.float32).reshape(-1)
        _check(self._lib.awpu_hip_set_band(self._h, _f32(c), c.size), "awpu_hip_set_band")

    def _calibrated(self, call):
        index = np.empty(64, np.int32)
        corr = np.empty(64, np.float32)
        med, n = C.c_float(0), C.c_int32(0)
        call(index, corr, med, n)
        return index[: n.value].copy(), corr[: n.value].copy(), med.value

    def calibrate_device(self, d_frame_ptr: int, array: int = 0, reference_power_level: float = 1e-5, stream: int = 0):
        """AWProcessingUnit::calibrate (aw_processing_unit.cpp:102-212) for one array of a snapshot in
        device memory -> (index, correction, median)."""
        return self._calibrated(lambda i, c, m, n: _check(self._lib.awpu_hip_calibrate_device(
            self._h, C.c_void_p(d_frame_ptr), array, reference_power_level, _i32(i), _f32(c), C.byref(m), C.byref(n),
            C.c_void_p(stream)), "awpu_hip_calibrate_device"))

    def calibrate_host(self, frame: np.ndarray, array: int = 0, reference_power_level: float = 1e-5):
        """The same for a snapshot [n_streams, hist] in host memory."""
        frame = np.ascontiguousarray(frame, np.float32)
        if frame.shape != (self.cfg.n_streams, self.cfg.hist):
            raise ValueError("frame must be [n_streams, hist]")
        return self._calibrated(lambda i, c, m, n: _check(self._lib.awpu_hip_calibrate_host(
            self._h, _f32(frame), array, reference_power_level, _i32(i), _f32(c), C.byref(m), C.byref(n)),
            "awpu_hip_calibrate_host"))

    def last_error(self) -> str:
        return self._lib.awpu_hip_last_error_of(self._h).decode()

    def calibrate_ring(self, array: int = 0, reference_power_level: float = 1e-5):
        """The same on the current snapshot of the ingest ring."""
        return self._calibrated(lambda i, c, m, n: _check(self._lib.awpu_hip_calibrate_ring(
            self._h, array, reference_power_level, _i32(i), _f32(c), C.byref(m), C.byref(n)), "awpu_hip_calibrate_ring"))

    def upscale_device(self, d_pix_ptr: int, rows: int, cols: int, batch: int, d_out_ptr: int, out_rows: int,
                       out_cols: int, d_colormap_ptr: int = 0, stream: int = 0) -> None:
        """The display upscale (aw_processing_unit.cpp:252), optionally through a 256x3 colour table
        (main.cpp:345), on device buffers; asynchronous on `stream`."""
        _check(self._lib.awpu_hip_upscale_u8_device(self._h, C.c_void_p(d_pix_ptr), rows, cols, batch,
                                                    C.c_void_p(d_colormap_ptr), C.c_void_p(d_out_ptr), out_rows,
                                                    out_cols, C.c_void_p(stream)), "awpu_hip_upscale_u8_device")

    def synchronize(self) -> None:
        _check(self._lib.awpu_hip_synchronize(self._h), "awpu_hip_synchronize")

    def peer_status(self) -> list:
        """Per device of the group: PEER_SAME_DEVICE / PEER_DIRECT / PEER_HOST_STAGED (awpu_hip_group_peer_status)."""
        buf = (C.c_int32 * 8)()
        n = self._lib.awpu_hip_group_peer_status(self._h, buf, 8)
        if n < 0:
            _check(n, "group_peer_status")
        return [int(buf[k]) for k in range(n)]

    def stats(self) -> Stats:
        st = Stats()
        _check(self._lib.awpu_hip_get_stats(self._h, C.byref(st)), "get_stats")
        return st
