"""The C ABI of libawpu_hip.so (include/awpu_hip*.h) as ctypes: constants, structures, one signature table per header, the record
dtypes, load() / loaded_library() and the helpers that turn Python values into a call's arguments.  The loaded library (_lib) is
owned here alone.  Imports nothing of the package but _build.
"""
from __future__ import annotations

import contextlib
import ctypes as C
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
