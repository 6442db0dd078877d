"""Geometry and the headers' rules as executable C on the host: functions that call exported entry points and need no handle,
and the parsers of the tools' text arguments.  Imports from abi and results only.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from .abi import *  # noqa: F401,F403  (the constants and structures), and the helpers by name:
from .abi import _check, _f32, _f32p, _f64_vector, _f64p, _i32, _i32p, _out_ptr, _u8p
from .results import FindResult, PeelResult

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


def watch_count(n_blocks: int, first: int, every: int):
    """(frames a call of n_blocks blocks shows, the `first` of the call that continues it) (awpu_hip_watch_count)."""
    n, nxt = C.c_int32(0), C.c_int32(0)
    _check(load().awpu_hip_watch_count(n_blocks, first, every, C.byref(n), C.byref(nxt)), "awpu_hip_watch_count")
    return int(n.value), int(nxt.value)


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
