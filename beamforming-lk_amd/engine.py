"""Engine: one awpu_hip handle and every call that takes it, one class in one file.  Imports from abi, results and rules; all it
uses is bound in this module's own globals, so no call looks a helper up through another module.
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import Optional

import numpy as np

from .abi import *  # noqa: F401,F403  (the constants, structures and dtypes), and the helpers by name:
from .abi import (_check, _dev, _f32, _f32p, _f64_vector, _f64p, _find_struct, _i32, _i32p, _out_ptr, _ref, _u8p, _watch_struct,
                  _wire_blocks)
from .results import *  # noqa: F401,F403
from .rules import *  # noqa: F401,F403
from .rules import _csm_clean_outputs, _csm_square, _particles


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
