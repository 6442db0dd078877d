"""What the host rules and Engine's methods hand back: one plain class per kind of result, fields named as the records' dtypes
name them.  Imports from abi only (the dtypes).
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from .abi import PARTICLE_DTYPE, SOURCE_DTYPE


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


class PeelRunResult:
    """What Engine.peel_blocks / peel_samples hand back: .image, .big, .power as a WatchResult has them -- of the map (or, by
    `show`, the clean or the residual) rows --, .steps [n_frames, steps] PEEL_STEP_DTYPE records, .sources and .count as a
    FindResult has them (None without `find`), .next_first for the call that continues the run."""

    def __init__(self, image, big, power, steps, sources, count, next_first: int):
        self.image, self.big, self.power, self.steps, self.sources, self.count, self.next_first = image, big, power, steps, sources, count, next_first

    def __len__(self):
        return len(self.steps)


class CohereResult:
    """What Engine.cohere_blocks / cohere_samples hand back: .image, .big, .power as a WatchResult has them -- of the weighted
    (or, with show=COHERE_FACTOR, the coherence) rows --, .sources and .count as a FindResult has them (None without `find`),
    .next_first for the call that continues the run."""

    def __init__(self, image, big, power, sources, count, next_first: int):
        self.image, self.big, self.power, self.sources, self.count, self.next_first = image, big, power, sources, count, next_first

    def __len__(self):
        return len(next(a for a in (self.image, self.big, self.power, self.count) if a is not None))


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
