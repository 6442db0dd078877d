"""beamforming-lk_amd -- MI355X (gfx950) delay-and-sum heatmap engine behind the
aw_processing_unit API of acoustic-warfare/beamforming-lk.

The product is the C-ABI library libawpu_hip.so (include/awpu_hip.h, sources in csrc/)
and the C++ host mirror of the reference's MIMO worker (host/).  This Python package is
plumbing: it builds and loads the library (ctypes) for the tests and bench.py.

The directory name has a hyphen; import it with
    importlib.import_module("beamforming-lk_amd")
"""
from . import _build, binding, synthetic  # noqa: F401
from .binding import (  # noqa: F401
    MATH_BF16_ACC,
    MATH_F32_EXACT,
    MATH_F32_FAST,
    AwpuError,
    Engine,
    band_design,
    band_filter,
    build_delay_table,
    build_delay_table_device,
    build_focus_table,
    build_focus_table_device,
    cohere_host,
    create_antenna,
    create_tiled_antenna,
    csm_accumulate_host,
    csm_clean_host,
    csm_clean_step_host,
    csm_eig_host,
    csm_eig_map_host,
    csm_eig_weigh_host,
    csm_invert_host,
    csm_invert_rule_host,
    csm_map_host,
    csm_spectra_host,
    csm_steer_host,
    expose_count,
    expose_rows,
    find_peaks,
    focus_delays,
    focus_steer_table,
    heatmap_u8,
    peel_beam_length,
    peel_host,
    peel_sources,
    peel_step_host,
    range_candidates,
    range_pick,
    resize_linear_u8,
    steer_table,
    steering_delays,
    tones_host,
    tones_linear,
    tones_of,
    tones_twiddles,
    tones_window,
)

__all__ = [
    "Engine", "AwpuError", "MATH_F32_EXACT", "MATH_F32_FAST", "MATH_BF16_ACC", "build_delay_table", "build_delay_table_device",
    "create_antenna", "create_tiled_antenna", "steering_delays", "heatmap_u8", "find_peaks", "expose_count", "expose_rows", "cohere_host", "peel_host", "peel_step_host", "peel_beam_length", "peel_sources", "band_design", "band_filter", "resize_linear_u8", "steer_table", "focus_delays", "focus_steer_table",
    "build_focus_table", "build_focus_table_device", "range_pick", "range_candidates", "tones_host", "tones_linear", "tones_of", "tones_twiddles",
    "tones_window", "csm_spectra_host", "csm_accumulate_host", "csm_steer_host", "csm_map_host", "csm_invert_host", "csm_invert_rule_host", "csm_clean_host", "csm_clean_step_host", "csm_eig_host",
    "csm_eig_weigh_host", "csm_eig_map_host", "binding",
    "synthetic", "_build",
]
