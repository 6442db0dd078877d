#!/usr/bin/env python3
"""What the cross-spectral maps cost (include/awpu_hip_csm.h): Engine.csm_map_device for 1 bin and for 8 bins, and
Engine.csm_samples_device for 8 bins, on device-resident buffers, at c1 (64 mics, 32 x 32), the reference's default (64 mics,
100 x 100) and the headline shape (256 mics, 128 x 128); --repeats launches of each, every launch timed by HIP events on the
stream it runs on.  One JSON line per shape: the median launch of each, maps per second, complex multiply-adds per second of the
quadratic form (pixels x bins x usable (usable - 1) / 2 a map) and accumulated blocks per second.  And the loaded inverse
(step 6a): Engine.csm_invert_device of the 8-bin matrix, timed the same way, beside awpu_hip_csm_invert_host on the host (wall
clock); and one Capon frame of --blocks blocks two ways, wall clock from an idle device to an idle device: everything enqueued on
one stream (accumulate, csm_invert_device, map: capon_device_ms) against the composition the device inverse replaces (accumulate,
the matrix to the host, csm_invert_host, the inverse back up, map: capon_host_inverse_ms).  And the Capon run
(Engine.csm_watch_samples_device, include/awpu_hip_csm_watch.h): 8 frames of length --blocks, one every --blocks blocks, in one call
-- run_frames_per_s -- beside composition_frames_per_s, the frames a second of capon_host_inverse, and the same frames through the
CLEAN-SC run (Engine.csm_clean_samples_device, 4 steps): clean_run_frames_per_s.

  tools/csm_rate.py --repeats 20

Measured on one MI355X (--repeats 20, 64 blocks, 8 bins; c1 / the reference's shape / the headline shape): invert_8 0.119 / 0.119 /
2.00 ms beside map_8 0.035 / 0.072 / 2.45 ms and invert_host_8 0.88 / 0.88 / 91.6 ms -- at 64 mics the inverse costs more than the
map it feeds (a chain of 64 dependent steps on 8 workgroups), at 256 less; one Capon frame 0.21 / 0.25 / 4.6 ms on the device against
1.05 / 1.08 / 93.5 ms through the host inverse; the Capon run 4 950 / 4 090 / 218 frames/s against 957 / 926 / 10.7 for the
composition.  And CLEAN-SC (step 7, include/awpu_hip_csm_clean.h): Engine.csm_clean_device at 4 steps, 1 bin and 8 bins
(clean_1, clean_8), beside the five maps the loop contains (clean_N_over_maps = clean_N / (5 map_N); clean_N_between_maps_ms = what
is left per step for the two launches between two maps), and Engine.csm_clean_step_device by itself (load, component, update).
Measured (--repeats 20; c1 / the reference's shape / the headline shape): clean_8 0.198 / 0.400 / 12.26 ms beside map_8 0.034 / 0.072 /
2.43 ms (1.18 / 1.12 / 1.01 x its five maps), clean_1 0.192 / 0.204 / 1.69 ms beside map_1 0.033 / 0.032 / 0.306 ms (1.16 / 1.29 / 1.11 x).
And the eigendecomposition (step 8, include/awpu_hip_csm_eig.h): Engine.csm_eig_device of the 8-bin matrix (eig_8) and one MUSIC and
one functional map of it (Engine.csm_eig_map_device: music_8, functional_8 with root 4), timed by events as the maps are, beside
numpy.linalg.eigh of the same eight matrices in complex128 on the host (eigh_host_8, wall clock).
Measured (--repeats 20, 8 bins; c1 / the reference's shape / the headline shape): eig_8 3.20 / 3.13 / 193.3 ms, music_8 3.25 / 3.22 /
196.0 ms, functional_8 3.28 / 3.22 / 196.2 ms beside eigh_host_8 2.52 / 2.51 / 77.4 ms -- the maps are the eigensolver plus 0.05 to 3 ms,
and the solver, eight workgroups of one compute unit each walking about 700 (64 mics) or 3 300 (256 mics) rounds of three barriers, is
slower than LAPACK on the host's cores at both sizes; what it buys is a result on the stream, with the host rule's bits.
No figure here is a gate."""
import argparse
import importlib
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
pkg = importlib.import_module("beamforming-lk_amd")


LOADING = 1e-2
CLEAN_STEPS = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="c1,ref_default,headline")
    ap.add_argument("--blocks", type=int, default=64, help="blocks per accumulate call")
    a = ap.parse_args()
    import torch  # (after the package: one HIP runtime)

    S = pkg.synthetic
    side = torch.cuda.Stream()  # (a stream of its own: 0 would mean the handle's, which torch's events do not see)
    for shape in a.shapes.split(","):
        spec = S.WORKLOADS[shape]
        xyz = S.geometry(spec)
        off, frac = S.delay_table(spec, xyz)
        U, P = spec.n_mics, spec.n_pixels
        samples = (torch.randn(U, 256 * a.blocks, device="cuda") * 1e-2).contiguous()
        matrix = torch.zeros(8, U, U, 2, device="cuda")
        plane = torch.empty(8, P, device="cuda")
        inverse = torch.empty_like(matrix)
        eig_values = torch.empty(8, U, device="cuda")
        frame = torch.zeros_like(matrix)
        pixels = torch.full((8,), P // 2 + spec.res // 2, dtype=torch.int32, device="cuda")
        with pkg.Engine(n_pixels=P, n_streams=U, grid_columns=spec.res, max_batch=8) as eng:
            eng.set_delay_table(off, frac)
            eng.set_active_mics(None)
            bins8, bins1 = [8, 16, 24, 32, 40, 48, 56, 64], [16]
            calls = {"accumulate_8": lambda: eng.csm_samples_device(samples.data_ptr(), samples.shape[1], a.blocks, bins8, matrix.data_ptr(),
                                                                    window=1, stream=side.cuda_stream),
                     "map_1": lambda: eng.csm_map_device(matrix.data_ptr(), a.blocks, bins1, 1, d_map_ptr=plane.data_ptr(), stream=side.cuda_stream),
                     "map_8": lambda: eng.csm_map_device(matrix.data_ptr(), a.blocks, bins8, 1, d_map_ptr=plane.data_ptr(), stream=side.cuda_stream)}
            calls["invert_8"] = lambda: eng.csm_invert_device(matrix.data_ptr(), a.blocks, bins8, inverse.data_ptr(), LOADING, stream=side.cuda_stream)
            # the eigendecomposition (step 8) of the 8-bin matrix, and one MUSIC and one functional map of it
            calls["eig_8"] = lambda: eng.csm_eig_device(matrix.data_ptr(), a.blocks, bins8, eig_values.data_ptr(), inverse.data_ptr(),
                                                        stream=side.cuda_stream)
            calls["music_8"] = lambda: eng.csm_eig_map_device(matrix.data_ptr(), a.blocks, bins8, plane.data_ptr(), pkg.binding.CSM_EIG_MUSIC, 2, 0, 1,
                                                              stream=side.cuda_stream)
            calls["functional_8"] = lambda: eng.csm_eig_map_device(matrix.data_ptr(), a.blocks, bins8, plane.data_ptr(), pkg.binding.CSM_EIG_FUNCTIONAL,
                                                                   0, 4, 1, stream=side.cuda_stream)
            # CLEAN-SC (step 7): the loop of CLEAN_STEPS steps -- CLEAN_STEPS + 1 maps and what runs between them --, and one step by itself
            # on a copy of the matrix (it updates in place)
            for n_bins, bins in ((1, bins1), (8, bins8)):
                calls[f"clean_{n_bins}"] = lambda bins=bins: eng.csm_clean_device(matrix.data_ptr(), a.blocks, bins, CLEAN_STEPS, window=1,
                                                                                  d_map_ptr=plane.data_ptr(), stream=side.cuda_stream)
                calls[f"clean_step_{n_bins}"] = lambda bins=bins: eng.csm_clean_step_device(frame.data_ptr(), pixels.data_ptr(), bins, window=1,
                                                                                            stream=side.cuda_stream)
            times = {name: [] for name in calls}
            for step in range(a.warmup + a.repeats):
                for name, call in calls.items():
                    if name.startswith("clean_step"):
                        frame.copy_(matrix)
                        torch.cuda.synchronize()
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record(side)
                    call()
                    t1.record(side)
                    torch.cuda.synchronize()
                    if step >= a.warmup:
                        times[name].append(t0.elapsed_time(t1))

            def capon_device():
                with torch.cuda.stream(side):
                    frame.zero_()
                eng.csm_samples_device(samples.data_ptr(), samples.shape[1], a.blocks, bins8, frame.data_ptr(), window=1, stream=side.cuda_stream)
                eng.csm_invert_device(frame.data_ptr(), a.blocks, bins8, inverse.data_ptr(), LOADING, stream=side.cuda_stream)
                eng.csm_map_device(inverse.data_ptr(), a.blocks, bins8, 1, pkg.binding.CSM_CAPON, d_map_ptr=plane.data_ptr(), stream=side.cuda_stream)

            def capon_host_inverse():
                with torch.cuda.stream(side):
                    frame.zero_()
                    eng.csm_samples_device(samples.data_ptr(), samples.shape[1], a.blocks, bins8, frame.data_ptr(), window=1, stream=side.cuda_stream)
                    host_matrix = frame.cpu().numpy()  # (waits for the stream)
                    host_inverse = pkg.csm_invert_host(host_matrix, a.blocks, bins8, loading=LOADING)
                    inverse.copy_(torch.from_numpy(host_inverse), non_blocking=True)
                eng.csm_map_device(inverse.data_ptr(), a.blocks, bins8, 1, pkg.binding.CSM_CAPON, d_map_ptr=plane.data_ptr(), stream=side.cuda_stream)

            run_frames = 8
            run_samples = (torch.randn(U, 256 * a.blocks * run_frames, device="cuda") * 1e-2).contiguous()
            run_carry = torch.zeros(max(a.blocks - 1, 1), 8, U, 2, device="cuda")
            run_power = torch.empty(run_frames, P, device="cuda")

            def capon_run():
                eng.csm_watch_samples_device(run_samples.data_ptr(), run_samples.shape[1], a.blocks * run_frames, spec.res, spec.res, bins8, 1,
                                             pkg.binding.CSM_CAPON, LOADING, a.blocks, pkg.binding.CSM_SHOW_SUM, a.blocks - 1, a.blocks,
                                             d_carry_ptr=run_carry.data_ptr(), carried=0, d_power_ptr=run_power.data_ptr(), stream=side.cuda_stream)

            def clean_run():  # the same frames through the CLEAN-SC run (Engine.csm_clean_samples_device, CLEAN_STEPS steps): clean_run_frames_per_s
                eng.csm_clean_samples_device(run_samples.data_ptr(), run_samples.shape[1], a.blocks * run_frames, spec.res, spec.res, bins8, CLEAN_STEPS,
                                             1.0, 0.0, pkg.binding.CSM_CLEAN_CLEAN, 1, a.blocks, pkg.binding.CSM_SHOW_SUM, a.blocks - 1, a.blocks,
                                             d_carry_ptr=run_carry.data_ptr(), carried=0, d_power_ptr=run_power.data_ptr(), stream=side.cuda_stream)

            host_matrix = matrix.cpu().numpy()
            host_complex = (host_matrix[..., 0] + 1j * host_matrix[..., 1]).astype(np.complex128) / a.blocks
            walls = {"eigh_host_8": lambda: np.linalg.eigh(host_complex), "capon_run": capon_run, "clean_run": clean_run, "invert_host_8": lambda: pkg.csm_invert_host(host_matrix, a.blocks, bins8, loading=LOADING), "capon_device": capon_device,
                     "capon_host_inverse": capon_host_inverse}
            for name, call in walls.items():
                times[name] = []
                for step in range(a.warmup + a.repeats):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    call()
                    torch.cuda.synchronize()
                    if step >= a.warmup:
                        times[name].append((time.perf_counter() - t0) * 1e3)
            row = {"shape": shape, "mics": U, "grid": f"{spec.res}x{spec.res}", "repeats": a.repeats, "blocks": a.blocks,
                   "device": torch.cuda.get_device_name(0)}
            for name, v in times.items():
                med = statistics.median(v)
                row[f"{name}_ms"] = round(med, 4)
                row[f"{name}_spread"] = round((max(v) - min(v)) / med, 4)
            for n_bins in (1, 8):
                med = statistics.median(times[f"map_{n_bins}"])
                row[f"map_{n_bins}_per_s"] = round(1e3 / med, 1)
                row[f"map_{n_bins}_gcmadd_per_s"] = round(P * n_bins * U * (U - 1) / 2 / med * 1e-6, 2)
            for n_bins in (1, 8):  # the loop beside the maps it contains, and what is left for the launches between them
                loop, maps = statistics.median(times[f"clean_{n_bins}"]), (CLEAN_STEPS + 1) * statistics.median(times[f"map_{n_bins}"])
                row[f"clean_{n_bins}_over_maps"] = round(loop / maps, 3)
                row[f"clean_{n_bins}_between_maps_ms"] = round((loop - maps) / CLEAN_STEPS, 4)
            row["run_frames_per_s"] = round(run_frames / statistics.median(times["capon_run"]) * 1e3, 1)
            row["clean_run_frames_per_s"] = round(run_frames / statistics.median(times["clean_run"]) * 1e3, 1)
            row["composition_frames_per_s"] = round(1e3 / statistics.median(times["capon_host_inverse"]), 1)
            row["blocks_per_s"] = round(a.blocks / statistics.median(times["accumulate_8"]) * 1e3, 1)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
