"""CLEAN-SC in runs of blocks (awpu_hip_csm_clean_blocks / _samples / _samples_device; include/awpu_hip_csm_clean.h).

1. Every shown frame equals, bit for bit, csm_accumulate_host over its window from zeros -> csm_clean_host -> the shown row ->
   heatmap_u8 / find_peaks: `what` map, clean and residual, one bin shown and the sum, length 1 and 5 with overlapping windows
   (every 2), max_batch 2 (several pieces), planes and steps included.  12 blocks, 64 mics, an 8 x 8 grid.  And 300 blocks (more
   than one chunk of 256 new blocks), 2 of 8 mics, a 4 x 4 grid.
2. A recording split over three calls gives one call's bits.
3. The three forms agree -- the device form between guards --, and the ring after each is the ring after watch_blocks.
4. Refusals: a bad cl, a bad `what`, kinds 1 and 2; a slab handle.
5. tools/pcap_video.py and tools/pcap_sources.py with --csm-clean on a capture, in chunks: one csm_clean_blocks call's frames and steps.
6. A run at 545 of 640 mics and the refusal at 2049: test_gpu_csm_large.py, with this file's check_run."""
import numpy as np
import pytest

import csm_util as CU
from test_gpu_blocks import engine
from test_gpu_csm_runs import Rig, same_where_not_nan, shown_sum
from test_gpu_find import c1 as find_c1  # noqa: F401  (c1's 23-block recording)

pytestmark = pytest.mark.gpu

RES = 8
BLOCKS = 12
BINS = [3, 16, 47]
FIND = dict(radius=2, max_sources=4, min_ratio=0.1)
STEPS, GAIN, STOP = 3, 0.75, 0.05
ROWS = ("map", "clean", "residual")  # by `what`


@pytest.fixture(scope="module")
def rig(pkg, oracle):
    return Rig(pkg, oracle, 64, list(range(64)), False, 41, n_blocks=BLOCKS, res=RES)


_frames = {}


def composition(pkg, rig, first, every, length, what, show, lo_block=0):
    """The frames shown at first, first + every, ...: planes, steps and the shown rows, by the host functions alone."""
    planes, steps = [], []
    for t in range(first, BLOCKS, every):
        key = (t, length)
        if key not in _frames:
            lo = max(t - length + 1, lo_block)
            Cm, n = pkg.csm_accumulate_host(np.ascontiguousarray(rig.samples[:, 256 * lo: 256 * (t + 1)]), BINS, 1)
            with np.errstate(all="ignore"):
                _frames[key] = pkg.csm_clean_host(Cm, n, rig.off, rig.frac, BINS, STEPS, GAIN, STOP, 1)
        planes.append(_frames[key][ROWS[what]])
        steps.append(_frames[key]["steps"])
    planes = np.stack(planes)
    rows = planes[:, show] if show >= 0 else shown_sum(planes)
    return dict(planes=planes, steps=np.stack(steps), power=np.ascontiguousarray(rows))


def check_run(pkg, got, want, where, res=RES, rows=None):
    rows = res if rows is None else rows  # (test_gpu_csm_large.py's grid is not square)
    same_where_not_nan(got.planes, want["planes"], (where, "planes"))
    same_where_not_nan(got.power, want["power"], (where, "power"))
    assert np.array_equal(got.steps["pixel"], want["steps"]["pixel"]), (where, "picks")
    same_where_not_nan(got.steps["before"], want["steps"]["before"], (where, "before"))
    same_where_not_nan(got.steps["removed"], want["steps"]["removed"], (where, "removed"))
    assert not np.isnan(want["power"]).any(), where
    image = np.stack([pkg.heatmap_u8(p) for p in want["power"]]).reshape(-1, rows, res)
    assert np.array_equal(got.image, image), (where, "image")
    found = pkg.find_peaks(want["power"], rows, res, **FIND)
    assert np.array_equal(got.count, found.count), (where, "count")
    assert np.array_equal(got.sources["pixel"], found.sources["pixel"]), (where, "sources")
    assert CU.same_bits(got.sources["power"], found.sources["power"]), (where, "source powers")


KW = dict(window=1, want_power=True, want_planes=True, find=FIND)


def test_runs_equal_the_composition(pkg, rig):
    B = pkg.binding
    with rig.engine(max_batch=2) as eng:
        for length in (1, 5):
            for what in (B.CSM_CLEAN_MAP, B.CSM_CLEAN_CLEAN, B.CSM_CLEAN_RESIDUAL):
                for show in (1, B.CSM_SHOW_SUM):
                    where = (length, what, show)
                    want = composition(pkg, rig, 1, 2, length, what, show)
                    got = eng.csm_clean_samples(rig.samples, RES, RES, BINS, STEPS, GAIN, STOP, what, length=length, show=show, first=1, every=2, **KW)
                    check_run(pkg, got, want, where)
                    assert got.carried == min(BLOCKS, length - 1) and got.next_first == B.watch_count(BLOCKS, 1, 2)[1]
        assert (want["steps"]["pixel"][:, :, 0] >= 0).all() and len(want["power"]) == 6  # (max_batch 2: three pieces)


def test_more_blocks_than_a_chunk(pkg, oracle):
    """300 blocks, 2 of 8 mics, a 4 x 4 grid, max_batch 2, length 3, 2 steps: frames at 99, 199, 299 (a full piece ends the first
    chunk behind block 199; the step records come back piece by piece) and at 127, 256 (the second chunk of new blocks starts at
    block 256, inside the second frame's window)."""
    B = pkg.binding
    rig = Rig(pkg, oracle, 8, [5, 2], False, 33, n_blocks=300, res=4)
    length, steps, bins, what = 3, 2, [16], B.CSM_CLEAN_CLEAN
    with rig.engine(max_batch=2) as eng:
        for first, every in ((99, 100), (127, 129)):
            frames = []
            for t in range(first, 300, every):
                Cm, n = pkg.csm_accumulate_host(np.ascontiguousarray(rig.samples[:, 256 * (t - length + 1): 256 * (t + 1)]), bins, 0, index=rig.index)
                assert n == length
                frames.append(pkg.csm_clean_host(Cm, n, rig.off, rig.frac, bins, steps, GAIN, STOP, 0, index=rig.index))
            planes = np.stack([fr[ROWS[what]] for fr in frames])
            want = dict(planes=planes, steps=np.stack([fr["steps"] for fr in frames]), power=np.ascontiguousarray(shown_sum(planes)))
            got = eng.csm_clean_samples(rig.samples, 4, 4, bins, steps, GAIN, STOP, what, length=length, show=B.CSM_SHOW_SUM, first=first, every=every,
                                        **dict(KW, window=0))
            check_run(pkg, got, want, (first, every), res=4)
            assert (want["steps"]["pixel"][:, :, 0] >= 0).all() and got.carried == length - 1


def test_a_split_recording_gives_one_calls_bits(pkg, rig):
    B = pkg.binding
    length, first, every, show, what = 5, 1, 2, -1, B.CSM_CLEAN_MAP
    with rig.engine() as eng:
        whole = eng.csm_clean_samples(rig.samples, RES, RES, BINS, STEPS, GAIN, STOP, what, length=length, show=show, first=first, every=every, **KW)
    check_run(pkg, whole, composition(pkg, rig, first, every, length, what, show), "whole")
    with rig.engine() as eng:
        parts, carry, carried, nxt, lo = [], None, 0, first, 0
        for hi in (3, 8, BLOCKS):  # every cut lies inside the windows of the frames behind it
            x = np.ascontiguousarray(rig.samples[:, 256 * lo: 256 * hi])
            r = eng.csm_clean_samples(x, RES, RES, BINS, STEPS, GAIN, STOP, what, length=length, show=show, first=nxt, every=every, carry=carry,
                                      carried=carried, **KW)
            parts.append(r)
            carry, carried, nxt, lo = r.carry, r.carried, r.next_first, hi
    assert nxt == whole.next_first and carried == whole.carried and CU.same_bits(carry, whole.carry)
    for field in ("power", "planes", "steps", "image", "count", "sources"):
        joined = np.concatenate([getattr(r, field) for r in parts])
        assert joined.tobytes() == getattr(whole, field).tobytes(), field


def test_the_three_forms_agree_and_leave_the_watch_runs_ring(pkg, rig):
    import torch

    B = pkg.binding
    length, first, every, show, what = 5, 1, 2, 1, B.CSM_CLEAN_CLEAN
    n_frames = len(range(first, BLOCKS, every))
    want = composition(pkg, rig, first, every, length, what, show)
    with rig.engine() as ref:
        ref.watch_blocks(rig.wire, RES, RES, first=first, every=every)
        ring = ref.ring_snapshot()
    kw = dict(KW, length=length, show=show, first=first, every=every)
    with rig.engine() as eng:
        check_run(pkg, eng.csm_clean_blocks(rig.wire, RES, RES, BINS, STEPS, GAIN, STOP, what, **kw), want, "blocks")
        assert np.array_equal(eng.ring_snapshot(), ring)
    with rig.engine() as eng:
        check_run(pkg, eng.csm_clean_samples(rig.samples, RES, RES, BINS, STEPS, GAIN, STOP, what, **kw), want, "samples")
        assert np.array_equal(eng.ring_snapshot(), ring)
    with rig.engine() as eng:  # the device form, every output between guards
        K, P, U = len(BINS), rig.P, 64
        outs = {"image": (n_frames * P, torch.uint8), "power": (n_frames * P, torch.float32), "sources": (n_frames * 4 * 40, torch.uint8),
                "count": (n_frames, torch.int32), "planes": (n_frames * K * P, torch.float32), "steps": (n_frames * K * STEPS * 3, torch.float32),
                "carry": ((length - 1) * K * U * 2, torch.float32)}
        fill = {torch.uint8: 0xA5, torch.float32: -3.0, torch.int32: -7}
        raw = {k: torch.full((n + 128,), fill[t], dtype=t, device="cuda") for k, (n, t) in outs.items()}
        ptr = {k: v.data_ptr() + 64 * v.element_size() for k, v in raw.items()}
        d_x = torch.from_numpy(rig.samples).cuda()
        torch.cuda.synchronize()
        nxt, carried = eng.csm_clean_samples_device(d_x.data_ptr(), rig.samples.shape[1], BLOCKS, RES, RES, BINS, STEPS, GAIN, STOP, what, 1, length, show,
                                                    first, every, d_carry_ptr=ptr["carry"], carried=0, d_image_ptr=ptr["image"],
                                                    d_power_ptr=ptr["power"], d_sources_ptr=ptr["sources"], d_count_ptr=ptr["count"],
                                                    d_planes_ptr=ptr["planes"], d_steps_ptr=ptr["steps"], find=FIND)
        eng.synchronize()
        host = {k: v.cpu().numpy() for k, v in raw.items()}
        for k, v in host.items():
            assert (v[:64] == fill[outs[k][1]]).all() and (v[-64:] == fill[outs[k][1]]).all(), k
        got = B.CsmCleanRunResult(host["image"][64:-64].reshape(n_frames, RES, RES), None, host["power"][64:-64].reshape(n_frames, P),
                                  host["sources"][64:-64].view(B.SOURCE_DTYPE).reshape(n_frames, 4), host["count"][64:-64],
                                  host["planes"][64:-64].reshape(n_frames, K, P),
                                  np.ascontiguousarray(host["steps"][64:-64]).view(B.CSM_CLEAN_STEP_DTYPE).reshape(n_frames, K, STEPS), nxt,
                                  host["carry"][64:-64].reshape(length - 1, K, U, 2), carried)
        check_run(pkg, got, want, "device")
        assert carried == length - 1 and nxt == B.watch_count(BLOCKS, first, every)[1]
        assert np.array_equal(eng.ring_snapshot(), ring)
        assert CU.same_bits(got.carry, pkg.csm_spectra_host(rig.samples, BINS, 1)[BLOCKS - (length - 1):])
    # the steps as sources, as the tools list them: merged per pixel over steps and bins
    sources, count = B.csm_clean_source_records(want["steps"], RES, RES, 4)
    assert sources.shape == (n_frames, 4) and (count >= 1).all() and (sources["pixel"][:, 0] >= 0).all()


def test_runs_refuse(pkg, rig):
    B = pkg.binding

    def status(eng, steps=STEPS, gain=GAIN, stop=STOP, what=0, kind=CU.CONVENTIONAL, **kw):
        try:
            if kind != CU.CONVENTIONAL:
                import ctypes as C

                w, c, cl = B.Watch(0, 1, RES, RES, 0, 0, 0, None), B.csm_of(BINS, 1, kind, 0.05), B.CsmClean(steps, gain, stop)
                held, power = C.c_int32(0), np.zeros((BLOCKS, rig.P), np.float32)
                return eng._lib.awpu_hip_csm_clean_samples(eng._h, B._f32(rig.samples), rig.samples.shape[1], BLOCKS, C.byref(w), C.byref(c), 1, -1, None,
                                                           None, C.cast(C.byref(held), B._i32p), C.byref(cl), what, None, None, B._f32(power), None, None,
                                                           None, None)
            eng.csm_clean_samples(rig.samples, RES, RES, BINS, steps, gain, stop, what, window=1, length=1, **kw)
            return B.OK
        except pkg.AwpuError as e:
            return e.status

    with rig.engine() as eng:
        assert status(eng) == B.OK
        before = eng.ring_snapshot()
        for bad in (dict(steps=0), dict(steps=33), dict(gain=0.0), dict(gain=1.5), dict(stop=1.0), dict(stop=-0.1), dict(what=3), dict(what=-1),
                    dict(kind=CU.DIAGONAL_REMOVED), dict(kind=CU.CAPON), dict(show=3), dict(every=0)):
            assert status(eng, **bad) == B.ERR_INVALID, bad
        assert np.array_equal(eng.ring_snapshot(), before)  # a refused run leaves the ring as it was
    with pkg.Engine(n_pixels=rig.P, n_streams=rig.S, grid_columns=RES, pixel_begin=0, pixel_count=32) as eng:  # a slab handle: the pick needs the whole map
        eng.set_delay_table(rig.off[:32], rig.frac[:32])
        eng.set_active_mics(rig.index)
        assert status(eng) == B.ERR_STATE
    with rig.engine(interp=B.INTERP_FIR8) as eng:
        assert status(eng) == B.ERR_STATE


def test_the_tools_show_and_search_clean_maps(pkg, find_c1, tmp_path):  # noqa: F811
    """tools/pcap_video.py --csm .. --csm-clean and tools/pcap_sources.py with the same flags on a capture of the first 11 blocks, in
    chunks of 4: the AVI's frames are those of one csm_clean_blocks call over the capture, and the CSV's lines its steps merged per
    pixel."""
    import importlib.util
    import sys

    import torch

    from test_blocks_cpu import udp_frame, write_pcap
    from test_find_cpu import REPO

    def load(name):
        spec = importlib.util.spec_from_file_location(name, REPO / "tools" / f"{name}.py")
        tool = importlib.util.module_from_spec(spec)
        sys.modules[name] = tool
        spec.loader.exec_module(tool)
        return tool

    B = pkg.binding
    video, sources = load("pcap_video"), load("pcap_sources")
    off, frac, _, wire, _ = find_c1
    BYTES = 256 * 1032
    pcap = tmp_path / "rec.pcap"
    write_pcap(pcap, [udp_frame(wire[k: k + 1032], 21844) for k in range(0, 11 * BYTES, 1032)])
    common = [str(pcap), "--port", "21844", "--cols", "32", "--every", "3", "--chunk", "4", "--max-batch", "4", "--csm", "7500:8000:hann",
              "--csm-length", "5", "--csm-clean", "3:0.75:0.05"]
    bins, window = B.csm_from_text("7500:8000:hann")
    assert bins == [40, 41] and window == 1 and B.csm_clean_from_text("3:0.75:0.05") == (3, 0.75, 0.05)
    d_table = torch.from_numpy(video.jet_table()).cuda()
    assert video.main(common + ["--size", "50", "--flip", "--out", str(tmp_path / "cleaned")]) == 0
    frames, rate, scale = video.read_avi(tmp_path / "cleaned.000.avi")
    assert (rate, scale) == video.frame_rate(3)
    with engine(pkg, off, frac, 64, 32, 4) as eng:
        want = eng.csm_clean_blocks(wire[: 11 * BYTES], 32, 32, bins, 3, 0.75, 0.05, window=window, length=5, every=3, out_rows=50, out_cols=50,
                                    d_colormap_ptr=d_table.data_ptr(), flip=True, want_image=False)
    assert len(want) == 4 and np.array_equal(frames, want.big) and frames.any()
    out = tmp_path / "sources.csv"
    assert sources.main(common + ["--max-sources", "3", "--out", str(out)]) == 0
    back = sources.read_rows(out)
    records, count = B.csm_clean_source_records(want.steps, 32, 32, 3)
    assert len(back) == int(count.sum()) >= 4
    k = 0
    for j, (entries, n) in enumerate(zip(records, count)):
        for rank in range(n):
            assert (back[k]["block"], back[k]["rank"], back[k]["pixel"]) == (3 * j, rank, entries[rank]["pixel"])
            assert back[k]["power"] == entries[rank]["power"]
            k += 1
    for tool in (video, sources):  # the flag's refusals
        for bad in (["--csm-clean", "0"], ["--csm-kind", "capon"]):
            with pytest.raises(SystemExit):
                tool.main(common + bad)
        with pytest.raises(SystemExit):
            tool.main([str(pcap), "--port", "21844", "--csm-clean", "3"])
