"""A sweep's per-call options -- whether the launch records the handle's event bracket, where the pre-epilogue sums go, whether the
kernel raises the one-frame host call's completion flag -- are arguments of the call that starts the sweep (SweepOpts in
csrc/awpu_handle.h), not state of the handle.  What that must leave as it was, and the one thing it repairs:

1. which calls update last_kernel_ms / total_kernel_ms (the host forms that wait) and which leave them alone (the asynchronous ones);
2. the sums pointer of awpu_hip_process_device_sums is not seen by any later call;
3. the completion flag's answer belongs to the call that armed it: one-frame host calls that move from a kernel that raises the flag
   to one that cannot must wait for the stream, not read a flag value left over from the last armed launch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CANARY = -3.0
GUARD = 64  # floats in front of and behind a guarded device output
N_BLOCKS = 3


class C1:
    """c1 (64 mics, 32 x 32): the table, four frames and three blocks of samples."""

    def __init__(self, pkg):
        S = pkg.synthetic
        self.pkg, self.spec = pkg, S.WORKLOADS["c1"]
        self.P = self.spec.n_pixels
        xyz = S.geometry(self.spec)
        self.off, self.frac = S.delay_table(self.spec, xyz)
        self.frames = S.make_frames(xyz, 4, seed=31)
        self.samples = np.ascontiguousarray(S.make_frames(xyz, 1, seed=32, hist=256 * N_BLOCKS)[0])

    def engine(self, max_batch=4):
        eng = self.pkg.Engine(n_pixels=self.P, n_streams=64, max_batch=max_batch, grid_columns=self.spec.res)
        eng.set_delay_table(self.off, self.frac)
        eng.set_active_mics(None)
        return eng


@pytest.fixture(scope="module")
def c1(pkg):
    return C1(pkg)


def clock(eng):
    st = eng.stats()
    return st.launches, st.last_kernel_ms, st.total_kernel_ms


def assert_timed(eng, call, what):
    before = clock(eng)
    call()
    after = clock(eng)
    print(f"{what}: launches {before[0]} -> {after[0]}, last_kernel_ms {after[1]:.6f}, total_kernel_ms {before[2]:.6f} -> {after[2]:.6f}")
    assert after[2] > before[2] and after[1] > 0, (what, before, after)


def assert_untimed(eng, call, what):
    before = clock(eng)
    call()
    eng.synchronize()
    after = clock(eng)
    print(f"{what}: launches {before[0]} -> {after[0]}, last_kernel_ms {after[1]:.6f}, total_kernel_ms {before[2]:.6f} -> {after[2]:.6f}")
    assert after[0] > before[0], (what, "no sweep ran", before, after)
    assert after[1:] == before[1:], (what, before, after)  # bit-equal: the call recorded and read no bracket


def test_host_forms_are_timed_and_asynchronous_forms_are_not(c1):
    import torch

    pkg, P = c1.pkg, c1.P
    band = [pkg.band_design(1000.0, 4000.0, 31)]
    two = c1.frames[:2]
    with c1.engine() as eng:
        assert_timed(eng, lambda: eng.process(two), "process, batch 2")

        def async_then_wait():
            eng.process_async(two)
            eng.wait()

        assert_timed(eng, async_then_wait, "process_async + wait")
        assert_timed(eng, lambda: eng.process_bands(two, band), "process_bands, one band")
        assert_timed(eng, lambda: eng.cohere(two), "cohere")
    with c1.engine() as eng:
        assert_timed(eng, lambda: eng.process_samples(c1.samples), "process_samples")
        assert_timed(eng, lambda: eng.watch_samples(c1.samples, c1.spec.res, c1.spec.res), "watch_samples")
        assert_timed(eng, lambda: eng.peel_samples(c1.samples, c1.spec.res, c1.spec.res, 2), "peel_samples")
    with c1.engine() as eng:
        d_x = torch.from_numpy(c1.frames.copy()).cuda()
        d_s = torch.from_numpy(c1.samples.copy()).cuda()
        d_p = torch.zeros((4, P), dtype=torch.float32, device="cuda")
        d_sums = torch.zeros((2, P, 256), dtype=torch.float32, device="cuda")
        d_image = torch.zeros((N_BLOCKS, P), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        x, p, pitch = d_x.data_ptr(), d_p.data_ptr(), c1.samples.shape[1]
        untimed = [
            ("process_device", lambda: eng.process_device(x, 2, p)),
            ("process_device_sums", lambda: eng.process_device_sums(x, 2, p, d_sums.data_ptr())),
            ("process_bands_device", lambda: eng.process_bands_device(x, 2, band, p)),
            ("cohere_device", lambda: eng.cohere_device(x, 2, d_power_ptr=p)),
            ("peel_device", lambda: eng.peel_device(x, 2, 2, d_map_ptr=p)),
            ("peel (host)", lambda: eng.peel(two, 2)),
            ("process_samples_device", lambda: eng.process_samples_device(d_s.data_ptr(), pitch, N_BLOCKS, p)),
            ("watch_samples_device", lambda: eng.watch_samples_device(d_s.data_ptr(), pitch, N_BLOCKS, c1.spec.res, c1.spec.res, d_image_ptr=d_image.data_ptr())),
        ]
        try:  # (the packed entry points refuse where this handle's sweep of four frames is no frame-pair shape)
            d_packed = torch.zeros((eng.packed_bytes(4) // 4,), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()

            def pack_then_sweep():
                eng.pack_frames(x, 4, d_packed.data_ptr())
                eng.process_packed(d_packed.data_ptr(), 4, p)

            untimed.append(("pack_frames + process_packed", pack_then_sweep))
        except pkg.AwpuError as e:
            assert e.status == pkg.binding.ERR_STATE, e
            print(f"packed frames are not taken at this shape: {e}")
        for what, call in untimed:
            assert_untimed(eng, call, what)
            assert_timed(eng, lambda: eng.process(two), f"process, batch 2, after {what}")  # the switch came back
    with c1.engine(max_batch=1) as eng:  # the one-frame host call samples its bracket: the first call and every 32nd after it
        changed = []
        for call in range(34):
            before = clock(eng)
            eng.process(c1.frames[call % 4:call % 4 + 1])
            after = clock(eng)
            assert after[0] > before[0]
            if after[2] != before[2]:
                changed.append(call)
        assert changed == [0, 32], changed


def test_the_sums_pointer_does_not_outlive_its_call(c1):
    import torch

    P = c1.P
    two = c1.frames[:2]
    with c1.engine() as eng:
        d_x = torch.from_numpy(two.copy()).cuda()
        d_p = torch.zeros((2, P), dtype=torch.float32, device="cuda")
        raw = torch.full((2 * P * 256 + 2 * GUARD,), CANARY, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        eng.process_device_sums(d_x.data_ptr(), 2, d_p.data_ptr(), raw.data_ptr() + 4 * GUARD)
        eng.synchronize()
        first = d_p.cpu().numpy()
        host = raw.cpu().numpy()
        assert (host[:GUARD] == CANARY).all() and (host[-GUARD:] == CANARY).all(), "sums: guard overwritten"
        assert (host[GUARD:-GUARD] != CANARY).any(), "no sums were exported"
        raw.fill_(CANARY)
        d_p.zero_()
        torch.cuda.synchronize()
        eng.process_device(d_x.data_ptr(), 2, d_p.data_ptr())
        eng.synchronize()
        assert np.array_equal(d_p.cpu().numpy(), first)
        assert np.array_equal(eng.process(two), first)
        assert (raw.cpu().numpy() == CANARY).all(), "a later call wrote through the sums pointer of awpu_hip_process_device_sums"


def test_the_completion_flag_belongs_to_the_call_that_armed_it(pkg):
    """One-frame host calls at the reference's shape raise and spin on the completion flag (exact_ndh_stationary).  A table whose
    horizontal neighbours always coincide and whose vertical ones never do takes the same calls to exact_pair, which cannot raise
    it: they must wait for the stream.  Before the flag's answer was returned by the call that arms it, the handle remembered
    "the sweep will raise the flag" from the last armed launch, the flag still held that launch's number, and such a call copied
    its powers out without waiting for the sweep just enqueued."""
    import torch

    S = pkg.synthetic
    names = pkg.binding.KERNEL_NAMES
    spec = S.WORKLOADS["ref_default"]
    xyz = S.geometry(spec)
    off, frac = S.delay_table(spec, xyz)
    frames = S.make_frames(xyz, 7, seed=99)
    frames *= (1.0 + np.arange(7, dtype=np.float32))[:, None, None]  # seven frames of different scale: powers differ by far more than an ulp
    rows = np.arange(spec.n_pixels, dtype=np.int32)[:, None] // spec.res
    off2 = np.ascontiguousarray(200 + (7 * rows + np.arange(off.shape[1], dtype=np.int32)[None, :]) % 90, dtype=np.int32)
    with pkg.Engine(n_pixels=spec.n_pixels, n_streams=64, max_batch=1, grid_columns=spec.res) as eng:
        eng.set_delay_table(off, frac)
        eng.set_active_mics(None)
        for k in range(5):
            eng.process(frames[k:k + 1])
        assert names[eng.stats().kernel_variant] == "exact_ndh_stationary"
        eng.set_delay_table(off2, frac)
        want = []
        for k in range(7):
            d_x = torch.from_numpy(frames[k:k + 1].copy()).cuda()
            d_p = torch.zeros((1, spec.n_pixels), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            eng.process_device(d_x.data_ptr(), 1, d_p.data_ptr())
            eng.synchronize()
            want.append(d_p.cpu().numpy()[0])
        assert names[eng.stats().kernel_variant] == "exact_pair"
        assert not np.array_equal(want[0], want[6])
        for call in range(40):
            k = 6 * (call & 1)  # alternating frames: a result left over from the call before differs
            got = eng.process(frames[k:k + 1])[0]
            assert names[eng.stats().kernel_variant] == "exact_pair"
            assert np.array_equal(got, want[k]), (call, k, np.argwhere(got != want[k])[:4])
