"""The harness of test_gpu_stream_order.py: one device-form call with work pending on its stream in front of it and behind it, and
no host synchronisation in between (include/awpu_hip.h, "Streams": (a) reads, (b) writes, (d) no caller sync).

A case is a Case: how to make its handle, its device inputs as (true, decoy) pairs of equal shape -- the decoy is valid data of
another seed, finite everywhere --, its device outputs as (shape, dtype), and the call.  run() does, on one side stream S:

  producer   busywork that keeps S occupied (~20 ms, sized once per module), then every input's true data copied over the decoy
             it was allocated with, and an event behind that
  the call   on S.  An asynchronous entry point must return while the producer's event is still unfinished; for the synchronous
             ones (they bring host data back) the event must be unfinished immediately before the call.  Either way a case whose
             precondition does not hold FAILS: it cannot pass because the device happened to be idle.
  consumer   on S: every output, guards included, copied to a second buffer; then the outputs overwritten with the canary and
             the inputs with the decoy again (the write-after-read half of (b))
  S.synchronize() only, then the comparison.

A call that read its inputs early saw the decoy; one whose outputs were not complete for S left canary in the copy; one that
still read or wrote after it had let S go on met the decoy or lost its output to the canary.  The reference is reference(): the
same call on a handle of its own with the device settled before and after -- the parity tests tie that answer to the oracle.
The comparison is of bytes: the same handle configuration and shape is the same kernel in every math mode.

Both handles serve one settled call on the decoy first (prime): the first call of a handle builds tables and allocates, some of it
behind a device-wide wait, which would empty S and void the precondition; a run of blocks also leaves its ring behind, the same
one on both handles."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Dict, Optional, Tuple

import numpy as np

GUARD = 256           # bytes in front of and behind every output
BUSY_MS = 20.0        # what the producer's busywork is sized to: not a tolerance, it only has to dwarf a call's enqueue time
BUSY_FLOATS = 1 << 27  # 512 MiB, in-place: about a quarter of a millisecond a pass


@dataclass
class Case:
    engine: Callable[[], object]
    ins: Dict[str, Tuple[np.ndarray, np.ndarray]]          # name -> (true, decoy)
    outs: Dict[str, Tuple[tuple, object]]                  # name -> (shape, numpy dtype)
    call: Callable[[object, dict, dict, int], object]      # (engine, inputs, outputs, stream) -> host result or None
    synchronous: bool = False                              # the header says so, or it returns host data
    inout: Tuple[str, ...] = ()                            # inputs the call also writes (a carry): compared like outputs
    variant: Optional[Callable[[object], object]] = field(default=None)  # what to print of the handle after the call


def bits(a) -> bytes:
    return np.ascontiguousarray(a).tobytes()


class Busy:
    """Repeated in-place elementwise passes over one large tensor, sized once with events on a settled device."""

    def __init__(self):
        import torch

        self.x = torch.ones(BUSY_FLOATS, dtype=torch.float32, device="cuda")
        for _ in range(3):
            self.x.mul_(1.0)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(16):
            self.x.mul_(1.0)
        t1.record()
        torch.cuda.synchronize()
        self.pass_ms = t0.elapsed_time(t1) / 16
        self.passes = max(8, int(np.ceil(BUSY_MS / self.pass_ms)))
        print(f"busywork: {self.pass_ms:.3f} ms a pass, {self.passes} passes")

    def __call__(self, factor: float = 1.0):  # on the current stream
        for _ in range(max(1, int(self.passes * factor))):
            self.x.mul_(1.0)


def _canary(dtype):
    return -3.0 if np.dtype(dtype) == np.float32 else None  # (other types: 0xA5 bytes)


class Buffers:
    """The device side of a case, allocated and filled on the default stream: inputs holding the decoy, outputs holding the canary
    between guards of canary."""

    def __init__(self, case: Case):
        import torch

        self.case = case
        self.true = {k: torch.from_numpy(np.ascontiguousarray(t)).cuda() for k, (t, _) in case.ins.items()}
        self.decoy = {k: torch.from_numpy(np.ascontiguousarray(d)).cuda() for k, (_, d) in case.ins.items()}
        for k, (t, d) in case.ins.items():
            assert t.shape == d.shape and t.dtype == d.dtype and bits(t) != bits(d), k
            assert d.dtype.kind != "f" or np.isfinite(d).all(), k
        self.ins = {k: v.clone() for k, v in self.decoy.items()}
        self.raw, self.fill, self.outs = {}, {}, {}
        for k, (shape, dtype) in case.outs.items():
            n = int(np.prod(shape)) * np.dtype(dtype).itemsize
            assert GUARD % np.dtype(dtype).itemsize == 0
            if _canary(dtype) is not None:
                fill = torch.full(((n + 2 * GUARD) // 4,), _canary(dtype), dtype=torch.float32, device="cuda").view(torch.uint8)
            else:
                fill = torch.full((n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            self.fill[k] = fill
            self.raw[k] = fill.clone()
            self.outs[k] = self.raw[k][GUARD: GUARD + n]
        self.copy = {k: torch.zeros_like(v) for k, v in self.raw.items()}
        self.copy_inout = {k: torch.zeros_like(self.ins[k]) for k in case.inout}

    def ptrs(self):
        return {k: v.data_ptr() for k, v in self.ins.items()}, {k: v.data_ptr() for k, v in self.outs.items()}

    def collect(self, host):
        """What the comparison sees: the copied outputs (guards checked here), the copied in/out inputs, the host result."""
        got = {}
        for k, (shape, dtype) in self.case.outs.items():
            raw = self.copy[k].cpu().numpy()
            want_guard = self.fill[k].cpu().numpy()
            assert bits(raw[:GUARD]) == bits(want_guard[:GUARD]), f"{k}: guard in front overwritten"
            assert bits(raw[-GUARD:]) == bits(want_guard[-GUARD:]), f"{k}: guard behind overwritten"
            got[k] = raw[GUARD:-GUARD].view(dtype).reshape(shape)
        for k in self.case.inout:
            got[k] = self.copy_inout[k].cpu().numpy()
        got["host"] = host
        return got


def _prime(case: Case, eng):
    """One settled call on the decoy, into buffers of its own."""
    import torch

    buf = Buffers(case)
    torch.cuda.synchronize()
    i, o = buf.ptrs()
    case.call(eng, i, o, 0)
    eng.synchronize()
    torch.cuda.synchronize()


def reference(case: Case):
    """The call on a handle of its own, the device settled before and after."""
    import torch

    with case.engine() as eng:
        _prime(case, eng)
        buf = Buffers(case)
        for k in buf.ins:
            buf.ins[k].copy_(buf.true[k])
        torch.cuda.synchronize()
        i, o = buf.ptrs()
        host = case.call(eng, i, o, 0)
        eng.synchronize()
        torch.cuda.synchronize()
        for k in buf.raw:
            buf.copy[k].copy_(buf.raw[k])
        for k in case.inout:
            buf.copy_inout[k].copy_(buf.ins[k])
        torch.cuda.synchronize()
        return buf.collect(host)


def run(case: Case, busy: Busy, library_stream="side"):
    """The call between a producer and a consumer on one side stream.  library_stream: "side" = that stream (the test);
    "own" = the handle's own stream, which entitles the library not to wait for the producer (the proof that the harness can
    fail; never part of the suite)."""
    import torch

    with case.engine() as eng:
        _prime(case, eng)
        buf = Buffers(case)
        side = torch.cuda.Stream()
        behind_producer = torch.cuda.Event()
        i, o = buf.ptrs()
        torch.cuda.synchronize()  # the last host synchronisation before the comparison's
        with torch.cuda.stream(side):
            busy()
            for k in buf.ins:
                buf.ins[k].copy_(buf.true[k], non_blocking=True)
            behind_producer.record(side)
            if case.synchronous:
                assert not behind_producer.query(), "precondition: the producer was over before a synchronous call began"
            host = case.call(eng, i, o, side.cuda_stream if library_stream == "side" else 0)
            if not case.synchronous:
                assert not behind_producer.query(), "precondition: the producer was over when the asynchronous call returned"
            for k in buf.raw:
                buf.copy[k].copy_(buf.raw[k], non_blocking=True)
            for k in case.inout:
                buf.copy_inout[k].copy_(buf.ins[k], non_blocking=True)
            for k in buf.raw:
                buf.raw[k].copy_(buf.fill[k], non_blocking=True)
            for k in buf.ins:
                buf.ins[k].copy_(buf.decoy[k], non_blocking=True)
        side.synchronize()
        got = buf.collect(host)
        if case.variant is not None:
            print("variant:", case.variant(eng))
        if library_stream != "side":
            eng.synchronize()
        return got


def assert_same(got: dict, want: dict):
    assert got.keys() == want.keys()
    for k in want:
        if k == "host":
            assert _host_bits(got[k]) == _host_bits(want[k]), "host result"
        else:
            assert bits(got[k]) == bits(want[k]), f"{k}: not the settled handle's bits"


def _host_bits(v):
    if v is None:
        return None
    if isinstance(v, (tuple, list)):
        return tuple(_host_bits(x) for x in v)
    if isinstance(v, np.ndarray):
        return bits(v)
    return v
