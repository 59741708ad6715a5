"""The stream gate of tests/test_stream_order_gpu.py: a way to see on which stream, and in what
order, a library call really ran.

A gated call on a stream `st` enqueues, in stream order on `st`,

    delay (about 20 ms)  ->  event  ->  outputs := sentinel, real inputs copied over decoys
        ->  THE CALL  ->  every output copied into a snapshot
        ->  inputs := second decoys, outputs := sentinel

and only then synchronises.  The decoys are valid inputs of the same shape from other seeds, so

  * work that lands on another stream runs while the delay still holds the gate shut: it reads
    the first decoy and its results are wiped before the snapshot -> wrong numbers, no NaN path;
  * work that runs late reads the second decoy, or writes over the sentinel.

What the gate cannot see: the runtime multiplexes streams onto a few hardware queues (four per
process on the test machines), and a launch on a wrong stream that shares the gated stream's queue
is held behind the delay all the same.  Measured with as_stream() mutated to ignore its argument:
17 of the 67 single-stream cases pass.  Streams are handed to the queues in turn, so of two streams
created one after the other -- the two-stream parametrisation -- at most one shares the queue of
the stream the work landed on: under the same mutation every two-stream case with a device output
fails (64 of 65).

The snapshots must be bit-identical to the same call made plainly (same buffers, NULL stream,
the device synchronised before and after), and after the final synchronise every output buffer
must hold the sentinel.  An entry point that does not synchronise by design must return while
the event after the delay is still pending: the host ran ahead of the gate, so the check was
not vacuous.

The delay is torch.cuda._sleep, calibrated once per module with events; it is finite and never
chained.  No graph capture, never more than two streams in flight.
"""
import ctypes

import numpy as np

TARGET_MS = 20.0        # 400 x the ~50 us host cost of one call (README.md)
DELAY_BOUNDS_MS = (10.0, 200.0)


def sentinel(t):
    import torch
    return {torch.float64: -3.0e55, torch.int32: -7, torch.int64: -7, torch.uint8: 0xA5}[t.dtype]


def vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def dev(torch, a, dtype=np.float64):
    return torch.as_tensor(np.array(a, dtype=dtype, order="C"), device="cuda:0")


def same_bits(a, b):
    """bit-identity of two device tensors (NaN payloads included)"""
    import torch
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float64:
        a, b = a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)
    return bool(torch.equal(a, b))


def holds_sentinel(t):
    import torch
    return same_bits(t, torch.full_like(t, sentinel(t)))


def _sleep_ms(torch, cycles):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    torch.cuda._sleep(int(cycles))
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def calibrate(torch):
    """-> (cycles, measured ms) of a torch.cuda._sleep of about TARGET_MS; raises (the module's
    setup fails, it does not skip) when the calibrated delay measures outside DELAY_BOUNDS_MS."""
    _sleep_ms(torch, 100_000)                       # the first launch loads the kernel
    probe = 1_000_000
    ms = _sleep_ms(torch, probe)
    for _ in range(3):                              # a probe too short to time: lengthen it (bounded)
        if ms >= 1.0:
            break
        probe *= 8
        ms = _sleep_ms(torch, probe)
    cycles = int(probe * TARGET_MS / max(ms, 1e-3))
    got = _sleep_ms(torch, cycles)
    print("stream gate: torch.cuda._sleep(%d) measures %.2f ms (probe %d cycles: %.3f ms)" % (cycles, got, probe, ms))
    if not DELAY_BOUNDS_MS[0] <= got <= DELAY_BOUNDS_MS[1]:
        raise RuntimeError("calibrated delay %.2f ms outside %s ms" % (got, DELAY_BOUNDS_MS))
    return cycles, got


class GIn:
    """One gated input: the buffer the call reads, and what is copied into it."""

    def __init__(self, torch, real, decoy, decoy2, dtype=np.float64):
        self.real, self.decoy, self.decoy2 = (dev(torch, a, dtype) for a in (real, decoy, decoy2))
        assert self.real.shape == self.decoy.shape == self.decoy2.shape
        self.buf = self.decoy.clone()


class Case:
    """One row of the table, built for one seed.

    ins      gated inputs (GIn); `outs` device tensors the call writes (a buffer that is both, like
             the NaN flags, is listed in both: ins[i].buf is outs[j])
    call     call(stream) -> status, stream a ctypes.c_void_p or None; values the entry point returns
             on the host are appended to self.host
    check    check(outs as numpy arrays, host values): the operator's bar against the oracle
    sync     None for an entry point expected to return before its work ran, else the reason
             (with the line of sts_api.cpp) why it synchronises by design
    """

    def __init__(self, ins, outs, call, check, sync=None, status=0):
        self.ins, self.outs, self._call, self.check, self.sync, self.status = ins, outs, call, check, sync, status
        self.host = []

    def call(self, stream):
        self.host = []
        return self._call(stream)

    def preset(self, which):
        """outputs := sentinel, inputs := real | decoy (on torch's current stream)"""
        for o in self.outs:
            o.fill_(sentinel(o))
        for g in self.ins:
            g.buf.copy_(getattr(g, which))


def plain(torch, case):
    """The reference run: same buffers, NULL stream, device synchronised before and after.
    -> (status, clones of the outputs, host values)"""
    case.preset("real")
    torch.cuda.synchronize()
    st = case.call(None)
    torch.cuda.synchronize()
    res = [o.clone() for o in case.outs]
    torch.cuda.synchronize()
    return st, res, list(case.host)


class Ticket:
    pass


def enqueue(torch, case, stream, cycles):
    """Queue one gated call on `stream` and return without waiting."""
    t = Ticket()
    t.case, t.stream = case, stream
    t.snaps = [torch.empty_like(o) for o in case.outs]
    case.preset("decoy")
    torch.cuda.synchronize()
    t.event = torch.cuda.Event()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)
        t.event.record(stream)
        for o in case.outs:                         # results written before the gate opened are wiped:
            o.fill_(sentinel(o))                    # an entry point without inputs is caught running early
        for g in case.ins:
            g.buf.copy_(g.real, non_blocking=True)
        t.status = case.call(ctypes.c_void_p(stream.cuda_stream))
        t.pending_at_return = not t.event.query()
        t.host = list(case.host)
        for s, o in zip(t.snaps, case.outs):
            s.copy_(o, non_blocking=True)
        for g in case.ins:
            g.buf.copy_(g.decoy2, non_blocking=True)
        for o in case.outs:
            o.fill_(sentinel(o))
    return t


def finish(torch, t):
    """Synchronise the ticket's stream, then the device; -> the outputs that do not hold the
    sentinel (indices): work of the call that ran after the snapshot."""
    t.stream.synchronize()
    torch.cuda.synchronize()
    return [i for i, o in enumerate(t.case.outs) if not holds_sentinel(o)]
