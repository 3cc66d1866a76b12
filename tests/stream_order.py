"""The delayed-operand harness of tests/test_stream_order_gpu.py: runs one asynchronous entry point the way a
multi-stream consumer does, so that an ordering bug gives a deterministic wrong answer instead of a race.

The legacy null stream synchronises with every blocking stream, so on it a kernel launched on stream 0 instead of the
caller's stream, a scratch block released on the wrong stream or a side lane that is never joined still computes the
right values.  Here every call runs on a ``hipStreamNonBlocking`` stream (``torch.cuda.Stream()``) whose operands
arrive late:

    s:  [delay] -> pending -> true operands -> sentinel fill of the outputs -> the call -> copy to pinned host memory

Before that the operand buffers hold *decoys* (a second valid input set) and the device is synchronised.  A stage of
the call that is not ordered behind ``s`` runs while the delay is still spinning: it reads the decoys (whose result
differs from the true one in every row) or writes early and is overwritten by the sentinel fill.  The harness requires
``not pending.query()`` right after the call returned to Python: a run whose delay had already drained proves nothing
and fails as inconclusive.  Only ``s`` is synchronised before the comparison, never the device.

Decoys and sentinels are valid data of the entry point (residues below p, indices in range), so a mis-ordered kernel
can only compute a wrong value: nothing here can index out of bounds.

The streams are created once and kept for the life of the process: the scratch pool orders its blocks by events
recorded on the caller's stream, and an event of a destroyed stream cannot be waited on reliably (scratch.cpp
wait_last_use), which is test_zz_scratch_oom_gpu.py's subject, not this file's.
"""
import time

import numpy as np

# Length of the delay in front of the operands, in milliseconds of device time.  DESIGN.md §5 records the host
# enqueue times it is sized from: the slowest sequence of the file took 6 ms of host time on an MI355X (the first call
# issued on a newly created stream), every other one under 0.3 ms.
DELAY_MS = 100.0
SENTINEL = 0x5E5E5E5E5E5E5E5E  # the word the outputs hold before the call writes them

_streams = {}
_rate = {}


def stream(name):
    """A non-blocking stream, one per name for the whole process."""
    import torch
    if name not in _streams:
        _streams[name] = torch.cuda.Stream()
    return _streams[name]


def _have_sleep():
    import torch
    return hasattr(torch.cuda, "_sleep")


def _busy(engine):
    """The fallback delay of the older tests: plan.fwd over an 8192 x 2048 buffer, repeated."""
    import torch
    if "busy" not in _rate:
        _rate["busy"] = (engine.Plan.cached(2048, engine.SOLINAS_P),
                         torch.zeros((8192, 2048), dtype=torch.int64, device="cuda"))
    return _rate["busy"]


def _spin(engine, units):
    """Queues `units` of delay on the current stream: cycles of the one spin kernel, or transforms of the loop."""
    import torch
    if _have_sleep():
        torch.cuda._sleep(int(units))
    else:
        plan, busy = _busy(engine)
        for _ in range(int(units)):
            plan.fwd(busy)


def delay_units(engine, ms=DELAY_MS):
    """How many units of _spin last `ms` on this device: measured once with events on an idle device."""
    import torch
    key = "sleep" if _have_sleep() else "loop"
    if key not in _rate:
        probe = 20_000_000 if _have_sleep() else 20
        s = stream("calibrate")
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            _spin(engine, probe if _have_sleep() else 2)  # first launch: module load, clocks
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            _spin(engine, probe)
            b.record(s)
        s.synchronize()
        _rate[key] = probe / max(a.elapsed_time(b), 1e-3)  # units per millisecond
    return max(1, int(_rate[key] * ms))


def queue_delay(engine, ms=DELAY_MS):
    """Queues the delay on the current stream."""
    _spin(engine, delay_units(engine, ms))


def to_dev(a):
    """A numpy array as a device tensor of the signed type of the same width (torch has no unsigned kernels)."""
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).cuda()


def to_host(t, like):
    """The host copy `t` as a numpy array of `like`'s dtype and shape."""
    return t.numpy().view(like.dtype).reshape(like.shape)


def sentinel_fill(t):
    """Fills `t` with the sentinel word (its low half for 32-bit tensors), whatever its dtype (f64 outputs too)."""
    import torch
    flat = t.view(-1)
    if flat.element_size() == 8:
        flat.view(torch.int64).fill_(SENTINEL)
    else:
        flat.view(torch.int32).fill_(SENTINEL & 0xFFFFFFFF)


def sentinel_like(a):
    """The sentinel fill as it reads back in `a`'s dtype and shape."""
    if a.dtype.itemsize == 8:
        return np.full(a.shape, SENTINEL, np.uint64).view(a.dtype)
    return np.full(a.shape, SENTINEL & 0xFFFFFFFF, np.uint32).view(a.dtype)


def holds_sentinel(a):
    """True when any word of `a` equals the sentinel: the expected results must not."""
    return bool(np.any(np.ascontiguousarray(a) == sentinel_like(a)))


class Result:
    """What one harness run saw: the host copies of the outputs, whether the delay was still pending when the call
    returned, and the host time the sequence took to enqueue."""

    def __init__(self, got, pending_when_returned, enqueue_ms, call_ms):
        self.got, self.pending_when_returned, self.enqueue_ms, self.call_ms = got, pending_when_returned, enqueue_ms, call_ms

    def mismatches(self, want):
        """Indices of the outputs whose host copy differs from the expected array, bit for bit."""
        return [i for i, (g, w) in enumerate(zip(self.got, want))
                if not np.array_equal(to_host(g, w).view(np.uint8), np.ascontiguousarray(w).view(np.uint8))]


def run_delayed(engine, call, operands, outputs, *, warm=True, call_stream=None, fill_stream=None, delay_ms=DELAY_MS):
    """Runs `call` (a closure that issues one entry point on the *current* torch stream) behind delayed operands.

    operands: (buffer, true, decoy) triples: the device tensor the call reads and two device tensors of the same shape
              and type holding the true and the decoy values (for an in-place entry the data buffer is one of them).
    outputs:  the device tensors the call writes (in-place data buffers included); those that are not operands get the
              sentinel fill.
    call_stream / fill_stream: the two negative controls: the call issued on another non-blocking stream (it must read
              decoys), or the sentinel fill issued on another stream behind a longer delay of its own (it must land
              over the results).  Both streams are synchronised before returning.
    Returns a Result; the comparison is the caller's."""
    import torch
    s = stream("s")
    op_bufs = [o[0] for o in operands]
    fresh = [t for t in outputs if not any(t is b for b in op_bufs)]
    pinned = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in outputs]

    def load_decoys():
        for buf, _, decoy in operands:
            buf.copy_(decoy)
        torch.cuda.synchronize()

    if warm:  # scratch growth (hipMalloc), lazy module loads and plan tables are not part of the timed sequence
        load_decoys()
        with torch.cuda.stream(s):
            call()
        s.synchronize()
    load_decoys()
    units = delay_units(engine, delay_ms)
    late_units = delay_units(engine, 2 * delay_ms) if fill_stream is not None else 0
    pending = torch.cuda.Event()
    filled = torch.cuda.Event()
    t0 = time.perf_counter()
    if fill_stream is not None:
        with torch.cuda.stream(fill_stream):
            _spin(engine, late_units)
            for t in fresh:
                sentinel_fill(t)
            filled.record(fill_stream)
    with torch.cuda.stream(s):
        _spin(engine, units)
        pending.record(s)
        for buf, true, _ in operands:
            buf.copy_(true, non_blocking=True)
        if fill_stream is None:
            for t in fresh:
                sentinel_fill(t)
        t1 = time.perf_counter()
        if call_stream is not None:
            with torch.cuda.stream(call_stream):
                call()
        else:
            call()
        t2 = time.perf_counter()
        still_pending = not pending.query()
        if fill_stream is not None:
            s.wait_event(filled)  # the consumer reads the buffers as both streams left them
        for host, t in zip(pinned, outputs):
            host.copy_(t, non_blocking=True)
    t3 = time.perf_counter()
    s.synchronize()
    for other in (call_stream, fill_stream):
        if other is not None:
            other.synchronize()
    return Result(pinned, still_pending, (t3 - t0) * 1e3, (t2 - t1) * 1e3)


class Case:
    """One entry point made ready for the harness.

    call:     the closure that issues it on the current torch stream
    operands: (buffer, true, decoy): the device tensor the call reads and the two host value sets (numpy arrays of the
              buffer's shape and width)
    outputs:  the device tensors it writes (in-place data buffers included)
    want:     want(values) -> the expected outputs for one value set, from the oracle / the family's reference; None
              for the f64-FFT entries, whose expected values are a quiescent run of the same call (shown to repeat
              bit for bit first)
    sync:     the entry is documented to synchronise `stream` before it returns: the delay must have drained when it
              does
    """

    def __init__(self, name, call, operands, outputs, want=None, sync=False):
        self.name, self.call, self.outputs, self.want, self.sync = name, call, list(outputs), want, sync
        self.decoy_may_match = ()  # outputs that cannot depend on the data at the case's parameters (say which, and why)
        self.bufs = [o[0] for o in operands]
        self.values = ([o[1] for o in operands], [o[2] for o in operands])
        self.staged = tuple([to_dev(v) for v in vs] for vs in self.values)
        for buf, t in zip(self.bufs, self.staged[0]):
            assert buf.shape == t.shape and buf.dtype == t.dtype, (name, buf.shape, t.shape, buf.dtype, t.dtype)

    def triples(self):
        return [(b, t, d) for b, t, d in zip(self.bufs, *self.staged)]

    def quiescent(self, which):
        """The outputs of the call on an idle device (synchronised before and after), value set `which`."""
        import torch
        torch.cuda.synchronize()
        for buf, v in zip(self.bufs, self.staged[which]):
            buf.copy_(v)
        for t in self.outputs:
            if not any(t is b for b in self.bufs):
                sentinel_fill(t)
        torch.cuda.synchronize()
        self.call()
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in self.outputs]

    def expected(self, which):
        if self.want is not None:
            return [np.ascontiguousarray(w) for w in self.want(self.values[which])]
        first = self.quiescent(which)
        if which == 0:
            again = self.quiescent(which)
            assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(first, again)), \
                f"{self.name}: the quiescent run does not repeat bit for bit"
        return first


TIMINGS = {}  # case name -> (host ms to enqueue the whole sequence, host ms inside the call)


def _batch_rows(a):
    """An output as (rows, bytes): one row per polynomial / ciphertext.  A trailing axis of 2 holds the (re, im) pair of
    a complex coefficient or the (lo, hi) words of a u128: such a polynomial is one row too."""
    a = np.ascontiguousarray(a)
    if a.ndim >= 3 and a.shape[-1] == 2:
        return a.reshape(-1, a.shape[-2] * 2).view(np.uint8)
    return a.reshape(-1, a.shape[-1]).view(np.uint8)


def every_row_differs(a, b):
    return bool(np.all(np.any(_batch_rows(a) != _batch_rows(b), axis=1)))


def check_case(engine, case, **control):
    """The acceptance of one entry: the decoys' result differs from the true one in every row, the delay was still
    pending when the call returned (or had drained, for an entry that synchronises by design), and the host copy equals
    the expected values bit for bit.  With a control (call_stream / fill_stream) it returns the mismatching outputs
    instead of asserting there are none."""
    want = case.expected(0)
    if case.bufs:
        for i, (w, d) in enumerate(zip(want, case.expected(1))):
            assert i in case.decoy_may_match or every_row_differs(w, d), \
                f"{case.name}: output {i} of the decoys equals the true one in some row"
    fresh = [i for i, t in enumerate(case.outputs) if not any(t is b for b in case.bufs)]
    for i in fresh:
        assert not holds_sentinel(want[i]), f"{case.name}: the expected output {i} holds the sentinel word"
    res = run_delayed(engine, case.call, case.triples(), case.outputs, **control)
    TIMINGS[case.name] = (res.enqueue_ms, res.call_ms)
    print(f"stream-order timing: {case.name}: sequence {res.enqueue_ms:.3f} ms, call {res.call_ms:.3f} ms, "
          f"delay {DELAY_MS:.0f} ms")
    if case.sync:
        assert not res.pending_when_returned, f"{case.name}: documented to synchronise the stream, but returned early"
    else:
        assert res.pending_when_returned, (f"{case.name}: inconclusive, the delay had drained when the call returned "
                                           f"(the call took {res.call_ms:.1f} ms of host time): it blocked the host")
    bad = res.mismatches(want)
    if control:
        return bad
    assert not bad, f"{case.name}: outputs {bad} differ from the expected values"
    return bad


def hand_over(engine, issue, sizes, reset):
    """The scratch hand-over between two non-blocking streams A and B.

    issue(side, round, size) queues on the current stream the call of `side` ("A" / "B", each with inputs of its own)
    for `round` (-1: the warm-up) into that call's own output; reset() clears the outputs.  Per round one stream issues
    its call behind the delay and the other one, with no delay, a call of the same size: the second call's scratch is the
    block the first one just released, so it may start only behind the first call.  The roles alternate.

    The sequence runs twice: on one stream (what the pool holds then is the reference for "shared, not doubled"), then
    on the two streams.  Returns (bytes after the one-stream run, bytes after the two-stream run, per round: whether
    the first call had completed when the second one had).

    The data alone cannot show a missing wait in this order: the first call's scratch *writer* pass is delayed together
    with its readers, so a second call that jumps ahead finishes before the first one starts and both compute the right
    values.  What is deterministic is the order: had the second call not waited on the first call's event, it would
    complete while the first call's delay is still spinning."""
    import torch
    M = engine.ntt64_pbs
    A, B = stream("A"), stream("B")
    names = {"A": A, "B": B}
    order = [("A", "B") if r % 2 == 0 else ("B", "A") for r in range(len(sizes))]

    torch.cuda.synchronize()
    M.scratch_trim(0)
    with torch.cuda.stream(A):
        issue("A", -1, sizes[0])
        for r, size in enumerate(sizes):
            issue(order[r][0], r, size)
            issue(order[r][1], r, size)
    A.synchronize()
    single = M.scratch_bytes(0)

    reset()
    torch.cuda.synchronize()
    M.scratch_trim(0)
    assert M.scratch_bytes(0) == 0, "the pool is not empty after a trim on an idle device"
    with torch.cuda.stream(A):
        issue("A", -1, sizes[0])
    A.synchronize()
    first_done = []
    for r, size in enumerate(sizes):
        f, s2 = order[r]
        done = torch.cuda.Event()
        with torch.cuda.stream(names[f]):
            queue_delay(engine)
            issue(f, r, size)
            done.record(names[f])
        with torch.cuda.stream(names[s2]):
            issue(s2, r, size)
        names[s2].synchronize()
        first_done.append(done.query())
        names[f].synchronize()
    return single, M.scratch_bytes(0), first_done
