"""Several calls of one plan in flight at once, for the GPU tests (a helper module, not a test file).

include/grbda_hip.h: a plan "is immutable after creation and may be shared by threads and streams".  What makes that true sits on the host
side of capi.cpp -- slabs keyed by (device, stream), grbda_plan::mu held until a call's last kernel is enqueued -- and a defect there gives
finite, plausible, wrong numbers only while two calls really overlap on the device.  The kernels are deterministic, so the tests built
on this module ask for BIT equality between a call made alone and the same call made with others in flight.

Gate(ms): a stream that runs torch's spin kernel for `ms` milliseconds and records an event; hold(streams) makes every worker stream
wait for that event.  While the gate spins the host can queue any number of calls on the workers; held() -- the event has not
completed -- directly after the enqueue loop says that all of it was queued before any of it ran.  The length comes from measurement:
cycles_per_ms() times the spin kernel once per process with events, gate_ms() is four times the host time the same calls took to enqueue
serially, and GATE_CAP_MS bounds it so that a miscalibration cannot hold a card.

round_robin(streams, calls, R, gate): R repetitions of calls[i](r) on streams[i], interleaved over the streams in the order a single
host thread issues them, each between two timing events on its stream; at the start of every call it samples the host clock, whether the
gate is still closed and whether work issued earlier on another stream is still incomplete.  windows() turns the events into (start, end) milliseconds after the
gate's origin event; overlapping() counts the pairs of repetitions on DIFFERENT streams whose windows intersect -- the evidence that two
calls of the plan were on the device at the same time.

in_threads(bodies): one host thread per body, released together by a barrier; an exception in a thread is re-raised in the caller, a
thread that does not come back within the timeout fails the test.  (ctypes drops the GIL for the length of a foreign call, so the
library calls of the threads contend on the plan's mutex.)"""
import threading
import time

import torch

N_STREAMS = 4        # the runtime's default number of hardware queues per process; also the most host threads any test here starts
GATE_CAP_MS = 2000.0
JOIN_TIMEOUT_S = 120.0

_cycles_per_ms = None


def cycles_per_ms():
    """spin-kernel cycles per millisecond, measured once per process: the count is raised until one spin lasts at least 5 ms (each
    step at most 8 times the one before, which lasted under 5 ms)"""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        torch.cuda._sleep(1000)  # (the kernel's first launch loads its code)
        torch.cuda.synchronize()
        n, ms = 250_000, 0.0
        while ms < 5.0 and n < (1 << 40):
            n *= 8
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(n)
            b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
        assert ms >= 5.0, f"the spin kernel returns after {ms} ms for {n} cycles"
        _cycles_per_ms = n / ms
    return _cycles_per_ms


def gate_ms(serial_enqueue_s, R):
    """four times the host time R repetitions of the serially measured calls take to enqueue, at most GATE_CAP_MS"""
    return min(GATE_CAP_MS, 4.0 * serial_enqueue_s * 1e3 * R)


class Gate:
    def __init__(self, ms):
        assert 0.0 < ms <= GATE_CAP_MS
        self.ms = ms
        self.stream = torch.cuda.Stream()
        self.origin = torch.cuda.Event(enable_timing=True)
        self.opened = torch.cuda.Event(enable_timing=True)
        cycles = int(ms * cycles_per_ms())
        with torch.cuda.stream(self.stream):
            self.origin.record()
            torch.cuda._sleep(cycles)
            self.opened.record()

    def hold(self, streams):
        for s in streams:
            s.wait_event(self.opened)

    def held(self):
        return not self.opened.query()


def round_robin(streams, calls, R, gate=None):
    """outs[i][r] = calls[i](r) with streams[i] current, r outermost; events[i][r] = (before, after) on streams[i]; trace = one
    record per call in the order of issue, (i, r, host time at its start, the gate was still closed then, an earlier call on ANOTHER
    stream had not completed then, host time at its end)"""
    outs = [[None] * R for _ in streams]
    events = [[None] * R for _ in streams]
    trace = []
    for r in range(R):
        for i, s in enumerate(streams):
            t0 = time.perf_counter()
            held = gate is not None and gate.held()
            # (a stream completes in order: its last call stands for all of them)
            last = [events[j][r if j < i else r - 1] for j in range(len(streams)) if j != i and (j < i or r > 0)]
            busy = any(not e[1].query() for e in last)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):
                a.record()
                outs[i][r] = calls[i](r)
                b.record()
            events[i][r] = (a, b)
            trace.append((i, r, t0, held, busy, time.perf_counter()))
    return outs, events, trace


def windows(origin, events):
    """win[i][r] = (start, end) in milliseconds after `origin`; everything must have completed"""
    return [[(origin.elapsed_time(a), origin.elapsed_time(b)) for a, b in per_stream] for per_stream in events]


def overlapping(win):
    """number of pairs (i, r), (j, r') with i < j whose windows intersect"""
    n = 0
    for i in range(len(win)):
        for j in range(i + 1, len(win)):
            for s0, e0 in win[i]:
                for s1, e1 in win[j]:
                    n += s0 < e1 and s1 < e0
    return n


def same_bits(a, b):
    """two tensors (or two sequences of tensors) of the same shapes and types holding the same bytes"""
    if isinstance(a, torch.Tensor):
        return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))
    return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))


def in_threads(bodies, timeout=JOIN_TIMEOUT_S):
    """bodies[k]() in a thread each, all released by one barrier; returns their results in order"""
    assert len(bodies) <= N_STREAMS
    barrier = threading.Barrier(len(bodies))
    results, errors = [None] * len(bodies), [None] * len(bodies)

    def work(k):
        try:
            barrier.wait(timeout)
            results[k] = bodies[k]()
        except BaseException as e:  # (carried to the caller)
            errors[k] = e
            barrier.abort()

    threads = [threading.Thread(target=work, args=(k,), daemon=True) for k in range(len(bodies))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout)
    alive = [k for k, t in enumerate(threads) if t.is_alive()]
    assert not alive, f"threads {alive} did not come back within {timeout} s"
    for e in errors:
        if e is not None and not isinstance(e, threading.BrokenBarrierError):
            raise e
    for e in errors:
        if e is not None:
            raise e
    return results
