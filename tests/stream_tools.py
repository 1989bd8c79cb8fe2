"""A side stream that is still busy: the tools of the stream-ordering tests (tests/test_gpu_streams.py and the four
older stream tests of the mel, Griffin-Lim and STFT-loss files).

``delayed(side, ms)`` makes ``side`` the current stream, enqueues a device-side delay on it first and yields a staging
``put``: every input then reaches the device behind the delay, through a pinned host buffer and a non-blocking copy
into a guarded block (tests/guarded_alloc.py) that holds NaN until the copy lands.  Every ``torch.empty`` / ``zeros``
of the library is served the same way.  Unlike ``Guard._alloc`` the blocks are filled with 0xFF on the NULL stream,
which is idle, and that fill is waited for: while the delay spins every input, output, workspace and arena of the call
under test really holds NaN.  A launch that went to any other stream than ``side`` runs at once, reads NaN (or its
consumer does) and equality with the reference fails.

The test is conclusive only if the delay was still running when the call under test returned: ``assert_busy(put)``
right after the call.  It is an assertion, not a measurement: an inconclusive run fails.  ``side_stream()`` is the
stream to use: one that a probe has shown to run beside the null stream (its docstring says why that matters).

This is an ordinary module that tests import; it is no pytest plugin."""
import contextlib
import time

import numpy as np
import torch

from tests import guarded_alloc as ga

DEV = "cuda:0"
FLOOR_MS, CAP_MS, FACTOR = 20.0, 1000.0, 3.0

_cycles_per_ms = None


def cycles_per_ms():
    """``torch.cuda._sleep`` cycles per millisecond, measured once per session with two events (printed)."""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        rate = None
        cycles = 1_000_000
        for _ in range(4):                                 # a first, short probe also pays the kernel's load
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.cuda._sleep(cycles)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            assert ms > 0.0, "torch.cuda._sleep does not delay on this device"
            rate = cycles / ms
            if ms >= 10.0:
                break
            cycles = int(rate * 20.0)
        _cycles_per_ms = rate
        print(f"stream_tools: torch.cuda._sleep runs {rate:.0f} cycles per ms (last probe: {cycles} cycles in {ms:.2f} ms)")
    return _cycles_per_ms


_side = None
PROBE_MS, CANDIDATES = 10.0, 8


def side_stream():
    """THE side stream of the ordering tests, chosen once per session: one that the device runs independently of the null
    stream.  Streams share a few hardware queues; a side stream on the null stream's queue is serialised with it, and a
    launch that went to the null stream by mistake -- where a forgotten stream argument lands -- would wait for the delay
    like a correct one: the test would be conclusive by its own condition and still blind.  The probe: the candidate sleeps,
    the null stream gets a small job and is waited for; if the candidate is still busy then, the two run side by side."""
    global _side
    if _side is None:
        rate = cycles_per_ms()
        null = torch.cuda.default_stream(torch.device(DEV))
        tried = []
        for _ in range(CANDIDATES):
            s = torch.cuda.Stream(device=DEV)
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                torch.cuda._sleep(int(rate * PROBE_MS))
            with torch.cuda.stream(null):
                torch.zeros(64, device=DEV).add_(1.0)
            null.synchronize()
            independent = not s.query()
            s.synchronize()
            tried.append(independent)
            if independent:
                _side = s
                break
        print(f"stream_tools: side stream {_side.cuda_stream if _side else None}: candidates independent of the null stream: {tried}")
        assert _side is not None, f"none of {CANDIDATES} streams runs beside the null stream: the ordering tests cannot see a launch on it"
    return _side


def delay_ms(reference_wall_s):
    """Length of the delay in front of a call whose REFERENCE run (default stream, its own module) took
    ``reference_wall_s`` of host time: three times that -- a fresh module's first call varies --, at least 20 ms, at most 1 s."""
    return min(CAP_MS, max(FLOOR_MS, FACTOR * 1e3 * reference_wall_s))


def timed(fn, *args):
    """(fn(*args), its host wall time in seconds): the reference run, which the delay is sized from."""
    t0 = time.perf_counter()
    out = fn(*args)
    return out, time.perf_counter() - t0


class _NullFillGuard(ga.Guard):
    """Guard whose blocks are poisoned on the idle null stream, completely, before the caller goes on."""

    def _alloc(self, shape, dtype, device, site, kind, zero):
        esize = torch._utils._element_size(dtype)
        n = 1
        for s in shape:
            n *= s
        nbytes = n * esize
        block = self._orig["empty"](ga.RED + ga._roundup(nbytes, ga.ALIGN) + ga.RED, dtype=torch.uint8, device=device)
        null = torch.cuda.default_stream(block.device)
        with torch.cuda.stream(null):
            block.fill_(ga.FILL)
        null.synchronize()                                  # the null stream alone: the busy side stream is not waited for
        view = block[ga.RED:ga.RED + nbytes].view(dtype).view(shape)
        if zero:
            view.zero_()                                    # part of the computation: on the current stream
        self.allocations.append(ga.Allocation(block, view, nbytes, site, kind))
        return view


ARENA_BYTES = 64 << 20
_arena = None


def _pinned_arena():
    """One pinned host buffer for the whole session: a pinned allocation per tensor costs milliseconds the first time, which
    would eat the delay."""
    global _arena
    if _arena is None:
        _arena = torch.empty(ARENA_BYTES, dtype=torch.uint8, pin_memory=True)
    return _arena


class Staged:
    """The staging variant of test_gpu_guarded._Put: ``Guard.place`` copies from pageable memory and would wait for the delay."""

    def __init__(self, guard, side, delay_end):
        self.g, self.side, self.delay_end = guard, side, delay_end
        self._used, self._hosts = 0, []

    def _host(self, t):
        nbytes = t.numel() * t.element_size()
        start = (self._used + 255) // 256 * 256
        if start + nbytes > ARENA_BYTES:                    # (larger than the arena: a pinned buffer of its own)
            host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            self._hosts.append(host)
            return host
        self._used = start + nbytes
        return _pinned_arena()[start:start + nbytes].view(t.dtype).view(t.shape)

    def __call__(self, a):
        t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        t = t.detach()
        if t.dtype == torch.float64:
            t = t.float()
        if t.is_cuda:                                       # (a view of something already placed)
            return t
        host = self._host(t)
        host.copy_(t)
        dst = self.g._alloc(tuple(t.shape), t.dtype, self.g.device, ga._site(2), "place", False)
        dst.copy_(host, non_blocking=True)
        return dst

    def module(self, m):
        """``m`` with every parameter and buffer staged into a guarded block (no ``m.to``: a pageable copy waits)."""
        with torch.no_grad():
            for t in list(m.parameters()) + list(m.buffers()):
                t.data = self(t.data)
        return m

    @staticmethod
    def ws(n, dtype=torch.float32):
        return torch.empty(max(int(n), 1), dtype=dtype, device=DEV)

    def still_delayed(self):
        """The conclusiveness condition: the DELAY ITSELF (an event recorded right behind it) is still running, and so the
        stream has not drained.  Stricter than ``not side.query()``, which also holds while the last copy is finishing."""
        return not self.delay_end.query() and not self.side.query()


@contextlib.contextmanager
def delayed(side, ms):
    """``side`` current and busy for ``ms`` milliseconds; yields the staging put."""
    cycles = int(cycles_per_ms() * ms)
    _pinned_arena()
    torch.cuda.synchronize()                                # nothing of an earlier case still reads the pinned arena
    g = _NullFillGuard(DEV)
    g._install()
    try:
        with torch.cuda.stream(side):
            torch.cuda._sleep(cycles)
            delay_end = torch.cuda.Event()
            delay_end.record(side)
            yield Staged(g, side, delay_end)
    finally:
        g._remove()


def assert_busy(put, what):
    """The conclusiveness condition (Staged.still_delayed), asserted: right after the call under test has returned."""
    assert put.still_delayed(), (f"{what}: inconclusive -- the delay on the side stream had ended when the call returned (the "
                                 "call synchronised, or the delay was too short), so a launch on another stream could not have shown")
