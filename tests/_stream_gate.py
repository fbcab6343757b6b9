"""The gate of tests/test_gpu_streams.py: a bounded piece of GPU work queued in
front of a call, so that the call has provably not started while the calls that
compete with it for the context's scratch are enqueued.

A gate is `torch.cuda._sleep` (one thread spinning on the clock for a number of
cycles, calibrated once per process against the stream's own events), never a
wait on something the host writes: a test that dies leaves no stream waiting.
`gate_end` is recorded right behind it; `Gate.open()` -- "the gate is still
running" -- is `not gate_end.query()`.

`run_gated(case)` runs `case(gate_ms)`: once with gate_ms = 0 (no gate: the
context's scratch buffers and staging reach the sizes the case needs, so that
no call of the gated runs blocks on a growth it does not mean to test), then
with the gate.  The case enqueues everything, reads the premise from the host,
synchronises, checks every result against the oracle and returns the premise.
A premise that did not hold (the gate ran out before the competitors were
enqueued) repeats the case with the gate doubled, three gates at the most; then
the test fails."""
import functools
import time

import pytest

# Host time to enqueue the competing calls of a case, measured on an MI355X
# host: 0.04 - 0.11 ms for two calls, 0.11 - 0.16 ms for four, 0.26 - 0.30 ms for
# seven on one stream, and up to 0.86 ms for the four ragged calls of the
# fallback shape (60, 20), which go out as runs of uniform launches.  The first
# gate is ten times the longest.
GATE_MS = 10.0
ATTEMPTS = 3


@functools.lru_cache(maxsize=None)
def _cycles_per_ms():
    """`torch.cuda._sleep` cycles per millisecond, measured on the current device."""
    import torch

    probe = 1_000_000
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = 0.0
    for _ in range(2):  # the first launch loads the kernel
        start.record()
        torch.cuda._sleep(probe)
        end.record()
        end.synchronize()
        ms = start.elapsed_time(end)
    assert ms > 0.01, f"{probe} sleep cycles took {ms} ms"
    return probe / ms


class Gate:
    """`ms` of sleep on `stream`, with `gate_end` recorded behind it.  ms = 0:
    no gate (open() is then False from the start)."""

    def __init__(self, stream, ms):
        import torch

        self.ms = ms
        self.end = torch.cuda.Event()
        cycles = int(ms * _cycles_per_ms()) if ms > 0 else 0  # (the first gate of a process calibrates)
        self.t0 = time.perf_counter()
        with torch.cuda.stream(stream):
            if cycles:
                torch.cuda._sleep(cycles)
            self.end.record()

    def open(self):
        """The gate is still running: nothing queued behind it has started."""
        return not self.end.query()

    def host_ms(self):
        """Host time since the gate was queued."""
        return (time.perf_counter() - self.t0) * 1e3


def run_gated(case, gate_ms=GATE_MS, label="", warm=True):
    """See the module docstring.  `case(gate_ms)` returns (premise, enqueue_ms):
    whether the gate was still running when the last competing call had been
    enqueued, and the host time from the gate to that moment."""
    if warm:
        case(0.0)
    for attempt in range(ATTEMPTS):
        held, enqueue_ms = case(gate_ms)
        print(f"[gate] {label}: gate {gate_ms:g} ms, competitors enqueued after {enqueue_ms:.3f} ms, "
              f"premise {'held' if held else 'MISSED'} (attempt {attempt + 1})")
        if held:
            return
        gate_ms *= 2
    pytest.fail(f"{label}: the gate ran out before the competing calls were enqueued, {ATTEMPTS} times "
                f"(last gate {gate_ms / 2:g} ms)")
