"""Holding a side stream back, for tests of stream ordering (tests/test_gpu_streams.py).  No tests in here.

A stream that is HELD has a long sleep at its head: whatever is enqueued on it afterwards has not started when the host
returns from the enqueue.  An input that arrives LATE holds a poison now and receives its true content by a copy enqueued
on the held stream: an operator that runs on that stream sees the true content; a launch, a memset, a copy or a host read
of the operator's that goes to another stream -- the null stream above all: torch's side streams do not order with it --
sees the poison, or has its own effect overwritten by what the held stream does later, and the result differs.

The poison is always a VALID input of the operator under test (a root of leaves, the empty sentinel, zeros, rays that
miss): a misrouted launch computes a wrong answer, it cannot leave the tables."""
from __future__ import annotations

import torch

_CYCLES_PER_MS: dict = {}       # device index -> cycles of torch.cuda._sleep per millisecond, measured once per session


def _cycles_per_ms(device) -> float:
    idx = torch.device(device).index or 0
    if idx not in _CYCLES_PER_MS:
        assert hasattr(torch.cuda, "_sleep"), "this torch build has no torch.cuda._sleep"
        with torch.cuda.device(idx):
            torch.cuda.synchronize()
            ms, cycles = 0.0, 250_000
            while ms < 2.0:                          # (a sleep long enough to time: at most a few doublings)
                cycles *= 4
                assert cycles < 1 << 36, "torch.cuda._sleep returns at once: it cannot hold a stream"
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                torch.cuda._sleep(cycles)
                e1.record()
                e1.synchronize()
                ms = e0.elapsed_time(e1)
            _CYCLES_PER_MS[idx] = cycles / ms
    return _CYCLES_PER_MS[idx]


_PENDING: dict = {}             # stream handle -> [(destination, staged source)]: the copies the next hold() enqueues behind its sleep


def late(stream, src, poison):
    """A tensor on `stream`'s device that holds `poison` NOW and receives `src` by a copy_ that the next hold(stream)
    enqueues on `stream` behind its sleep.  `src` and `poison`: CPU tensors of one shape and dtype.  Both are put on the
    device here, on the default stream, which is then synchronised: the poison is written and the source staged BEFORE the
    hold begins, so that nothing runs on the default stream while `stream` is held (a side stream may share a hardware queue
    with it, and work on one then waits for the sleep on the other), and nothing but the held stream's own copy_ ever
    writes the tensor again."""
    assert isinstance(src, torch.Tensor) and isinstance(poison, torch.Tensor) and not src.is_cuda and not poison.is_cuda
    assert src.shape == poison.shape and src.dtype == poison.dtype, (src.shape, poison.shape, src.dtype, poison.dtype)
    dev = stream.device
    dst = poison.contiguous().to(dev)
    staged = src.contiguous().to(dev)
    torch.cuda.default_stream(dev).synchronize()
    _PENDING.setdefault(stream.cuda_stream, []).append((dst, staged))
    return dst


def hold(stream, ms: float = 30.0):
    """Enqueue a sleep of about `ms` milliseconds on `stream`, and behind it the copies of every late() tensor made for
    `stream` since the last hold; returns an event recorded right behind the sleep.  While event.query() is False nothing
    enqueued on `stream` after the sleep has started.  30 ms is no tolerance: it only has to outlast the host's enqueue of
    one operator (about a millisecond); callers assert `not event.query()` immediately before the operator and fail with
    "hold too short" otherwise."""
    cycles = int(_cycles_per_ms(stream.device) * ms)
    pending = _PENDING.pop(stream.cuda_stream, [])
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)
        ev = torch.cuda.Event()
        ev.record(stream)
        for dst, staged in pending:
            with torch.no_grad():                    # (a destination may be a leaf that requires grad)
                dst.copy_(staged, non_blocking=True)
            dst.record_stream(stream)
            staged.record_stream(stream)
    return ev


def assert_held(event) -> None:
    """The condition every late-input case checks right before its operator: the hold has not run out."""
    assert not event.query(), "hold too short"
