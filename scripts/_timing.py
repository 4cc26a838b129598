"""The timed windows of the front-end bench scripts: after `warmup` calls, `repeats` windows of
`calls` calls each; (median, min, max) of the milliseconds per call."""
import statistics
import time

import torch


def timed_events(fn, repeats, warmup, calls=1):
    """Device events around each window."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / calls)
    return statistics.median(ms), min(ms), max(ms)


def timed_host(fn, repeats, warmup, calls=1):
    """The host clock around each window, a device synchronisation at its end."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / calls)
    return statistics.median(ms), min(ms), max(ms)
