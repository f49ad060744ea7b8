"""The timing method the extension benches share (bench_auggrid.py, bench_obb.py, bench_lowp.py): device events around
back-to-back launches, and legs that take turns so that a drift of the machine meets all alike."""
from __future__ import annotations

import numpy as np
import torch


def timed_us(fn, iters: int) -> float:
    """Microseconds per launch: device events around ``iters`` back-to-back launches."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / iters


def take_turns(legs: dict, iters: int, warmup: int, rounds: int) -> dict:
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            times[k].append(timed_us(fn, iters))
    return {k: dict(us=round(float(np.median(v)), 2), us_min=round(min(v), 2), us_max=round(max(v), 2))
            for k, v in times.items()}
