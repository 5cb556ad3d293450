"""What the tracking timing tools share (track_stream_timing.py, track_events_timing.py, track_history_timing.py):
the walkers scene and the timing loop.  (track_timing.py's walkers are never missed and draw from the generator in
another order: it keeps its own.)"""
import numpy as np
import torch

DT = 0.1  # seconds between frames


def timed(fn, reps, warm=3, windows=5):
    """ms per call: (median, fastest, slowest) over `windows` windows of `reps` calls."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    ms.sort()
    return [round(v, 4) for v in (ms[len(ms) // 2], ms[0], ms[-1])]


def walkers(T, n, seed, miss):
    """(people (T, n, 2), k (T,), side): n walkers in a square of side 0.75 sqrt(n) m, each with its own velocity of
    up to 1.5 m/s plus 0.1 m/s of jitter per frame, reflected at the walls; each left out of a frame with probability
    `miss` (a missed detection); the rows permuted per frame."""
    rng = np.random.default_rng(seed)
    side = 0.75 * np.sqrt(n)
    pos = rng.uniform(0, side, (n, 2))
    vel = rng.uniform(-1.5, 1.5, (n, 2)) / np.sqrt(2)
    out = np.full((T, n, 2), np.nan)
    k = np.empty(T, dtype=np.int64)
    for t in range(T):
        seen = np.flatnonzero(rng.random(n) >= miss)
        seen = seen[rng.permutation(len(seen))]
        k[t] = len(seen)
        out[t, :len(seen)] = pos[seen]
        pos = pos + (vel + rng.normal(0, 0.1, (n, 2))) * DT
        hit = (pos < 0) | (pos > side)
        vel = np.where(hit, -vel, vel)
        pos = np.clip(pos, 0, side)
    return out, k, side
