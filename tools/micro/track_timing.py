"""People-tracking timings on the GPU: people_tracking.track_people + flow_cells on 32 frames of
78, 1 024 and 4 096 people each, against a device-side torch composition of the same association: per pair of
frames a float64 torch.cdist, the gated argmin both ways and the mutual test, all on the device, then the
track ids on the host (numpy, after one read-back of prev).  The composition's matches are compared with the
exact ones (cdist takes a square root, and above 25 rows goes through a matrix product: it is not the
specification's arithmetic), and the share of rows that differ is reported; so are the two calls' own spans
(lidar_profile).

Every figure: HIP events around `reps` back-to-back calls after 3 warm-up calls, 5 windows; the median window's
ms per call is reported with the fastest and slowest.  LIDAR_AMD_LIB selects another build of the library.
usage: python tools/micro/track_timing.py [reps] [small] [out=FILE]   (small: toy shapes, a rehearsal of the
script; out=FILE: also write the record there)"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from lidar_ai_recommendation_software_amd import _native as nat  # noqa: E402
from lidar_ai_recommendation_software_amd import people_tracking as pt  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 5
small = "small" in sys.argv[1:]
if not torch.cuda.is_available():
    sys.exit("track_timing.py measures on the GPU: no device visible")
dev = torch.device("cuda:0")
DT, MAX_SPEED = 0.1, 3.0
GATE = MAX_SPEED * DT


def timed(fn, reps=reps, warm=3, windows=5):
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
    return ms[len(ms) // 2], ms[0], ms[-1]


def walkers(T, n, seed):
    """(people (T, n, 2), side): n walkers in a square of side 0.75 sqrt(n) m, each with its own velocity of up
    to 1.5 m/s plus 0.1 m/s of jitter per frame, reflected at the walls; the rows permuted per frame."""
    rng = np.random.default_rng(seed)
    side = 0.75 * np.sqrt(n)
    pos = rng.uniform(0, side, (n, 2))
    vel = rng.uniform(-1.5, 1.5, (n, 2)) / np.sqrt(2)
    out = np.empty((T, n, 2))
    for t in range(T):
        out[t] = pos[rng.permutation(n)]
        pos = pos + (vel + rng.normal(0, 0.1, (n, 2))) * DT
        hit = (pos < 0) | (pos > side)
        vel = np.where(hit, -vel, vel)
        pos = np.clip(pos, 0, side)
    return out, side


def torch_prev(people):
    """The composition: prev (T, n) int64 on the device (every row live), nothing synchronised."""
    T, n, _ = people.shape
    rows = torch.arange(n, device=dev)
    prev = [torch.full((n,), -1, dtype=torch.int64, device=dev)]
    inf = torch.tensor(float("inf"), dtype=torch.float64, device=dev)
    for t in range(1, T):
        D = torch.cdist(people[t - 1], people[t])
        ok = D <= GATE
        Dm = torch.where(ok, D, inf)
        fwd, bwd = torch.argmin(Dm, dim=1), torch.argmin(Dm, dim=0)
        mutual = ok.any(dim=0) & (fwd[bwd] == rows)
        prev.append(torch.where(mutual, bwd, torch.full_like(bwd, -1)))
    return torch.stack(prev)


def host_ids(prev):
    """track ids from prev (T, n) on the host: new detections numbered in (t, j) order, matched rows inherit."""
    ids = np.empty(prev.shape, dtype=np.int64)
    nxt = 0
    for t in range(prev.shape[0]):
        new = prev[t] < 0
        ids[t] = np.where(new, nxt + np.cumsum(new) - 1, ids[t - 1][np.maximum(prev[t], 0)] if t else 0)
        nxt += int(new.sum())
    return ids, nxt


T = 4 if small else 32
rows_out = []
for n in ((20, 300) if small else (78, 1024, 4096)):
    ph, side = walkers(T, n, 40 + n)
    people = torch.from_numpy(ph).to(dev)
    k = torch.full((T,), n, dtype=torch.int64, device=dev)
    xr = yr = (0.0, float(side))

    def ours():
        prev, tid, vel, nt = pt.track_people(people, k, DT, GATE)
        count, vsum, _ = pt.flow_cells(people, k, prev, vel, xr, yr, 1.0)
        return prev, tid, nt, count, vsum

    def composed():
        prev = torch_prev(people)
        return host_ids(prev.cpu().numpy())

    prev_o, tid_o, nt_o, count_o, _ = ours()
    prev_t = torch_prev(people)
    ids_t, nt_t = host_ids(prev_t.cpu().numpy())
    torch.cuda.synchronize()
    differ = float((prev_o.long() != prev_t).double().mean())
    same_ids = bool(differ == 0.0 and np.array_equal(tid_o.cpu().numpy(), ids_t) and int(nt_o) == nt_t)
    nat.profile(nat.handle(dev.index), True)  # the two calls' own spans, one run
    ours()
    spans = {name: round(ms, 4) for name, ms in nat.profile_read(nat.handle(dev.index))}
    nat.profile(nat.handle(dev.index), False)
    rows_out.append({"frames": T, "people": n, "cells": int(count_o.numel()),
                     "matched_share": float((prev_o[1:] >= 0).double().mean()), "tracks": int(nt_o),
                     "track_and_cells_ms": timed(ours), "torch_device_ms": timed(lambda: torch_prev(people)),
                     "torch_with_host_ids_ms": timed(composed), "rows_that_differ": differ,
                     "ids_equal": same_ids, "spans_ms": spans})
    print(json.dumps(rows_out[-1]), flush=True)

out = {"library": nat.LIB_PATH, "reps": reps, "dt": DT, "gate": GATE, "rows": rows_out}
outs = [a[4:] for a in sys.argv[1:] if a.startswith("out=")]
if outs:
    with open(outs[0], "w") as f:
        json.dump(out, f, indent=1)
