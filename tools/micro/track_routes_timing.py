"""Routes timings on the GPU: 32 frames of 78, 1 024 and 4 096 walkers each (track_common.py's
walkers, every walker left out of a frame with probability 0.1), max_gap = 1, with Z = 8 and 64 zones, through
  * people_tracking.track_stream + flow_cells alone (the tracking the routes follow), in the same visit,
  * people_tracking.track_routes on their prev / gap, outputs allocated and state= / trips= given,
  * people_tracking.track_history on the same links with the same zones, in the same visit: the neighbour, which
    writes 32 + 4 Z bytes per row where the routes write 24,
  * a host walk of the same links (numpy arrays, a Python loop over the rows in (t, j) order), which the kernel's
    outputs are first checked against: on a tracker's links every linked row is an heir.

Every figure: HIP events around `reps` back-to-back calls after 3 warm-up calls, 5 windows; the median window's
ms per call is reported with the fastest and slowest.
usage: python tools/micro/track_routes_timing.py [reps] [small] [out=FILE]   (small: toy shapes, a rehearsal of the
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
from track_common import DT, timed, walkers  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 10
small = "small" in sys.argv[1:]
if not torch.cuda.is_available():
    sys.exit("track_routes_timing.py measures on the GPU: no device visible")
dev = torch.device("cuda:0")
MAX_SPEED, MISS, MAX_GAP = 3.0, 0.1, 1
GATE = MAX_SPEED * DT


def zone_table(n, side, seed):
    """n zones: boxes inside the square, 0.1 to 0.3 of its side wide and high (track_history_timing.py's)."""
    rng = np.random.default_rng(seed)
    lo = rng.uniform(0, 0.7 * side, (n, 2))
    size = rng.uniform(0.1 * side, 0.3 * side, (n, 2))
    return pt.check_zones(np.column_stack([lo[:, 0], lo[:, 0] + size[:, 0], lo[:, 1], lo[:, 1] + size[:, 1]]))


def host_walk(people, k, prev, gap, zones):
    """track_routes' seven outputs on the host, row by row; valid where every linked row is an heir."""
    T, cap = prev.shape
    Z = len(zones)
    x, y = people[:, :, 0, None], people[:, :, 1, None]
    hit = (zones[:, 0] <= x) & (x < zones[:, 1]) & (zones[:, 2] <= y) & (y < zones[:, 3])
    c_of = np.where(hit.any(axis=2), hit.argmax(axis=2), -1)
    out = [np.full((T, cap), v, dtype=np.int32) for v in (-1, -1, -1, 0, -1, 0)]
    first, last, away, legs, leg_from, leg_frames = out
    trips = np.zeros((Z, Z, 3), dtype=np.int64)
    for t in range(T):
        for j in range(min(max(int(k[t]), 0), cap)):
            c, i, g = int(c_of[t, j]), int(prev[t, j]), int(gap[t, j])
            if not (i >= 0 and 1 <= g <= 8 and g <= t and i < k[t - g]):
                first[t, j] = last[t, j] = c
                away[t, j] = 0 if c >= 0 else -1
                continue
            F, L, A, N = (int(a[t - g, i]) for a in (first, last, away, legs))
            if c < 0:
                first[t, j], last[t, j], legs[t, j], away[t, j] = F, L, N, (A + g if L >= 0 else -1)
                continue
            leg = L >= 0 and (L != c or A > 0)
            first[t, j], last[t, j], away[t, j], legs[t, j] = (F if F >= 0 else c), c, 0, N + leg
            if leg:
                leg_from[t, j], leg_frames[t, j] = L, A + g
                trips[L, c] = (trips[L, c, 0] + 1, trips[L, c, 1] + A + g, max(trips[L, c, 2], A + g))
    return out + [trips]


def check(out, want, what):
    torch.cuda.synchronize()
    for name, a, b in zip(pt.ROUTES + ("trips",), out, want):
        if not np.array_equal(a.cpu().numpy(), b):
            sys.exit(f"track_routes_timing.py: the host walk differs from the kernel in {name} at {what}")


T = 4 if small else 32
rows_out = []
for n in ((20, 300) if small else (78, 1024, 4096)):
    ph, kh, side = walkers(T, n, 40 + n, MISS)
    people, k = torch.from_numpy(ph).to(dev), torch.from_numpy(kh).to(dev)
    xr = yr = (0.0, float(side))

    def tracking():
        prev, gap, succ, vel, tid, nt = pt.track_stream(people, k, DT, GATE, MAX_GAP)
        count, vsum, _ = pt.flow_cells(people, k, prev, vel, xr, yr, 1.0)
        return prev, gap

    row = {"frames": T, "people": n, "detections": int(kh.sum()), "max_gap": MAX_GAP,
           "track_stream_and_cells_ms": timed(tracking, reps)}
    prev, gap = tracking()
    for Z in (8, 64):
        table = zone_table(Z, side, 7 + Z)
        zones = torch.from_numpy(table).to(dev)
        out = pt.track_routes(people, k, prev, gap, zones)
        check(out, host_walk(ph, kh, prev.cpu().numpy(), gap.cpu().numpy(), table), f"{n} people, Z = {Z}")
        state, trips = out[:6], out[6]
        nat.profile(nat.handle(dev.index), True)
        pt.track_routes(people, k, prev, gap, zones, state=state, trips=trips)
        spans = {name: round(ms, 4) for name, ms in nat.profile_read(nat.handle(dev.index))}
        nat.profile(nat.handle(dev.index), False)
        ms = timed(lambda: pt.track_routes(people, k, prev, gap, zones), reps)
        hist = timed(lambda: pt.track_history(people, k, prev, gap, zones), reps)
        hstate = pt.track_history(people, k, prev, gap, zones)[:5]
        row[f"zones_{Z}"] = {
            "links": int((prev >= 0).sum()), "walk_starts": int((prev < 0).sum() - (T * n - int(kh.sum()))),
            "legs": int(out[6][:, :, 0].sum()), "returns": int(out[6][:, :, 0].diagonal().sum()),
            "rows_in_a_zone": int((out[2] == 0).sum()), "host_walk_equals_kernel": True,
            "track_routes_ms": ms,
            "track_routes_state_ms": timed(lambda: pt.track_routes(people, k, prev, gap, zones, state=state, trips=trips),
                                           reps),
            "track_history_ms": hist,
            "track_history_state_ms": timed(lambda: pt.track_history(people, k, prev, gap, zones, state=hstate), reps),
            "routes_over_history": round(ms[0] / hist[0], 3),
            "share_of_tracking": round(ms[0] / row["track_stream_and_cells_ms"][0], 3),
            "spans_ms": spans}
    rows_out.append(row)
    print(json.dumps(row), flush=True)

record = {"library": nat.LIB_PATH, "reps": reps, "dt": DT, "gate": GATE, "miss": MISS, "rows": rows_out}
outs = [a[4:] for a in sys.argv[1:] if a.startswith("out=")]
if outs:
    with open(outs[0], "w") as f:
        json.dump(record, f, indent=1)
