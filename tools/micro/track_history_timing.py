"""Track history timings on the GPU: 32 frames of 78, 1 024 and 4 096 walkers each
(track_common.py's walkers, every walker left out of a frame with probability 0.1), max_gap = 1, through
  * people_tracking.track_stream + flow_cells alone (the tracking the history follows), in the same visit,
  * people_tracking.track_history on their prev / gap with Z = 0, 8 and 64 zones, outputs allocated and state= given,
  * a device-side torch composition of the same recurrence, frame by frame: a gather of the sources' state per frame
    (on a tracker's links every linked row is an heir, so the composition needs no heir rule).  The composition is
    first checked against the kernel: the integer outputs equal, path equal to within one ulp per hit.

Every figure: HIP events around `reps` back-to-back calls after 3 warm-up calls, 5 windows; the median window's
ms per call is reported with the fastest and slowest.
usage: python tools/micro/track_history_timing.py [reps] [small] [out=FILE]   (small: toy shapes, a rehearsal of the
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

reps = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 20
small = "small" in sys.argv[1:]
if not torch.cuda.is_available():
    sys.exit("track_history_timing.py measures on the GPU: no device visible")
dev = torch.device("cuda:0")
MAX_SPEED, MISS, MAX_GAP = 3.0, 0.1, 1
GATE = MAX_SPEED * DT


def zone_table(n, side, seed):
    """n zones: boxes inside the square, 0.1 to 0.3 of its side wide and high."""
    rng = np.random.default_rng(seed)
    lo = rng.uniform(0, 0.7 * side, (n, 2))
    size = rng.uniform(0.1 * side, 0.3 * side, (n, 2))
    return pt.check_zones(np.column_stack([lo[:, 0], lo[:, 0] + size[:, 0], lo[:, 1], lo[:, 1] + size[:, 1]]))


def composed(people, k, prev, gap, zones):
    """track_history's six outputs from torch operators on the device, a frame at a time: the sources' state is
    gathered from the frames already computed.  Valid where every linked row is an heir (a tracker's links)."""
    T, cap = prev.shape
    Z = 0 if zones is None else zones.shape[0]
    K = k.clamp(0, cap)
    age = torch.empty((T, cap), dtype=torch.int32, device=dev)
    hits = torch.empty((T, cap), dtype=torch.int32, device=dev)
    path = torch.empty((T, cap), dtype=torch.float64, device=dev)
    origin = torch.empty((T, cap, 2), dtype=torch.float64, device=dev)
    stay = torch.empty((T, cap, Z), dtype=torch.int32, device=dev)
    dwell = torch.zeros((T, Z, 3), dtype=torch.int64, device=dev)
    rows = torch.arange(cap, device=dev)
    flat = people.view(-1, 2)
    if Z:
        x0, x1, y0, y1 = zones.unbind(1)
    for t in range(T):
        live = rows < K[t]
        g, i = gap[t].long(), prev[t].long().clamp(0, cap - 1)
        s = (t - g).clamp(0, T - 1)
        linked = live & (prev[t] >= 0) & (g >= 1) & (g <= 8) & (g <= t) & (i < K[s])
        a = s * cap + i
        Q = people[t]
        d = Q - flat[a]
        step = torch.sqrt((d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1]))
        g32 = g.int()
        age[t] = torch.where(linked, age.view(-1)[a] + g32, torch.where(live, 0, -1).int())
        hits[t] = torch.where(linked, hits.view(-1)[a] + 1, live.int())
        path[t] = torch.where(linked, path.view(-1)[a] + step, 0.0)
        origin[t] = torch.where(linked[:, None], origin.view(-1, 2)[a], torch.where(live[:, None], Q, 0.0))
        if Z:
            qx, qy = Q[:, :1], Q[:, 1:]
            inq = (x0 <= qx) & (qx < x1) & (y0 <= qy) & (qy < y1) & live[:, None]
            was = torch.where(linked[:, None], stay.view(-1, Z)[a], -1)
            stay[t] = torch.where(inq, torch.where(was >= 0, was + g32[:, None], 0), -1).int()
            ended = (was >= 0) & ~inq
            length = torch.where(ended, was, 0).long()
            dwell[t] = torch.stack([ended.sum(0), length.sum(0), length.amax(0)], dim=-1)
    return (age, hits, path, origin, stay, dwell) if Z else (age, hits, path, origin, None, None)


def check(out, ref, what):
    """The integer outputs equal; origin equal; path within one ulp per hit."""
    torch.cuda.synchronize()
    for name, a, b in zip(("age", "hits", "path", "origin", "stay", "dwell"), out, ref):
        if a is None and b is None:
            continue
        if name == "path":
            x, y, h = a.cpu().numpy(), b.cpu().numpy(), out[1].cpu().numpy()
            ok = bool(np.all(np.abs(x - y) <= h * np.spacing(np.maximum(x, y))))
        else:
            ok = a.dtype == b.dtype and torch.equal(a, b)
        if not ok:
            sys.exit(f"track_history_timing.py: the torch composition differs from the kernel in {name} at {what}")


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
    for Z in (0, 8, 64):
        zones = torch.from_numpy(zone_table(Z, side, 7 + Z)).to(dev) if Z else None
        out = pt.track_history(people, k, prev, gap, zones)
        check(out, composed(people, k, prev, gap, zones), f"{n} people, Z = {Z}")
        state = out[:5] if Z else out[:4]
        nat.profile(nat.handle(dev.index), True)
        pt.track_history(people, k, prev, gap, zones, state=state)
        spans = {name: round(ms, 4) for name, ms in nat.profile_read(nat.handle(dev.index))}
        nat.profile(nat.handle(dev.index), False)
        ms = timed(lambda: pt.track_history(people, k, prev, gap, zones), reps)
        row[f"zones_{Z}"] = {
            "links": int((prev >= 0).sum()), "walk_starts": int((prev < 0).sum() - (T * n - int(kh.sum()))),
            "completed_stays": int(out[5][:, :, 0].sum()) if Z else 0, "composition_equals_kernel": True,
            "track_history_ms": ms,
            "track_history_state_ms": timed(lambda: pt.track_history(people, k, prev, gap, zones, state=state), reps),
            "share_of_tracking": round(ms[0] / row["track_stream_and_cells_ms"][0], 3),
            "torch_composition_ms": timed(lambda: composed(people, k, prev, gap, zones), reps),
            "spans_ms": spans}
    rows_out.append(row)
    print(json.dumps(row), flush=True)

record = {"library": nat.LIB_PATH, "reps": reps, "dt": DT, "gate": GATE, "miss": MISS, "rows": rows_out}
outs = [a[4:] for a in sys.argv[1:] if a.startswith("out=")]
if outs:
    with open(outs[0], "w") as f:
        json.dump(record, f, indent=1)
