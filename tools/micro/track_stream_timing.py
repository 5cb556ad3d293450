"""Continuous-tracking timings on the GPU: 32 frames of 78, 1 024 and 4 096 walkers each, every
walker left out of a frame with probability 0.1 (a missed detection), through
  * people_tracking.track_people + flow_cells (the yardstick: §4.9's operator on the same inputs),
  * people_tracking.track_stream(max_gap = 0 / 1 / 2) + flow_cells in one call,
  * the same frames pushed as 4 x 8 through people_tracking.PeopleTracker (max_gap = 0 / 1 / 2, flow cells
    accumulated), a new tracker per repetition,
and the spans of one track_stream call per max_gap (lidar_profile: init, every pass, ids).

Every figure: HIP events around `reps` back-to-back calls after 3 warm-up calls, 5 windows; the median window's
ms per call is reported with the fastest and slowest.  LIDAR_AMD_LIB selects another build of the library
(a build with -DLIDAR_TRACK_GAP_MASKED runs the masked form of the nearest kernel in every pass).
usage: python tools/micro/track_stream_timing.py [reps] [small] [out=FILE]   (small: toy shapes, a rehearsal of
the script; out=FILE: also write the record there)"""
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from lidar_ai_recommendation_software_amd import _native as nat  # noqa: E402
from lidar_ai_recommendation_software_amd import people_tracking as pt  # noqa: E402
from track_common import DT, timed, walkers  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 5
small = "small" in sys.argv[1:]
if not torch.cuda.is_available():
    sys.exit("track_stream_timing.py measures on the GPU: no device visible")
dev = torch.device("cuda:0")
MAX_SPEED, MISS = 3.0, 0.1
GATE = MAX_SPEED * DT

T, PIECE = (4, 2) if small else (32, 8)
rows_out = []
for n in ((20, 300) if small else (78, 1024, 4096)):
    ph, kh, side = walkers(T, n, 40 + n, MISS)
    people, k = torch.from_numpy(ph).to(dev), torch.from_numpy(kh).to(dev)
    xr = yr = (0.0, float(side))

    def pairwise():
        prev, tid, vel, nt = pt.track_people(people, k, DT, GATE)
        return pt.flow_cells(people, k, prev, vel, xr, yr, 1.0)

    def one_call(max_gap):
        prev, gap, succ, vel, tid, nt = pt.track_stream(people, k, DT, GATE, max_gap)
        count, vsum, _ = pt.flow_cells(people, k, prev, vel, xr, yr, 1.0)
        return prev, gap, nt, count, vsum

    def pushed(max_gap):
        tracker = pt.PeopleTracker(DT, GATE, max_gap, xr, yr, 1.0)
        for lo in range(0, T, PIECE):
            tracker.push(people[lo:lo + PIECE], k[lo:lo + PIECE])
        return tracker

    row = {"frames": T, "people": n, "detections": int(kh.sum()), "piece": PIECE,
           "track_people_and_cells_ms": timed(pairwise, reps)}
    for max_gap in (0, 1, 2):
        prev, gap, nt, count, vsum = one_call(max_gap)
        tracker = pushed(max_gap)
        torch.cuda.synchronize()
        same = bool(torch.equal(count, tracker.count) and torch.equal(vsum, tracker.vsum)
                    and int(nt) == int(tracker.ntracks))
        nat.profile(nat.handle(dev.index), True)
        pt.track_stream(people, k, DT, GATE, max_gap)
        spans = {name: round(ms, 4) for name, ms in nat.profile_read(nat.handle(dev.index))}
        nat.profile(nat.handle(dev.index), False)
        row[f"max_gap_{max_gap}"] = {
            "tracks": int(nt), "matched_share": float((prev[1:] >= 0).sum()) / max(1, int(kh[1:].sum())),
            "stitched_share_of_matched": float((gap >= 2).sum()) / max(1, int((prev >= 0).sum())),
            "one_call_ms": timed(lambda: one_call(max_gap), reps), "pushed_ms": timed(lambda: pushed(max_gap), reps),
            "pushed_equals_one_call": same, "spans_ms": spans}
    rows_out.append(row)
    print(json.dumps(row), flush=True)

out = {"library": nat.LIB_PATH, "reps": reps, "dt": DT, "gate": GATE, "miss": MISS, "rows": rows_out}
outs = [a[4:] for a in sys.argv[1:] if a.startswith("out=")]
if outs:
    with open(outs[0], "w") as f:
        json.dump(out, f, indent=1)
