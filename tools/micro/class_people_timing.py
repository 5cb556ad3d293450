"""class_people timings on the GPU: one batched lidar_class_people_f32 call on 32 x 65 536-point
frames with about 30 % of the points in the class, in blob-like clusters, against the composition available
without it, run per frame: boolean mask -> .double() -> lidar_dbscan_f64 -> lidar_people_f64 (both of which
synchronise the stream).  The two results are compared bit for bit, and the batched call's per-phase spans
(lidar_profile) are listed.

Every figure: HIP events around `reps` back-to-back calls after 3 warm-up calls, 5 windows; the median window's
ms per call is reported with the fastest and slowest.  LIDAR_AMD_LIB selects another build of the library.
usage: python tools/micro/class_people_timing.py [reps] [small] [out=FILE]   (small: toy shapes, a rehearsal of
the script; out=FILE: also write the record there)"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from lidar_ai_recommendation_software_amd import _native as nat  # noqa: E402
from lidar_ai_recommendation_software_amd import density_abi as abi  # noqa: E402
from lidar_ai_recommendation_software_amd import pointnet2 as pn  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
small = "small" in sys.argv[2:]
if not torch.cuda.is_available():
    sys.exit("class_people_timing.py measures on the GPU: no device visible")
dev = torch.device("cuda:0")
EPS, MIN_SAMPLES, CLS = 0.3, 5, 1


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


def venue_frames(B, N, seed):
    """(xyz float32 metres, labels int32): a 40 m x 40 m floor; about 30 % of the points on people (class 1:
    blobs of sigma 0.12 m x 0.12 m x 0.45 m around random standing positions), the rest background (class 0:
    floor and clutter), shuffled."""
    rng = np.random.default_rng(seed)
    xs, ls = [], []
    for _ in range(B):
        n_person = int(0.3 * N)
        people = max(4, N // 800)
        centres = np.column_stack([rng.uniform(-20, 20, (people, 2)), np.full(people, 0.9)])
        who = rng.integers(0, people, n_person)
        p = centres[who] + rng.normal(0, 1, (n_person, 3)) * np.array([0.12, 0.12, 0.45])
        bg = np.column_stack([rng.uniform(-20, 20, (N - n_person, 2)), np.abs(rng.normal(0, 0.05, N - n_person))])
        x = np.concatenate([p, bg]).astype(np.float32)
        lab = np.concatenate([np.full(n_person, CLS), np.zeros(N - n_person)]).astype(np.int32)
        perm = rng.permutation(N)
        xs.append(x[perm])
        ls.append(lab[perm])
    return np.stack(xs), np.stack(ls)


B, N = (3, 4096) if small else (32, 65536)
xyz_h, lab_h = venue_frames(B, N, 900)
xyz, labels = torch.from_numpy(xyz_h).to(dev), torch.from_numpy(lab_h).to(dev)
h = nat.handle(dev.index)


def per_frame():
    """The per-frame composition: (instance (B, N) int32, [people (k, 2)], [k])."""
    sp = nat.stream_ptr()
    instance = torch.full((B, N), -1, dtype=torch.int32, device=dev)
    people, ks = [], []
    for f in range(B):
        mask = (labels[f] == CLS) & torch.isfinite(xyz[f]).all(dim=1)
        x = xyz[f][mask].double().contiguous()
        n = x.shape[0]
        lab = torch.empty(n, dtype=torch.int64, device=dev)
        nat.call("lidar_dbscan_f64", h, nat.ptr(x), n, EPS, MIN_SAMPLES, nat.ptr(lab), None, sp)
        p, k = abi.people(h, x, lab, n, sp)
        instance[f][mask] = lab.int()
        people.append(p)
        ks.append(k)
    return instance, people, ks


def batched():
    return pn.class_people(xyz, labels, CLS, EPS, MIN_SAMPLES)


inst_b, people_b, k_b, nsel_b, _ = batched()
inst_p, people_p, k_p = per_frame()
torch.cuda.synchronize()
same = bool(torch.equal(inst_b, inst_p)) and k_b.tolist() == k_p and all(
    people_b[f, :k_p[f]].cpu().numpy().tobytes() == people_p[f].cpu().numpy().tobytes() for f in range(B))

t_b = timed(batched)
t_p = timed(per_frame, reps=max(1, reps // 2))

nat.profile(h, True)
batched()
spans = {}
for name, ms in nat.profile_read(h):
    spans[name] = round(spans.get(name, 0.0) + ms, 4)
nat.profile(h, False)

out = {"library": nat.LIB_PATH, "reps": reps, "B": B, "N": N, "eps": EPS, "min_samples": MIN_SAMPLES,
       "selected_per_frame": [int(v) for v in nsel_b.tolist()][:4], "clusters_per_frame": k_p[:4],
       "batched_ms": t_b, "per_frame_ms": t_p, "ratio": t_p[0] / t_b[0], "bit_identical": same, "spans_ms": spans}
print(json.dumps(out), flush=True)
outs = [a[4:] for a in sys.argv[2:] if a.startswith("out=")]
if outs:
    with open(outs[0], "w") as f:
        json.dump(out, f, indent=1)
if not same:
    sys.exit("the batched call and the per-frame composition differ")
