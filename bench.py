#!/usr/bin/env python3
"""bench.py — M points/s through the PointNet++ SetAbstraction stack on 65 536-point frames.

BASELINE.json metric: "M points/sec through SetAbstraction, 65k-pt frames; 1->8 GPU
scaling".  Workload (configs[2] / configs[3]): the 3-level SSG encoder
(SA1 N/16 r=0.2 ns=32 [64,64,128]; SA2 N/64 r=0.4 ns=64 [128,128,256]; group_all
[256,512,1024]) in fp32 on 65 536-point frames; per GPU a batch of 32 frames — the
per-GPU share of configs[3] (256 frames over 8 GPUs) — so N GPUs process 32*N frames
per step (weak scaling, per-frame data parallel, no collective on the data path).

A step = one 32-frame batch through FPS + ball query + fused group/MLP/max-pool for SA1 and
SA2, then group_all (three MFMA dense layers with a fused max-pool), inputs resident in HBM.
Steps run through pointnet2.StreamingSSG's persistent feed — the steady state of a LiDAR
stream: later batches' SA1 FPS + ball queries (latency-bound, one 512-thread workgroup per
frame) run on `depth` side streams while earlier batches' MFMA levels run on the main stream;
G batches share one FPS launch and one main-stream pass.  The warm-up fills the pipeline
(`depth` groups in flight), then the timed window pushes exactly K batches and completes
exactly K (K a multiple of G): every stage processes K batches of work inside the window.
The input rotates over 8 distinct device-resident batches; with --full every output of warm-up,
window and drain is checked bit for bit against one-batch forward() of its batch.
Synthetic data: uniform [-1, 1]^3 float32 frames (seeded per rank), random-init weights.

Run:  python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]
A plain run does what the headline needs and nothing else: it builds the inputs and the backbone, fills
the pipeline, times the window of K steps, writes the last step's outputs (--dump-outputs) and prints the
line.  --full adds everything else the benchmark measures or checks: the bit-equality check of every
pipeline output against one-batch forward(), the host-frame, native-fp32-MFMA and standalone legs, the
other BASELINE configs, the density / variant / voxel / host-frame legs, the CPU baselines and the
precision check against the oracle (each still has its own --no-... switch under --full).
With --gpus N > 1 and no torch.distributed.run environment, bench.py starts
`python -m torch.distributed.run --nproc-per-node N ... bench.py ...` as a CHILD process (before
anything touches the GPU) and relays its output and exit code; under torch.distributed.run
(WORLD_SIZE set) every rank checks WORLD_SIZE == --gpus.

Output: the LAST stdout line is a compact JSON record (<= LINE_MAX bytes: the driver keeps only
the tail of stdout) with the contract keys, the headline roofline (from the HIP events of the timed
window itself) and the distributed record, and with --full the CPU baseline and the precision check;
the full record (every kernel's roofline and, with --full, the standalone timings and the density /
voxel / host-frame / variant legs) goes to --detail.

--dump-outputs DIR: after the timed window, what its last step returned to the caller (the (B, 1024)
float32 global features of the last batch the window completed) is written to DIR/global_features.npy
(rank r > 0 of an N-rank run: DIR/global_features.rank<r>.npy).  Inputs and weights are seeded, so two
runs with the same arguments write the same array.
"""
import argparse
import hashlib
import json
import os
import platform
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

# MI355X_MICROARCH.md peaks
FP32_MFMA_PEAK_TFLOPS = 157.3   # fp32 matrix (= vector) peak
BF16_MFMA_PEAK_TFLOPS = 2500.0  # bf16 dense matrix peak
# the x3 kernels carry each fp32 product as 3 bf16 MFMA products: their fp32-equivalent peak
X3_PEAK_TFLOPS = BF16_MFMA_PEAK_TFLOPS / 3
FP64_VALU_PEAK_TFLOPS = 78.6
HBM_PEAK_GBS = 8000.0
F64_ADD_LATENCY_CYCLES = 6.3  # dependent v_add_f64, operand in a register (tools/micro/f64_chain.hip)
X3_KERNELS = ("sa1_group_mlp", "sa2_group_mlp", "sa2_layer1_points", "sa3_dense1", "sa3_dense2", "sa3_dense3_pool")


def mlp_flops(rows, widths_in):
    return 2 * rows * sum(a * b for a, b in zip(widths_in[:-1], widths_in[1:]))


def ssg_kernel_work(n):
    """Algorithmic work per FRAME of each kernel of the SSG stack at n points."""
    m1, m2 = n // 16, n // 64
    return {
        "sa1_group_mlp": ("mfma", mlp_flops(m1 * 32, [3, 64, 64, 128])),
        # SA2 layer 1 runs per point (N/16 rows of [f, x] W1 + b1, N/64 centre rows of
        # c W1_xyz); the fused kernel computes layers 2-3 of every grouped row
        "sa2_layer1_points": ("mfma", 2 * m1 * 131 * 128 + 2 * m2 * 3 * 128),
        "sa2_group_mlp": ("mfma", mlp_flops(m2 * 64, [128, 128, 256])),
        "sa3_dense1": ("mfma", mlp_flops(m2, [259, 256])),
        "sa3_dense2": ("mfma", mlp_flops(m2, [256, 512])),
        "sa3_dense3_pool": ("mfma", mlp_flops(m2, [512, 1024])),
        # compulsory bytes: read xyz, write idx + new_xyz
        "sa1_fps": ("hbm", 12 * n + 16 * m1),
        "sa2_fps": ("hbm", 12 * m1 + 16 * m2),
        # read points + centres, write idx (the binning inside the call reads the points once more)
        "sa1_ball_query": ("hbm", 12 * (n + m1) + 4 * m1 * 32),
        # SA1's binning (side stream; the queries run inside sa1_group_mlp): read the points,
        # write the (x, y, z, index) copy and the 16 K-slot table
        "sa1_bq_bin": ("hbm", 12 * n + 16 * n + 4 * 16448),
        "sa2_ball_query": ("hbm", 12 * (m1 + m2) + 4 * m2 * 64),
    }


def stack_mfma_work(cfg, n):
    """Algorithmic MFMA work PER FRAME of every MLP kernel of a PointNet++ stack (`pointnet2` config,
    n points), under the kernel names the backbone's timers use: level 1's grouped branches
    (sa1[_b<i>]_group_mlp, xyz rows), level 2's per-point layer 1 (sa2_layer1_points: N/16 rows of [f, x]
    and N/64 centre rows of c, every branch) and its grouped layers 2-3, group_all's three GEMMs."""
    work = {}
    m = [n // lv["npoint_div"] for lv in cfg["levels"] if not lv.get("group_all")]
    cin = 0
    for li, lv in enumerate(cfg["levels"]):
        if lv.get("group_all"):
            widths = [cin + 3] + lv["mlps"][0]
            for j in range(3):
                work[f"sa{li + 1}_dense{j + 1}" + ("_pool" if j == 2 else "")] = mlp_flops(m[-1], widths[j:j + 2])
            break
        many = len(lv["mlps"]) > 1
        for b, (ns, mlp) in enumerate(zip(lv["nsamples"], lv["mlps"])):
            tag = f"sa{li + 1}" + (f"_b{b}" if many else "")
            if li == 0:
                work[f"{tag}_group_mlp"] = mlp_flops(m[0] * ns, [3] + mlp)
            else:
                work[f"sa{li + 1}_layer1_points"] = (work.get(f"sa{li + 1}_layer1_points", 0)
                                                     + 2 * m[li - 1] * (cin + 3) * mlp[0] + 2 * m[li] * 3 * mlp[0])
                work[f"{tag}_group_mlp"] = mlp_flops(m[li] * ns, mlp)
        cin = sum(mlp[-1] for mlp in lv["mlps"])
    return work


def pick_group(steps, want):
    """Batches per FPS launch: the steady-state window must hold whole groups (every launch
    inside it covers the same number of frames), so G divides K; `want` first, then 3, 4, 5, 2."""
    for g in (want, 3, 4, 5, 2, 1):
        if g >= 1 and steps % g == 0:
            return g
    return 1


def latest_profile(name):
    """The newest profiles/r*/<name> (committed PMC reductions), or None."""
    import glob
    files = sorted(glob.glob(os.path.join(REPO, "profiles", "r*", name)))
    if not files:
        return None
    with open(files[-1]) as f:
        return json.load(f), os.path.relpath(files[-1], REPO)


def pmc_per_frame(N):
    """Memory-side bytes and VALU activity PER FRAME per kernel from the committed PMC passes
    (tools/pmc_traffic.py, tools/pmc_valu.py), when they were taken on this frame size."""
    out = {}
    got = latest_profile("pmc_traffic.json")
    if got and got[0].get("config", {}).get("points_per_frame") == N:
        d, src = got
        fpl = d["config"].get("frames_per_launch", 96)
        for k, v in d.get("kernels", {}).items():
            out.setdefault(k, {})["traffic_per_frame"] = v["traffic_bytes"] / fpl
            out[k]["traffic_source"] = src
    got = latest_profile("pmc_valu.json")
    if got and got[0].get("config", {}).get("points_per_frame") == N:
        d, src = got
        for k, v in d.get("kernels", {}).items():
            out.setdefault(k, {}).update({"valu_issue_frac": v.get("valu_issue_frac"),
                                          "valu_insts_per_frame": v.get("valu_insts_per_frame"), "valu_source": src})
    return out


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            return next(l.split(":", 1)[1].strip() for l in f if l.startswith("model name"))
    except Exception:
        return platform.processor() or platform.machine()


LINE_MAX = 4096  # bytes of the last stdout line (the driver keeps ~8 KB of stdout tail)


def _sig(x, digits=4):
    """Round every float in a JSON-able value to `digits` significant digits."""
    if isinstance(x, float):
        return float(f"{x:.{digits}g}") if np.isfinite(x) else None
    if isinstance(x, dict):
        return {k: _sig(v, digits) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_sig(v, digits) for v in x]
    return x


def compact_line(rec, detail_path=None):
    """The driver-facing line: the contract keys of the full record `rec`, the headline roofline
    and CPU baseline without their long prose, the distributed record, and one number per side
    measurement.  Optional parts are dropped (last first) until the line fits LINE_MAX bytes."""
    keep_roof = ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "work_per_launch",
                 "avg_launch_ms", "launches", "frames", "measured_gbs", "valu_issue_frac")
    line = {k: rec.get(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
                                    "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config")}
    roof = rec.get("roofline") or {}
    line["roofline"] = {k: roof[k] for k in keep_roof if k in roof}
    if roof.get("traffic") is not None:
        line["roofline"]["traffic_basis"] = "HBM-side bytes per launch, rocprofv3 PMC (FETCH_SIZE x2 + WRITE_SIZE)"
    if roof.get("kernel") == "sa1_group_mlp":
        line["roofline"]["note"] = "time includes SA1's ball queries, whose work is not priced"
    gm = rec.get("roofline_grouped_mlp")
    if gm:  # north_star's MFMA figure (SA2 layers 2-3), whichever kernel dominates the window
        line["roofline_grouped_mlp"] = {k: gm[k] for k in ("kernel", "frac", "achieved", "avg_launch_ms") if k in gm}
    cb = rec.get("cpu_baseline")
    line["cpu_baseline"] = None if cb is None else {
        "value": cb["value"], "unit": cb["unit"], "cores": cb["cores"], "kind": cb["kind"], "sample": cb["sample"][:200]}
    line["speedup_vs_cpu"] = rec.get("speedup_vs_cpu")
    if rec.get("ssg_host_feed"):  # the H2D-inclusive rate, reported beside the device-resident value
        line["ssg_host_feed"] = {"value": rec["ssg_host_feed"]["value"], "unit": "M points/s",
                                 "input": "host NumPy frames, PCIe included"}
        lw = rec["ssg_host_feed"].get("long_window")
        if lw:
            line["ssg_host_feed"][f"value_{lw['batches']}_batches"] = round(lw["value"], 1)
    if rec.get("arithmetic_short"):
        line["arithmetic"] = rec["arithmetic_short"]
    bq = (rec.get("roofline_all") or {}).get("sa2_ball_query")
    if bq:
        # north_star asks >= 50 % of HBM on ball_query; the query is a chain of dependent loads
        # (latency-bound), so the target is reported as unmet by design
        line["ball_query_hbm"] = {"kernel": "sa2_ball_query", "frac_compulsory": bq["frac"],
                                  "frac_measured": (bq.get("measured_gbs") or 0) / HBM_PEAK_GBS or None,
                                  "target": 0.5, "met": False, "why": "latency-bound by design"}
    if rec.get("precision") is not None:  # the worst over the checked frames (each frame's own: --detail)
        line["precision"] = {k: v for k, v in rec["precision"].items() if k != "per_frame"}
    d = rec.get("distributed") or {}
    line["distributed"] = {"backend": d.get("backend"), "world_size": d.get("world_size"),
                           "device_count": d.get("device_count"),
                           "ranks": [[r["rank"], r["device"], r["frames"], r["ms"]] for r in d.get("ranks", [])],
                           "ranks_cols": ["rank", "device", "frames", "ms"]}
    optional = []
    pipe = rec.get("pipeline") or {}
    if pipe:
        optional.append(("chains_ms_per_group", {"main": pipe.get("main_ms_per_group"),
                                                 "side": pipe.get("side_ms_per_group"),
                                                 "frames_per_launch": pipe.get("frames_per_launch")}))
    allr = rec.get("roofline_all") or {}
    if allr:
        optional.append(("kernels", {k: [v["avg_launch_ms"], v["frac"]] for k, v in allr.items()}))
        optional.append(("kernels_cols", ["avg_launch_ms", "frac"]))
    legs = {}
    if rec.get("fp32_mfma_kernels"):
        legs["ssg_native_fp32_mfma"] = rec["fp32_mfma_kernels"]["value"]
    for k, v in (rec.get("other_configs") or {}).items():
        legs[k] = v["M_points_per_s"]
        if v.get("chains_ms_per_group"):
            optional.append((f"chains_{k.split('_')[0]}", v["chains_ms_per_group"]))
        if v.get("roofline"):
            r = v["roofline"]
            optional.insert(0, (f"roofline_{k.split('_')[0]}", {x: r[x] for x in (
                "kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "stack_mfma_frac") if x in r}))
    dp_ = rec.get("density_path")
    if dp_:
        legs["density_path_32"] = dp_["value"]
        if dp_.get("wide_batch"):
            legs["density_path_256"] = dp_["wide_batch"]["value"]
        if dp_.get("pipelined_batches"):
            legs["density_path_lanes"] = dp_["pipelined_batches"]["value"]
        if dp_.get("cpu_baseline"):
            legs["density_path_cpu_sklearn"] = dp_["cpu_baseline"]["value"]
        if dp_.get("roofline"):
            legs["density_roofline_frac"] = dp_["roofline"]["frac"]
    if rec.get("voxel_downsample"):
        legs["voxel_downsample"] = rec["voxel_downsample"]["value"]
        legs["voxel_roofline_frac"] = rec["voxel_downsample"]["roofline"]["frac"]
    if rec.get("host_frames"):
        legs["host_frame_feed"] = rec["host_frames"]["host_frame_feed"]["value"]
    if rec.get("variant_path"):
        legs["variant_path"] = rec["variant_path"]["value"]
    if legs:
        optional.append(("legs_M_points_per_s", legs))
    if detail_path:
        optional.insert(0, ("detail", detail_path))
    for k, v in optional:
        line[k] = v
    exact = {k: line[k] for k in ("value", "ms_per_step")}
    line = _sig(line)
    line.update(exact)  # the headline numbers at full precision
    while len(json.dumps(line)) > LINE_MAX and optional:
        line.pop(optional.pop()[0], None)
    if len(json.dumps(line)) > LINE_MAX and line.get("cpu_baseline"):
        line["cpu_baseline"]["sample"] = line["cpu_baseline"]["sample"][:60]
    return line


def launch_ranks(n, argv, script=None):
    """`--gpus N` outside torch.distributed.run: start N ranks of `script` (this file) as a child
    `python -m torch.distributed.run` process on 127.0.0.1, relay its stdout line by line, and
    return its exit code.  The parent never touches the GPU (no exec from a GPU process)."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), script or os.path.abspath(__file__), *argv]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    p = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True, bufsize=1)
    for line in p.stdout:
        sys.stdout.write(line)
        sys.stdout.flush()
    return p.wait()


REL_FLOOR = 1e-2  # pure relative error is reported over elements with |want| >= REL_FLOOR * RMS(want)


def rel_stats(got, want, rtol=1e-4):
    """Tier N's feature contract on one array: the max pure relative error over elements with
    |want| >= REL_FLOOR * RMS, and the max of err / (rtol |want| + rtol RMS) (the tests' feat_close,
    <= 1 passes)."""
    got = np.asarray(got, np.float64).ravel()
    want = np.asarray(want, np.float64).ravel()
    rms = float(np.sqrt(np.mean(want ** 2))) + 1e-30
    err = np.abs(got - want)
    big = np.abs(want) >= REL_FLOOR * rms
    rel = err[big] / np.abs(want[big]) if big.any() else np.zeros(1)
    return {"max_rel": float(rel.max()), "n_rel": int(big.sum()), "n": int(want.size),
            "max_tol_ratio": float((err / (rtol * np.abs(want) + rtol * rms)).max())}


PRECISION_PICKS = tuple((b, 0) for b in range(8)) + ((0, 31), (7, 31))


def precision_check(bb, xs, cfg, n, picks=PRECISION_PICKS):
    """Frames of the bench's input batches (picks: (batch, frame) — the first frame of each of the 8
    rotating 32-frame batches, both groups of the driver's window, and the last frame of the first and
    last batch) through forward(keep_levels) against the fp32 oracle (the checker, in the CPU-baseline
    leg): per level and for the global feature the worst rel_stats over the frames, each frame's own
    numbers beside; FPS indices compared bit for bit."""
    import torch
    from oracle import tier_n
    from lidar_ai_recommendation_software_amd import pointnet2 as pn
    B = xs[0].shape[0]
    picks = [(bi, fi) for bi, fi in picks if bi < len(xs) and fi < xs[bi].shape[0]]
    out = {"contract": "max |got-want|/|want| over |want| >= 1e-2 RMS, and max err/(1e-4|want| + 1e-4 RMS)",
           "frames": [bi * B + fi for bi, fi in picks], "fps_exact": True, "per_frame": {}}
    worst = {}
    done = {}
    for bi, fi in picks:
        if bi not in done:
            done[bi] = bb.forward(xs[bi], keep_levels=True)
            torch.cuda.synchronize()
        g, levels = done[bi]
        x = xs[bi][fi].cpu().numpy()
        want, wl = tier_n.sa_stack(x, {"levels": pn.resolve(cfg, n)}, bb.weights)
        fr = {}
        for li, ((nx, nf, ni, _), (ox, of, oi)) in enumerate(zip(levels, wl)):
            out["fps_exact"] &= bool(np.array_equal(ni[fi].cpu().numpy(), oi))
            fr[f"level{li + 1}"] = rel_stats(nf[fi].cpu().numpy(), of)
        fr["global"] = rel_stats(g[fi].cpu().numpy(), want)
        for k, v in fr.items():
            w = worst.setdefault(k, {"max_rel": 0.0, "max_tol_ratio": 0.0})
            w["max_rel"] = max(w["max_rel"], v["max_rel"])
            w["max_tol_ratio"] = max(w["max_tol_ratio"], v["max_tol_ratio"])
        out["per_frame"][str(bi * B + fi)] = {k: round(v["max_rel"], 9) for k, v in fr.items()}
    out.update(worst)
    return out


def cpu_baseline(n, budget_s=20.0):
    """The oracle SA stack (C FPS / ball query + numpy MLP, BLAS pinned to 1 thread) on
    frames of the same workload, on this host.  kind = "port" (the reference has no
    SetAbstraction code to time)."""
    from threadpoolctl import threadpool_limits
    from oracle import tier_n
    from lidar_ai_recommendation_software_amd import pointnet2 as pn
    from lidar_ai_recommendation_software_amd.synthetic import unit_frames
    cfg = pn.SSG
    w = pn.init_weights(cfg, 0)
    frames, t0 = 0, time.perf_counter()
    with threadpool_limits(limits=1):
        while True:
            x = unit_frames(1, n, 1000 + frames)[0]
            tier_n.sa_stack(x, {"levels": pn.resolve(cfg, n)}, w)
            frames += 1
            if time.perf_counter() - t0 > budget_s or frames >= 64:
                break
    dt = time.perf_counter() - t0
    return {"value": frames * n / dt / 1e6, "unit": "M points/s", "cores": 1, "kind": "port",
            "sample": f"{frames} x {n}-point SSG frame(s) through oracle/tier_n.sa_stack "
                      f"(C FPS + C ball query + numpy fp32 MLP, 1 thread) in {dt:.1f} s on {cpu_model()}; "
                      f"host has {os.cpu_count()} logical CPUs"}


def tier_r_cpu_baseline(n, budget_s=12.0):
    """The reference's density path with the reference's own library calls: oracle/tier_r's
    restatement with scikit-learn's StandardScaler -> DBSCAN(eps, min_samples=5) (the calls at
    utils/data_processing.py:190-197, kd-tree neighbour search), numpy for the rest; falls back
    to the byte-identical C DBSCAN when scikit-learn is not importable."""
    from threadpoolctl import threadpool_limits
    from oracle import tier_r
    from lidar_ai_recommendation_software_amd.synthetic import uniform_frame
    try:
        import sklearn  # noqa: F401
        dbscan = "sklearn"
    except ImportError:
        dbscan = "c"
    frames, t0 = 0, time.perf_counter()
    with threadpool_limits(limits=1):
        while True:
            pd = tier_r.preprocess_lidar_data(uniform_frame(n, 2000 + frames), dbscan=dbscan)
            tier_r.analyze(pd)
            frames += 1
            if time.perf_counter() - t0 > budget_s or frames >= 32:
                break
    dt = time.perf_counter() - t0
    what = ("scikit-learn StandardScaler + DBSCAN(min_samples=5), as the reference calls them"
            if dbscan == "sklearn" else "the C DBSCAN of the same neighbourhood rule (scikit-learn not importable)")
    return {"value": frames * n / dt / 1e6, "unit": "M points/s", "cores": 1, "kind": "port",
            "sample": f"{frames} x {n}-point uniform frame(s) through oracle/tier_r preprocess + analyze "
                      f"({what}; numpy for the rest, 1 thread) in {dt:.1f} s on {cpu_model()}"}


# algorithmic work per input point of the density path's phases: bytes for the
# byte-moving phases, fp64 FLOP for the eps tests (8 per eps-pair: 3 sub, 3 mul, 2 add)
DENSITY_BYTES_PER_POINT = {
    # xyz in (24) + mask (1) + colours, normals, inlier rows (72) + scaled non-ground rows (~0.7 * 24 + 4 pos)
    "preprocess": 24 + 1 + 72 + 21,
    "dbscan_grid": 24 + 4 + 4 + 24 + 4,  # read scaled rows, cell id, order, sorted rows, parent
    "label_scatter": 8 + 4 + 8,
    "people": 16 + 8,
}


def eps_pairs(x):
    """Unordered eps-neighbour pairs DBSCAN's graph has for frame x under preprocess_lidar_data
    (utils/data_processing.py:164-197): the non-ground inliers (z above the 30th percentile),
    standardised, eps from the heuristic; counted on the GPU by radius_count."""
    from lidar_ai_recommendation_software_amd import data_processing as dp
    pts = dp.preprocess_lidar_data(x)["points"]
    ng = pts[pts[:, 2] > np.percentile(pts[:, 2], 30)]
    sc = (ng - ng.mean(axis=0)) / ng.std(axis=0)
    eps = max(0.2, min(0.5, float(np.mean(np.std(sc, axis=0))) * 0.5))
    cnt = dp.radius_count(sc, eps)
    return (int(cnt.sum()) - len(sc)) // 2


def tier_r_leg(dev, rank, world, frames=32, n=65536, steps=3, cpu=True, cpu_budget=12.0, wide=256,
               lanes=int(os.environ.get("LIDAR_DENSITY_LANES", "3"))):
    """The reference's own path (Tier R: preprocess -> DBSCAN -> people -> density grid) on
    device-resident uniform +-15 m frames: batches of `frames` frames through
    density_stream.DensityStream.run_batch (one launch per phase over the CSR batch), with
    per-phase HIP-event durations from the library (lidar_profile) in a second window; then
    the same with `wide` frames per launch (wide_batch)."""
    import torch
    from lidar_ai_recommendation_software_amd import sharding
    from lidar_ai_recommendation_software_amd.density_stream import DensityStream
    from lidar_ai_recommendation_software_amd.synthetic import uniform_frame
    xs = [torch.from_numpy(uniform_frame(n, sharding.frame_seed(rank, base=1000 + i))).to(dev) for i in range(frames)]
    ds = DensityStream(dev)
    ref = ds.run_batch(xs)  # warm-up: workspaces sized
    el = sharding.timed(lambda: [ds.run_batch(xs) for _ in range(steps)], dev, world)
    ds.profile(True)
    for _ in range(steps):
        got = ds.run_batch(xs)
    torch.cuda.synchronize(dev)
    phases = ds.profile_read()
    ds.profile(False)
    assert all(a["total_people"] == b["total_people"] and np.array_equal(a["density_map"], b["density_map"])
               for a, b in zip(ref, got)), "density path not deterministic"
    per_launch_ms = {k: t / c for k, (c, t) in phases.items()}
    dom = max(phases, key=lambda k: phases[k][1])
    pts = frames * n
    rec = {"metric": "M points/s through the reference density path (preprocess + DBSCAN + people + "
                     "density grid), device-resident frames",
           "value": sharding.aggregate_rate(frames * n * steps, world, el) / 1e6, "unit": "M points/s",
           "ms_per_frame": el / (frames * steps) * 1e3, "frames_per_gpu": frames, "points_per_frame": n,
           "executor": "DensityStream.run_batch (CSR batch, one launch per phase)", "dtype": "f64",
           "parity": "byte-identical to the reference (tests/golden)",
           "phase_ms_per_launch": per_launch_ms, "dominant_phase": dom, "cpu_baseline": None}
    if dom.startswith("dbscan"):
        # DBSCAN decides the eps-graph of the scaled non-ground points: SURVEY §8d prices it as
        # 8 fp64 FLOP (3 sub, 3 mul, 2 add) per eps-pair against the FP64 VALU peak.  The pairs are
        # counted exactly on the GPU (radius_count over each frame's scaled non-ground points, the
        # fp64 test DBSCAN uses); the DBSCAN phases together are the "kernel" priced.
        pairs = sum(eps_pairs(x.cpu().numpy()) for x in xs)
        db_ms = sum(v for k, v in per_launch_ms.items() if k.startswith("dbscan"))
        a = 8.0 * pairs / (db_ms / 1e3) / 1e12
        rec["roofline"] = {"kernel": "dbscan (grid + count + union + labels)", "bound": "fp64-valu", "achieved": a,
                           "peak": FP64_VALU_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": a / FP64_VALU_PEAK_TFLOPS,
                           "traffic": None, "work_per_launch": 8.0 * pairs, "eps_pairs_per_frame": pairs / frames,
                           "avg_launch_ms": db_ms,
                           "peak_basis": "FP64 vector peak (FMA counted as 2) over 8 FLOP per eps-pair; the kernels "
                                         "prune most pairs (same-cell shortcut, cell-pair links stop at the first "
                                         "link), so this is work avoided, not work done"}
    elif dom == "preprocess":
        # the preprocess is bound by the dependent fp64 chains numpy's sequential axis-0 sums force
        # (utils/data_processing.py:151-152, :191-194): per frame 4 signed sums of n dependent
        # v_add_f64 plus the two emulated sums of squares (~0.2 of a pass each), one workgroup per
        # frame, all frames of the launch in parallel.  Floor: 4.4 n dependent adds at the measured
        # 6.3-cycle v_add_f64 latency (tools/micro/f64_chain.hip) at 2.4 GHz; frac = floor / achieved
        floor_ns = F64_ADD_LATENCY_CYCLES / 2.4
        ns_row = per_launch_ms["preprocess"] * 1e6 / (4.4 * n)
        rec["roofline"] = {"kernel": "preprocess", "bound": "fp64-add-latency", "achieved": ns_row,
                           "peak": floor_ns, "unit": "ns per dependent row", "frac": floor_ns / ns_row,
                           "traffic": None, "work_per_launch": 4.4 * n, "avg_launch_ms": per_launch_ms["preprocess"],
                           "peak_basis": "one dependent v_add_f64 per row of a sequential sum: 6.3 cycles measured "
                                         "(tools/micro/f64_chain.hip) at 2.4 GHz; 4.4 passes of n rows per frame (4 "
                                         "signed sums + 2 emulated sums of squares at ~0.2 of a pass), frames in "
                                         "parallel (one workgroup each), so the launch time is one frame's chain",
                           "hbm_frac": DENSITY_BYTES_PER_POINT["preprocess"] * pts
                                       / (per_launch_ms["preprocess"] / 1e3) / 1e9 / HBM_PEAK_GBS,
                           # one frame's 65 536-row chain in a 1 024-thread workgroup, wall time
                           # (tools/micro/seq_chain.hip): the dependent adds alone, and fed from LDS
                           # in the kernel's 16-row batches (the form block_seq_chain runs)
                           "in_situ_ns_per_row": {"adds_only": 4.04, "lds_fed": 5.8}}
    elif dom in DENSITY_BYTES_PER_POINT:
        algo = DENSITY_BYTES_PER_POINT[dom] * pts
        a = algo / (per_launch_ms[dom] / 1e3) / 1e9
        rec["roofline"] = {"kernel": dom, "bound": "hbm", "achieved": a, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                           "frac": a / HBM_PEAK_GBS, "traffic": None, "work_per_launch": algo,
                           "avg_launch_ms": per_launch_ms[dom],
                           "peak_basis": "HBM peak over algorithmic bytes; the phase is latency-bound (numpy's "
                                         "sequential axis-0 sums: four dependent fp64 chains per frame plus two "
                                         "sums of squares emulated in parallel, DESIGN.md §2)"}
    if "preprocess" in per_launch_ms:
        # the sequential chains: 4 passes of n dependent fp64 adds per frame (frames in parallel), plus
        # the two emulated sums of squares (~1/5 of a pass each): time per row of one dependent pass
        rec["preprocess_chain_ns_per_row"] = per_launch_ms["preprocess"] * 1e6 / (4.4 * n)
    if wide and wide > frames:
        # the same path with `wide` frames per launch: preprocess and people run one workgroup
        # per frame (sequential chains), so 32 frames leave most CUs idle in those phases
        xw = xs + [torch.from_numpy(uniform_frame(n, sharding.frame_seed(rank, base=1000 + i))).to(dev)
                   for i in range(frames, wide)]
        ds.run_batch(xw)
        elw = sharding.timed(lambda: [ds.run_batch(xw) for _ in range(steps)], dev, world)
        rec["wide_batch"] = {"frames_per_launch": wide,
                             "value": sharding.aggregate_rate(wide * n * steps, world, elw) / 1e6,
                             "unit": "M points/s", "ms_per_launch": elw / steps * 1e3}
        # the same frames as `wide // frames` batches of `frames`, `lanes` batches in flight (round 6, lanes 3 / 4:
        # 663-704 / 602-650 M pts/s on 8 batches of 32 x 65 536 points, profiles/r06/density_lanes_ab.txt: a process
        # has 4 hardware queues, and a fourth lane's stream shares one)
        # (DensityStream.run_batches: a host thread + HIP stream + handle per lane)
        bl = [xw[i:i + frames] for i in range(0, wide, frames)]
        ref_b = ds.run_batches(bl, lanes=lanes)
        elp = sharding.timed(lambda: [ds.run_batches(bl, lanes=lanes) for _ in range(steps)], dev, world)
        got_b = ds.run_batches(bl, lanes=lanes)
        assert all(a["total_people"] == b["total_people"] and np.array_equal(a["density_map"], b["density_map"])
                   for ra, rb in zip(ref_b, got_b) for a, b in zip(ra, rb)), "pipelined batches not deterministic"
        rec["pipelined_batches"] = {"frames_per_launch": frames, "batches_in_flight": lanes, "batches": len(bl),
                                    "value": sharding.aggregate_rate(wide * n * steps, world, elp) / 1e6,
                                    "unit": "M points/s", "ms_per_batch": elp / (steps * len(bl)) * 1e3}
        del xw, bl
    if cpu and rank == 0:
        rec["cpu_baseline"] = tier_r_cpu_baseline(n, cpu_budget)
        rec["speedup_vs_cpu"] = rec["value"] / rec["cpu_baseline"]["value"]
    # SURVEY §8e's optional global density: every frame's people binned into one fixed venue grid
    # per rank, then ONE RCCL all-reduce (int32 sum) over the ranks
    from lidar_ai_recommendation_software_amd.global_density import VenueGrid
    vg = VenueGrid((-15.0, 15.0), (-15.0, 15.0), 1.0, device=dev)
    people = ds.people_of_last_batch()
    vg.add(people)
    gd = {"venue_cells": int(vg.counts.numel()), "people_per_rank": int(people.shape[0])}
    if world > 1:
        # the collective alone: everything queued before it has finished and every rank has arrived
        torch.cuda.synchronize(dev)
        torch.distributed.barrier()
        t0 = time.perf_counter()
        vg.all_reduce()
        torch.cuda.synchronize(dev)
        gd["all_reduce_ms"] = (time.perf_counter() - t0) * 1e3
        gd["collective"] = "torch.distributed all_reduce(int32, SUM) over " + (
            "RCCL" if vg.backend() == "nccl" else vg.backend())
    else:
        gd["collective"] = "none (1 rank: the venue grid is this rank's own)"
    gd["people_all_ranks"] = int(vg.counts.sum().item())
    rec["global_density"] = gd
    return rec


def host_frame_leg(rank, world, frames=16, n=65536, cpu=True, feed_frames=192, feed_batch=32):
    """host frames through the drop-in API — preprocess_lidar_data(numpy) ->
    CrowdDensityModel().analyze -> dict, PCIe included, one frame per call (what app.py does);
    and the same frames through frame_feed.HostFrameFeed (pinned staging, H2D on a copy stream
    overlapped with the previous batch's kernels, one launch per phase per batch)."""
    import torch
    from lidar_ai_recommendation_software_amd import data_processing as dp
    from lidar_ai_recommendation_software_amd.crowd_density_model import CrowdDensityModel
    from lidar_ai_recommendation_software_amd.frame_feed import HostFrameFeed
    from lidar_ai_recommendation_software_amd.synthetic import uniform_frame
    xs = [uniform_frame(n, 7000 + 131 * rank + i) for i in range(max(frames, feed_frames))]
    model = CrowdDensityModel()
    model.analyze(dp.preprocess_lidar_data(xs[0]))  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want = [model.analyze(dp.preprocess_lidar_data(x)) for x in xs[:frames]]
    dt = time.perf_counter() - t0
    # the feed in 32-frame batches, three in flight, over 192 frames (two windows; tools/micro/frame_feed_ab.py,
    # profiles/r06/frame_feed_ab.txt)
    feed = HostFrameFeed(batch=feed_batch)
    feed.run(xs[:feed_batch * feed.lanes])  # warm-up: every lane's pinned buffers, handle and workspaces sized
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = feed.run(xs[:feed_frames])
    dt2 = time.perf_counter() - t0
    assert all(a["total_people"] == b["total_people"] and np.array_equal(a["density_map"], b["density_map"])
               for a, b in zip(want, got)), "HostFrameFeed differs from the drop-in API"
    return {"metric": "M points/s, host numpy frames -> preprocess_lidar_data -> CrowdDensityModel.analyze "
                      "dicts (PCIe-inclusive)",
            "drop_in_per_frame": {"value": frames * n / dt / 1e6, "unit": "M points/s", "ms_per_frame": dt / frames * 1e3},
            "host_frame_feed": {"value": feed_frames * n / dt2 / 1e6, "unit": "M points/s",
                                "ms_per_frame": dt2 / feed_frames * 1e3, "batch": feed_batch, "frames": feed_frames},
            "frames": frames, "points_per_frame": n, "parity": "HostFrameFeed == the drop-in API, frame for frame"}


def voxel_leg(dev, rank, world, B=32, n=65536, voxel=0.05, steps=20, cpu=True):
    """voxel downsampling of the SA batch (B x n uniform frames, device-resident)
    on the chip-wide path (lidar_voxel_downsample_batch_f32).  Roofline: algorithmic bytes per
    launch (12 B per point in + 4 B voxel id out + 16 B per voxel out) over 8 TB/s."""
    import torch
    from lidar_ai_recommendation_software_amd import pointnet2 as pn
    from lidar_ai_recommendation_software_amd.synthetic import unit_frames
    from lidar_ai_recommendation_software_amd import sharding
    x = torch.from_numpy(unit_frames(B, n, seed=sharding.frame_seed(rank, base=77))).to(dev)
    out = pn.voxel_downsample_batch(x, voxel)
    torch.cuda.synchronize(dev)
    # the timed loop leaves nvox on the device (no host read-back per call); checked afterwards
    # a stream of batches: the outputs allocated once and written by every call, nvox left on the device
    # (no host read-back per call) and checked afterwards
    res = tuple(torch.empty_like(t) for t in out)

    def loop():
        for _ in range(steps):
            pn.voxel_downsample_batch(x, voxel, check=False, out=res)

    el = sharding.timed(loop, dev, world)
    pn.check_voxel_counts(res[3])
    assert torch.equal(res[3], out[3]) and torch.equal(res[1], out[1]), "voxel path not deterministic"
    del res
    nv = int(out[3].sum().item())
    per_launch = el / steps
    algo = B * n * 16 + nv * 16
    rec = {"metric": "M points/s through voxel_downsample (batched, device-resident frames)",
           "value": sharding.aggregate_rate(B * n * steps, world, el) / 1e6, "unit": "M points/s",
           "ms_per_launch": per_launch * 1e3, "frames": B, "points_per_frame": n, "voxel": voxel,
           "voxels_per_frame": nv / B, "parity": "bit-exact vs oracle/tier_n.voxel_downsample "
           "(tests/test_gpu_tier_r.py::test_voxel_downsample_batch_vs_oracle)",
           "roofline": {"kernel": "voxel_downsample_batch (2 launches: extents + keys + coarse-bin scatter with "
                                  "in-launch hand-offs; one round of 2048-point buckets: LDS counting sort + "
                                  "look-back + ids / centroids; no memset)", "bound": "hbm",
                        "achieved": algo / per_launch / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": algo / per_launch / 1e9 / HBM_PEAK_GBS, "traffic": None,
                        "work_per_launch": algo, "avg_launch_ms": per_launch * 1e3,
                        "peak_basis": "HBM peak; algorithmic bytes 16 B per point + 16 B per voxel (the two-level "
                                      "sort moves more: traffic)"},
           "cpu_baseline": None}
    got = latest_profile("pmc_voxel.json")
    if got and got[0]["config"].get("points_per_frame") == n and got[0]["config"].get("voxel") == voxel:
        d, src = got
        t = d["traffic_bytes_per_point"] * B * n
        rec["roofline"].update({"traffic": t, "traffic_unit": "bytes per launch (PMC FETCH_SIZE*2 + WRITE_SIZE, "
                                + src + ")", "measured_gbs": t / per_launch / 1e9})
    if cpu and rank == 0:
        from oracle import tier_n
        xs = x[:2].cpu().numpy()
        t0 = time.perf_counter()
        for f in xs:
            tier_n.voxel_downsample(f, voxel)
        dt = time.perf_counter() - t0
        rec["cpu_baseline"] = {"value": len(xs) * n / dt / 1e6, "unit": "M points/s", "cores": 1, "kind": "port",
                               "sample": f"{len(xs)} x {n}-point frame(s) through oracle/tier_n.voxel_downsample "
                                         f"(C keys + numpy unique + the sequential sums) in {dt:.1f} s"}
    return rec


def variant_leg(rank, world, frames=8, n=65536, cpu=True, cpu_budget=6.0):
    """the Streamlit apps' own pipeline (app_simplified.py:76-137 ->
    :234-316, DBSCAN eps 0.3 on unscaled points + KDTree r = 2 cell counts) through the
    drop-in API, host NumPy frame in -> host dicts out (PCIe included), crowd frames."""
    import torch
    from lidar_ai_recommendation_software_amd import variant_pipeline as vp
    from lidar_ai_recommendation_software_amd.synthetic import crowd_frame
    xs = [crowd_frame(n, 500 + 97 * rank + i) for i in range(frames)]
    vp.analyze_crowd_density(vp.preprocess_point_cloud(xs[0]))  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for x in xs:
        vp.analyze_crowd_density(vp.preprocess_point_cloud(x))
    dt = time.perf_counter() - t0
    rec = {"metric": "M points/s through app_simplified.py's preprocess_point_cloud + analyze_crowd_density "
                     "(drop-in API, host frames in / dicts out, one frame per call)",
           "value": frames * n / dt / 1e6, "unit": "M points/s", "ms_per_frame": dt / frames * 1e3,
           "points_per_frame": n, "frames": frames, "data": "synthetic crowd frames (people clumps, metres)",
           "parity": "byte-identical to scikit-learn's DBSCAN / KDTree results (tests/golden/variant.json)",
           "cpu_baseline": None}
    if cpu and rank == 0:
        from oracle import tier_r
        k, t0 = 0, time.perf_counter()
        while True:
            tier_r.variant_analyze_crowd_density(tier_r.variant_preprocess_point_cloud(xs[k % frames]))
            k += 1
            if time.perf_counter() - t0 > cpu_budget or k >= frames:
                break
        dtc = time.perf_counter() - t0
        rec["cpu_baseline"] = {"value": k * n / dtc / 1e6, "unit": "M points/s", "cores": 1, "kind": "port",
                               "sample": f"{k} x {n}-point crowd frame(s) through oracle/tier_r's variant "
                                         f"restatement (numpy + the C DBSCAN, 1 thread) in {dtc:.1f} s"}
        rec["speedup_vs_cpu"] = rec["value"] / rec["cpu_baseline"]["value"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=240,
                    help="timed steps (32-frame batches) of the steady-state window")
    ap.add_argument("--warmup", type=int, default=3, help="warm-up groups beyond the pipeline fill")
    ap.add_argument("--batch", type=int, default=32, help="frames per GPU per step")
    ap.add_argument("--points", type=int, default=65536)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-budget", type=float, default=12.0, help="seconds of CPU work per baseline sample")
    ap.add_argument("--depth", type=int, default=3, help="side streams (SA1-FPS groups in flight ahead of the MLPs)")
    ap.add_argument("--fps-group", type=int, default=3,
                    help="batches per SA1-FPS launch (StreamingSSG fps_group); must divide --steps, else the "
                         "nearest of 3, 4, 5, 2 that does")
    ap.add_argument("--fps-threads", type=int, default=512, choices=[512, 1024],
                    help="SA1 FPS workgroup size in the pipeline (512: half the CU footprint beside the MLPs)")
    ap.add_argument("--x3", type=int, default=1,
                    help="1: MLPs on the split-bf16 (x3) kernels, fp32 arithmetic within the 1e-4 contract; "
                         "0: the native fp32-MFMA kernels")
    ap.add_argument("--slots", type=int, default=0,
                    help="StreamingSSG staging slots (0: its default, depth + 3)")
    ap.add_argument("--bq", default="bin", choices=["side", "bin", "main"],
                    help="SA1 ball queries (StreamingSSG bq): binning on the FPS side streams and the queries "
                         "inside the SA1 MLP kernel (bin), both on the main stream (main), or binning + a "
                         "query launch on the side streams (side)")
    ap.add_argument("--l2-side", type=int, default=1,
                    help="1: SA2's nested FPS and ball queries on the side streams as well (StreamingSSG l2_side; "
                         "1 213-1 227 vs 1 195-1 207 M pts/s in one A/B); 0: on the main stream")
    ap.add_argument("--rotate", type=int, default=8, help="distinct device-resident input batches the feed cycles over")
    ap.add_argument("--hw-queues", type=int, default=0,
                    help="GPU_MAX_HW_QUEUES for this process (HIP's hardware queues per priority level; 0: leave "
                         "the environment's, HIP's default 4); set before HIP initialises")
    ap.add_argument("--no-fp32-mfma-leg", action="store_true",
                    help="skip the extra measurement of the native fp32-MFMA kernels (when --x3 is on)")
    ap.add_argument("--no-standalone", action="store_true",
                    help="skip the standalone (no pipeline) kernel timings of one 96-frame forward()")
    ap.add_argument("--msg-batch", type=int, default=32,
                    help="frames per GPU per step of the configs[4] MSG leg (32: the per-GPU share of 256 frames)")
    ap.add_argument("--msg-steps", type=int, default=30)
    ap.add_argument("--msg-group", type=int, default=3, help="configs[4] leg: batches per SA1-FPS launch")
    ap.add_argument("--cfg1-group", type=int, default=8,
                    help="configs[1] leg: batches per SA1-FPS launch (16 384-point frames: 8 measured 2 678-2 751 "
                         "vs 2 262-2 297 M points/s at 4, tools/micro/cfg1_ab.py)")
    ap.add_argument("--msg-depth", type=int, default=3, help="configs[4] leg: side streams")
    ap.add_argument("--no-layer1-fuse", action="store_true",
                    help="configs[4] leg: one per-point layer-1 GEMM per branch (pointnet2.FUSE_LAYER1 off)")
    ap.add_argument("--msg-fps-threads", type=int, default=0, choices=[0, 512, 1024],
                    help="configs[4] leg: SA1 FPS workgroup size (0: --fps-threads)")
    ap.add_argument("--no-host-feed", action="store_true", help="skip the host-frame (PCIe-inclusive) SSG leg")
    ap.add_argument("--host-threads", type=int, default=4, help="host-frame leg: threads filling the pinned ring (4: 1 062-1 083, 8: 1 011-1 053, 16: 998-1 057 M points/s in one A/B)")
    ap.add_argument("--no-extras", action="store_true", help="skip the configs[1]/[4] side measurements")
    ap.add_argument("--no-density", action="store_true", help="skip the Tier R / variant / voxel / host-frame legs")
    ap.add_argument("--seed-rank", type=int, default=None,
                    help="generate the frames of this rank (a 1-process run reproducing one rank of an N-rank run)")
    ap.add_argument("--dump", default=None,
                    help="write this rank's output digests (of the forward() references: with --full) to "
                         "DUMP.rank<r>.json")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed step returned (the global features of "
                         "the last batch the window completed, float32) to DIR/global_features.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beside the headline window: the bit-equality check against forward(), "
                         "the host-feed / fp32-MFMA / standalone legs, the other configs, the density legs, the CPU "
                         "baselines and the precision check (a plain run skips them all)")
    ap.add_argument("--no-verify", action="store_true",
                    help="skip the one-batch forward() references and the bit-equality check of every pipeline "
                         "output (PMC passes: only the pipeline's own launches are then counted)")
    ap.add_argument("--detail", default=os.path.join(REPO, "gpurun_out", "bench_detail.json"),
                    help="file for the full record (rank 0); the last stdout line is the compact one")
    args = ap.parse_args()
    if not args.full:
        # a plain run: the headline window alone
        args.no_verify = args.no_host_feed = args.no_fp32_mfma_leg = args.no_standalone = True
        args.no_extras = args.no_density = args.no_cpu_baseline = True

    if args.hw_queues:
        os.environ["GPU_MAX_HW_QUEUES"] = str(min(32, max(1, args.hw_queues)))
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # N ranks, one per GPU: a child torch.distributed.run, started before any GPU call
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))
    if int(os.environ.get("WORLD_SIZE", "1")) != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={os.environ.get('WORLD_SIZE', '1')}")

    import torch
    import torch.distributed as dist
    from lidar_ai_recommendation_software_amd import pointnet2 as pn
    from lidar_ai_recommendation_software_amd import sharding
    from lidar_ai_recommendation_software_amd.synthetic import unit_frames

    rank, world, local = sharding.world_info()
    dev = torch.device("cuda", sharding.init_distributed(world, local))
    torch.cuda.set_device(dev)
    seed_rank = rank if args.seed_rank is None else args.seed_rank

    B, N = args.batch, args.points
    G = pick_group(args.steps, args.fps_group)
    digests = {}
    last_out = {}  # per leg: what the last step of its timed window returned
    local_ms = {}  # this rank's own window time per leg (the line reports the max over ranks)

    def measure(key, cfg, dtype, B, N, steps, warmup, depth, G, x3=True, events=True,
                host=False, bb=None, xs=None, refs=None, fps_threads=None):
        """Steady-state window of `steps` batches through StreamingSSG's feed.  events: HIP
        events around every launch inside the timed window (the headline: the roofline durations
        come from the same window); False: the window runs clean and the per-kernel durations come
        from a second window of the same length (with ~25 launches per step, as MSG has, the
        events cost ~1/3).  host: the batches enter as host NumPy frames through feed().push_host
        (pinned staging, the device copy on the side streams: PCIe-inclusive), reusing the device
        leg's backbone, batches and references."""
        bb = bb or pn.PointNet2Backbone(cfg, device=dev, seed=0, dtype=dtype, x3=x3)
        nb = max(1, args.rotate)
        if xs is None:
            xs = [torch.from_numpy(unit_frames(B, N, seed=sharding.frame_seed(seed_rank, step=i))).to(dev)
                  for i in range(nb)]
        # one-batch forward(): what every pipeline output must equal (--no-verify: not issued, so a
        # counter pass sees only the pipeline's launches)
        if refs is None and not args.no_verify:
            refs = [bb.forward(x)[0] for x in xs]
        hxs = [x.cpu().numpy() for x in xs] if host else None
        ready = torch.cuda.Event()  # the inputs exist: the feed's FPS launches wait only for their slots
        ready.record()
        pipe = pn.StreamingSSG(bb, B, N, depth=depth, fps_group=G, fps_threads=fps_threads or args.fps_threads,
                               ramp=False,
                               slots=args.slots or None, bq=args.bq,
                               l2_side=bool(args.l2_side))
        feed = pipe.feed()
        push = ((lambda i: feed.push_host(hxs[i % nb], threads=args.host_threads)) if host
                else (lambda i: feed.push(xs[i % nb], ready)))
        nwarm = (depth + max(1, warmup)) * G  # whole groups; `depth` groups in flight when the window opens
        outs = []
        for i in range(nwarm):
            outs += push(i)
        timers = pn._Timers()
        win = []

        def window(i0, sink):
            for i in range(i0, i0 + steps):
                sink.extend(push(i))

        if events:
            bb.timers = timers
            elapsed, local = sharding.timed_detail(lambda: window(nwarm, win), dev, world)  # max over ranks
            bb.timers = None
            outs += win
            i_end = nwarm + steps
        else:
            elapsed, local = sharding.timed_detail(lambda: window(nwarm, win), dev, world)
            outs += win
            bb.timers = timers
            win2 = []
            window(nwarm + steps, win2)
            bb.timers = None
            outs += win2
            i_end = nwarm + 2 * steps
        assert len(win) == steps, f"window completed {len(win)} batches, expected {steps}"
        outs += feed.flush()
        torch.cuda.synchronize(dev)
        assert len(outs) == i_end, (len(outs), i_end)
        if refs is not None:
            bad = [i for i, o in enumerate(outs) if not torch.equal(o, refs[i % nb])]
            assert not bad, f"{key}: streaming outputs differ from forward() for batches {bad[:5]}"
            digests[key] = [hashlib.sha256(r.cpu().numpy().tobytes()).hexdigest() for r in refs]
        local_ms[key] = local * 1e3
        last_out[key] = win[-1]
        return elapsed, timers.totals(), bb, xs, refs

    tot_x3 = None
    pn.FUSE_LAYER1 = not args.no_layer1_fuse
    elapsed, tot, bb, xs, refs = measure("ssg", pn.SSG, "f32", B, N, args.steps, args.warmup, args.depth, G,
                                         x3=bool(args.x3))
    if args.dump_outputs:
        os.makedirs(args.dump_outputs, exist_ok=True)
        name = "global_features" + (f".rank{rank}" if rank else "") + ".npy"
        np.save(os.path.join(args.dump_outputs, name), last_out["ssg"].cpu().numpy().astype(np.float32, copy=False))
    host_feed = None
    if not args.no_host_feed:
        # the same workload entering as host NumPy frames (PCIe-inclusive: pinned staging by host threads,
        # the device copy on the side streams); outputs checked against the same forward() references
        el_h, _, _, _, _ = measure("ssg_host", pn.SSG, "f32", B, N, args.steps, args.warmup, args.depth, G,
                                   x3=bool(args.x3), events=False, host=True, bb=bb, xs=xs, refs=refs)
        host_feed = {"value": sharding.aggregate_rate(B * N * args.steps, world, el_h) / 1e6, "unit": "M points/s",
                     "ms_per_step": el_h / args.steps * 1e3,
                     "input": f"host NumPy (B, N, 3) float32 batches -> feed().push_host ({args.host_threads} host threads "
                              "into a pinned ring, H2D on the side streams ahead of each group's FPS)",
                     "parity": "every output bit-equal to forward() of the same batch"}
        if args.steps < 80:
            # the same feed over a longer window as well: the host feed pays more of its start than the device
            # one does within a short window
            n_long = G * -(-80 // G)
            el_l, _, _, _, _ = measure("ssg_host_long", pn.SSG, "f32", B, N, n_long, args.warmup, args.depth, G,
                                       x3=bool(args.x3), events=False, host=True, bb=bb, xs=xs, refs=refs)
            host_feed["long_window"] = {"batches": n_long, "value": sharding.aggregate_rate(B * N * n_long, world,
                                                                                            el_l) / 1e6}
    fp32_mfma = None
    if args.x3 and not args.no_fp32_mfma_leg:
        # the same workload on the native fp32-MFMA kernels (clean window), for comparison
        el_f, t_f, _, _, _ = measure("ssg_fp32_mfma", pn.SSG, "f32", B, N, args.steps, args.warmup, args.depth, G,
                                  x3=False, events=False)
        fp32_mfma = {"value": sharding.aggregate_rate(B * N * args.steps, world, el_f) / 1e6, "unit": "M points/s",
                     "ms_per_step": el_f / args.steps * 1e3,
                     "kernel_ms_per_launch": {k: t / c for k, (c, f, t) in t_f.items()}}
    standalone = None
    if not args.no_standalone:
        # the kernels alone: one forward() over a group's frames (G*B), nothing else on the chip
        xg = torch.cat(xs[:G])
        bb.forward(xg)
        torch.cuda.synchronize(dev)
        st = pn._Timers()
        bb.timers = st
        for _ in range(3):
            bb.forward(xg)
        torch.cuda.synchronize(dev)
        bb.timers = None
        standalone = st.totals()
        # SA1's fused kernel answers its ball queries itself; the same MLP on precomputed indices (the
        # separate grid query, then lidar_sa_group_mlp_x3 over the index tensor) decomposes its time
        lvl0 = bb.levels[0]["branches"][0]
        fz1 = torch.empty(xg.shape[0], dtype=torch.int32, device=dev)
        idx1, nx1 = pn.farthest_point_sample(xg, N // bb.levels[0]["div"], return_xyz=True, first_zero=fz1)
        st2 = pn._Timers()
        bb.timers = st2
        for _ in range(3):
            gidx1 = pn._call(st2, "sa1_ball_query", xg.shape[0], pn.ball_query, lvl0["r"], lvl0["ns"], xg, nx1)
            bb.forward_from_sa1_fps(xg, idx1, nx1, fz1, gidx1=[gidx1])
        torch.cuda.synchronize(dev)
        bb.timers = None
        t2 = st2.totals()
        standalone["sa1_group_mlp_given_idx"] = t2["sa1_group_mlp"]
        standalone["sa1_ball_query_separate"] = t2["sa1_ball_query"]
        del xg, idx1, nx1, fz1, gidx1
    extras = {}
    if not args.no_extras:
        # the other BASELINE.json configs, measured the same way (not the headline metric)
        legs = [("configs[1]_sa1_16k_f32", pn.SA1_ONLY, "f32", 32, 16384, 40),
                ("configs[4]_msg_131k_bf16", pn.MSG, "bf16", args.msg_batch, 131072, args.msg_steps)]
        for key, cfg, dtype, b2, n2, st2 in legs:
            msg = cfg is pn.MSG
            g2 = pick_group(st2, args.msg_group if msg else args.cfg1_group)
            d2 = args.msg_depth if msg else 3
            el2, t2, _, _, _ = measure(key, cfg, dtype, b2, n2, st2, 1, d2, g2, events=False,
                                       fps_threads=(args.msg_fps_threads or None) if msg else None)
            pl2 = {k: t / c for k, (c, f, t) in t2.items()}
            # the two chains per group: the side streams' FPS / binning / queries (3 streams) and the
            # main stream's MLP kernels, from the per-launch HIP-event durations of the second window
            side_k = [k for k in pl2 if k.endswith("_fps") or "_bq_bin" in k or "_ball_query" in k]
            extras[key] = {"M_points_per_s": sharding.aggregate_rate(b2 * n2 * st2, world, el2) / 1e6,
                           "ms_per_step": el2 / st2 * 1e3, "frames_per_gpu": b2, "points_per_frame": n2,
                           "dtype": dtype, "batches_per_group": g2, "side_streams": d2,
                           "chains_ms_per_group": {"main": sum(v for k, v in pl2.items() if k not in side_k),
                                                   "side": sum(pl2[k] for k in side_k) / d2,
                                                   "step_ms_per_group": el2 / st2 * 1e3 * g2},
                           "kernel_ms_per_launch": pl2}
            mw = stack_mfma_work(cfg, n2)
            mk = {k: v for k, v in t2.items() if k in mw}
            if mk:
                # the leg's dominant MFMA kernel (most device time), priced on the dense peak of its
                # arithmetic: bf16 (X1 kernels, one bf16 product per MFMA) or h3 (fp32 contract)
                dk = max(mk, key=lambda k: mk[k][2])
                c, f, ms = mk[dk]
                peak = BF16_MFMA_PEAK_TFLOPS if dtype == "bf16" else X3_PEAK_TFLOPS
                ach = mw[dk] * f / (ms / 1e3) / 1e12
                extras[key]["roofline"] = {
                    "kernel": dk, "bound": "mfma", "achieved": ach, "peak": peak, "unit": "TFLOP/s", "frac": ach / peak,
                    "traffic": None, "work_per_launch": mw[dk] * f / c, "avg_launch_ms": ms / c, "launches": c,
                    "frames": f, "peak_basis": "bf16 MFMA dense peak" if dtype == "bf16" else "bf16 dense peak / 3 (h3)",
                    "stack_mfma_frac": sum(mw[k] * v[1] for k, v in mk.items()) / (sum(v[2] for v in mk.values()) / 1e3)
                                       / 1e12 / peak}
                got = latest_profile("pmc_traffic_msg.json" if msg else "pmc_traffic_cfg1.json")
                if got and got[0]["config"].get("points_per_frame") == n2 and dk in got[0]["kernels"]:
                    tpf = got[0]["kernels"][dk]["traffic_per_frame"]  # memory-side bytes per frame (PMC)
                    r4 = extras[key]["roofline"]
                    r4["traffic"] = tpf * f / c
                    r4["traffic_unit"] = "bytes per launch (PMC FETCH_SIZE*2 + WRITE_SIZE, " + got[1] + ")"
                    r4["measured_gbs"] = r4["traffic"] / (ms / c / 1e3) / 1e9

    density = variant = voxel = host = None
    if not args.no_density:
        cpu = not args.no_cpu_baseline
        density = tier_r_leg(dev, seed_rank, world, cpu=cpu, cpu_budget=args.cpu_budget)
        variant = variant_leg(seed_rank, world, cpu=cpu)
        voxel = voxel_leg(dev, seed_rank, world, cpu=cpu)
        host = host_frame_leg(seed_rank, world, cpu=cpu)
    work = ssg_kernel_work(N)
    pmc = pmc_per_frame(N)

    def sa1_split(totals):
        """The fused SA1 kernel's time (ball queries + MLP, standalone) against the same MLP on
        precomputed indices: the difference is what answering the queries costs inside it."""
        if not totals or "sa1_group_mlp_given_idx" not in totals:
            return None
        f_l, f_f, f_ms = totals["sa1_group_mlp"]
        m_l, m_f, m_ms = totals["sa1_group_mlp_given_idx"]
        q_l, q_f, q_ms = totals["sa1_ball_query_separate"]
        per_frame = work["sa1_group_mlp"][1]
        return {"fused_ms_per_launch": f_ms / f_l, "mlp_given_idx_ms_per_launch": m_ms / m_l,
                "query_ms_inside_fused": f_ms / f_l - m_ms / m_l, "separate_query_ms_per_launch": q_ms / q_l,
                "frames_per_launch": f_f / f_l, "mlp_only_frac": per_frame * m_f / (m_ms / 1e3) / 1e12 / X3_PEAK_TFLOPS,
                "fused_frac": per_frame * f_f / (f_ms / 1e3) / 1e12 / X3_PEAK_TFLOPS,
                "basis": "one forward() over a group's frames, nothing else on the chip; the MLP on given indices "
                         "is lidar_sa_group_mlp_x3 over the (B, M, 32) index tensor of the separate grid query"}

    def roof(name, totals):
        """Roofline of one kernel over the launches `totals` recorded: achieved = the algorithmic
        work of all frames those launches processed / the sum of their durations (so frac = Σwork /
        Σtime / peak by construction, whatever the frames per launch)."""
        bound, per_frame = work[name]
        launches, frames, ms = totals[name]
        s = ms / 1e3
        w_total = per_frame * frames
        if bound == "mfma":
            x3k = bool(args.x3) and name in X3_KERNELS
            a, p, u = w_total / s / 1e12, X3_PEAK_TFLOPS if x3k else FP32_MFMA_PEAK_TFLOPS, "TFLOP/s"
            basis = ("bf16 MFMA dense peak / 3 (x3: 3 bf16 products per fp32 product)" if x3k else "fp32 MFMA peak")
        else:
            a, p, u = w_total / s / 1e9, HBM_PEAK_GBS, "GB/s"
            basis = "HBM peak over compulsory bytes"
        if name == "sa1_group_mlp" and args.bq in ("bin", "main"):
            basis += "; the kernel also answers SA1's ball queries (lidar_sa_group_mlp_bq_f32), whose time is " \
                     "included and whose work is not priced"
        r = {"kernel": name, "bound": bound, "achieved": a, "peak": p, "unit": u, "frac": a / p,
             "traffic": None, "work_per_launch": w_total / launches, "avg_launch_ms": ms / launches,
             "launches": launches, "frames": frames, "total_ms": ms, "peak_basis": basis}
        pm = pmc.get(name, {})
        if "traffic_per_frame" in pm:
            r["traffic"] = pm["traffic_per_frame"] * frames / launches
            r["traffic_unit"] = "bytes per launch (PMC FETCH_SIZE*2 + WRITE_SIZE, " + pm["traffic_source"] + ")"
            r["measured_gbs"] = r["traffic"] / (ms / launches / 1e3) / 1e9
        if pm.get("valu_issue_frac") is not None:
            # VALU-throughput roofline: 2 SIMD cycles per wave64 VALU instruction over all SIMD-cycles
            # of the dispatch alone (PMC pass, tools/pmc_valu.py)
            r["valu_issue_frac"] = pm["valu_issue_frac"]
            r["valu_source"] = pm["valu_source"]
        return r

    # Two chains per group of batches: the side streams' SA1 FPS + ball queries (`depth` groups
    # in flight; FPS is one workgroup per frame, latency-bound: read as us/step) and the main
    # stream's full-chip kernels.  The roofline is reported for the kernel that dominates the
    # main chain's device time; the chain lengths say which chain bounds a step.
    side = ("sa1_fps", "sa1_ball_query", "sa1_bq_bin") if args.bq == "side" else ("sa1_fps", "sa1_bq_bin")
    if args.l2_side:
        side = side + ("sa2_fps", "sa2_ball_query")
    per_launch = {k: t / c for k, (c, f, t) in tot.items()}
    main_k = {k: v for k, v in per_launch.items() if k not in side}
    side_ms = sum(per_launch.get(k, 0) for k in side) / args.depth
    main_ms = sum(main_k.values())
    dom = max((k for k in main_k if k in work), key=lambda k: tot[k][2])
    chains = {"side_ms_per_group": side_ms, "main_ms_per_group": main_ms,
              "bound_by": "side (SA1 FPS latency)" if side_ms > main_ms else "main (MFMA levels)",
              "sa1_fps_us_per_step": per_launch.get("sa1_fps", 0) * 1e3 / max(1, N // 16)}

    value = sharding.aggregate_rate(B * N * args.steps, world, elapsed) / 1e6
    # what the process group saw (backend, ranks, GPUs) and each rank's own frames and window time:
    # an N-GPU line shows by itself that RCCL ran N ranks, one per GPU
    group = sharding.group_report(dev, world, B * args.steps, local_ms["ssg"] / 1e3)
    sharding.check_backend(world, group["backend"], group["device_count"])
    if args.dump:
        with open(f"{args.dump}.rank{rank}.json", "w") as f:
            json.dump({"rank": rank, "seed_rank": seed_rank, "world": world, "digests": digests,
                       "value": value, "ms_per_step": elapsed / args.steps * 1e3}, f)
    if rank == 0:
        rec = {
            "metric": "M points/sec through SetAbstraction, 65k-pt frames; 1->8 GPU scaling",
            "value": value, "unit": "M points/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32",
            "arithmetic": ("fp32 inputs/weights/outputs; SA layers 2-3, SA2's per-point layer 1 and group_all in h3 "
                           "arithmetic: each fp32 operand scaled by a power of two and split exactly into fp16 hi+lo, "
                           "products ah*bh + ah*bl + al*bh accumulated in fp32 (<= 3*2^-22 per product, csrc/h3.hpp); "
                           "layer-1 xyz terms on fp32 MFMA; features within 1e-4 pure relative of the fp32 oracle on "
                           "every element >= 1e-2 RMS (tests/test_gpu_tier_n.py; `precision` below)")
                          if args.x3 else "fp32 MFMA (v_mfma_f32_*_f32)",
            "arithmetic_short": ("h3: fp32 as fp16 hi+lo on fp16 MFMA (3 products), fp32 accumulate; "
                                 "<=1e-4 rel on every element >=1e-2 RMS" if args.x3 else "fp32 MFMA"),
            "precision": None,
            "data": "synthetic: uniform [-1,1]^3 float32 frames (seeded per rank, %d distinct batches cycled), "
                    "random-init SSG weights" % max(1, args.rotate),
            "config": {"workload": "PointNet++ SSG encoder (SA1 N/16 r0.2 ns32 [64,64,128]; "
                                   "SA2 N/64 r0.4 ns64 [128,128,256]; group_all [256,512,1024]) fp32",
                       "points_per_frame": N, "frames_per_gpu": B, "global_batch_frames": B * world,
                       "parallelism": f"per-frame data parallel x{world} (no collectives)"},
            "roofline": roof(dom, tot),
            # the north_star's MFMA figure: the grouped MLP (SA2 layers 2-3), whatever dominates
            "roofline_grouped_mlp": roof("sa2_group_mlp", tot) if "sa2_group_mlp" in tot else None,
            "roofline_all": {k: roof(k, tot) for k in tot if k in work},
            "roofline_standalone": ({k: roof(k, standalone) for k in standalone if k in work}
                                    if standalone else None),
            "sa1_fused_split": sa1_split(standalone),
            "kernel_ms_per_launch": per_launch,
            "distributed": group,
            "pipeline": {"executor": "pointnet2.StreamingSSG feed (steady state: the window pushes and completes "
                                     "exactly `steps` batches; pipeline fill and drain outside it)",
                         "side_streams": args.depth, "batches_per_group": G, "frames_per_launch": G * B,
                         "fps_threads": args.fps_threads,
                         "sa1_ball_queries": args.bq, **chains},
            "fp32_mfma_kernels": fp32_mfma,
            "ssg_host_feed": host_feed,
            "other_configs": extras,
            "density_path": density,
            "host_frames": host,
            "variant_path": variant,
            "voxel_downsample": voxel,
            "cpu_baseline": None,
        }
        if not args.no_cpu_baseline:
            # rank 0 at every world size, after the timed windows (the other ranks wait at the
            # final barrier); the oracle also checks ten frames spread over the 8 input batches
            rec["cpu_baseline"] = cpu_baseline(N, args.cpu_budget)
            rec["speedup_vs_cpu"] = value / rec["cpu_baseline"]["value"]
            rec["precision"] = precision_check(bb, xs, pn.SSG, N)
        detail = None
        if args.detail:
            try:
                os.makedirs(os.path.dirname(os.path.abspath(args.detail)), exist_ok=True)
                with open(args.detail, "w") as f:
                    json.dump(rec, f, indent=1)
                detail = os.path.relpath(os.path.abspath(args.detail), REPO)
            except OSError as e:
                print(f"bench.py: could not write {args.detail}: {e}", file=sys.stderr)
        print(json.dumps(compact_line(rec, detail)), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
