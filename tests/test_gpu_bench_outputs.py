"""A plain `bench.py` run (no --full) times the headline window alone, and `--dump-outputs DIR` writes
what the window's last step returned: the global features of the last batch it completed.  The inputs
and weights are seeded, so the test rebuilds that batch, runs one-batch forward() on it and requires
the dumped array bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N, STEPS, WARMUP, ROTATE, DEPTH = 4, 8192, 6, 1, 3, 3
G = 3  # bench.pick_group(6, 3)


def test_plain_run_dumps_the_last_steps_outputs(cuda, tmp_path):
    import torch
    from lidar_ai_recommendation_software_amd import pointnet2 as pn
    from lidar_ai_recommendation_software_amd import sharding
    from lidar_ai_recommendation_software_amd.synthetic import unit_frames
    out = tmp_path / "outputs"
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--points", str(N), "--batch", str(B), "--steps", str(STEPS),
           "--warmup", str(WARMUP), "--rotate", str(ROTATE), "--depth", str(DEPTH), "--dump-outputs", str(out),
           "--detail", str(tmp_path / "detail.json")]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == STEPS and line["ms_per_step"] > 0 and line["dtype"] == "f32"
    assert line["value"] == pytest.approx(B * N * STEPS / (line["ms_per_step"] * STEPS / 1e3) / 1e6, rel=1e-6)
    # nothing beside the headline ran
    assert line["cpu_baseline"] is None and line.get("precision") is None and "ssg_host_feed" not in line
    detail = json.load(open(tmp_path / "detail.json"))
    assert not detail["other_configs"] and detail["density_path"] is None and detail["roofline_standalone"] is None
    assert sorted(os.listdir(out)) == ["global_features.npy"]
    got = np.load(out / "global_features.npy")
    assert got.dtype == np.float32 and got.shape == (B, 1024)
    # the feed completes batches in input order, `depth` groups behind the pushes: after the fill
    # ((depth + warmup) groups) and the window the last completed batch is this one
    last = (DEPTH + WARMUP) * G + STEPS - DEPTH * G - 1
    x = torch.from_numpy(unit_frames(B, N, seed=sharding.frame_seed(0, step=last % ROTATE))).to(cuda)
    bb = pn.PointNet2Backbone(pn.SSG, device=cuda, seed=0, dtype="f32", x3=True)
    want = bb.forward(x)[0].cpu().numpy()
    assert np.array_equal(got, want), "the dumped outputs differ from forward() of the same batch"
