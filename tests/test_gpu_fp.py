"""Feature propagation on the GPU against the numpy restatement of its spec (tests/fp_reference.py):
three_nn (distances, indices and weights), three_interpolate and row_argmax bit for bit; the decoder's
interpolated rows bit for bit and its layers against the exact float64 result of those same rows; the
segmenter's plumbing (encoder + decode, batch independence, chunking, argmax).

Measured on an MI355X, decoder on synthetic levels (test_decoder_on_synthetic_levels), the worst pure
relative error feat_close reports (elements >= 1e-2 RMS; printed, not asserted): h3 fp0 8.4e-5,
fp1 4.6e-5, fp2 5.5e-5, head 6.9e-5, classifier 7.0e-6; native fp32 fp0 1.5e-4, fp1 7.6e-5, fp2 3.3e-5,
head 8.3e-5, classifier 4.9e-6."""
import numpy as np
import pytest
import torch

import fp_reference as ref
from oracle import tier_n
from lidar_ai_recommendation_software_amd import _native as nat
from lidar_ai_recommendation_software_amd import pointnet2 as pn
from lidar_ai_recommendation_software_amd._native import LidarError
from test_gpu_tier_n import feat_close, frames_for, h3_forward_bound, h3_gemm_bound

pytestmark = pytest.mark.gpu
CH = pn.THREE_NN_CHUNK


def _known(x, m):
    """The oracle's FPS subset (m points) of every frame of x."""
    idx = tier_n.fps(x, m).astype(np.int64)
    return np.ascontiguousarray(np.take_along_axis(x, idx[..., None], 1))


def _three_nn_gpu(cuda, u, k, weights=True):
    out = pn.three_nn(torch.from_numpy(u).to(cuda), torch.from_numpy(k).to(cuda), weights=weights)
    return [t.cpu().numpy() for t in out]


def _three_nn_want(u, k, fourth=False):
    res = [ref.three_nn_ref(a, b, fourth=fourth) for a, b in zip(u, k)]
    d3, i3 = np.stack([r[0] for r in res]), np.stack([r[1] for r in res])
    w = np.stack([ref.weights_ref(r[0]) for r in res])
    return (d3, i3, w) + ((np.stack([r[2] for r in res]),) if fourth else ())


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = ~((got == want) | ((got != got) & (want != want)))
    assert not bad.any(), f"{what}: {bad.sum()} / {bad.size} differ, first at {np.argwhere(bad)[:3].tolist()}"
    if got.dtype == np.float32:  # bit for bit where not NaN (the sign of a zero included)
        ok = got == got
        assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32)), f"{what}: bits differ"


@pytest.mark.parametrize("kind,b,n,m", [
    ("uniform", 2, 4096, 1024), ("grid", 1, 4096, 256), ("dups", 1, 2048, 512), ("clumped", 1, 2048, 128),
    ("offset", 1, 2048, 128), ("uniform", 1, 777, 1), ("uniform", 1, 777, 2), ("uniform", 1, 777, 3),
    ("uniform", 1, 777, 5), ("uniform", 1, 1, 1), ("uniform", 3, 513, 64),
    ("uniform", 1, 4100, 4097), ("uniform", 1, 9003, 9000),
    ("uniform", 1, CH + 40, CH - 1), ("uniform", 1, CH + 40, CH), ("uniform", 1, CH + 40, CH + 1),
    ("dups", 1, 2 * CH + 8, 2 * CH + 1),
    # four unknown points per thread from THREE_NN_WIDE_MIN points up (two below); a block's tail threads
    ("uniform", 1, pn.THREE_NN_WIDE_MIN + 5, 5), ("grid", 129, 4096, 27),
])
def test_three_nn_bit_exact(cuda, kind, b, n, m):
    """dist2, idx and weight equal the reference bit for bit: ties (lattice, duplicates) resolve to the
    lowest index, also across the kernel's LDS chunks (m around THREE_NN_CHUNK and multiples)."""
    x = frames_for(kind, b, n, 21)
    k = _known(x, m)
    d3, i3, w = _three_nn_gpu(cuda, x, k)
    wd, wi, ww, d4 = _three_nn_want(x, k, fourth=True)
    _same(i3, wi, "idx")
    _same(d3, wd, "dist2")
    _same(w, ww, "weight")
    if m == 1:
        assert np.array_equal(w, np.broadcast_to(np.float32([1, 0, 0]), w.shape))
    if kind == "grid" and m == 256:  # the case must exercise the tie rule
        assert (wd[..., 2] == d4).mean() >= 0.10
    d_only = _three_nn_gpu(cuda, x, k, weights=False)
    assert len(d_only) == 2 and np.array_equal(d_only[1], wi)


def test_three_nn_nonfinite(cuda):
    """Non-finite known points are never chosen, non-finite unknown points come out unfilled with NaN
    weights, and every other point is untouched."""
    x = frames_for("uniform", 1, 2048, 22)
    k = _known(x, 256)
    clean = _three_nn_gpu(cuda, x, k)
    xb, kb = x.copy(), k.copy()
    kb[0, 3, 0] = np.nan
    kb[0, 7, 1] = np.inf
    xb[0, 11, 2] = np.inf
    xb[0, 12, 1] = np.nan
    got = _three_nn_gpu(cuda, xb, kb)
    for g, w, what in zip(got, _three_nn_want(xb, kb), ("dist2", "idx", "weight")):
        _same(g, w, what)
    d3, i3, w = got
    assert not np.isin(i3, [3, 7]).any()
    for p in (11, 12):
        assert np.array_equal(d3[0, p], [np.inf] * 3) and np.array_equal(i3[0, p], [0] * 3) and np.isnan(w[0, p]).all()
    untouched = ~np.isin(clean[1][0], [3, 7]).any(axis=1)
    untouched[[11, 12]] = False
    assert untouched.sum() > 1900
    for g, c in zip(got, clean):
        assert np.array_equal(g[0, untouched], c[0, untouched])
    assert np.isfinite(w[0, untouched]).all()


def test_three_nn_rejects_bad_shapes(cuda):
    u = torch.zeros((2, 8, 3), device=cuda)
    with pytest.raises(ValueError, match="share B"):
        pn.three_nn(u, torch.zeros((1, 4, 3), device=cuda))
    with pytest.raises(ValueError, match="m >= 1"):
        pn.three_nn(u, torch.zeros((2, 0, 3), device=cuda))
    with pytest.raises(ValueError, match=r"\(B, n, 3\) float32"):
        pn.three_nn(u.double(), torch.zeros((2, 4, 3), device=cuda))


@pytest.mark.parametrize("c2,c1", [(128, 0), (256, 128), (13, 3), (1024, 256)])
def test_three_interpolate_bit_exact(cuda, c2, c1):
    """Random features, indices and weights; the coarse and skip rows are column slices of wider rows, the
    output is wider and longer than needed: its pad columns and tail rows must be exactly zero."""
    rng = np.random.default_rng(c2)
    B, n, m = 2, 301, 40
    ldk, lds = c2 + (8 if c2 % 4 == 0 else 5), c1 + 4
    kf = rng.standard_normal((B, m, ldk)).astype(np.float32)
    sk = rng.standard_normal((B, n, lds)).astype(np.float32)
    idx = rng.integers(0, m, (B, n, 3)).astype(np.int32)
    w = rng.uniform(0, 1, (B, n, 3)).astype(np.float32)
    ldo = (c1 + c2 + 3) // 4 * 4 + 8
    R = (B * n + 127) // 128 * 128 + 128
    out = torch.full((R, ldo), float("nan"), device=cuda)
    kft, skt = torch.from_numpy(kf).to(cuda), torch.from_numpy(sk).to(cuda)
    res = pn.three_interpolate(kft[..., :c2], torch.from_numpy(idx).to(cuda), torch.from_numpy(w).to(cuda),
                               skt[..., :c1] if c1 else None, out=out)
    assert res is out
    got = out.cpu().numpy()
    want = np.concatenate([ref.interpolate_ref(kf[b, :, :c2], idx[b], w[b], sk[b, :, :c1] if c1 else None)
                           for b in range(B)])
    _same(got[:B * n, :c1 + c2], want, "rows")
    assert not got[:B * n, c1 + c2:].any() and not got[B * n:].any()
    assert np.array_equal(got.view(np.uint32)[B * n:], np.zeros((R - B * n, ldo), np.uint32))
    # default output: the dense GEMMs' A operand
    res = pn.three_interpolate(kft[..., :c2], torch.from_numpy(idx).to(cuda), torch.from_numpy(w).to(cuda),
                               skt[..., :c1] if c1 else None)
    assert tuple(res.shape) == ((B * n + 127) // 128 * 128, (c1 + c2 + 15) // 16 * 16)
    _same(res.cpu().numpy()[:B * n, :c1 + c2], want, "rows (default out)")
    assert not res.cpu().numpy()[B * n:].any()


def test_three_interpolate_one_known_point_is_a_broadcast(cuda):
    rng = np.random.default_rng(3)
    B, n, c2 = 3, 200, 64
    x = frames_for("uniform", B, n, 23)
    g = rng.standard_normal((B, c2)).astype(np.float32)
    _, idx, w = pn.three_nn(torch.from_numpy(x).to(cuda), torch.zeros((B, 1, 3), device=cuda))
    out = pn.three_interpolate(torch.from_numpy(g).to(cuda).reshape(B, 1, c2), idx, w)
    got = out.cpu().numpy()[:B * n, :c2].reshape(B, n, c2)
    assert np.array_equal(got, np.broadcast_to(g[:, None], got.shape))


def test_three_interpolate_rejects_bad_arguments(cuda):
    kf = torch.zeros((1, 4, 8), device=cuda)
    idx = torch.zeros((1, 5, 3), dtype=torch.int32, device=cuda)
    w = torch.zeros((1, 5, 3), device=cuda)
    with pytest.raises(ValueError, match="ldo % 4 == 0"):
        pn.three_interpolate(kf, idx, w, out=torch.zeros((128, 6), device=cuda))
    with pytest.raises(ValueError, match="ldo % 4 == 0"):
        pn.three_interpolate(kf, idx, w, out=torch.zeros((4, 8), device=cuda))
    with pytest.raises(ValueError, match="skip must be"):
        pn.three_interpolate(kf, idx, w, skip=torch.zeros((1, 4, 2), device=cuda))
    with pytest.raises(LidarError, match="rows < batch"):
        o = torch.zeros((8, 8), device=cuda)
        nat.call("lidar_three_interpolate_f32", nat.handle(0), nat.ptr(kf), 8, 8, nat.ptr(idx), nat.ptr(w), None, 0, 0,
                 1, 5, 4, nat.ptr(o), 4, 8, nat.stream_ptr())


@pytest.mark.parametrize("c", [2, 13, 128])
def test_row_argmax(cuda, c):
    rng = np.random.default_rng(c)
    rows, ldx = 1003, c + 3
    x = (np.round(rng.standard_normal((rows, ldx)) * 2) / 2).astype(np.float32)  # quantised: many ties
    x[:, c:] = 100.0  # columns past c are not looked at
    x[5, :c] = 1.5  # a whole row tied
    x[6, :c] = np.nan
    x[7, c - 1] = np.nan  # a NaN counts as the maximum
    x[8, 0] = np.nan
    x[9, :c] = -np.inf
    if c > 2:
        x[10, [1, c - 2]] = np.nan  # the first NaN
        x[11, :c] = np.arange(c)  # the last column
    got = pn.row_argmax(torch.from_numpy(x).to(cuda)[:, :c], c).cpu().numpy()
    want = np.argmax(x[:, :c], axis=1).astype(np.int32)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert (x[:, :c] == x[:, :c].max(axis=1, keepdims=True)).sum(axis=1).max() > 1  # ties were present


def _synthetic_levels(B, n, seed):
    """A frame, its nested FPS subsets (n / 16 and n / 64 points) and standard-normal level features."""
    rng = np.random.default_rng(seed)
    x = frames_for("uniform", B, n, seed)
    x1 = _known(x, n // 16)
    x2 = _known(x1, n // 64)
    f1 = rng.standard_normal((B, n // 16, 128)).astype(np.float32)
    f2 = rng.standard_normal((B, n // 64, 256)).astype(np.float32)
    g = rng.standard_normal((B, 1024)).astype(np.float32)
    return x, [(x1, f1), (x2, f2)], g


@pytest.fixture(scope="module")
def synthetic():
    return _synthetic_levels(2, 2048, 31)


@pytest.mark.parametrize("x3", [True, False])
def test_decoder_on_synthetic_levels(cuda, synthetic, x3):
    """Every FP level's rows, rebuilt in numpy float32 from the GPU's own previous output, equal what the
    kernels wrote bit for bit; every level's layers, the head and the classifier hold the project's
    feature tolerance against the float64 result of those same rows (and, h3, the rigorous forward bound).
    The strict pure-relative figure is printed, not asserted (un-pooled per-point features)."""
    x, levels, g = synthetic
    B, n, _ = x.shape
    seg = pn.PointNet2Segmenter(pn.SSG, pn.FP_SSG, num_classes=5, device=cuda, seed=4, x3=x3)
    t = lambda a: torch.from_numpy(a).to(cuda)
    logits, kept = seg.decode(t(x), [(t(a), t(f)) for a, f in levels], t(g), keep_levels=True)
    assert tuple(logits.shape) == (B, n, 5)
    sets = [(x, None)] + levels + [(np.zeros((B, 1, 3), np.float32), g[:, None, :])]
    kfeat = sets[3][1]
    worst = {}
    for i, (fp, layers) in enumerate(zip(kept["fp"], seg.fp_weights["fp"])):
        uxyz, skip = sets[2 - i]
        kxyz = sets[3 - i][0]
        want = [ref.fp_rows_ref(uxyz[b], kxyz[b], kfeat[b], None if skip is None else skip[b]) for b in range(B)]
        rows = fp["rows"].cpu().numpy()
        _same(fp["idx"].cpu().numpy(), np.stack([w[1] for w in want]), f"fp{i} idx")
        _same(rows, np.stack([w[0] for w in want]), f"fp{i} rows")
        if i:  # (level 0 interpolates one global vector: a broadcast)
            assert (rows.std(axis=1) > 0).mean() > 0.5  # the rows vary across the points
        got = fp["feats"].cpu().numpy()
        flat = rows.reshape(-1, rows.shape[-1])
        exact = ref.fp_level_exact(flat, layers)
        worst[f"fp{i}"] = feat_close(got.reshape(exact.shape), exact, f"fp{i} (x3={x3})", strict=False)
        if x3:
            ex, bound = h3_forward_bound(flat, layers, 1)
            assert np.all(np.abs(got.reshape(ex.shape) - ex) <= bound), f"fp{i}: outside the h3 forward bound"
        kfeat = got
    head = seg.fp_weights["head"]
    flat = kfeat.reshape(-1, kfeat.shape[-1])
    hidden = kept["head"].cpu().numpy().reshape(-1, head[-1][0].shape[0])
    exact = ref.fp_level_exact(flat, head[:-1])
    worst["head"] = feat_close(hidden, exact, f"head (x3={x3})", strict=False)
    if x3:
        ex, bound = h3_forward_bound(flat, head[:-1], 1)
        assert np.all(np.abs(hidden - ex) <= bound), "head: outside the h3 forward bound"
    lg = logits.cpu().numpy().reshape(-1, 5)
    exact = ref.fp_level_exact(hidden, head[-1:], last_relu=False)
    worst["classifier"] = feat_close(lg, exact, f"classifier (x3={x3})", strict=False)
    if x3:
        ex, bound = h3_gemm_bound(hidden, *head[-1])
        assert np.all(np.abs(lg - ex) <= bound), "classifier: outside the h3 GEMM bound"
    print(f"decoder x3={x3}: worst pure relative error per stage {worst}")


@pytest.mark.parametrize("cfg_name", ["ssg", "msg"])
def test_segmenter_plumbing(cuda, cfg_name):
    cfg = pn.CONFIGS[cfg_name]
    B, n = 3, 2048
    x = torch.from_numpy(frames_for("uniform", B, n, 33)).to(cuda)
    seg = pn.PointNet2Segmenter(cfg, pn.FP_SSG, num_classes=4, device=cuda, seed=2)
    logits = seg.forward(x)
    assert tuple(logits.shape) == (B, n, 4) and logits.dtype == torch.float32
    assert torch.isfinite(logits).all()
    # forward = the encoder with its levels kept, then decode
    g, levels = seg.backbone.forward(x, keep_levels=True)
    assert torch.equal(seg.decode(x, levels, g), logits)
    # the decoder leaves the encoder alone
    g_alone, _ = pn.PointNet2Backbone(cfg, device=cuda, seed=2).forward(x)
    assert torch.equal(g_alone, g)
    # per frame: a batch equals its frames one at a time, and chunking changes nothing
    for b in range(B):
        assert torch.equal(seg.forward(x[b:b + 1])[0], logits[b]), f"frame {b}"
    assert torch.equal(seg.forward(x, max_bytes=1), logits)
    assert torch.equal(seg.forward(x, max_bytes=seg._frame_bytes(seg.point_sets(x, levels, g)) * 2), logits)
    labels = seg.segment(x)
    assert labels.dtype == torch.int32 and tuple(labels.shape) == (B, n)
    assert np.array_equal(labels.cpu().numpy(), np.argmax(logits.cpu().numpy(), axis=2))
