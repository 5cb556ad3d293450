"""PointNet++ SetAbstraction operators and backbones on liblidar_amd (gfx950 HIP).

These are the north_star operators that the reference does not have (SURVEY.md §0,
§8a N2-N6).  They sit beside the reference's operator set
(``utils/data_processing.py:231`` ``downsample_point_cloud`` and the density model,
``models/crowd_density_model.py:14``), and every one runs on the HIP kernels behind
``include/lidar_amd.h``.  Torch only holds device memory and the stream.

Spec (frozen in DESIGN.md §3, restated by ``oracle/tier_n.py``): fp32 coordinates,
distances ``(dx*dx + dy*dy) + dz*dz`` with one rounding per operation;
FPS starts at index 0 and breaks ties to the lowest index; ball query keeps the first
``nsample`` hits in index order; grouping is ``[xyz - centre, features]`` (use_xyz);
each SA branch is a 3-layer shared MLP (conv1x1 + folded BN + ReLU) max-pooled over
its neighbourhood; the last level is group_all.  The decoder (feature propagation): three_nn keeps
the three nearest coarse points in (distance, index) order, three_interpolate mixes their features
with inverse-distance weights, the fine level's features are concatenated and a shared MLP follows
per level; PointNet2Segmenter adds a per-point head and argmax.

Layouts: xyz (B, N, 3) float32; features channels-last (B, N, C) float32.
"""
import ctypes
import warnings

import numpy as np
import torch

from . import _native as nat
from .streams import side_streams

# ------------------------------------------------------------------ configs
# BASELINE.json configs: C2 = one SA1 layer, C3 = 3-level SSG, C5 = 3-level MSG.
SSG = {
    "name": "ssg",
    "levels": [
        {"npoint_div": 16, "radii": [0.2], "nsamples": [32], "mlps": [[64, 64, 128]]},
        {"npoint_div": 64, "radii": [0.4], "nsamples": [64], "mlps": [[128, 128, 256]]},
        {"group_all": True, "mlps": [[256, 512, 1024]]},
    ],
}
MSG = {
    "name": "msg",
    "levels": [
        {"npoint_div": 16, "radii": [0.1, 0.2, 0.4], "nsamples": [16, 32, 128],
         "mlps": [[32, 32, 64], [64, 64, 128], [64, 96, 128]]},
        {"npoint_div": 64, "radii": [0.2, 0.4, 0.8], "nsamples": [32, 64, 128],
         "mlps": [[64, 64, 128], [128, 128, 256], [128, 128, 256]]},
        {"group_all": True, "mlps": [[256, 512, 1024]]},
    ],
}
SA1_ONLY = {  # C2: 16 384 points -> 1 024 centroids, r = 0.2, nsample 32
    "name": "sa1",
    "levels": [{"npoint_div": 16, "radii": [0.2], "nsamples": [32], "mlps": [[64, 64, 128]]}],
}
CONFIGS = {"ssg": SSG, "msg": MSG, "sa1": SA1_ONLY}


def resolve(cfg, n):
    """Per-level dicts with concrete npoint for an n-point frame (oracle format)."""
    out = []
    for lvl in cfg["levels"]:
        d = dict(lvl)
        if not lvl.get("group_all"):
            d["npoint"] = max(1, n // lvl["npoint_div"])
        out.append(d)
    return out


# One codec for every weight tree here (the encoder's [level][branch][layer], the decoder's {"fp", "head"}):
# a tree is lists of layers, a layer list is described by its [(cin, cout)], and these four do the work.
def _draw_layers(rng, dims):
    """[(W (cin, cout), b (cout,))] float32 for dims = [(cin, cout)]: conv1x1's default U(-1/sqrt(cin),
    1/sqrt(cin)), W then b per layer (the order of draws is part of the seeds' meaning)."""
    layers = []
    for cin, cout in dims:
        bound = 1.0 / np.sqrt(cin)
        W = rng.uniform(-bound, bound, (cin, cout)).astype(np.float32)
        b = rng.uniform(-bound, bound, cout).astype(np.float32)
        layers.append((W, b))
    return layers


def _check_layers(what, dims, layers):
    """layers = [(W, b)] against dims = [(cin, cout)] -> contiguous float32 arrays; ValueError, prefixed
    `what`, on the first mismatch."""
    if len(layers) != len(dims):
        raise ValueError(f"{what}: {len(layers)} layers, expected {len(dims)}")
    out = []
    for j, ((cin, cout), (W, b)) in enumerate(zip(dims, layers)):
        W = np.ascontiguousarray(W, dtype=np.float32)
        b = np.ascontiguousarray(b, dtype=np.float32).reshape(-1)
        if W.shape != (cin, cout) or b.shape != (cout,):
            raise ValueError(f"{what} layer {j}: W {W.shape}, b {b.shape}; expected ({cin}, {cout}) and ({cout},)")
        out.append((W, b))
    return out


def _layer_arrays(prefix, layers):
    """{<prefix>_<layer>_{W,b}: array}: a layer list as the flat entries of an .npz."""
    return {f"{prefix}_{j}_{k}": a for j, wb in enumerate(layers) for k, a in zip("Wb", wb)}


def _read_layers(z, prefix, n):
    """The n layers _layer_arrays(prefix, ...) wrote into z."""
    return [(z[f"{prefix}_{j}_W"], z[f"{prefix}_{j}_b"]) for j in range(n)]


def _chain(cin, widths):
    """[(cin, cout)] of consecutive layers of the given output widths."""
    return list(zip([cin] + list(widths[:-1]), widths))


def _sa_layer_dims(cfg):
    """[level][branch] = [(cin, cout) per layer]: cin of a branch's first layer is 3 + the previous level's
    channels."""
    return [[_chain(3 + cin_feat, widths) for widths in lvl["mlps"]]
            for lvl, cin_feat in zip(cfg["levels"], level_channels(cfg))]


def init_weights(cfg, seed=0):
    """Deterministic random init (conv1x1 default: U(-1/sqrt(cin), 1/sqrt(cin)), BN folded
    at its fresh-init identity).  Returns [level][branch][layer] = (W (cin, cout), b)."""
    rng = np.random.default_rng(seed)
    return [[_draw_layers(rng, dims) for dims in lvl] for lvl in _sa_layer_dims(cfg)]


def check_weights(cfg, weights):
    """Validate [level][branch][layer] = (W (cin, cout), b (cout,)) against cfg's widths (cin = 3 + the
    previous level's channels); returns them as contiguous float32 arrays.  Raises ValueError naming the
    first mismatch."""
    dims = _sa_layer_dims(cfg)
    if len(weights) != len(dims):
        raise ValueError(f"weights: {len(weights)} levels, the configuration has {len(dims)}")
    out = []
    for li, (dl, wl) in enumerate(zip(dims, weights)):
        if len(wl) != len(dl):
            raise ValueError(f"weights level {li}: {len(wl)} branches, the configuration has {len(dl)}")
        out.append([_check_layers(f"weights level {li} branch {bi}", d, layers)
                    for bi, (d, layers) in enumerate(zip(dl, wl))])
    return out


def save_weights(path, weights):
    """Weights to an .npz of plain arrays (keys l<level>_b<branch>_<layer>_{W,b}; no pickled objects)."""
    arrs = {}
    for li, wl in enumerate(weights):
        for bi, layers in enumerate(wl):
            arrs.update(_layer_arrays(f"l{li}_b{bi}", layers))
    np.savez(path, **arrs)


def load_weights(path, cfg):
    """The .npz save_weights wrote, in cfg's layout (loaded with allow_pickle=False), validated."""
    with np.load(path, allow_pickle=False) as z:
        w = [[_read_layers(z, f"l{li}_b{bi}", len(widths)) for bi, widths in enumerate(lvl["mlps"])]
             for li, lvl in enumerate(cfg["levels"])]
    return check_weights(cfg, w)


# --------------------------------------------------------------- functional ops
def _dev_check(*ts):
    for t in ts:
        if t is not None and (not t.is_cuda or not t.is_contiguous()):
            raise ValueError("liblidar_amd operators take contiguous CUDA tensors")


def farthest_point_sample(xyz, npoint, return_xyz=False, first_zero=None, prefix_ok=None, slot=0,
                          out_idx=None, out_xyz=None, threads=0):
    """xyz (B, N, 3) float32 CUDA -> idx (B, npoint) int32 [, new_xyz (B, npoint, 3)].

    threads: workgroup size per frame (0 = 1024, 512; frames above 262 144 points always take 512).
    n <= 4 194 304 points per frame.

    first_zero: optional (B,) int32 output — first step whose winning distance was 0 or not finite.
    prefix_ok: optional (B,) int32 — the parent run's first_zero when xyz is the parent's
    FPS-ordered sample set (nested SA levels): the exact identity result is copied."""
    _dev_check(xyz, first_zero, prefix_ok)
    if xyz.dtype != torch.float32 or xyz.dim() != 3 or xyz.shape[2] != 3:
        raise ValueError("xyz must be (B, N, 3) float32")
    B, N, _ = xyz.shape
    idx = out_idx if out_idx is not None else torch.empty((B, npoint), dtype=torch.int32, device=xyz.device)
    new_xyz = None
    if return_xyz:
        new_xyz = out_xyz if out_xyz is not None else torch.empty((B, npoint, 3), dtype=torch.float32,
                                                                  device=xyz.device)
    nat.call("lidar_fps_ex_f32", nat.handle(xyz.device.index, slot), nat.ptr(xyz), B, N, npoint,
             nat.ptr(idx), nat.ptr(new_xyz), nat.ptr(first_zero), nat.ptr(prefix_ok),
             int(threads), nat.stream_ptr())
    return (idx, new_xyz) if return_xyz else idx


def voxel_downsample_batch(xyz, voxel, slot=0, check=True, out=None):
    """Voxel downsampling of (B, N, 3) float32 CUDA frames on the whole chip
    (lidar_voxel_downsample_batch_f32; per frame equal to data_processing.voxel_downsample).
    Returns device tensors (centroids (B, N, 3), voxel_id (B, N) int32, counts (B, N) int32,
    nvox (B,) int32): the first nvox[f] centroid / count rows of frame f are valid; nvox -1 marks
    a frame whose extent is not finite or whose voxel grid has 2^32 keys or more.  Voxels are
    calculate_grid_density's grid extended to z (data_processing.voxel_downsample).

    nvox <= -2 is a library failure, never expected: -2 one of the launch's bounded in-launch waits
    timed out, -3 a bucket table that is not a partition of the frame.  check=True (default) reads
    nvox back (a host synchronisation on the stream) and raises LidarError on either; check=False
    leaves nvox on the device (throughput loops: check_voxel_counts(nvox) later).  out: the four output
    tensors of an earlier call of the same shape, written again (a stream of batches allocates once)."""
    _dev_check(xyz)
    if xyz.dtype != torch.float32 or xyz.dim() != 3 or xyz.shape[2] != 3:
        raise ValueError("xyz must be (B, N, 3) float32")
    B, N, _ = xyz.shape
    dev = xyz.device
    if out is not None:
        cent, vid, cnt, nvox = out
        if (tuple(cent.shape) != (B, N, 3) or tuple(vid.shape) != (B, N) or tuple(cnt.shape) != (B, N)
                or tuple(nvox.shape) != (B,) or cent.dtype != torch.float32
                or any(t.dtype != torch.int32 for t in (vid, cnt, nvox))):
            raise ValueError("voxel_downsample_batch: out must be (B, N, 3) float32, (B, N) int32 x 2, (B,) int32")
        _dev_check(cent, vid, cnt, nvox)
    else:
        cent = torch.empty((B, N, 3), dtype=torch.float32, device=dev)
        vid = torch.empty((B, N), dtype=torch.int32, device=dev)
        cnt = torch.empty((B, N), dtype=torch.int32, device=dev)
        nvox = torch.empty(B, dtype=torch.int32, device=dev)
    if B and N:
        nat.call("lidar_voxel_downsample_batch_f32", nat.handle(dev.index, slot), nat.ptr(xyz), B, N,
                 float(voxel), nat.ptr(vid), nat.ptr(cent), nat.ptr(cnt), nat.ptr(nvox), nat.stream_ptr())
        if check:
            check_voxel_counts(nvox)
    return cent, vid, cnt, nvox


VOXEL_FAILURES = {-2: "an in-launch hand-off of the voxel launches timed out",
                  -3: "a voxel bucket table is not a partition of its frame"}


def check_voxel_counts(nvox):
    """Raise LidarError if any frame's nvox reports a library failure (<= -2; reads nvox back)."""
    bad = nvox[nvox <= -2]
    if bad.numel():
        code = int(bad.min().item())
        raise nat.LidarError(f"voxel_downsample_batch: {VOXEL_FAILURES.get(code, 'unknown failure')} "
                             f"(nvox {code} in {bad.numel()} frame(s); a library bug, please report)")


BQ_MODES = {"auto": 0, "scan": 1, "grid": 2}
BQ_GRID_MIN_N = 1024  # csrc/bq_grid.hpp kGridMinN: "auto" bins frames of at least this many points


def ball_query(radius, nsample, xyz, new_xyz, out=None, slot=0, mode="auto", grid=None):
    """-> idx (B, M, nsample) int32 (pointnet2 argument order).

    mode: "auto" (the (index window, cell) grid for N >= 1024, else the index-order scan),
    "scan" or "grid" — identical results.  grid: a buffer filled by ball_query_bin for
    these xyz (the binning then does not run here)."""
    _dev_check(xyz, new_xyz, out)
    B, N, _ = xyz.shape
    M = new_xyz.shape[1]
    idx = out if out is not None else torch.empty((B, M, nsample), dtype=torch.int32, device=xyz.device)
    h = nat.handle(xyz.device.index, slot)
    if grid is not None:
        nat.call("lidar_ball_query_binned_f32", h, nat.ptr(xyz), nat.ptr(grid), nat.ptr(new_xyz),
                 B, N, M, float(radius), int(nsample), nat.ptr(idx), nat.stream_ptr())
    else:
        nat.call("lidar_ball_query_mode_f32", h, nat.ptr(xyz), nat.ptr(new_xyz),
                 B, N, M, float(radius), int(nsample), BQ_MODES[mode], nat.ptr(idx), nat.stream_ptr())
    return idx


def ball_query_grid_buffer(B, N, device):
    """Device buffer for ball_query_bin over (B, N, 3) frames."""
    nbytes = nat.load_library().lidar_ball_query_grid_bytes(B, N)
    return torch.empty((max(1, nbytes),), dtype=torch.uint8, device=device)


def ball_query_bin(radius, nsample, xyz, grid, slot=0):
    """Bin (B, N, 3) frames for later ball_query(..., grid=grid) calls (any stream order
    that puts this launch first).  Depends only on xyz."""
    _dev_check(xyz, grid)
    B, N, _ = xyz.shape
    nat.call("lidar_ball_query_bin_f32", nat.handle(xyz.device.index, slot), nat.ptr(xyz), B, N,
             float(radius), int(nsample), nat.ptr(grid), nat.stream_ptr())
    return grid


# (xyz_level, c1, c2, c3, nsample) of the fused kernels: csrc/sa_shapes.hpp's LIDAR_SA_SHAPES is the source (every
# fused entry point expands it); repeated here because the library has no call that lists it
MLP16_SHAPES = {(True, 64, 64, 128, 32), (True, 32, 32, 64, 16), (True, 64, 96, 128, 128), (False, 128, 128, 256, 64),
                (False, 128, 128, 256, 128), (False, 64, 64, 128, 32)}


_PACKERS = {"16": ("lidar_mlp_packed_size16", "lidar_mlp_pack16_f32", np.float32),
            "x3": ("lidar_mlp_packed_size_x3", "lidar_mlp_pack_x3_f32", np.uint8),
            "x1": ("lidar_mlp_packed_size_x1", "lidar_mlp_pack_x1_f32", np.uint8)}


# per arithmetic of a fused-kernel branch: (the image's key in the branch entry, its _PACKERS kind)
_IMAGE = {"x1": ("packed_x1", "x1"), "x3": ("packed_x3", "x3"), "f32": ("packed16", "16")}


def _pack_branch(kind, layers, xyz_level=None):
    """Host-side packed image of a branch's three layers for the fused kernel of `kind` (_PACKERS: the
    library's size and pack calls and the image's dtype; the x1 calls take no xyz_level)."""
    size, pack, dtype = _PACKERS[kind]
    (w1, _), (w2, _), (w3, _) = layers
    dims = ([] if kind == "x1" else [int(xyz_level)]) + [w1.shape[1], w2.shape[1], w3.shape[1]]
    if kind == "x3":
        spread, outlier = h3_envelope(layers)
        if spread > H3_SPREAD_LOG2_MAX or outlier > H3_BIAS_OUTLIER_LOG2_MAX:
            warnings.warn(f"SA branch weights outside the h3 kernels' measured 1e-4 envelope: channel spread 2^{spread:.1f} "
                          f"(limit 2^{H3_SPREAD_LOG2_MAX:g}), |b2| outlier 2^{outlier:.1f} (limit "
                          f"2^{H3_BIAS_OUTLIER_LOG2_MAX:g}); results stay within the h3 forward bound but small features "
                          "may miss 1e-4: use x3=False (native fp32) for such weights", RuntimeWarning, stacklevel=3)
    lib = nat.load_library()
    out = np.zeros(getattr(lib, size)(*dims), dtype=dtype)
    arrs = [np.ascontiguousarray(a, dtype=np.float32) for layer in layers for a in layer]
    nat.check(getattr(lib, pack)(*dims, *[a.ctypes.data_as(ctypes.c_void_p) for a in arrs],
                                 out.ctypes.data_as(ctypes.c_void_p)), pack)
    return out


def pack_branch16(layers, xyz_level):
    """Host-side packed image for lidar_sa_group_mlp16_f32 (16x16x4 MFMA fragments)."""
    return _pack_branch("16", layers, xyz_level)


def group_mlp16(p, q, idx, n, packed, widths, out, out_offset=0, xyz_level=False):
    """16-row fused branch.  xyz_level: p = xyz (B, N, 3), q = centres (B, M, 3); else
    p / q are group_mlp_pre's per-point / per-centre layer-1 rows.  -> out[..., off:off+c3]."""
    B, M, ns = idx.shape
    c1, c2, c3 = widths
    if xyz_level:
        if p.numel() < B * n * 3 or q.numel() < B * M * 3 or not (p.is_contiguous() and q.is_contiguous()):
            raise ValueError("group_mlp16: xyz / centres must be contiguous (B, N, 3) / (B, M, 3)")
        stride = 3
    else:
        if p.shape[0] < B * n or q.shape[0] < B * M or p.shape[1] < c1 or q.shape[1] != p.shape[1]:
            raise ValueError("group_mlp16: p/q shapes do not match the batch")
        stride = p.shape[1]
    _dev_check(p, q, idx, packed, out)
    nat.call("lidar_sa_group_mlp16_f32", nat.handle(p.device.index), int(xyz_level), nat.ptr(p), stride,
             nat.ptr(q), nat.ptr(idx), B, n, M, ns, c1, c2, c3, nat.ptr(packed), nat.ptr(out), out.shape[-1],
             out_offset, nat.stream_ptr())
    return out


# The weights inside which the h3 SA kernels were measured to hold the 1e-4 contract (INTEGRATION.md "Weights
# outside the h3 envelope"; tests/test_gpu_sa_precision.py): h3 scales a layer's weights by ONE power of two and
# layer 3's input by a bound fed by max |b2|, so a channel far below its layer's maximum, or one huge |b2|,
# costs the small values their low piece.  log2 thresholds of h3_envelope()'s two figures.
H3_SPREAD_LOG2_MAX = 10.0   # held at 2^9.6 (per-channel scales spread over 2^8 in both layers), lost by 2^16.4
H3_BIAS_OUTLIER_LOG2_MAX = 17.0  # held with one |b2| 2^16.6 above the median (layer 3's scale 2^15 above the data), lost by 2^24.6


def h3_envelope(layers):
    """(channel spread, bias outlier), log2, of a branch's [(W, b)] x 3 for the h3 kernels.  Channel spread:
    over W2 and W3, how far the smallest input-row or output-column maximum lies below the layer's maximum
    (all-zero rows and columns aside).  Bias outlier: max |b2| over the median |b2| (over the median column
    maximum of |W2| when that median is zero): what lifts layer 3's scale above its data."""
    spread = 0.0
    for W, _ in layers[1:]:
        A = np.abs(np.asarray(W, np.float64))
        for axis in (0, 1):
            m = A.max(axis=axis)
            m = m[m > 0]
            if m.size:
                spread = max(spread, float(np.log2(A.max() / m.min())))
    W2, b2 = (np.abs(np.asarray(a, np.float64)) for a in layers[1])
    ref = np.median(b2) if np.median(b2) > 0 else np.median(W2.max(axis=0))
    outlier = float(np.log2(b2.max() / ref)) if b2.max() > 0 and ref > 0 else 0.0
    return spread, outlier


def pack_branch_x3(layers, xyz_level):
    """Host-side packed image (uint8) for lidar_sa_group_mlp_x3_f32 (fp16 hi/lo fragments of each layer's
    W 2^s, h3 arithmetic; csrc/h3.hpp).  Warns (RuntimeWarning) for weights outside the envelope in which
    the h3 kernels hold the 1e-4 contract (h3_envelope; PointNet2Backbone(x3=False) is the strict-fp32 path)."""
    return _pack_branch("x3", layers, xyz_level)


def pack_branch_x1(layers):
    """Host-side packed image (uint8) for lidar_sa_group_mlp_x1_f32 (bf16 spec: bf16-rounded
    W1 xyz rows, hi fragments of W2 / W3, fp32 biases)."""
    return _pack_branch("x1", layers)


def group_mlp_x1(p, idx, n, packed, widths, out, out_offset=0, xyz=None, centres=None):
    """One SA branch in the bf16 spec (lidar_sa_group_mlp_x1_f32).  xyz level: p = the level's
    points (B, n, 3), centres (B, M, 3).  Feature level: p (B*n, >= c1) = bf16(f) bf16(W1_f) + b1
    per point (layer1_points_x1): rows of one stride, possibly a column slice of the level's fused
    layer-1 output; xyz = the level's points, centres."""
    B, M, ns = idx.shape
    c1, c2, c3 = widths
    mode = 2 if xyz is not None else 0
    if mode == 0:
        _dev_check(p, centres, idx, packed, out)
        stride = 3
    else:
        _dev_check(xyz, centres, idx, packed, out)
        if not p.is_cuda or p.dim() != 2 or p.stride(1) != 1:
            raise ValueError("group_mlp_x1: per-point rows must be a CUDA (rows, cols) tensor with unit column stride")
        stride = p.stride(0)
        if p.shape[0] < B * n or p.shape[1] < c1:
            raise ValueError("group_mlp_x1: per-point rows do not match the batch")
    nat.call("lidar_sa_group_mlp_x1_f32", nat.handle(p.device.index), mode, nat.ptr(p), stride,
             nat.ptr(centres) if mode == 0 else None, nat.ptr(xyz), nat.ptr(centres), nat.ptr(idx), B, n, M, ns,
             c1, c2, c3, nat.ptr(packed), nat.ptr(out), out.shape[-1], out_offset, nat.stream_ptr())
    return out


def layer1_points_x1(x_rows, xyz, cfeat, branches, cat=None):
    """Per-point layer-1 feature part of a bf16-spec level: P = bf16(f) bf16(W1_f) + b1 for every
    branch (x_rows: the level's padded rows [f, x, y, z, 0-pad]; the xyz rows of W1_f are zero,
    the offsets' part runs per grouped row in lidar_sa_group_mlp_x1_f32).  cat: the branches' W1_f
    side by side (fused_layer1_x1): one GEMM reads the rows once for every branch, and each branch's
    P is its column slice — the same products in the same order per column (the bf16 spec's image has
    no per-matrix scale), so bit-identical to one GEMM per branch."""
    B, N, _ = xyz.shape
    nat.call("lidar_concat_xyz_pad_f32", nat.handle(xyz.device.index), nat.ptr(xyz), B * N, nat.ptr(x_rows),
             x_rows.shape[1], cfeat, nat.stream_ptr())
    if cat is not None:
        full = run_dense(x_rows, cat)
        return [full[:, o:o + w] for o, w in cat["cols"]]
    return [run_dense(x_rows, br["pre_x1"]) for br in branches]


FUSE_LAYER1 = True  # backbones built while True fuse a bf16 level's per-point layer-1 GEMMs (A/B switch)


def fused_layer1_x1(branches):
    """The bf16-spec branches' per-point layer-1 weights ("pre_x1") side by side: one dense_stack layer
    (k, sum cp) plus "cols": [(column offset, cp) per branch] — None for fewer than two branches."""
    if len(branches) < 2 or any("pre_x1" not in br for br in branches):
        return None
    ws = [br["pre_x1"]["w"] for br in branches]
    cols, o = [], 0
    for w in ws:
        cols.append((o, w.shape[1]))
        o += w.shape[1]
    w1f = torch.cat(ws, dim=1).contiguous()
    b1 = torch.cat([br["pre_x1"]["b"] for br in branches]).contiguous()
    cat, = dense_stack([(w1f, b1)], "x1", [False], lambda a: a)
    cat["cols"] = cols
    return cat


def group_mlp_x3(p, q, idx, n, packed, widths, out, out_offset=0, xyz_level=False):
    """group_mlp16 with layers 2-3 in h3 arithmetic (scaled fp16 hi/lo pieces on the fp16 MFMAs,
    fp32-class products, see sa_mlp_x3.hip)."""
    B, M, ns = idx.shape
    c1, c2, c3 = widths
    stride = 3 if xyz_level else p.shape[1]
    if xyz_level and not (p.is_contiguous() and q.is_contiguous()):
        raise ValueError("group_mlp_x3: xyz / centres must be contiguous")
    if not xyz_level and (p.shape[0] < B * n or q.shape[0] < B * M or p.shape[1] < c1 or q.shape[1] != p.shape[1]):
        raise ValueError("group_mlp_x3: p/q shapes do not match the batch")
    _dev_check(p, q, idx, packed, out)
    nat.call("lidar_sa_group_mlp_x3_f32", nat.handle(p.device.index), int(xyz_level), nat.ptr(p), stride,
             nat.ptr(q), nat.ptr(idx), B, n, M, ns, c1, c2, c3, nat.ptr(packed), nat.ptr(out), out.shape[-1],
             out_offset, nat.stream_ptr())
    return out


def group_mlp_bq(xyz, centres, grid, radius, nsample, packed, widths, out, out_offset=0, x1=False, out_idx=None):
    """One xyz-level SA branch with its ball queries answered inside the MLP kernel
    (lidar_sa_group_mlp_bq_f32): grid = ball_query_bin(radius, nsample, xyz, ...) of these
    frames; packed = the branch's x3 image (x1=False) or bf16-spec image (x1=True).  Equal bit
    for bit to ball_query(..., grid=grid) then group_mlp_x3 / group_mlp_x1; out_idx (B, M, ns)
    int32, optional, receives the ball-query indices."""
    B, n, _ = xyz.shape
    M = centres.shape[1]
    c1, c2, c3 = widths
    if not (xyz.is_contiguous() and centres.is_contiguous()):
        raise ValueError("group_mlp_bq: xyz / centres must be contiguous")
    if out_idx is not None and (tuple(out_idx.shape) != (B, M, nsample) or out_idx.dtype != torch.int32):
        raise ValueError("group_mlp_bq: out_idx must be (B, M, nsample) int32")
    _dev_check(xyz, centres, grid, packed, out, *([out_idx] if out_idx is not None else []))
    nat.call("lidar_sa_group_mlp_bq_f32", nat.handle(xyz.device.index), int(bool(x1)), nat.ptr(xyz), nat.ptr(grid),
             nat.ptr(centres), B, n, M, float(radius), int(nsample), c1, c2, c3, nat.ptr(packed), nat.ptr(out),
             out.shape[-1], out_offset, nat.ptr(out_idx) if out_idx is not None else None, nat.stream_ptr())
    return out


def _kpad(cfeat):
    """Width of a level's padded input rows [f (cfeat), x, y, z, 0-pad]: k padded to 16."""
    return (cfeat + 3 + 15) // 16 * 16


def pad_layer(w, b, kin):
    """(W (cin, c), b) of a later layer -> (wp (kin, cp), bp (cp,)) float32: rows zero-padded to kin (the
    previous layer's padded width), columns and bias to a multiple of 128 (the dense kernel's tile)."""
    w = np.asarray(w, np.float32)
    cin, c = w.shape
    cp = (c + 127) // 128 * 128
    wp = np.zeros((kin, cp), np.float32)
    wp[:cin, :c] = w
    bp = np.zeros(cp, np.float32)
    bp[:c] = b
    return wp, bp


def layer1_layout(w, b, cfeat, xyz_rows=True):
    """(W1 (3 + cfeat, c), b1) -> (wp (kp, cp), bp (cp,)) in the physical row order every GEMM here
    reads: canonical rows [x, y, z, f...] become [f..., x, y, z, 0-pad] (k padded to 16), columns and
    bias zero-padded to a multiple of 128.  xyz_rows=False leaves the three xyz rows zero (the bf16
    spec's W1_f: the offsets' part runs per grouped row)."""
    w = np.asarray(w, np.float32)
    wp, bp = pad_layer(w[3:], b, _kpad(cfeat))
    if xyz_rows:
        wp[cfeat:cfeat + 3, :w.shape[1]] = w[:3]
    return wp, bp


def pad_chain(layers, kin):
    """[(wp, bp)] of consecutive later layers: pad_layer, each layer's rows padded to the columns of what
    feeds it (kin for the first)."""
    out = []
    for w, b in layers:
        out.append(pad_layer(w, b, kin))
        kin = out[-1][0].shape[1]
    return out


def mlp_layout(layers, cfeat):
    """[(wp, bp)] of a whole MLP: layer1_layout, then every later layer's rows padded to the columns
    of the one before it."""
    first = layer1_layout(*layers[0], cfeat)
    return [first] + pad_chain(layers[1:], first[0].shape[1])


def dense_stack(padded, arith, relus, to_dev):
    """The device operands of dense layers for run_dense: padded = [(wp (k, cp), bp (cp,))] in the padded
    layout (pad_layer / layer1_layout: columns a multiple of 128), arith "x3" (h3 GEMM), "x1" (the bf16
    spec's) or "f32" (the native fp32 GEMM), relus one flag per layer.  -> [{"w", "b", "cout" (= cp), "relu",
    "arith" and, unless f32, "packed": pack_dense_x3's image}].  Moved to the device kind by kind: every w,
    every b, then the images."""
    ws = [to_dev(wp) for wp, _ in padded]
    bs = [to_dev(bp) for _, bp in padded]
    out = [{"w": w, "b": b, "cout": w.shape[1], "relu": bool(relu), "arith": arith}
           for w, b, relu in zip(ws, bs, relus)]
    if arith != "f32":
        for lay in out:
            lay["packed"] = pack_dense_x3(lay["w"], x1=arith == "x1")
    return out


def run_dense(a, layer, slot=0, out=None, pool_rows=0):
    """a (rows, k) through one dense_stack layer: a W + b [ReLU] [max over runs of pool_rows rows], on the
    GEMM of the layer's arithmetic — the one place that chooses between dense and dense_x3s."""
    if layer["arith"] == "f32":
        return dense(a, layer["w"], layer["b"], relu=layer["relu"], pool_rows=pool_rows, out=out)
    return dense_x3s(a, layer["packed"], layer["b"], layer["cout"], relu=layer["relu"], pool_rows=pool_rows,
                     out=out, x1=layer["arith"] == "x1", slot=slot)


def generic_branch_weights(layers, cfeat, to_dev, arith):
    """Dense-GEMM operands of an SA branch of any shape (sa_branch_generic): the dense_stack of mlp_layout
    (layer 1's rows in the grouped rows' order [f..., x, y, z, 0-pad], every layer's columns and the next
    layer's rows zero-padded to a multiple of 128), ReLU after every layer.  arith as dense_stack's."""
    return {"k": _kpad(cfeat), "c3": layers[-1][0].shape[1], "arith": arith,
            "layers": dense_stack(mlp_layout(layers, cfeat), arith, [True] * len(layers), to_dev)}


def sa_branch_generic(feat, cfeat, xyz, centres, idx, gw, out, out_offset=0, max_bytes=1 << 30, slot=0):
    """One SA branch of any (widths, nsample) on the byte-moving kernels of csrc/sa_generic.hip and the
    dense GEMMs: grouped rows [f[idx], xyz[idx] - centre, 0-pad] -> per layer x W + b, ReLU (h3 / bf16
    spec / fp32 as gw["arith"]) -> max over each centre's nsample rows -> out[..., off:off + c3].
    feat: (B, n, >= cfeat) fp32 with unit column stride (None when cfeat = 0); idx (B, M, ns) int32
    (ball_query); gw = generic_branch_weights(...).  Frames run in chunks whose activations stay
    under max_bytes."""
    B, M, ns = idx.shape
    n = xyz.shape[1]
    if out.dim() != 3 or out.shape[0] != B or out.shape[1] != M or out.stride(2) != 1 or out.stride(1) != out.shape[2]:
        raise ValueError("sa_branch_generic: out must be a contiguous (B, M, stride) tensor")
    if out_offset < 0 or out_offset + gw["c3"] > out.shape[2]:
        raise ValueError("sa_branch_generic: out columns out of range")
    if cfeat and (feat is None or feat.shape[0] != B or feat.shape[1] != n or feat.shape[2] < cfeat
                  or feat.stride(2) != 1 or feat.stride(0) != n * feat.stride(1)):
        raise ValueError("sa_branch_generic: feat must be (B, n, >= cfeat) with rows of one stride")
    if not (xyz.is_contiguous() and centres.is_contiguous() and idx.is_contiguous()):
        raise ValueError("sa_branch_generic: xyz / centres / idx must be contiguous")
    _dev_check(xyz, centres, idx, out)
    if cfeat and not feat.is_cuda:  # strided rows (checked above), not necessarily contiguous
        raise ValueError("sa_branch_generic: feat must be a CUDA tensor")
    dev = xyz.device
    h = nat.handle(dev.index, slot)
    kp = gw["k"]
    cmax = max([kp] + [lay["cout"] for lay in gw["layers"]])
    fc = max(1, min(B, max_bytes // max(1, 2 * M * ns * cmax * 4)))
    ldf = feat.stride(1) if cfeat else 0
    for b0 in range(0, B, fc):
        nb = min(B, b0 + fc) - b0
        grouped = nb * M * ns
        R = (grouped + 127) // 128 * 128
        rows = torch.empty((R, kp), dtype=torch.float32, device=dev)
        nat.call("lidar_sa_group_rows_f32", h, nat.ptr(feat[b0:b0 + nb]) if cfeat else None, ldf, cfeat,
                 nat.ptr(xyz[b0:b0 + nb]), nat.ptr(centres[b0:b0 + nb]), nat.ptr(idx[b0:b0 + nb]), nb, n, M, ns,
                 nat.ptr(rows), R, kp, nat.stream_ptr())
        a = rows
        for lay in gw["layers"]:
            a = run_dense(a, lay, slot=slot)
        dst = out[b0:b0 + nb]
        nat.call("lidar_group_max_f32", h, nat.ptr(a), a.shape[1], nb * M, ns, gw["c3"], nat.ptr(dst),
                 out.shape[2], out_offset, nat.stream_ptr())
    return out


def layer1_weights(layer, cfeat, to_dev, arith="f32"):
    """(W1 (3 + cfeat, c1), b1) -> the per-point GEMM operands of layer1_per_point, two dense_stack layers
    without ReLU: "w1" rows [f..., x, y, z, 0-pad] (k padded to 16) with b1, "wq" rows [x, y, z, 0-pad] (16)
    with a zero bias; columns zero-padded to a multiple of 128 (the dense kernel's tile)."""
    w1, b1 = layer
    w1p, bp = layer1_layout(w1, b1, cfeat)
    wq, _ = pad_layer(w1[:3], b1, 16)
    return {"w1": dense_stack([(w1p, bp)], arith, [False], to_dev)[0],
            "wq": dense_stack([(wq, np.zeros_like(bp))], arith, [False], to_dev)[0]}


def centre_layer1(new_xyz, branches, out=None, slot=0):
    """Q = [c, 0-pad] W1_xyz' per centre of a feature level, every branch (the per-centre half of
    layer1_per_point, h3 GEMM; rows B*M rounded up to 128) -> [Q per branch].  out: [(cpad (R, 16) zeroed
    past the centres' rows, Q (R, cp))] per branch, preallocated."""
    B, M, _ = new_xyz.shape
    dev = new_xyz.device
    h = nat.handle(dev.index, slot)
    rq = (B * M + 127) // 128 * 128
    res = []
    for i, br in enumerate(branches):
        cpad, q = out[i] if out is not None else (torch.zeros((rq, 16), dtype=torch.float32, device=dev), None)
        cpad, q = cpad[:rq], (q[:rq] if q is not None else None)
        nat.call("lidar_concat_xyz_pad_f32", h, nat.ptr(new_xyz), B * M, nat.ptr(cpad), 16, 0, nat.stream_ptr())
        res.append(run_dense(cpad, br["pre"]["wq"], slot=slot, out=q))
    return res


def layer1_per_point(x_rows, xyz, cfeat, new_xyz, branches, x3=True):
    """Layer 1 of every branch of a level, per point instead of per grouped row.

    x_rows: (R, kp) padded rows [f (cfeat), x, y, z, 0...] of the level's B*N points
    (R = B*N rounded up to 128; the previous level wrote f in place), xyz (B, N, 3);
    new_xyz (B, M, 3).  Returns per branch (P, Q): P = x_rows W1' + b1 (R, c1),
    Q = [c, 0] W1_xyz' (B*M rounded to 128, c1), both without ReLU (columns padded to a
    multiple of 128 with zero weights), each on the GEMM of its layer1_weights arithmetic.  x3: the
    launch order of the h3 path (every Q by centre_layer1, then every P); else P, Q branch by branch."""
    B, N, _ = xyz.shape
    M = new_xyz.shape[1]
    R, kp = x_rows.shape
    dev = xyz.device
    h = nat.handle(dev.index)
    nat.call("lidar_concat_xyz_pad_f32", h, nat.ptr(xyz), B * N, nat.ptr(x_rows), kp, cfeat, nat.stream_ptr())
    if x3:
        qs = centre_layer1(new_xyz, branches)
        return [(run_dense(x_rows, br["pre"]["w1"]), q) for br, q in zip(branches, qs)]
    rq = (B * M + 127) // 128 * 128
    cpad = torch.zeros((rq, 16), dtype=torch.float32, device=dev)
    nat.call("lidar_concat_xyz_pad_f32", h, nat.ptr(new_xyz), B * M, nat.ptr(cpad), 16, 0, nat.stream_ptr())
    return [(run_dense(x_rows, br["pre"]["w1"]), run_dense(cpad, br["pre"]["wq"])) for br in branches]


def pack_dense_x3(w, x1=False):
    """(k, cout) fp32 CUDA weights -> the dense GEMM's packed image (device): the h3 image (fp16 hi /
    lo of W 2^s, lidar_dense_x3_pack_f32) or, x1, the bf16 spec's image (lidar_dense_x1_pack_f32)."""
    _dev_check(w)
    k, cout = w.shape
    nbytes = nat.load_library().lidar_dense_x3_packed_size(k, cout)
    out = torch.empty((nbytes,), dtype=torch.uint8, device=w.device)
    nat.call("lidar_dense_x1_pack_f32" if x1 else "lidar_dense_x3_pack_f32", nat.handle(w.device.index), nat.ptr(w),
             k, cout, nat.ptr(out), nat.stream_ptr())
    return out


def dense(x, w, b, relu=True, pool_rows=0, out=None):
    """x (rows, k) @ w (k, cout) + b [-> ReLU] [-> max over runs of pool_rows rows] on the native
    fp32 matrix cores (lidar_dense_f32)."""
    rows, k = x.shape
    cout = w.shape[1]
    if out is None:
        shape = (rows // pool_rows, cout) if pool_rows else (rows, cout)
        out = (torch.zeros if pool_rows else torch.empty)(shape, dtype=torch.float32, device=x.device)
    _dev_check(x, w, b, out)
    nat.call("lidar_dense_f32", nat.handle(x.device.index), nat.ptr(x), rows, k, nat.ptr(w), nat.ptr(b), cout,
             1 if relu else 0, pool_rows, nat.ptr(out), nat.stream_ptr())
    return out


def dense_relu(x, w, b, pool_rows=0, out=None):
    return dense(x, w, b, True, pool_rows, out)


def dense_x3s(a, wpack, b, cout, relu=True, pool_rows=0, out=None, x1=False, slot=0):
    """a (rows, k) fp32 @ W + b on the dense GEMM of csrc/dense_x3s.hip (lidar_dense_x3f_f32; wpack =
    pack_dense_x3(W), h3 arithmetic; x1: pack_dense_x3(W, x1=True), the bf16 spec).  Returns fp32
    rows (rows, cout) or, with pool_rows, the fp32 max over runs of pool_rows rows (ReLU)."""
    rows, lda = a.shape
    dev = a.device
    if pool_rows:
        mode = 2
        if out is None:
            out = torch.zeros((rows // pool_rows, cout), dtype=torch.float32, device=dev)
    else:
        mode = 0
        if out is None:
            out = torch.empty((rows, cout), dtype=torch.float32, device=dev)
    _dev_check(a, wpack, b, out)
    nat.call("lidar_dense_x3f_f32", nat.handle(dev.index, slot), nat.ptr(a), lda, rows, lda, nat.ptr(wpack), nat.ptr(b),
             cout, mode | (4 if x1 else 0), 1 if relu else 0, pool_rows, nat.ptr(out), 0, out.shape[1],
             nat.stream_ptr())
    return out


def h3_bounds(w, b):
    """(w_colsum, b_max) of a dense layer for lidar_dense_h3p_f32's mode-1 exponent bound: the largest
    column sum of |W| and the largest |b|, each rounded up to the next float32."""
    cs = np.abs(np.asarray(w, np.float64)).sum(axis=0).max() if np.size(w) else 0.0
    bm = np.abs(np.asarray(b, np.float64)).max() if np.size(b) else 0.0
    up = lambda v: float(np.nextafter(np.float32(v), np.float32(np.inf)))
    return up(cs), up(bm)


def dense_h3p(a, a_exp, wpack, b, cout, mode, bounds=(0.0, 0.0), relu=True, pool_rows=0, out=None):
    """One layer of group_all's h3 chain (lidar_dense_h3p_f32).  A: fp32 rows (rows, k) with a_exp None,
    or h3 planes (2, rows, k) float16 (hi, lo) with a_exp (rows,) int32 — mode 1's output.  mode 0 ->
    fp32 rows (rows, cout); 1 -> (planes (2, rows, cout) float16, exponents (rows,) int32), the next
    layer's A; 2 -> ReLU + max over runs of pool_rows rows (rows / pool_rows, cout) fp32.  bounds: the
    layer's h3_bounds(W, b) (mode 1)."""
    dev = a.device
    # the two operand forms are told apart only by a_exp: check that the tensors match the form, so a
    # mismatch raises instead of being reinterpreted by the kernel
    if a_exp is None:
        if a.dtype != torch.float32 or a.dim() != 2:
            raise ValueError(f"dense_h3p: fp32 rows (rows, k) expected without a_exp, got {a.dtype} {tuple(a.shape)}")
        rows, k = a.shape
    else:
        if a.dtype != torch.float16 or a.dim() != 3 or a.shape[0] != 2:
            raise ValueError(f"dense_h3p: h3 planes (2, rows, k) float16 expected with a_exp, got {a.dtype} "
                             f"{tuple(a.shape)}")
        _, rows, k = a.shape
        if a_exp.dtype != torch.int32 or tuple(a_exp.shape) != (rows,):
            raise ValueError(f"dense_h3p: a_exp must be int32 of shape ({rows},), got {a_exp.dtype} "
                             f"{tuple(a_exp.shape)}")
    lda = k
    if mode not in (0, 1, 2):
        raise ValueError(f"dense_h3p: mode must be 0, 1 or 2, got {mode}")
    if mode == 2 and (pool_rows <= 0 or rows % pool_rows):
        raise ValueError(f"dense_h3p: pool_rows ({pool_rows}) must divide rows ({rows})")
    if mode == 2:
        out = torch.zeros((rows // pool_rows, cout), dtype=torch.float32, device=dev) if out is None else out
        oexp = None
    elif mode == 1:
        out = torch.empty((2, rows, cout), dtype=torch.float16, device=dev) if out is None else out
        oexp = torch.empty(rows, dtype=torch.int32, device=dev)
    else:
        out = torch.empty((rows, cout), dtype=torch.float32, device=dev) if out is None else out
        oexp = None
    _dev_check(a, a_exp, wpack, b, out, oexp)
    nat.call("lidar_dense_h3p_f32", nat.handle(dev.index), nat.ptr(a), lda, rows, k, nat.ptr(a_exp), nat.ptr(wpack),
             nat.ptr(b), cout, mode, 1 if relu else 0, pool_rows, nat.ptr(out), nat.ptr(oexp), cout, float(bounds[0]),
             float(bounds[1]), nat.stream_ptr())
    return (out, oexp) if mode == 1 else out


# --------------------------------------------------- feature propagation (the decoder's operators)
def _rows_check(t, what, rows, cols):
    """t: a CUDA float32 (rows..., >= cols) tensor whose rows have one stride and unit column stride
    (a column slice of padded rows is fine); returns the row stride."""
    if t.dtype != torch.float32 or not t.is_cuda or t.dim() not in (2, 3) or (t.shape[-1] > 1 and t.stride(-1) != 1):
        raise ValueError(f"{what} must be a CUDA float32 tensor of rows with unit column stride")
    shape = (1,) + tuple(t.shape) if t.dim() == 2 else tuple(t.shape)
    stride = (0,) + tuple(t.stride()) if t.dim() == 2 else tuple(t.stride())
    # the stride of a dimension of size 1 is arbitrary: the rows' stride is the first that is not
    if shape[1] > 1:
        ld = stride[1]
    else:
        ld = stride[0] if shape[0] > 1 else shape[2]
    if shape[0] > 1 and shape[1] > 1 and stride[0] != shape[1] * ld:
        raise ValueError(f"{what}: the frames' rows must share one stride")
    if shape[0] * shape[1] != rows or shape[2] < cols or ld < shape[2]:
        raise ValueError(f"{what}: expected {rows} rows of at least {cols} columns, got {tuple(t.shape)}")
    return ld


THREE_NN_CHUNK = 2048  # csrc/feature_prop.hip NN_CH: known points staged in LDS at a time
THREE_NN_WIDE_MIN = 1 << 19  # B * n from which a thread owns four unknown points instead of two


def three_nn(unknown, known, weights=True, slot=0):
    """unknown (B, n, 3), known (B, m, 3) float32 CUDA -> (dist2 (B, n, 3), idx (B, n, 3) int32[, weight
    (B, n, 3)]): per unknown point the three nearest known points of its frame in (distance, index)
    order (exact fp32 (dx*dx + dy*dy) + dz*dz, lowest index on ties; a NaN or +inf distance never wins;
    unfilled slots hold (+inf, 0)) and the inverse-distance weights r_i / ((r_0 + r_1) + r_2), r_i = 1 /
    (sqrt(d2_i) + 1e-8).  m >= 1: one known point gives the weights [1, 0, 0]."""
    _dev_check(unknown, known)
    for t, what in ((unknown, "unknown"), (known, "known")):
        if t.dtype != torch.float32 or t.dim() != 3 or t.shape[2] != 3:
            raise ValueError(f"three_nn: {what} must be (B, n, 3) float32")
    B, n, _ = unknown.shape
    m = known.shape[1]
    if known.shape[0] != B or n < 1 or m < 1:
        raise ValueError(f"three_nn: unknown {tuple(unknown.shape)} and known {tuple(known.shape)} must share B, "
                         "with n >= 1 and m >= 1")
    dev = unknown.device
    d2 = torch.empty((B, n, 3), dtype=torch.float32, device=dev)
    idx = torch.empty((B, n, 3), dtype=torch.int32, device=dev)
    w = torch.empty((B, n, 3), dtype=torch.float32, device=dev) if weights else None
    nat.call("lidar_three_nn_f32", nat.handle(dev.index, slot), nat.ptr(unknown), nat.ptr(known), B, n, m,
             nat.ptr(d2), nat.ptr(idx), nat.ptr(w), nat.stream_ptr())
    return (d2, idx, w) if weights else (d2, idx)


def three_interpolate(known_feats, idx, weight, skip=None, out=None, slot=0):
    """known_feats (B, m, c2), idx / weight (B, n, 3) (three_nn), skip (B, n, c1) or None -> rows
    [(w0 f[i0] + w1 f[i1]) + w2 f[i2] | skip | 0-pad]: out (R, ldo) float32 contiguous with R >= B n and
    ldo % 4 == 0, ldo >= c2 + c1 (default: R = B n rounded up to 128, ldo = c2 + c1 rounded up to 16 —
    the dense GEMMs' A operand); rows past B n are zeroed.  known_feats and skip may be column slices of
    wider rows (unit column stride, one row stride)."""
    _dev_check(idx, weight, out)
    if idx.dim() != 3 or idx.shape[2] != 3 or idx.dtype != torch.int32 or weight.dtype != torch.float32 \
            or tuple(weight.shape) != tuple(idx.shape):
        raise ValueError("three_interpolate: idx (B, n, 3) int32 and weight (B, n, 3) float32 expected")
    B, n, _ = idx.shape
    if known_feats.dim() != 3 or known_feats.shape[0] != B:
        raise ValueError("three_interpolate: known_feats must be (B, m, c2)")
    m, c2 = known_feats.shape[1], known_feats.shape[2]
    if n < 1 or m < 1 or c2 < 1:
        raise ValueError("three_interpolate: n, m and c2 must be at least 1")
    ldk = _rows_check(known_feats, "three_interpolate: known_feats", B * m, c2)
    c1, lds = 0, 0
    if skip is not None:
        if skip.dim() != 3 or skip.shape[0] != B or skip.shape[1] != n:
            raise ValueError("three_interpolate: skip must be (B, n, c1)")
        c1 = skip.shape[2]
        lds = _rows_check(skip, "three_interpolate: skip", B * n, c1) if c1 else 0
    dev = idx.device
    if out is None:
        out = torch.empty(((B * n + 127) // 128 * 128, (c2 + c1 + 15) // 16 * 16), dtype=torch.float32, device=dev)
    if out.dim() != 2 or out.dtype != torch.float32 or out.shape[0] < B * n or out.shape[1] % 4 \
            or out.shape[1] < c1 + c2:
        raise ValueError(f"three_interpolate: out must be (>= {B * n}, ldo) float32 with ldo % 4 == 0 and "
                         f"ldo >= {c1 + c2}, got {tuple(out.shape)}")
    nat.call("lidar_three_interpolate_f32", nat.handle(dev.index, slot), nat.ptr(known_feats), ldk, c2, nat.ptr(idx),
             nat.ptr(weight), nat.ptr(skip) if c1 else None, lds, c1, B, n, m, nat.ptr(out), out.shape[0],
             out.shape[1], nat.stream_ptr())
    return out


def row_argmax(x, c, out=None, slot=0):
    """x (rows, >= c) float32 with unit column stride -> (rows,) int32: argmax over the first c columns,
    lowest index on ties, a NaN counts as the maximum (np.argmax)."""
    if x.dim() != 2 or c < 1:
        raise ValueError("row_argmax: x must be (rows, >= c) with c >= 1")
    ldx = _rows_check(x, "row_argmax: x", x.shape[0], c)
    if out is None:
        out = torch.empty((x.shape[0],), dtype=torch.int32, device=x.device)
    _dev_check(out)
    if out.dtype != torch.int32 or out.numel() != x.shape[0]:
        raise ValueError("row_argmax: out must be (rows,) int32")
    nat.call("lidar_row_argmax_f32", nat.handle(x.device.index, slot), nat.ptr(x), x.shape[0], ldx, int(c),
             nat.ptr(out), nat.stream_ptr())
    return out


def class_people(xyz, labels, cls, eps, min_samples=5, cap=None, slot=0):
    """xyz (B, N, 3) float32, labels (B, N) int32 (segment()'s output), both contiguous on one CUDA device ->
    (instance (B, N) int32, people (B, cap, 2) float64, k (B,) int64, nsel (B,) int64, extent (B, 4)
    float64), device tensors, nothing synchronised.  Per frame: the points of class `cls` with finite
    coordinates, widened to float64 in index order (nsel of them), clustered by DBSCAN(eps, min_samples)
    exactly as lidar_dbscan_f64 / sklearn; instance: a selected point's cluster, -1 for every other point
    (wrong class, non-finite, noise); people[f, :min(k[f], cap)]: the clusters' (x, y) centroids (np.mean of
    the member rows), rows past that untouched; k: the cluster counts (also when above cap; cap defaults to
    N); extent: x_min, x_max, y_min, y_max over all finite points of the frame (lidar_class_people_f32)."""
    _dev_check(xyz, labels)
    if xyz.dtype != torch.float32 or xyz.dim() != 3 or xyz.shape[2] != 3 or xyz.shape[1] < 1:
        raise ValueError("class_people: xyz must be (B, N, 3) float32 with N >= 1")
    B, N, _ = xyz.shape
    if labels.dtype != torch.int32 or tuple(labels.shape) != (B, N):
        raise ValueError(f"class_people: labels must be ({B}, {N}) int32, got {labels.dtype} {tuple(labels.shape)}")
    if labels.device != xyz.device:
        raise ValueError("class_people: xyz and labels must be on the same device")
    cap = N if cap is None else int(cap)
    dev = xyz.device
    instance = torch.empty((B, N), dtype=torch.int32, device=dev)
    people = torch.empty((B, max(cap, 0), 2), dtype=torch.float64, device=dev)
    k = torch.empty((B,), dtype=torch.int64, device=dev)
    nsel = torch.empty((B,), dtype=torch.int64, device=dev)
    extent = torch.empty((B, 4), dtype=torch.float64, device=dev)
    nat.call("lidar_class_people_f32", nat.handle(dev.index, slot), nat.ptr(xyz), nat.ptr(labels), B, N, int(cls),
             float(eps), int(min_samples), cap, nat.ptr(instance), nat.ptr(people), nat.ptr(k), nat.ptr(nsel),
             nat.ptr(extent), nat.stream_ptr())
    return instance, people, k, nsel, extent


# ----------------------------------------------------------------- decoder configuration and weights
# Feature-propagation MLPs, deepest level first (one per encoder level), then the head's hidden layers;
# the input widths follow from the encoder configuration (fp_input_widths), so it serves SSG and MSG.
FP_SSG = {"mlps": [[256, 256], [256, 128], [128, 128, 128]], "head": [128]}


def level_channels(cfg):
    """Feature channels of the encoder's point sets P_0 (the input frame: 0) .. P_L (the last level's output)."""
    return [0] + [sum(w[-1] for w in lvl["mlps"]) for lvl in cfg["levels"]]


def fp_input_widths(cfg, fp_cfg):
    """Per FP level (deepest first) (c2, c1): the channels interpolated from the coarser set and the skip
    channels of the finer one.  Level i propagates P_(L-i) onto P_(L-i-1)."""
    ch = level_channels(cfg)
    L = len(cfg["levels"])
    if len(fp_cfg["mlps"]) != L:
        raise ValueError(f"fp_cfg: {len(fp_cfg['mlps'])} FP levels, the encoder has {L} levels")
    out, c2 = [], ch[L]
    for i, widths in enumerate(fp_cfg["mlps"]):
        if not widths:
            raise ValueError(f"fp_cfg level {i}: an FP level needs at least one layer")
        out.append((c2, ch[L - i - 1]))
        c2 = widths[-1]
    return out


def _fp_layer_dims(cfg, fp_cfg, num_classes):
    """[(name, [(cin, cout) per layer])]: the FP levels ("fp<i>"), then "head" (its hidden layers and the
    classifier)."""
    if num_classes < 1:
        raise ValueError("num_classes must be at least 1")
    dims = []
    for i, ((c2, c1), widths) in enumerate(zip(fp_input_widths(cfg, fp_cfg), fp_cfg["mlps"])):
        dims.append((f"fp{i}", _chain(c2 + c1, widths)))
    dims.append(("head", _chain(dims[-1][1][-1][1], list(fp_cfg["head"]) + [num_classes])))
    return dims


def init_fp_weights(cfg, fp_cfg=FP_SSG, num_classes=2, seed=0):
    """Deterministic random init of the decoder (as init_weights: U(-1/sqrt(cin), 1/sqrt(cin)), BN folded at
    its identity).  Returns {"fp": [level][layer] = (W (cin, cout), b), "head": [layer] = (W, b)}: an FP
    level's rows are [interpolated (c2), skip (c1)]; the head's last layer is the classifier (no ReLU)."""
    rng = np.random.default_rng(seed)
    trees = [_draw_layers(rng, lay) for _, lay in _fp_layer_dims(cfg, fp_cfg, num_classes)]
    return {"fp": trees[:-1], "head": trees[-1]}


def check_fp_weights(cfg, fp_cfg, num_classes, fp_weights):
    """Validate {"fp": [level][layer], "head": [layer]} = (W (cin, cout), b (cout,)) against the widths cfg,
    fp_cfg and num_classes give; returns them as contiguous float32 arrays.  Raises ValueError naming the
    first mismatch."""
    dims = _fp_layer_dims(cfg, fp_cfg, num_classes)
    if not isinstance(fp_weights, dict) or "fp" not in fp_weights or "head" not in fp_weights:
        raise ValueError("fp_weights must be a dict with the keys 'fp' and 'head'")
    if len(fp_weights["fp"]) != len(dims) - 1:
        raise ValueError(f"fp_weights: {len(fp_weights['fp'])} FP levels, the configuration has {len(dims) - 1}")
    trees = [_check_layers(f"fp_weights {name}", lay, layers)
             for (name, lay), layers in zip(dims, list(fp_weights["fp"]) + [fp_weights["head"]])]
    return {"fp": trees[:-1], "head": trees[-1]}


def save_fp_weights(path, fp_weights):
    """Decoder weights to an .npz of plain arrays (keys fp<level>_<layer>_{W,b}, head_<layer>_{W,b})."""
    arrs = _layer_arrays("head", fp_weights["head"])
    for i, layers in enumerate(fp_weights["fp"]):
        arrs.update(_layer_arrays(f"fp{i}", layers))
    np.savez(path, **arrs)


def load_fp_weights(path, cfg, fp_cfg=FP_SSG, num_classes=2):
    """The .npz save_fp_weights wrote (loaded with allow_pickle=False), validated by check_fp_weights."""
    with np.load(path, allow_pickle=False) as z:
        w = {"fp": [_read_layers(z, f"fp{i}", len(widths)) for i, widths in enumerate(fp_cfg["mlps"])],
             "head": _read_layers(z, "head", len(fp_cfg["head"]) + 1)}
    return check_fp_weights(cfg, fp_cfg, num_classes, w)


# ----------------------------------------------------------------------- backbone
class _Timers:
    """Optional per-launch HIP-event timing on the launching stream (bench.py): per kernel name
    the launches made, each with the number of frames it processed."""

    def __init__(self):
        self.ev = {}

    def __call__(self, name, frames, fn, *a, **k):
        s = torch.cuda.current_stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        out = fn(*a, **k)
        e1.record(s)
        self.ev.setdefault(name, []).append((e0, e1, int(frames)))
        return out

    def totals(self):
        """{name: (launches, frames over all launches, total ms)} (waits for the events)."""
        return {k: (len(v), sum(f for _, _, f in v), sum(a.elapsed_time(b) for a, b, _ in v))
                for k, v in self.ev.items()}

    def mean_ms(self):
        return {k: t / n for k, (n, _, t) in self.totals().items()}


def _call(timers, name, frames, fn, *a, **k):
    return timers(name, frames, fn, *a, **k) if timers is not None else fn(*a, **k)


def _tag(li, lvl, bi):
    """A branch's launch-tag prefix (the timers' keys): sa<level>, and _b<branch> on a multi-branch level."""
    return f"sa{li + 1}" + (f"_b{bi}" if len(lvl["branches"]) > 1 else "")


class PointNet2Backbone:
    """SSG / MSG PointNet++ encoder on liblidar_amd.  ``forward(xyz)`` -> global feature
    (B, C_last) plus, with keep_levels, per level (new_xyz, features, fps_idx, [ball-query
    idx per branch])."""

    def __init__(self, cfg=SSG, weights=None, device="cuda", seed=0, dtype="f32", x3=True):
        """dtype "f32" (the fp32 contract: features within 1e-4 of the fp32 oracle): x3=True (default)
        runs the MLPs on the fp16 matrix cores in h3 arithmetic (lidar_sa_group_mlp_x3_f32,
        lidar_dense_x3f_f32), x3=False on the native fp32 matrix cores (lidar_sa_group_mlp16_f32,
        lidar_dense_f32) — the strict-fp32 path.
        dtype "bf16" (BASELINE configs[4]): the SA branches in the bf16 spec on the X1 kernels
        (inputs, activations and weights rounded to bf16, fp32 accumulation); group_all stays in
        fp32 arithmetic on the x3 GEMM.
        Levels with point features run layer 1 per point (layer1_per_point / layer1_points_x1) and
        the fused kernel from layer 2 on.

        cfg: any SSG / MSG configuration (levels of radii / nsamples / mlps with three layers per
        branch, then optionally group_all).  The fused branch kernels are instantiated for the six
        (xyz level, c1, c2, c3, nsample) shapes of MLP16_SHAPES (the SSG / MSG configurations of
        SURVEY §8a); a branch of any other shape runs sa_branch_generic — its grouped rows
        materialised in HBM, the same dense GEMMs (same arithmetic: h3, bf16 spec or fp32), then the
        max over nsample — with the same results contract and HBM-bound speed."""
        if dtype not in ("f32", "bf16"):
            raise ValueError("dtype must be 'f32' or 'bf16'")
        self.bf16 = dtype == "bf16"
        self.x3 = bool(x3) or self.bf16  # the dense GEMMs (per-point layer 1, group_all)
        self.cfg = cfg
        self.device = torch.device(device)
        self.weights = weights if weights is not None else init_weights(cfg, seed)
        self.levels = []
        cfeat = 0
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.device)
        for lvl, wl in zip(cfg["levels"], self.weights):
            if lvl.get("group_all"):
                self.levels.append(self._build_group_all(wl[0], cfeat, t))
                cfeat = self.levels[-1]["cout"]
                continue
            branches = [self._build_branch(r, ns, widths, layers, cfeat, t)
                        for r, ns, widths, layers in zip(lvl["radii"], lvl["nsamples"], lvl["mlps"], wl)]
            entry = {"div": lvl["npoint_div"], "branches": branches, "cfeat": cfeat}
            if cfeat:  # the previous level writes this level's padded rows [f, x, y, z, 0]
                entry.update(pre=True, k=_kpad(cfeat))
                if self.bf16 and FUSE_LAYER1 and all("pre_x1" in br for br in branches):
                    entry["pre_x1_cat"] = fused_layer1_x1(branches)  # one layer-1 GEMM for every branch
            self.levels.append(entry)
            cfeat = sum(w[-1] for w in lvl["mlps"])
        self.out_channels = cfeat
        self.timers = None  # set to a _Timers() to time every launch

    def _build_group_all(self, layers, cfeat, t):
        """The group_all level's entry: "layers", the dense_stack of its MLP in mlp_layout, and, for the
        h3 chain, each layer's exponent bounds."""
        lay = mlp_layout(layers, cfeat)
        entry = {"group_all": True, "k": _kpad(cfeat), "cfeat": cfeat, "cout": layers[-1][0].shape[1],
                 "layers": dense_stack(lay, "x3" if self.x3 else "f32", [True] * len(lay), t)}
        if self.x3:
            entry["h3_bounds"] = [h3_bounds(w, b) for w, b in lay]
        return entry

    def _build_branch(self, r, ns, widths, layers, cfeat, t):
        """One SA branch's entry.  "kind", decided here once, is what forward() switches on: "x1" (bf16
        spec), "x3" (h3) or "f32" (native fp32) — the fused kernel of that arithmetic, its image under
        "packed_x1" / "packed_x3" / "packed16" and, on a feature level, the per-point layer-1 operands
        under "pre_x1" / "pre" — or "generic": no fused kernel for this shape, grouped rows in HBM + the
        dense GEMMs of the same arithmetic (sa_branch_generic)."""
        xyz_level = cfeat == 0
        arith = "x1" if self.bf16 else ("x3" if self.x3 else "f32")
        br = {"r": r, "ns": ns, "widths": widths, "kind": arith}
        if (xyz_level, *widths, ns) not in MLP16_SHAPES:
            br.update(kind="generic", generic=generic_branch_weights(layers, cfeat, t, arith))
            return br
        key, pk = _IMAGE[arith]
        br[key] = torch.from_numpy(_pack_branch(pk, layers, xyz_level)).to(self.device)
        if not xyz_level and arith == "x1":  # W1_f: rows [f..., (x, y, z) = 0, 0-pad], columns to 128
            br["pre_x1"], = dense_stack([layer1_layout(*layers[0], cfeat, xyz_rows=False)], "x1", [False], t)
        elif not xyz_level:
            br["pre"] = layer1_weights(layers[0], cfeat, t, arith)
        return br

    def _grid_buffer(self, B, N, device):
        """The ball-query grid buffer forward() bins xyz levels into (grown on demand, reused by
        every branch and call on this backbone's stream)."""
        need = nat.load_library().lidar_ball_query_grid_bytes(B, N)
        if getattr(self, "_grid", None) is None or self._grid.numel() < need:
            self._grid = torch.empty((max(1, need),), dtype=torch.uint8, device=device)
        return self._grid

    def forward_from_sa1_fps(self, xyz, idx1, new_xyz1, fz1, gidx1=None, keep_levels=False, grids1=None, pre2=None):
        """forward() with level 0's FPS (and its ball queries: gidx1, or their binning: grids1)
        already computed (StreamingSSG); pre2: level 1's {"fps": ..., "bq": ...} likewise."""
        pre = {0: {"fps": (idx1, new_xyz1, fz1), "bq": gidx1, "grid": grids1}}
        if pre2 is not None:
            pre[1] = pre2
        return self.forward(xyz, keep_levels, pre=pre)

    def forward(self, xyz, keep_levels=False, pre=None):
        """pre: {level: {"fps": (idx, new_xyz, first_zero), "bq": [gidx per branch] | "grid": [ball_query_bin
        buffer per branch]}} — work already done for those levels (StreamingSSG's side streams);
        every other step runs here."""
        pre = pre or {}
        B, N, _ = xyz.shape
        N0 = N  # npoint_div is relative to the input frame (N/16, N/64)
        feats = None
        rows = None  # flat padded (R, k) rows behind `feats` when the next level reads them
        out_levels = []
        fz = None  # previous level's FPS first_zero (nested-FPS shortcut)
        t = self.timers
        for li, lvl in enumerate(self.levels):
            if lvl.get("group_all"):
                g = self._group_all(xyz, feats, lvl, rows)
                return (g if g.shape[1] == lvl["cout"] else g[:, :lvl["cout"]].contiguous()), out_levels
            M = max(1, N0 // lvl["div"])
            pl = pre.get(li, {})
            if pl.get("fps") is not None:
                idx, new_xyz, nfz = pl["fps"]
            else:
                nfz = torch.empty(B, dtype=torch.int32, device=xyz.device)
                idx, new_xyz = _call(t, f"sa{li + 1}_fps", B, farthest_point_sample, xyz, M, return_xyz=True,
                                     first_zero=nfz, prefix_ok=fz)
            fz = nfz
            ctot = sum(br["widths"][-1] for br in lvl["branches"])
            nxt = self.levels[li + 1] if li + 1 < len(self.levels) else None
            # a level feeding group_all or a per-point layer 1 writes straight into the
            # next level's padded input rows [f, x, y, z, 0-pad] (R = B*M rounded to 128)
            padded = nxt is not None and (nxt.get("group_all") or nxt.get("pre"))
            stride = nxt["k"] if padded else ctot
            R = (B * M + 127) // 128 * 128 if padded else B * M
            out_rows = torch.empty((R, stride), dtype=torch.float32, device=xyz.device)
            out = out_rows[:B * M].view(B, M, stride)
            pq = {}  # per-point layer 1 of the fused-kernel branches: {branch index: rows}
            fb = [i for i, br in enumerate(lvl["branches"]) if br["kind"] != "generic"]
            if lvl.get("pre") and fb:
                fbr = [lvl["branches"][i] for i in fb]
                if self.bf16:
                    cat = lvl.get("pre_x1_cat") if len(fbr) == len(lvl["branches"]) else None
                    res = _call(t, f"sa{li + 1}_layer1_points", B, layer1_points_x1, rows, xyz, lvl["cfeat"], fbr,
                                cat=cat)
                else:
                    res = _call(t, f"sa{li + 1}_layer1_points", B, layer1_per_point, rows, xyz, lvl["cfeat"],
                                new_xyz, fbr, x3=self.x3)
                pq = dict(zip(fb, res))
            off, gidxs = 0, []
            for bi_, br in enumerate(lvl["branches"]):
                gidxs.append(self._branch(li, bi_, xyz, new_xyz, feats, pq.get(bi_), out, off, pl, keep_levels))
                off += br["widths"][-1]
            if keep_levels:
                out_levels.append((new_xyz, out[..., :ctot], idx, gidxs))
            xyz, feats, rows = new_xyz, (out[..., :ctot] if padded else out), out_rows
            N = M
        return feats, out_levels

    def _branch(self, li, bi, xyz, new_xyz, feats, pq, out, off, pl, keep_levels):
        """Branch bi of level li into out[..., off:off + c3]; returns its ball-query indices (None when
        the MLP kernel answered its own queries and keep_levels is off).  pq: the branch's per-point
        layer-1 rows (a fused-kernel branch of a feature level), else None; pl: forward()'s pre[li]."""
        t = self.timers
        B, N, _ = xyz.shape
        lvl = self.levels[li]
        br, tag = lvl["branches"][bi], _tag(li, lvl, bi)
        kind, r, ns, widths = br["kind"], br["r"], br["ns"], br["widths"]
        # work done elsewhere for this branch (StreamingSSG's side streams): its ball-query
        # indices, or the binning of its frames (None per branch: not done)
        pb = pl["bq"][bi] if pl.get("bq") is not None else None
        pg = pl["grid"][bi] if pl.get("grid") is not None else None
        if kind in ("x1", "x3") and pq is None and pb is None and (pg is not None or N >= BQ_GRID_MIN_N):
            # xyz level: the MLP kernel answers the ball queries from the frame's grid
            if pg is None:
                pg = _call(t, f"{tag}_bq_bin", B, ball_query_bin, r, ns, xyz, self._grid_buffer(B, N, xyz.device))
            gidx = (torch.empty((B, new_xyz.shape[1], ns), dtype=torch.int32, device=xyz.device)
                    if keep_levels else None)
            _call(t, f"{tag}_group_mlp", B, group_mlp_bq, xyz, new_xyz, pg, r, ns, br[_IMAGE[kind][0]], widths,
                  out=out, out_offset=off, x1=kind == "x1", out_idx=gidx)
            return gidx
        gidx = pb if pb is not None else _call(t, f"{tag}_ball_query", B, ball_query, r, ns, xyz, new_xyz, grid=pg)
        if kind == "generic":
            _call(t, f"{tag}_group_mlp", B, sa_branch_generic, feats, lvl["cfeat"], xyz, new_xyz, gidx,
                  br["generic"], out, off)
        elif kind == "x1":  # a feature level reads the per-point layer-1 rows, and the points beside them
            _call(t, f"{tag}_group_mlp", B, group_mlp_x1, pq if pq is not None else xyz, gidx, N, br["packed_x1"],
                  widths, out=out, out_offset=off, xyz=xyz if pq is not None else None, centres=new_xyz)
        else:
            p16, q16 = pq if pq is not None else (xyz, new_xyz)
            _call(t, f"{tag}_group_mlp", B, group_mlp_x3 if kind == "x3" else group_mlp16, p16, q16, gidx, N,
                  br[_IMAGE[kind][0]], widths, out=out, out_offset=off, xyz_level=pq is None)
        return gidx

    def _group_all(self, xyz, feats, lvl, rows=None):
        B, M, _ = xyz.shape
        kp, cfeat = lvl["k"], lvl["cfeat"]
        # the previous level wrote its features into padded rows [f, x, y, z, 0-pad]
        x = rows[:B * M].view(B, M, kp) if rows is not None and rows.shape[1] == kp else None
        if x is None:  # previous level did not pre-pad (only when group_all is level 0)
            x = torch.empty((B, M, kp), dtype=torch.float32, device=xyz.device)
            if feats is not None:
                x[..., :cfeat] = feats
        nat.call("lidar_concat_xyz_pad_f32", nat.handle(xyz.device.index), nat.ptr(xyz), B * M,
                 nat.ptr(x), kp, cfeat, nat.stream_ptr())
        rows = B * M
        x2 = x.view(rows, kp)
        if M % 128:
            # the MFMA tiles want 128-row runs: pad each frame with copies of its first row
            # (the max-pool is invariant to duplicated rows)
            mp = (M + 127) // 128 * 128
            sel = torch.cat([torch.arange(M, device=x.device),
                             torch.zeros(mp - M, dtype=torch.long, device=x.device)])
            x2 = x.view(B, M, kp)[:, sel].reshape(B * mp, kp).contiguous()
            M, rows = mp, B * mp
        t = self.timers
        l1, l2, l3 = lvl["layers"]
        if self.x3:  # h3 planes between the layers (split once, by the producer); dense3 fuses the max-pool
            bd = lvl["h3_bounds"]
            h1, e1 = _call(t, "sa3_dense1", B, dense_h3p, x2, None, l1["packed"], l1["b"], l1["cout"], 1, bd[0])
            h2, e2 = _call(t, "sa3_dense2", B, dense_h3p, h1, e1, l2["packed"], l2["b"], l2["cout"], 1, bd[1])
            return _call(t, "sa3_dense3_pool", B, dense_h3p, h2, e2, l3["packed"], l3["b"], l3["cout"], 2, pool_rows=M)
        h1 = _call(t, "sa3_dense1", B, run_dense, x2, l1)
        h2 = _call(t, "sa3_dense2", B, run_dense, h1, l2)
        out = torch.zeros((rows // M, l3["cout"]), dtype=torch.float32, device=x.device)
        return _call(t, "sa3_dense3_pool", B, run_dense, h2, l3, pool_rows=M, out=out)

    __call__ = forward


# ---------------------------------------------------------------------- segmentation
class PointNet2Segmenter:
    """PointNet++ per-point segmentation on liblidar_amd: a PointNet2Backbone, its feature-propagation
    decoder (three_nn -> three_interpolate -> shared MLP per level, deepest first) and a per-point head
    (ReLU layers, then a linear classifier).  ``forward(xyz)`` -> logits (B, N, num_classes);
    ``segment(xyz)`` -> labels (B, N) int32 (argmax, lowest class on ties)."""

    def __init__(self, cfg=SSG, fp_cfg=FP_SSG, num_classes=2, weights=None, fp_weights=None, device="cuda", seed=0,
                 x3=True):
        """weights / fp_weights: the encoder's (init_weights layout) and the decoder's (init_fp_weights
        layout); default: their deterministic random init from `seed`.  x3=True runs the decoder's layers
        in h3 arithmetic on the fp16 matrix cores (lidar_dense_x3f_f32), x3=False on the native fp32 ones
        (lidar_dense_f32), as the backbone's MLPs."""
        self.backbone = PointNet2Backbone(cfg, weights=weights, device=device, seed=seed, x3=x3)
        self.cfg, self.fp_cfg, self.num_classes = cfg, fp_cfg, int(num_classes)
        self.device, self.x3 = self.backbone.device, bool(x3)
        self.fp_weights = (check_fp_weights(cfg, fp_cfg, num_classes, fp_weights) if fp_weights is not None
                           else init_fp_weights(cfg, fp_cfg, num_classes, seed))
        self.fp = []
        cp = 0
        arith, t = "x3" if self.x3 else "f32", lambda a: torch.from_numpy(a).to(self.device)
        for (c2, c1), layers in zip(fp_input_widths(cfg, fp_cfg), self.fp_weights["fp"]):
            ldo = (c2 + c1 + 15) // 16 * 16  # the interpolated rows' stride: k of the level's first GEMM
            lay = dense_stack(pad_chain(layers, ldo), arith, [True] * len(layers), t)
            self.fp.append({"c2": c2, "c1": c1, "ldo": ldo, "layers": lay, "cout": layers[-1][0].shape[1]})
            cp = lay[-1]["cout"]
        head = self.fp_weights["head"]
        # the classifier: no ReLU
        self.head = dense_stack(pad_chain(head, cp), arith, [True] * (len(head) - 1) + [False], t)

    def point_sets(self, xyz, levels, global_feat):
        """[(xyz, features or None)] of P_0 (the frame) .. P_L from forward(keep_levels=True)'s output: a
        group_all level is one point (at the origin: with one known point the weights are [1, 0, 0]
        wherever it lies) carrying the global feature."""
        sets = [(xyz, None)] + [(lv[0], lv[1]) for lv in levels]
        if self.cfg["levels"][-1].get("group_all"):
            B = xyz.shape[0]
            sets.append((torch.zeros((B, 1, 3), dtype=torch.float32, device=xyz.device),
                         global_feat.reshape(B, 1, -1)))
        if len(sets) != len(self.cfg["levels"]) + 1:
            raise ValueError(f"decode: {len(levels)} encoder levels given, the configuration has "
                             f"{len(self.cfg['levels'])}")
        return sets

    def _frame_bytes(self, sets):
        """Upper estimate of one frame's live decoder activations: per level its padded rows and two layer
        outputs."""
        L = len(self.fp)
        need = 0
        for i, fp in enumerate(self.fp):
            n = sets[L - i - 1][0].shape[1]
            wide = max(lay["cout"] for lay in fp["layers"] + (self.head if i == L - 1 else []))
            need = max(need, n * 4 * (fp["ldo"] + 2 * wide))
        return need

    def decode(self, xyz, levels, global_feat, keep_levels=False, max_bytes=1 << 30):
        """The decoder on an encoder pass: xyz (B, N, 3), levels = per SA level (new_xyz (B, M, 3),
        features (B, M, C), ...) and global_feat (B, C) as PointNet2Backbone.forward(xyz,
        keep_levels=True) returns them.  -> logits (B, N, num_classes); with keep_levels also {"fp": per FP
        level (deepest first) {"rows": the interpolated rows [interp | skip] (B, n, c2 + c1), "idx",
        "weight", "feats": the level's output (B, n, cout)}, "head": the head's last hidden layer
        (B, N, c)}.  Frames run in chunks whose activations stay under max_bytes (every operator is per
        frame: the chunking does not change a bit)."""
        sets = self.point_sets(xyz, levels, global_feat)
        _dev_check(xyz)
        B, N, _ = xyz.shape
        nc = self.num_classes
        logits = torch.empty((B, N, nc), dtype=torch.float32, device=xyz.device)
        fc = max(1, min(B, max_bytes // max(1, self._frame_bytes(sets))))
        # the neighbours depend on the point sets alone (36 bytes per point): one launch per level over the
        # whole batch, ahead of the chunks
        t, L = self.backbone.timers, len(self.fp)
        nn = [_call(t, f"fp{i}_three_nn", B, three_nn, sets[L - i - 1][0], sets[L - i][0])[1:] for i in range(L)]
        kept = []
        for b0 in range(0, B, fc):
            part = [(x[b0:b0 + fc], f[b0:b0 + fc] if f is not None else None) for x, f in sets]
            a, k = self._decode_frames(part, [(i[b0:b0 + fc], w[b0:b0 + fc]) for i, w in nn], keep_levels)
            nb = part[0][0].shape[0]
            logits[b0:b0 + nb] = a[:nb * N, :nc].view(nb, N, nc)
            kept.append(k)
        if not keep_levels:
            return logits
        cat = lambda ts: ts[0] if len(ts) == 1 else torch.cat(ts, dim=0)
        out = {"fp": [{key: cat([k["fp"][i][key] for k in kept]) for key in kept[0]["fp"][i]}
                      for i in range(len(self.fp))],
               "head": cat([k["head"] for k in kept])}
        return logits, out

    def _decode_frames(self, sets, nn, keep):
        """Every FP level and the head on the frames of `sets` (nn: per FP level their three_nn (idx, weight));
        -> (the classifier's padded rows (R, 128 k), what decode() keeps)."""
        t = self.backbone.timers
        L = len(self.fp)
        kxyz, kfeat = sets[L]
        kept = {"fp": [], "head": None}
        a = None
        for i, fp in enumerate(self.fp):
            uxyz, skip = sets[L - i - 1]
            nb, n, _ = uxyz.shape
            c2, c1 = fp["c2"], fp["c1"]
            if kfeat.shape[2] != c2 or (c1 and (skip is None or skip.shape[2] != c1)):
                raise ValueError(f"decode: FP level {i} expects {c2} coarse and {c1} skip channels")
            idx, w = nn[i]
            rows = torch.empty(((nb * n + 127) // 128 * 128, fp["ldo"]), dtype=torch.float32, device=uxyz.device)
            _call(t, f"fp{i}_interpolate", nb, three_interpolate, kfeat, idx, w, skip if c1 else None, rows)
            a = rows
            for j, lay in enumerate(fp["layers"]):
                a = _call(t, f"fp{i}_dense{j + 1}", nb, run_dense, a, lay)
            feats = a[:nb * n].view(nb, n, a.shape[1])[..., :fp["cout"]]
            if keep:
                kept["fp"].append({"rows": rows[:nb * n].view(nb, n, fp["ldo"])[..., :c2 + c1], "idx": idx, "weight": w,
                                   "feats": feats})
            kxyz, kfeat = uxyz, feats
        nb, n, _ = kxyz.shape
        for j, lay in enumerate(self.head):
            if keep and j == len(self.head) - 1:
                kept["head"] = a[:nb * n].view(nb, n, a.shape[1])[..., :self.fp_weights["head"][-1][0].shape[0]]
            a = _call(t, f"head_dense{j + 1}", nb, run_dense, a, lay)
        return a, kept

    def forward(self, xyz, max_bytes=1 << 30):
        """xyz (B, N, 3) float32 CUDA -> logits (B, N, num_classes): the encoder pass with its levels kept,
        then decode()."""
        g, levels = self.backbone.forward(xyz, keep_levels=True)
        return self.decode(xyz, levels, g, max_bytes=max_bytes)

    def segment(self, xyz, max_bytes=1 << 30):
        """-> labels (B, N) int32: the argmax of forward()'s logits over the classes (lowest class on ties,
        a NaN counts as the maximum)."""
        logits = self.forward(xyz, max_bytes=max_bytes)
        B, N, nc = logits.shape
        return row_argmax(logits.view(B * N, nc), nc).view(B, N)

    def people(self, xyz, person_class, eps, min_samples=5, metric_xyz=None):
        """-> (labels, (instance, people, k, nsel, extent)): segment(xyz), then class_people of the points
        labelled `person_class`.  The network sees xyz (normalised coordinates); the clustering runs on
        metric_xyz (the same points in metres, (B, N, 3) float32) when given, else on xyz."""
        labels = self.segment(xyz)
        return labels, class_people(xyz if metric_xyz is None else metric_xyz, labels, person_class, eps, min_samples)

    __call__ = forward


# ------------------------------------------------------------------ streaming executor
class _Slot:
    """One staging slot of StreamingSSG: the group's frames, what a side stream computes from them, and the
    two events of the hand-off.  levels: per side-stream level (StreamingSSG.side) forward()'s `pre`
    entry over the slot's G*B frames — {"fps": (idx, centroids, first_zero), "bq": [ball-query indices
    per branch] or None, "grid": [ball_query_bin buffer per branch] or None}."""

    def __init__(self, stage, levels, main):
        self.stage = stage  # (G*B, N, 3); with G = 1 allocated once a host batch needs it (StreamingSSG._stage)
        self.staged = stage is not None  # the slot's group lives in stage (else in the caller's batch)
        self.levels = levels
        self.fps_done = torch.cuda.Event()  # recorded by the side stream behind the group's work
        self.slot_free = torch.cuda.Event()  # recorded by the main stream behind the pass that read the slot
        self.slot_free.record(main)

    def pre(self, g, clone=False):
        """forward()'s `pre` mapping for the slot's first g frames: views, or with clone copies (made on
        the current stream).  The grids cover whole frames and are read in place."""
        cut = (lambda a: a[:g].clone()) if clone else (lambda a: a[:g])
        return {li: {"fps": tuple(cut(a) for a in lv["fps"]),
                     "bq": [cut(a) for a in lv["bq"]] if lv["bq"] is not None else None, "grid": lv["grid"]}
                for li, lv in enumerate(self.levels)}


class StreamingSSG:
    """Frame-batch pipeline for a continuous feed (SSG/MSG backbone).

    SA1's farthest-point sampling is a serial chain of N/16 argmax steps per frame
    (latency-bound, one workgroup per frame), while everything after it (fused MFMA MLPs,
    SA2's nested FPS and ball queries, group_all) fills the whole GPU.  Later batches' SA1 FPS
    and level-0 ball queries therefore run on `depth` side streams (own library handles /
    workspaces) while earlier batches' remaining levels run on the main stream; events order
    the hand-off and a ring of `slots` (default depth + 3) staging slots bounds memory.

    fps_group = G > 1: G consecutive batches are staged into one (G*B, N, 3) buffer; one
    side-stream launch runs their SA1 FPS (G*B workgroups share the serial chain of steps
    without needing more streams than the device's hardware queues) and one main-stream
    pass runs their MFMA levels (larger launches fill the chip better).  Every operator is
    per frame, so results are identical to ``PointNet2Backbone.forward`` per batch.

    ``run(batches)`` processes a finite list (pipeline fill and drain included); ``feed()``
    returns a persistent feed whose ``push(batch)`` keeps `depth` groups in flight (the steady
    state of a LiDAR stream) and ``flush()`` drains it.
    """

    def __init__(self, backbone, batch, n, depth=1, fps_group=1, fps_threads=0, side_priority=0,
                 ramp=True,
                 reserve=True, keep_levels=False, slots=None, bq="bin", l2_side=False):
        """fps_threads: SA1 FPS workgroup size (0 = 1024; 512: half the CU footprint beside the
        MLPs).  ramp: in run(), the first groups hold 1, 2, ... batches (a shorter pipeline fill).
        slots: staging slots (>= depth + 1; default depth + 3).  Group k's FPS reuses the slot of
        group k - slots, so it waits for that group's main-stream pass: with depth + 1 slots the
        side chain could only start a group once the main stream was `depth` groups behind it,
        which left the main stream idle whenever FPS took about `depth` main passes.
        keep_levels: every output is (global feature, per-level (new_xyz, features, fps idx,
        [ball-query idx per branch])) instead of the global feature alone.  l2_side: level 1's FPS
        (nested: the prefix shortcut over SA1's centroids) and ball queries depend only on SA1's
        FPS output, so they run on the side stream too (the main stream then runs only MLP work
        and level 1's per-point layer 1).

        Host frames: feed().push_host(frames) takes a batch of host NumPy frames, stages it in
        pinned memory (parallel host threads) and copies it to the device on the group's side
        stream ahead of its FPS (the PCIe-inclusive feed; results equal push() of the same data)."""
        self.bb = backbone
        self.B, self.N, self.depth, self.G = batch, n, depth, max(1, int(fps_group))
        self.ramp = bool(ramp)
        self.fps_threads = int(fps_threads)
        self.keep = bool(keep_levels)
        if bq not in ("side", "bin", "main"):
            raise ValueError("StreamingSSG: bq must be 'side', 'bin' or 'main'")
        self.bq = bq
        dev = backbone.device
        # side_priority < 0 puts the latency-bound FPS chains ahead of the MLP waves in the
        # dispatcher (HIP stream priority); results do not depend on it
        # the process's shared side streams: a pipeline created after another keeps its queues
        # (streams.py: fresh streams can land on the main stream's hardware queue)
        self.fps_streams = side_streams(dev, depth, priority=side_priority)
        nslot = depth + 3 if slots is None else int(slots)
        if nslot < depth + 1:
            raise ValueError("StreamingSSG: slots must be >= depth + 1")
        self.nslot = nslot
        GB = self.G * batch
        # the levels whose FPS the side streams run: (level, centroids per frame, ball queries there,
        # their binning there).  Level 0's queries run there with bq="side"; with "bin" the MLP kernel
        # answers them on the main stream from the side streams' grids
        lv = backbone.levels
        self.side = [(lv[0], max(1, n // lv[0]["div"]), bq == "side", bq == "bin")]
        if l2_side and len(lv) > 1 and not lv[1].get("group_all"):
            self.side.append((lv[1], max(1, n // lv[1]["div"]), True, False))
        # the slots' buffers, allocated kind by kind over all slots (not slot by slot): the order, and so the
        # placement in device memory, under which the executor's recorded speeds were measured
        new = lambda dtype, *shape: [torch.empty(shape, dtype=dtype, device=dev) for _ in range(nslot)]
        stage = new(torch.float32, GB, n, 3) if self.G > 1 else [None] * nslot
        levels = [[] for _ in range(nslot)]
        for lvl, M, idx, grid in self.side:
            fps = zip(new(torch.int32, GB, M), new(torch.float32, GB, M, 3), new(torch.int32, GB))
            for sl, f in zip(levels, fps):
                sl.append({"fps": f,
                           "bq": [torch.empty((GB, M, br["ns"]), dtype=torch.int32, device=dev)
                                  for br in lvl["branches"]] if idx else None,
                           "grid": [ball_query_grid_buffer(GB, n, dev) for _ in lvl["branches"]] if grid else None})
        # setup-time workspace sizing of the side handles (FPS + ball queries), so no stage's
        # first call grows a workspace (lidar_reserve; growth retires the old block, no device sync)
        if reserve:
            lib = nat.load_library()
            need = max(lib.lidar_fps_workspace_bytes(GB, n), lib.lidar_ball_query_grid_bytes(GB, n))
            for sl in range(1, depth + 1):
                nat.call("lidar_reserve", nat.handle(dev.index, sl), need)
        main = torch.cuda.current_stream(dev)
        self.slots = [_Slot(st, pre, main) for st, pre in zip(stage, levels)]

    def _stage(self, s, fs, main):
        """The slot's staging buffer (allocated on first use when G = 1) — from the pool of the side stream
        that writes it: a block the caching allocator took from the main stream's pool could be one a
        main-stream pass still queued on the device has just freed, and the side stream does not wait
        for the main stream.  Main-stream passes read it too (record_stream: its block outlives them)."""
        if s.stage is None:
            with torch.cuda.stream(fs):
                s.stage = torch.empty((self.G * self.B, self.N, 3), dtype=torch.float32, device=self.bb.device)
            s.stage.record_stream(main)
        return s.stage

    def _copy_in(self, x, xs, fs):
        """The group's batches into its staging rows x, on the side stream fs (the current stream): a
        device batch by its own copy, a run of host batches by one."""
        B, j = self.B, 0
        grp = None
        while j < len(xs):
            if isinstance(xs[j], _HostBatch):
                # a run of host batches (consecutive rows of one pinned group buffer): one DMA copy
                e = j
                while e + 1 < len(xs) and isinstance(xs[e + 1], _HostBatch):
                    e += 1
                grp = xs[j].grp
                x[j * B:(e + 1) * B].copy_(grp.pinned[j * B:(e + 1) * B], non_blocking=True)
                j = e + 1
            else:
                x[j * B:(j + 1) * B].copy_(xs[j], non_blocking=True)
                j += 1
        if grp is not None:  # the group buffer may be refilled once its copies have completed
            grp.copied.record(fs)

    def _fps(self, k, xs, ready, main=None):
        """SA1 FPS + level-0 ball queries (and what else self.side lists) of group k (the batches in xs,
        readable after the events in `ready`) on a side stream; `main` the stream the group's MFMA levels
        will run on."""
        slot = k % self.nslot
        s = self.slots[slot]
        fs = self.fps_streams[k % self.depth]
        hs = 1 + k % self.depth  # the side stream's own library handle
        fs.wait_event(s.slot_free)
        for ev in ready:
            fs.wait_event(ev)
        g = len(xs) * self.B
        t = self.bb.timers
        s.staged = self.G > 1 or any(isinstance(xj, _HostBatch) for xj in xs)
        if s.staged:
            self._stage(s, fs, main if main is not None else torch.cuda.current_stream(self.bb.device))
        with torch.cuda.stream(fs):
            if s.staged:
                x = s.stage[:g]
                self._copy_in(x, xs, fs)
            else:
                x = xs[0]
            for xj in xs:  # read on this stream: keep the caller's buffers alive until then
                if not isinstance(xj, _HostBatch):
                    xj.record_stream(fs)
            src, pfz = x, None
            for li, ((lvl, M, _, _), lv) in enumerate(zip(self.side, s.pre(g).values())):
                idx, c, fz = lv["fps"]
                # (level 1's FPS is nested: the prefix shortcut over SA1's centroids)
                _call(t, f"sa{li + 1}_fps", g, farthest_point_sample, src, M, return_xyz=True, first_zero=fz,
                      prefix_ok=pfz, slot=hs, out_idx=idx, out_xyz=c, threads=self.fps_threads if li == 0 else 0)
                for bi_, br in enumerate(lvl["branches"]):
                    tag = _tag(li, lvl, bi_)
                    if lv["bq"] is not None:
                        _call(t, f"{tag}_ball_query", g, ball_query, br["r"], br["ns"], src, c, out=lv["bq"][bi_],
                              slot=hs)
                    elif lv["grid"] is not None:  # depends only on the points: the queries run on the main stream
                        _call(t, f"{tag}_bq_bin", g, ball_query_bin, br["r"], br["ns"], src, lv["grid"][bi_], slot=hs)
                src, pfz = c, fz
            s.fps_done.record(fs)
        return slot

    def _rest(self, slot, xs, main):
        """The MFMA levels of a group: one pass over its staged frames (every operator is per
        frame, so the per-batch outputs are views of the group's), split back per batch."""
        s = self.slots[slot]
        main.wait_event(s.fps_done)
        B, g = self.B, len(xs) * self.B
        x = s.stage[:g] if s.staged else xs[0]
        # keep_levels: the outputs keep copies (the slot's buffers are reused by a later group)
        out, levels = self.bb.forward(x, self.keep, pre=s.pre(g, clone=self.keep))
        s.slot_free.record(main)
        outs = list(out.split(B))
        if not self.keep:
            return outs
        per = []
        for j in range(len(xs)):
            sl = slice(j * B, (j + 1) * B)
            per.append((outs[j], [(nx[sl], nf[sl], ni[sl], [gi[sl] for gi in ng]) for nx, nf, ni, ng in levels]))
        return per

    def feed(self):
        return _Feed(self)

    def run(self, inputs):
        """inputs: list of (B, N, 3) CUDA tensors -> list of global features (B, C), in order."""
        f = _Feed(self)
        outs, i, k = [], 0, 0
        while i < len(inputs):
            # ramp: groups of 1, 2, ... G batches — the first group's FPS (the pipeline fill,
            # during which the main stream waits) is a third as long as a full group's
            sz = min(self.G, k + 1) if self.ramp else self.G
            outs += f._issue(list(inputs[i:i + sz]))
            i, k = i + sz, k + 1
        return outs + f.flush()


_HOST_READY = object()  # push_host's "ready" marker: the batch sits in pinned host memory already


class _HostGroup:
    """A group's pinned host buffer (G batches of rows); `copied` is recorded on the side stream after its
    host-to-device copy (the buffer may be refilled once it has completed)."""

    def __init__(self, pinned):
        self.pinned = pinned
        self.copied = torch.cuda.Event()
        self.copied.record()  # (a fresh buffer is free)


class _HostBatch:
    """One batch of host frames: rows j*B .. (j+1)*B of a pinned group buffer."""

    def __init__(self, grp, j):
        self.grp, self.j = grp, j


class _Feed:
    """StreamingSSG's persistent feed: push(batch) stages batches; every full group of G issues
    its SA1 FPS on a side stream and, once `depth` groups are in flight, the oldest group's
    remaining levels on the main stream (the caller's current stream).  push returns the
    outputs of the batches that call completed (in input order); flush() issues a partial last
    group and drains the pipeline.  push_host(frames) is push() for host NumPy frames."""

    def __init__(self, pipe):
        self.p = pipe
        self.main = torch.cuda.current_stream(pipe.bb.device)
        self.buf, self.pending, self.k = [], [], 0
        self.readies = []  # push()'s ready event per buffered batch
        # push_host's ring of pinned group buffers, the current group's, and the fill threads
        self._ring, self._ri, self._grp, self._pool = [], 0, None, None

    def push_host(self, frames, threads=4):
        """frames: one batch of host frames, a (B, N, 3) array or B arrays of shape (N, 3), of any real
        dtype: boolean, integer or floating (converted to float32 as numpy's astype does).  Shape and
        dtype are checked before the call does anything else: a rejected batch raises ValueError and
        leaves the feed exactly as it was (no pending group retired, no pinned buffer claimed, nothing
        buffered).  The frames are copied into the group's pinned
        buffer (G batches of rows) by `threads` host threads (frames split between them; numpy releases
        the GIL in the copy), and the group's side stream copies the buffer to the device ahead of its FPS
        in one DMA copy (a copy per batch, queued behind the side stream's kernels, held the calling
        thread for milliseconds now and then).  The pinned ring holds depth + 2 groups; a buffer is
        refilled only after its device copy has completed (a host wait on that event, the feed's
        back-pressure).  The batch that opens a group issues the oldest
        in-flight group's main-stream pass (push() issues it when the new group completes), so the main
        stream works while the host fills.  Returns the outputs of the batches that call completed, in
        input order; every output equals forward() of the same frames on the device."""
        p = self.p
        B, N = p.B, p.N
        if isinstance(frames, np.ndarray):
            if frames.shape != (B, N, 3):
                raise ValueError(f"push_host: frames must be ({B}, {N}, 3), got {frames.shape}")
            parts = list(frames)
        else:
            parts = [np.asarray(f) for f in frames]
            if len(parts) != B or any(f.shape != (N, 3) for f in parts):
                raise ValueError(f"push_host: {B} frames of shape ({N}, 3) expected")
        if any(f.dtype.kind not in "biuf" for f in parts):
            raise ValueError(f"push_host: frames must be boolean, integer or floating, got "
                             f"{sorted({str(f.dtype) for f in parts})}")
        out = []
        if not self.buf and len(self.pending) >= p.depth:
            # the batch opens a group whose completion would issue the oldest group's main-stream pass:
            # issue it now, so the main stream runs it while the host fills this group's batches
            slot, pxs = self.pending.pop(0)
            out = p._rest(slot, pxs, self.main)
        if not self._ring:
            import concurrent.futures
            self._ring = [_HostGroup(torch.empty((p.G * B, N, 3), dtype=torch.float32, pin_memory=True))
                          for _ in range(p.depth + 2)]
            self._nthreads = max(1, int(threads))
            self._pool = concurrent.futures.ThreadPoolExecutor(max_workers=self._nthreads)
        if self._grp is None:  # the group's first host batch takes the next pinned group buffer
            self._grp = self._ring[self._ri]
            self._ri = (self._ri + 1) % len(self._ring)
            self._grp.copied.synchronize()  # its previous group has reached the device
        hb = _HostBatch(self._grp, len(self.buf))
        dst = self._grp.pinned[hb.j * B:(hb.j + 1) * B].numpy()
        step = -(-B // self._nthreads)

        def fill(lo):
            for j in range(lo, min(B, lo + step)):
                np.copyto(dst[j], parts[j], casting="unsafe")

        for f in [self._pool.submit(fill, lo) for lo in range(0, B, step)]:
            f.result()
        self.buf.append(hb)
        self.readies.append(_HOST_READY)  # filled by the host: no device event to wait for
        if len(self.buf) < p.G:
            return out
        xs, evs = self.buf, self.readies
        self.buf, self.readies = [], []
        return out + self._issue(xs, evs)

    def _issue(self, xs, readies=None):
        self._grp = None  # the next group's host batches take a fresh pinned group buffer
        evs = [e for e in (readies or [None]) if e is not None and e is not _HOST_READY]
        if readies is None or any(e is None for e in readies):
            ev = torch.cuda.Event()
            ev.record(self.main)  # the inputs exist on the caller's stream
            evs.append(ev)
        self.pending.append((self.p._fps(self.k, xs, evs, self.main), xs))
        self.k += 1
        if len(self.pending) > self.p.depth:
            slot, pxs = self.pending.pop(0)
            return self.p._rest(slot, pxs, self.main)
        return []

    def push(self, x, ready=None):
        """ready: a CUDA event after which x is readable; None records one on the caller's stream
        when the group issues — which also orders the group's FPS after every main-stream pass
        issued so far, so a feed whose inputs were produced earlier passes the producer's event."""
        self.buf.append(x)
        self.readies.append(ready)
        if len(self.buf) < self.p.G:
            return []
        xs, evs = self.buf, self.readies
        self.buf, self.readies = [], []
        return self._issue(xs, evs)

    def close(self):
        """Stop push_host's copy threads and free the pinned ring (once its copies have completed)."""
        if self._pool is not None:
            self._pool.shutdown(wait=False)
            self._pool = None
            for grp in self._ring:
                grp.copied.synchronize()
            self._ring, self._grp = [], None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def flush(self, trim=True):
        """Issue a partial last group and drain the pipeline.  trim: then wait for the side streams
        and free the workspaces the library's handles retired while growing (lidar_trim)."""
        out = []
        if self.buf:
            xs, evs = self.buf, self.readies
            self.buf, self.readies = [], []
            out += self._issue(xs, evs)
        while self.pending:
            slot, pxs = self.pending.pop(0)
            out += self.p._rest(slot, pxs, self.main)
        if trim:
            for fs in self.p.fps_streams:
                fs.synchronize()
            self.main.synchronize()
            nat.trim(self.p.bb.device.index)
        return out
