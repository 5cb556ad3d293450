"""The Tier R C-ABI contract (``include/lidar_amd.h``), stated once for the Python host layer.

``data_processing``, ``variant_pipeline``, ``density_stream`` and ``crowd_density_model`` all
drive the same entry points (preprocess -> people -> density grid) and read the same two
records back: the 64-double scalars block of a preprocessed frame and the density grid record.
This module names the scalar slots (``tests/test_density_abi_cpu.py`` pins them to the header's
``LIDAR_S_*`` enum), maps the status slot to the reference's exceptions, turns a scalars row into
the reference's ``dimensions`` / ``ground_plane`` values, allocates and fills the preprocess
outputs, and encodes / decodes the grid record and the ``analyze`` result dicts.

torch is imported inside the functions that need it: the CPU tests import this module.
"""
import ctypes

import numpy as np

from . import _native as nat

# ------------------------------------------------------------------ scalars (LIDAR_S_*)
S_N_IN = 0
S_N_GROUND = 1
S_N_NONGROUND = 2
S_Z_THRESHOLD = 3
S_EPS = 4
S_DIMS = 5            # x_min, x_max, y_min, y_max, z_min, z_max
S_PLANE = 11          # a, b, c, d
S_STATUS = 15
S_MEAN = 16           # 3-sigma mean (3)
S_STD = 19            # 3-sigma std (3)
S_SCALER_MEAN = 22    # StandardScaler mean (3)
S_SCALER_SCALE = 25   # StandardScaler scale (3)
S_SCALED_BBOX = 28    # lo (3), hi (3) of the scaled non-ground points
S_N_CLUSTERS = 39
S_PLANE_KIND = 40     # 0 lstsq, 1 min-z fallback, 2 rank-deficient ground
SCALARS = 64

STATUS_OK = 0
STATUS_NO_INLIER = 1
STATUS_EMPTY = 2


def raise_for_status(status):
    """The reference's exception for a frame's status slot: its ``np.min`` of an empty z column
    (empty frame), its ``np.percentile`` of an empty inlier set (any other failure)."""
    if status == STATUS_EMPTY:
        raise ValueError("zero-size array to reduction operation minimum which has no identity")
    if status != STATUS_OK:
        raise IndexError("index -1 is out of bounds for axis 0 with size 0")


def xy_extent(S):
    """(x_min, x_max, y_min, y_max) of a scalars row: the extent the density grid is laid over."""
    return S[S_DIMS:S_DIMS + 4]


def dimensions(S, int_dtype=None):
    """The reference's ``dimensions`` dict of a scalars row.  An integer input frame
    (``int_dtype``: its dtype) gets its bounds cast back first, so the spans are integer too."""
    mins, maxs = S[S_DIMS:S_DIMS + 6:2], S[S_DIMS + 1:S_DIMS + 6:2]
    if int_dtype is not None:
        mins, maxs = mins.astype(int_dtype), maxs.astype(int_dtype)
    (x_min, y_min, z_min), (x_max, y_max, z_max) = mins, maxs
    return {"x_range": (x_min, x_max), "y_range": (y_min, y_max), "z_range": (z_min, z_max),
            "width": x_max - x_min, "length": y_max - y_min, "height": z_max - z_min}


def ground_plane(S, is_int):
    """The reference's ``ground_plane`` of a scalars row (utils/data_processing.py:173-195): the
    min-z fallback is ``[0, 0, 1, -z_min]`` in the input's own arithmetic, so an integer frame gives
    an integer array."""
    if S[S_PLANE_KIND] == 1.0 and is_int:
        return np.array([0, 0, 1, -int(S[S_DIMS + 4])])
    if S[S_PLANE_KIND] == 1.0:
        return np.array([0.0, 0.0, 1.0, S[S_PLANE + 3]])
    return np.array([S[S_PLANE], S[S_PLANE + 1], -1, S[S_PLANE + 3]], dtype=np.float64)


# ------------------------------------------------------------------ preprocess / people
def preprocess_outputs(rows, device, frames=None):
    """The caller-allocated outputs of the preprocess entry points for ``rows`` points:
    {mask, colors, normals, comp, labels, scal}; ``scal`` is one scalars row, or
    (frames, SCALARS) for a batch."""
    import torch
    f64 = dict(dtype=torch.float64, device=device)
    return {"mask": torch.empty(rows, dtype=torch.uint8, device=device),
            "colors": torch.empty((rows, 3), **f64),
            "normals": torch.empty((rows, 3), **f64),
            "comp": torch.empty((rows, 3), **f64),
            "labels": torch.empty(rows, dtype=torch.int64, device=device),
            "scal": torch.empty(SCALARS if frames is None else (frames, SCALARS), **f64)}


def preprocess(h, x, offsets, frames, max_n, eps, out, stream):
    """Fill ``out`` (``preprocess_outputs``) from the frames in x.  ``eps`` given: the Streamlit
    variant's fixed-eps DBSCAN (``offsets`` None: one frame of max_n points); else ``offsets`` (device
    CSR row offsets) given: the batch entry point; else the single frame of max_n points."""
    tail = (nat.ptr(out["mask"]), nat.ptr(out["colors"]), nat.ptr(out["normals"]), nat.ptr(out["comp"]),
            nat.ptr(out["labels"]), nat.ptr(out["scal"]), stream)
    if eps is not None:
        nat.call("lidar_preprocess_eps_batch_f64", h, nat.ptr(x), nat.ptr(offsets), frames, max_n, float(eps), *tail)
    elif offsets is not None:
        nat.call("lidar_preprocess_batch_f64", h, nat.ptr(x), nat.ptr(offsets), frames, max_n, *tail)
    else:
        nat.call("lidar_preprocess_f64", h, nat.ptr(x), max_n, *tail)


def people(h, x, labels, n, stream, out=None):
    """``lidar_people_f64`` over the first n rows of (x, labels) -> (people[:k], k): the (k, 2)
    cluster centroids on the device.  ``out``: an (>= n, 2) float64 buffer to reuse."""
    if out is None:
        import torch
        out = torch.empty((n, 2), dtype=torch.float64, device=x.device)
    k = nat.I64(0)
    nat.call("lidar_people_f64", h, nat.ptr(x), nat.ptr(labels), n, nat.ptr(out), ctypes.byref(k), stream)
    return out[:k.value], k.value


# ------------------------------------------------------------------ grid record
# density (nx*ny) | flat_x | flat_y | stats (8) | hot (5 int64); lidar_density_batch_f64 puts
# grid_x (nx) | grid_y (ny) in front.
def record_doubles(nx, ny, edges):
    return (nx + ny if edges else 0) + 3 * nx * ny + 13


def scratch_doubles(nx, ny):
    """A frame's share of lidar_density_batch_f64's scratch (mirrors density_batch_kernel)."""
    m = nx * ny
    return m + (m + 1) // 2 + nx + ny + 2


def job_row(x_min, y_min, grid_size, nx, ny, out_off, scr_off):
    """A frame's row of lidar_density_batch_f64's jobs array."""
    g2 = grid_size * 2.0
    return (x_min - g2, y_min - g2, grid_size, nx, ny, out_off, scr_off, 0)


def decode_record(b, nx, ny, edges, at=0):
    """Views of the grid record that starts at element ``at`` of the host float64 buffer b ->
    (grid_x, grid_y, density (nx, ny), flat_x, flat_y, stats, hot); grid_x / grid_y are None without
    ``edges``.  ``hot``: the int64 flat indices of the hotspots, stats[3] of them."""
    m = nx * ny
    gx = gy = None
    if edges:
        gx, gy = b[at:at + nx], b[at + nx:at + nx + ny]
        at += nx + ny
    s = at + 3 * m
    stats = b[s:s + 8]
    hot = b[s + 8:s + 13].view(np.int64)[: int(stats[3])]
    return gx, gy, b[at:at + m].reshape(nx, ny), b[at + m:at + 2 * m], b[at + 2 * m:s], stats, hot


# ------------------------------------------------------------------ analyze results
def empty_result():
    """The reference's ``analyze`` result when nobody is found (models/crowd_density_model.py:33-42);
    fresh objects on every call, callers may edit them."""
    return {"total_people": 0, "avg_density": 0.0, "max_density": 0.0, "density_map": np.zeros((1, 1)),
            "grid_coordinates": (np.array([0]), np.array([0])), "density_values": np.array([0]),
            "hotspots": []}


def analyze_result(total_people, density, flat_x, flat_y, stats, hot):
    """The reference's populated ``analyze`` result from a decoded grid record."""
    flat = density.flatten()
    return {"total_people": total_people, "avg_density": np.float64(stats[1]), "max_density": np.float64(stats[0]),
            "density_map": density, "grid_coordinates": (flat_x, flat_y), "density_values": flat,
            "hotspots": [{"x": flat_x[i], "y": flat_y[i], "density": flat[i]} for i in hot.tolist()]}
