"""People tracked across consecutive frames and their measured flow on the venue grid (csrc/track.hip;
DESIGN.md §3 "People tracking", §4.9).

``track_people`` associates the people of T consecutive frames (``pointnet2.class_people``'s ``people`` and
``k``, still on the device) by mutual nearest neighbour within a gate; ``flow_cells`` bins every matched
detection into the grid ``global_density.VenueGrid`` builds for a venue extent and sums the velocities per
cell in a fixed order.  Both are asynchronous: device tensors in, device tensors out, nothing synchronised.
"""
import math

import torch

from . import _native as nat
from .global_density import venue_grid


def _check_people(what, people, k):
    for t in (people, k):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"{what}: liblidar_amd operators take contiguous CUDA tensors")
    if people.dtype != torch.float64 or people.dim() != 3 or people.shape[2] != 2 or people.shape[1] < 1:
        raise ValueError(f"{what}: people must be (T, cap, 2) float64 with cap >= 1")
    T = people.shape[0]
    if k.dtype != torch.int64 or tuple(k.shape) != (T,):
        raise ValueError(f"{what}: k must be ({T},) int64, got {k.dtype} {tuple(k.shape)}")
    if k.device != people.device:
        raise ValueError(f"{what}: people and k must be on the same device")
    return T, people.shape[1]


def _positive(what, name, v):
    v = float(v)
    if not (v > 0.0 and math.isfinite(v)):
        raise ValueError(f"{what}: {name} must be positive and finite, got {v}")
    return v


def track_people(people, k, dt, gate, slot=0):
    """people (T, cap, 2) float64, k (T,) int64 (class_people's outputs for T consecutive frames), dt seconds
    between frames, gate metres (the largest displacement accepted between two frames) ->
    (prev (T, cap) int32, track_id (T, cap) int32, velocity (T, cap, 2) float64, ntracks () int64), device
    tensors, nothing synchronised (lidar_track_people_f64).  prev[t, j]: the row of frame t - 1 that row j
    of frame t continues (mutual nearest neighbour within the gate), -1 for an unmatched row, frame 0 and
    rows at or past min(max(k[t], 0), cap); velocity: the displacement over dt for a matched row, (0, 0)
    otherwise; track_id: new detections numbered in (t, j) order, matched rows inherit; ntracks: how many."""
    T, cap = _check_people("track_people", people, k)
    dt, gate = _positive("track_people", "dt", dt), _positive("track_people", "gate", gate)
    dev = people.device
    prev = torch.empty((T, cap), dtype=torch.int32, device=dev)
    track_id = torch.empty((T, cap), dtype=torch.int32, device=dev)
    velocity = torch.empty((T, cap, 2), dtype=torch.float64, device=dev)
    ntracks = torch.zeros((), dtype=torch.int64, device=dev)  # T == 0: no new detection
    if T:  # an empty tensor has no address to pass
        nat.call("lidar_track_people_f64", nat.handle(dev.index, slot), nat.ptr(people), nat.ptr(k), T, cap, dt, gate,
                 nat.ptr(prev), nat.ptr(track_id), nat.ptr(velocity), nat.ptr(ntracks), nat.stream_ptr())
    return prev, track_id, velocity, ntracks


def flow_cells(people, k, prev, velocity, x_range, y_range, grid_size=1.0, slot=0):
    """The matched detections of track_people on the venue grid -> (count (nx, ny) int32, vsum (nx, ny, 2)
    float64, (x0, y0, nx, ny)), device tensors, nothing synchronised (lidar_flow_cells_f64).  A matched
    detection is binned by its own position with VenueGrid's binning; vsum adds the velocities of a cell's
    detections sequentially in (t, j) order, so it is the same bits on every run."""
    T, cap = _check_people("flow_cells", people, k)
    for t in (prev, velocity):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or not t.is_contiguous() or t.device != people.device:
            raise ValueError("flow_cells: prev and velocity must be contiguous CUDA tensors on people's device")
    if prev.dtype != torch.int32 or tuple(prev.shape) != (T, cap):
        raise ValueError(f"flow_cells: prev must be ({T}, {cap}) int32, got {prev.dtype} {tuple(prev.shape)}")
    if velocity.dtype != torch.float64 or tuple(velocity.shape) != (T, cap, 2):
        raise ValueError(f"flow_cells: velocity must be ({T}, {cap}, 2) float64, got {velocity.dtype} "
                         f"{tuple(velocity.shape)}")
    g = _positive("flow_cells", "grid_size", grid_size)
    x0, y0, nx, ny = venue_grid(x_range, y_range, g)
    dev = people.device
    with nat.grid_alloc():
        count = torch.zeros((nx, ny), dtype=torch.int32, device=dev)  # T == 0: no detection
        vsum = torch.zeros((nx, ny, 2), dtype=torch.float64, device=dev)
    if T:
        nat.call("lidar_flow_cells_f64", nat.handle(dev.index, slot), nat.ptr(people), nat.ptr(k), nat.ptr(prev),
                 nat.ptr(velocity), T, cap, x0, y0, g, nx, ny, nat.ptr(count), nat.ptr(vsum), nat.stream_ptr())
    return count, vsum, (x0, y0, nx, ny)
