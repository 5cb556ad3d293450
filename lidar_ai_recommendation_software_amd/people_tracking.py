"""People tracked across consecutive frames and their measured flow on the venue grid (csrc/track.hip;
DESIGN.md §3 "People tracking", §4.9).

``track_people`` associates the people of T consecutive frames (``pointnet2.class_people``'s ``people`` and
``k``, still on the device) by mutual nearest neighbour within a gate; ``flow_cells`` bins every matched
detection into the grid ``global_density.VenueGrid`` builds for a venue extent and sums the velocities per
cell in a fixed order.  Both are asynchronous: device tensors in, device tensors out, nothing synchronised.

On a live feed (DESIGN.md §3 "Continuous people tracking", §4.10) ``PeopleTracker`` takes batch after batch:
its ids last across ``push`` calls and a track survives up to ``max_gap`` frames without a detection;
``track_stream`` is the call underneath (lidar_track_stream_f64), with the carried frames' state explicit.
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


# ------------------------------------------------------------------ continuous tracking
MAX_GAP = 7
STATE = (("prev", torch.int32, ()), ("gap", torch.int32, ()), ("succ", torch.uint8, ()),
         ("velocity", torch.float64, (2,)), ("track_id", torch.int32, ()))


def _max_gap(what, max_gap):
    if int(max_gap) != max_gap or not 0 <= max_gap <= MAX_GAP:
        raise ValueError(f"{what}: max_gap must be an integer in 0 .. {MAX_GAP}, got {max_gap}")
    return int(max_gap)


def track_stream(people, k, dt, gate, max_gap=0, carry=0, state=None, ntracks=None, slot=0):
    """track_people carried across calls and stitched over up to max_gap missed frames
    (lidar_track_stream_f64; DESIGN.md §3 "Continuous people tracking").  people (T, cap, 2), k (T,): the
    frames, the first `carry` of them (0 .. min(max_gap + 1, T)) with their association state given in
    `state` = (prev, gap, succ, velocity, track_id), each (T, cap[, 2]) int32 / int32 / uint8 / float64 /
    int32; the call fills the other frames in place (and may set succ in the carried ones).  Without a state
    (carry 0) the five are allocated.  ntracks: the () int64 device tensor holding the id base, updated in
    place (a zero is allocated without one).  -> (prev, gap, succ, velocity, track_id, ntracks), device
    tensors, nothing synchronised.  gap[t, j]: the predecessor of row j lives in frame t - gap (0: none)."""
    T, cap = _check_people("track_stream", people, k)
    dt, gate = _positive("track_stream", "dt", dt), _positive("track_stream", "gate", gate)
    max_gap = _max_gap("track_stream", max_gap)
    if int(carry) != carry or not 0 <= carry <= min(max_gap + 1, T):
        raise ValueError(f"track_stream: carry must be an integer in 0 .. min(max_gap + 1, T) = "
                         f"{min(max_gap + 1, T)}, got {carry}")
    dev = people.device
    if state is None:
        if carry:
            raise ValueError("track_stream: carried frames need their state")
        state = tuple(torch.empty((T, cap) + tail, dtype=dtype, device=dev) for _, dtype, tail in STATE)
    if len(state) != len(STATE):
        raise ValueError("track_stream: state is (prev, gap, succ, velocity, track_id)")
    for t, (name, dtype, tail) in zip(state, STATE):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"track_stream: {name} must be a contiguous CUDA tensor on people's device")
        if t.dtype != dtype or tuple(t.shape) != (T, cap) + tail:
            raise ValueError(f"track_stream: {name} must be {(T, cap) + tail} {dtype}, got {t.dtype} {tuple(t.shape)}")
    if ntracks is None:
        ntracks = torch.zeros((), dtype=torch.int64, device=dev)
    if (not isinstance(ntracks, torch.Tensor) or ntracks.dtype != torch.int64 or ntracks.dim() != 0
            or ntracks.device != dev):
        raise ValueError("track_stream: ntracks must be a () int64 tensor on people's device")
    if T:
        prev, gap, succ, velocity, track_id = state
        nat.call("lidar_track_stream_f64", nat.handle(dev.index, slot), nat.ptr(people), nat.ptr(k), T, cap, int(carry),
                 dt, gate, max_gap, nat.ptr(prev), nat.ptr(gap), nat.ptr(succ), nat.ptr(velocity), nat.ptr(track_id),
                 nat.ptr(ntracks), nat.stream_ptr())
    return (*state, ntracks)


class PeopleTracker:
    """A sensor's people tracked batch after batch: ids that last across push() calls, tracks stitched over up
    to max_gap missed frames, and (with a venue extent) the flow cells of everything pushed so far.

    push(people, k) takes a batch of any T >= 0 consecutive frames (cap is fixed by the first push).  The
    tracker keeps the last min(max_gap + 1, frames seen) frames on the device — people, k and the five state
    arrays — prepends them to the batch, and calls lidar_track_stream_f64 with them as the carry; with an
    extent it then calls lidar_flow_cells_acc_f64(first = carry, accumulate = 1) into its own count / vsum.
    Whatever the batch sizes, the outputs are those of one call over the whole stream, bit for bit.  Nothing
    is synchronised.  ntracks () int64, matched () int64 (detections with a measured velocity), count (nx, ny)
    int32 and vsum (nx, ny, 2) float64 are device tensors (count / vsum None without an extent); frames is the
    number of frames seen."""

    def __init__(self, dt, gate, max_gap=0, x_range=None, y_range=None, grid_size=1.0, slot=0):
        self.dt, self.gate = _positive("PeopleTracker", "dt", dt), _positive("PeopleTracker", "gate", gate)
        self.max_gap = _max_gap("PeopleTracker", max_gap)
        if (x_range is None) != (y_range is None):
            raise ValueError("PeopleTracker: x_range and y_range go together")
        self.x_range, self.y_range, self.grid = x_range, y_range, None
        self.grid_size = _positive("PeopleTracker", "grid_size", grid_size)
        if x_range is not None:
            self.grid = venue_grid(x_range, y_range, self.grid_size)  # (x0, y0, nx, ny)
        self.slot = slot
        self.frames = 0
        self.cap = None
        self.ntracks = self.matched = self.count = self.vsum = None
        self._carry = None  # (people, k, prev, gap, succ, velocity, track_id) of the last frames

    def push(self, people, k):
        """-> (prev, gap, track_id, velocity) of the T new frames, device tensors."""
        T, cap = _check_people("PeopleTracker.push", people, k)
        dev = people.device
        if self.cap is None:
            self.cap = cap
            self.ntracks = torch.zeros((), dtype=torch.int64, device=dev)
            self.matched = torch.zeros((), dtype=torch.int64, device=dev)
            if self.grid is not None:
                with nat.grid_alloc():
                    self.count = torch.zeros(self.grid[2:], dtype=torch.int32, device=dev)
                    self.vsum = torch.zeros(self.grid[2:] + (2,), dtype=torch.float64, device=dev)
            self._carry = (people[:0], k[:0]) + tuple(torch.empty((0, cap) + tail, dtype=dtype, device=dev)
                                                      for _, dtype, tail in STATE)
        if cap != self.cap or dev != self.ntracks.device:
            raise ValueError(f"PeopleTracker.push: cap and device are fixed by the first push ({self.cap}, "
                             f"{self.ntracks.device}), got {cap}, {dev}")
        if (self.frames + T) * cap >= 1 << 31:  # every row could be a new detection: the ids are int32
            raise ValueError(f"PeopleTracker.push: {self.frames + T} frames of {cap} rows could pass 2^31 track ids")
        C = self._carry[0].shape[0]
        if T == 0:
            return tuple(self._carry[i][C:] for i in (2, 3, 6, 5))
        people = torch.cat([self._carry[0], people])
        k = torch.cat([self._carry[1], k])
        state = tuple(torch.cat([c, torch.empty((T, cap) + tail, dtype=dtype, device=dev)])
                      for c, (_, dtype, tail) in zip(self._carry[2:], STATE))
        prev, gap, succ, velocity, track_id, _ = track_stream(people, k, self.dt, self.gate, self.max_gap, C, state,
                                                              self.ntracks, self.slot)
        self.matched += (prev[C:] >= 0).sum()
        if self.grid is not None:
            x0, y0, nx, ny = self.grid
            nat.call("lidar_flow_cells_acc_f64", nat.handle(dev.index, self.slot), nat.ptr(people), nat.ptr(k),
                     nat.ptr(prev), nat.ptr(velocity), C + T, cap, C, 1, x0, y0, self.grid_size, nx, ny,
                     nat.ptr(self.count), nat.ptr(self.vsum), nat.stream_ptr())
        self.frames += T
        keep = min(self.max_gap + 1, self.frames)
        self._carry = tuple(t[C + T - keep:] for t in (people, k, prev, gap, succ, velocity, track_id))
        return prev[C:], gap[C:], track_id[C:], velocity[C:]
