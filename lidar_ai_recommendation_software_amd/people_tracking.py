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


def _check_tensor(what, name, t, dev=None, dtype=None, shape=None):
    """t is a contiguous CUDA tensor; with dev, on that device (people's); with dtype and shape, of those."""
    on = dev is not None
    if not isinstance(t, torch.Tensor) or not t.is_cuda or not t.is_contiguous() or (on and t.device != dev):
        raise ValueError(f"{what}: {name} must be a contiguous CUDA tensor" + (" on people's device" if on else ""))
    if dtype is not None and (t.dtype != dtype or tuple(t.shape) != shape):
        raise ValueError(f"{what}: {name} must be {shape} {dtype}, got {t.dtype} {tuple(t.shape)}")


def _check_people(what, people, k):
    _check_tensor(what, "people", people)
    if people.dtype != torch.float64 or people.dim() != 3 or people.shape[2] != 2 or people.shape[1] < 1:
        raise ValueError(f"{what}: people must be (T, cap, 2) float64 with cap >= 1")
    T = people.shape[0]
    _check_tensor(what, "k", k, people.device, torch.int64, (T,))
    return T, people.shape[1]


def _flow_cells_acc(people, k, prev, velocity, first, accumulate, grid, grid_size, count, vsum, slot):
    """lidar_flow_cells_acc_f64 over checked tensors: the frames >= first into count / vsum, which it overwrites
    (accumulate = 0) or continues (1); first = 1, accumulate = 0 is lidar_flow_cells_f64."""
    x0, y0, nx, ny = grid
    T, cap = people.shape[:2]
    nat.call("lidar_flow_cells_acc_f64", nat.handle(people.device.index, slot), nat.ptr(people), nat.ptr(k),
             nat.ptr(prev), nat.ptr(velocity), T, cap, first, accumulate, x0, y0, grid_size, nx, ny, nat.ptr(count),
             nat.ptr(vsum), nat.stream_ptr())


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
    float64, (x0, y0, nx, ny)), device tensors, nothing synchronised (lidar_flow_cells_f64's computation).  A matched
    detection is binned by its own position with VenueGrid's binning; vsum adds the velocities of a cell's
    detections sequentially in (t, j) order, so it is the same bits on every run."""
    T, cap = _check_people("flow_cells", people, k)
    _check_tensor("flow_cells", "prev", prev, people.device, torch.int32, (T, cap))
    _check_tensor("flow_cells", "velocity", velocity, people.device, torch.float64, (T, cap, 2))
    g = _positive("flow_cells", "grid_size", grid_size)
    grid = venue_grid(x_range, y_range, g)  # (x0, y0, nx, ny)
    with nat.grid_alloc():
        count = torch.zeros(grid[2:], dtype=torch.int32, device=people.device)  # T == 0: no detection
        vsum = torch.zeros(grid[2:] + (2,), dtype=torch.float64, device=people.device)
    if T:  # a frame-0 row has no predecessor in this call: first = 1
        _flow_cells_acc(people, k, prev, velocity, 1, 0, grid, g, count, vsum, slot)
    return count, vsum, grid


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
        _check_tensor("track_stream", name, t, dev, dtype, (T, cap) + tail)
    if ntracks is None:
        ntracks = torch.zeros((), dtype=torch.int64, device=dev)
    _check_tensor("track_stream", "ntracks", ntracks, dev, torch.int64, ())
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
            _flow_cells_acc(people, k, prev, velocity, C, 1, self.grid, self.grid_size, self.count, self.vsum,
                            self.slot)
        self.frames += T
        keep = min(self.max_gap + 1, self.frames)
        self._carry = tuple(t[C + T - keep:] for t in (people, k, prev, gap, succ, velocity, track_id))
        return prev[C:], gap[C:], track_id[C:], velocity[C:]
