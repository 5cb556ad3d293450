"""People tracked across consecutive frames and their measured flow on the venue grid (csrc/track.hip;
DESIGN.md §3 "People tracking", §4.9).

``track_people`` associates the people of T consecutive frames (``pointnet2.class_people``'s ``people`` and
``k``, still on the device) by mutual nearest neighbour within a gate; ``flow_cells`` bins every matched
detection into the grid ``global_density.VenueGrid`` builds for a venue extent and sums the velocities per
cell in a fixed order.  Both are asynchronous: device tensors in, device tensors out, nothing synchronised.

On a live feed (DESIGN.md §3 "Continuous people tracking", §4.10) ``PeopleTracker`` takes batch after batch:
its ids last across ``push`` calls and a track survives up to ``max_gap`` frames without a detection;
``track_stream`` is the call underneath (lidar_track_stream_f64), with the carried frames' state explicit.

``track_events`` (csrc/track_events.hip; DESIGN.md §3 "Gate and zone events", §4.12) turns the links into counts:
crossings of gate lines, forward and backward, and occupancy, entries and exits of zones, per frame, with a bit
mask per row; ``check_gates`` / ``check_zones`` validate a user's tables on the host, and
``PeopleTracker(gates=, zones=)`` totals the counts across ``push`` calls.

``track_history`` (csrc/track_history.hip; DESIGN.md §3 "Track history", §4.13) follows the links forward: per
detection the age, the hits, the path length and the origin of its track and how long it has been in each zone, per
frame and zone the stays that ended; ``PeopleTracker(history=True)`` carries that state across ``push`` calls.

``track_crowding`` (csrc/track_crowding.hip; DESIGN.md §3 "Crowding", §4.15) sweeps every frame against itself: per
person the neighbours within a radius, the nearest one and the spacing, the local density, the variance of the
velocities around it and their product, the crowd pressure; per frame and venue cell the people above two limits and
the peaks; ``PeopleTracker(crowding=)`` totals them across ``push`` calls.

``track_routes`` (csrc/track_routes.hip; DESIGN.md §3 "Routes", §4.16) joins a track's visit to one zone with its
visit to the next: per detection the first and the last zone of its track, the frames since, its legs and the leg it
completes, per pair of zones the trips and their travel times; ``PeopleTracker(routes=True)`` carries that state and
totals the trips across ``push`` calls.
"""
import math

import numpy as np
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


def _check_links(what, people, prev, gap=None):
    """prev, and gap if given, are (T, cap) int32 on people's device."""
    _check_tensor(what, "prev", prev, people.device, torch.int32, tuple(people.shape[:2]))
    if gap is not None:
        _check_tensor(what, "gap", gap, people.device, torch.int32, tuple(people.shape[:2]))


def _check_device_table(what, name, t, dev):
    """A gate or zone table on people's device, (n, 4) float64 with 1 .. MAX_TABLE rows -> n; None (no table) -> 0."""
    if t is None:
        return 0
    _check_tensor(what, name, t, dev)
    if t.dtype != torch.float64 or t.dim() != 2 or t.shape[1] != 4 or not 1 <= t.shape[0] <= MAX_TABLE:
        raise ValueError(f"{what}: {name} must be (n, 4) float64 with 1 <= n <= {MAX_TABLE}, got {t.dtype} "
                         f"{tuple(t.shape)}")
    return t.shape[0]


def _integer(what, name, v, hi, bound=""):
    """v is an integer in 0 .. hi -> int(v); bound: how the message spells hi ("T = ")."""
    if int(v) != v or not 0 <= v <= hi:
        raise ValueError(f"{what}: {name} must be an integer in 0 .. {bound}{hi}, got {v}")
    return int(v)


def _take(what, which, given, layout, dev, note="", holes=False, carry=0):
    """The caller's arrays `given` (its argument `which`) or, without them, fresh ones, each checked against its
    (name, dtype, shape) row of the layout; a row with shape None (an absent kind) takes None only.  holes: a None
    among the given ones is allocated too.  carry: the leading frames the arrays must bring with them."""
    if given is None and carry:
        raise ValueError(f"{what}: carried frames need their {which}")
    fresh = holes or given is None
    given = (None,) * len(layout) if given is None else tuple(given)
    if len(given) != len(layout):
        raise ValueError(f"{what}: {which} is ({', '.join(name for name, _, _ in layout)}){note}")
    out = []
    for t, (name, dtype, shape) in zip(given, layout):
        if shape is None:
            if t is not None:
                raise ValueError(f"{what}: {which}'s {name} must be None without its table")
        elif t is None and fresh:
            t = torch.empty(shape, dtype=dtype, device=dev)
        else:
            _check_tensor(what, name, t, dev, dtype, shape)
        out.append(t)
    return tuple(out)


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
    _check_links("flow_cells", people, prev)
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


def state_layout(T, cap):
    """(name, dtype, shape) of track_stream's five state arrays over T frames."""
    return tuple((name, dtype, (T, cap) + tail) for name, dtype, tail in STATE)


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
    max_gap = _integer("track_stream", "max_gap", max_gap, MAX_GAP)
    carry = _integer("track_stream", "carry", carry, min(max_gap + 1, T), "min(max_gap + 1, T) = ")
    dev = people.device
    state = _take("track_stream", "state", state, state_layout(T, cap), dev, carry=carry)
    if ntracks is None:
        ntracks = torch.zeros((), dtype=torch.int64, device=dev)
    _check_tensor("track_stream", "ntracks", ntracks, dev, torch.int64, ())
    if T:
        nat.call("lidar_track_stream_f64", nat.handle(dev.index, slot), nat.ptr(people), nat.ptr(k), T, cap, carry, dt,
                 gate, max_gap, *(nat.ptr(t) for t in state), nat.ptr(ntracks), nat.stream_ptr())
    return (*state, ntracks)


# ------------------------------------------------------------------ gate and zone events
MAX_TABLE = 64  # gates, and zones, per call: a bit of an int64 mask each
EVENTS = ("gate_counts", "zone_counts", "gate_fwd", "gate_bwd", "zone_in")  # track_events' outputs, in order


def _check_table(what, name, rows):
    a = np.ascontiguousarray(rows, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 4 or not 1 <= a.shape[0] <= MAX_TABLE:
        raise ValueError(f"{what}: {name} must be (n, 4) with 1 <= n <= {MAX_TABLE}, got {a.shape}")
    for r, row in enumerate(a):
        if not np.all(np.isfinite(row)):
            raise ValueError(f"{what}: row {r} is not finite: {row.tolist()}")
    return a


def check_gates(gates):
    """Array-like (G, 4) rows (ax, ay, bx, by), 1 <= G <= 64, finite, A != B -> contiguous float64 ndarray;
    ValueError names the offending row.  Host only: no GPU or library call."""
    a = _check_table("check_gates", "gates", gates)
    for r, (ax, ay, bx, by) in enumerate(a):
        if ax == bx and ay == by:
            raise ValueError(f"check_gates: row {r} is degenerate (A == B): {a[r].tolist()}")
    return a


def check_zones(zones):
    """Array-like (Z, 4) rows (x0, x1, y0, y1), 1 <= Z <= 64, finite, x0 < x1 and y0 < y1 -> contiguous float64
    ndarray; ValueError names the offending row.  Host only: no GPU or library call."""
    a = _check_table("check_zones", "zones", zones)
    for r, (x0, x1, y0, y1) in enumerate(a):
        if not (x0 < x1 and y0 < y1):
            raise ValueError(f"check_zones: row {r} needs x0 < x1 and y0 < y1: {a[r].tolist()}")
    return a


def event_layout(nf, cap, G, Z):
    """(name, dtype, shape) of track_events' five outputs over nf frames; a mask of an absent kind has shape None."""
    return tuple(zip(EVENTS, (torch.int32, torch.int32, torch.int64, torch.int64, torch.int64),
                     ((nf, G, 2), (nf, Z, 3), (nf, cap) if G else None, (nf, cap) if G else None,
                      (nf, cap) if Z else None)))


def track_events(people, k, prev, gap=None, gates=None, zones=None, first=0, out=None, slot=0):
    """Gate crossings and zone occupancy of the links (prev, gap) track_people / track_stream left on the device
    (lidar_track_events_f64; DESIGN.md §3 "Gate and zone events").  people (T, cap, 2), k (T,), prev (T, cap)
    int32; gap (T, cap) int32, or None for track_people's prev (every link spans one frame); gates (G, 4) and
    zones (Z, 4): float64 device tensors, at least one of them, 1 .. 64 rows each (check_gates / check_zones
    validate what a user passes; here only device, dtype and shape are checked); only the frames t >= first
    are evaluated.  -> (gate_counts (T - first, G, 2) int32 forward / backward, zone_counts (T - first, Z, 3)
    int32 occupancy / entries / exits, gate_fwd, gate_bwd, zone_in (T - first, cap) int64 bit masks per row),
    device tensors, nothing synchronised; an absent kind has G or Z = 0 and None for its masks.  out: the five
    preallocated (None where the result has None); every element is written, none when first == T."""
    what = "track_events"
    T, cap = _check_people(what, people, k)
    dev = people.device
    _check_links(what, people, prev, gap)
    if gates is None and zones is None:
        raise ValueError(f"{what}: needs gates or zones")
    G, Z = _check_device_table(what, "gates", gates, dev), _check_device_table(what, "zones", zones, dev)
    first = _integer(what, "first", first, T, "T = ")
    out = _take(what, "out", out, event_layout(T - first, cap, G, Z), dev, holes=True)
    if T > first:  # an empty tensor has no address to pass
        nat.call("lidar_track_events_f64", nat.handle(dev.index, slot), nat.ptr(people), nat.ptr(k), nat.ptr(prev),
                 nat.ptr(gap), T, cap, first, nat.ptr(gates), G, nat.ptr(zones), Z,
                 *(nat.ptr(t) if t is not None and t.numel() else None for t in out), nat.stream_ptr())
    return out


# ------------------------------------------------------------------ track history
HISTORY = (("age", torch.int32, ()), ("hits", torch.int32, ()), ("path", torch.float64, ()),
           ("origin", torch.float64, (2,)))


def history_layout(T, cap, Z):
    """(name, dtype, shape) of track_history's state arrays over T frames: HISTORY's four, and stay with zones."""
    return tuple((name, dtype, (T, cap) + tail) for name, dtype, tail in HISTORY) + (
        (("stay", torch.int32, (T, cap, Z)),) if Z else ())


def track_history(people, k, prev, gap=None, zones=None, carry=0, state=None, slot=0):
    """Age, hits, path length, origin and zone dwell of every tracked detection, from the links (prev, gap)
    track_people / track_stream left on the device (lidar_track_history_f64; DESIGN.md §3 "Track history").
    people (T, cap, 2), k (T,), prev (T, cap) int32; gap (T, cap) int32, or None for track_people's prev (every link
    spans one frame); zones (Z, 4) float64 device tensor, 1 .. 64 rows as track_events takes it, or None; the first
    `carry` (0 .. T) frames' history is given in `state` = (age, hits, path, origin), or (age, hits, path, origin,
    stay) with zones, each with T frames: (T, cap) int32, (T, cap) int32, (T, cap) float64, (T, cap, 2) float64,
    (T, cap, Z) int32; the call fills the other frames in place.  Without a state (carry 0) they are allocated.
    -> (age, hits, path, origin, stay, dwell (T - carry, Z, 3) int64: the stays that ended in each frame, their
    number, their summed and their largest length in frames), device tensors, nothing synchronised; stay and dwell
    are None without zones.  T == carry: no native call, nothing is written."""
    what = "track_history"
    T, cap = _check_people(what, people, k)
    dev = people.device
    _check_links(what, people, prev, gap)
    Z = _check_device_table(what, "zones", zones, dev)
    carry = _integer(what, "carry", carry, T, "T = ")
    state = _take(what, "state", state, history_layout(T, cap, Z), dev, " with zones" if Z else " without zones",
                  carry=carry)
    # age, hits, path, origin, stay, dwell: without zones the state has no stay
    out = state + ((torch.empty((T - carry, Z, 3), dtype=torch.int64, device=dev),) if Z else (None, None))
    if T > carry:  # an empty tensor has no address to pass
        nat.call("lidar_track_history_f64", nat.handle(dev.index, slot), nat.ptr(people), nat.ptr(k), nat.ptr(prev),
                 nat.ptr(gap), T, cap, carry, nat.ptr(zones), Z, *(nat.ptr(t) for t in out), nat.stream_ptr())
    return out


# ------------------------------------------------------------------ routes
ROUTES = ("first_zone", "last_zone", "away", "legs", "leg_from", "leg_frames")  # track_routes' state arrays, in order


def routes_layout(T, cap, Z):
    """(name, dtype, shape) of track_routes' outputs over T frames: ROUTES' six (T, cap) int32, then trips (Z, Z, 3)
    int64."""
    return tuple((name, torch.int32, (T, cap)) for name in ROUTES) + (("trips", torch.int64, (Z, Z, 3)),)


def track_routes(people, k, prev, gap=None, zones=None, carry=0, state=None, trips=None, accumulate=False, slot=0):
    """Where every tracked person goes next: zone-to-zone trips and their travel times from the links (prev, gap)
    track_people / track_stream left on the device (lidar_track_routes_f64; DESIGN.md §3 "Routes").  people
    (T, cap, 2), k (T,), prev (T, cap) int32; gap (T, cap) int32, or None for track_people's prev (every link spans
    one frame); zones (Z, 4) float64 device tensor, 1 .. 64 rows as track_events takes it, needed: a position belongs
    to the lowest zone that holds it, so the table is ordered by priority; the first `carry` (0 .. T) frames' route
    state is given in `state` = ROUTES' six arrays, each (T, cap) int32; the call fills the other frames in place.
    Without a state (carry 0) they are allocated.  -> (first_zone, last_zone, away, legs, leg_from, leg_frames, trips),
    device tensors, nothing synchronised: per row the first zone the track was seen in and the zone of its most
    recent detection inside any zone (-1: none yet), the frames since that detection, the legs made so far, and, on
    the row that completes a leg (an arrival from another zone, or back into the same one after a detection outside
    every zone), the zone left and the frames from the last detection there to this one (-1 and 0 otherwise); trips
    (Z, Z, 3) int64 indexed [from][to]: the legs, their summed and their longest length in frames.  trips: the array
    to use; accumulate=True goes on from what it holds (a stream's calls then give one call's numbers), otherwise it
    counts from zero.  T == carry: no row is written."""
    what = "track_routes"
    T, cap = _check_people(what, people, k)
    dev = people.device
    _check_links(what, people, prev, gap)
    Z = _check_device_table(what, "zones", zones, dev)
    if not Z:
        raise ValueError(f"{what}: needs zones")
    carry = _integer(what, "carry", carry, T, "T = ")
    layout = routes_layout(T, cap, Z)
    state = _take(what, "state", state, layout[:6], dev, carry=carry)
    if trips is None and accumulate:
        raise ValueError(f"{what}: accumulate needs the trips to go on from")
    trips, = _take(what, "trips", None if trips is None else (trips,), layout[6:], dev)
    if T > carry:  # an empty tensor has no address to pass
        nat.call("lidar_track_routes_f64", nat.handle(dev.index, slot), nat.ptr(people), nat.ptr(k), nat.ptr(prev),
                 nat.ptr(gap), T, cap, carry, nat.ptr(zones), Z, *(nat.ptr(t) for t in state), nat.ptr(trips),
                 1 if accumulate else 0, nat.stream_ptr())
    elif not accumulate:  # no native call: the trips count from zero all the same
        trips.zero_()
    return state + (trips,)


# ------------------------------------------------------------------ crowding
# track_crowding's outputs, in order: seven per row, two per frame, two per cell of the venue grid
CROWDING = ("neighbours", "nearest", "spacing", "density", "movers", "variance", "pressure", "crowded", "peaks",
            "cell_peak", "cell_crowded")
DENSITY_LIMIT = 4.0    # people per m^2: the "Critical" edge of CrowdDensityModel.calculate_risk_level
PRESSURE_LIMIT = 0.02  # 1/s^2: the crowd pressure at which Helbing et al. (2007) report turbulence


def crowding_layout(nf, cap, grid):
    """(name, dtype, shape) of track_crowding's eleven outputs over nf frames; grid: (x0, y0, nx, ny) or None, the
    two cell arrays then with shape None."""
    cells = (None, None) if grid is None else (tuple(grid[2:]) + (2,), tuple(grid[2:]))
    i32, f64 = torch.int32, torch.float64
    return tuple(zip(CROWDING, (i32, i32, f64, f64, i32, f64, f64, i32, f64, f64, i32),
                     ((nf, cap),) * 7 + ((nf, 2), (nf, 3)) + cells))


def _limit(what, name, v):
    v = float(v)
    if not v >= 0.0:
        raise ValueError(f"{what}: {name} must be >= 0 (inf: never), got {v}")
    return v


def _crowding(people, k, prev, velocity, first, radius, limits, grid, grid_size, accumulate, out, slot):
    """lidar_track_crowding_f64 over checked tensors: out = the eleven arrays, the last two None without a grid."""
    x0, y0, nx, ny = grid or (0.0, 0.0, 0, 0)
    T, cap = people.shape[:2]
    nat.call("lidar_track_crowding_f64", nat.handle(people.device.index, slot), nat.ptr(people), nat.ptr(k),
             nat.ptr(prev), nat.ptr(velocity), T, cap, first, radius, *limits, x0, y0, grid_size, nx, ny,
             1 if accumulate else 0, *(nat.ptr(t) for t in out), nat.stream_ptr())


def track_crowding(people, k, prev, velocity, radius, density_limit=DENSITY_LIMIT, pressure_limit=PRESSURE_LIMIT,
                   x_range=None, y_range=None, grid_size=1.0, first=0, out=None, cells=None, accumulate=False, slot=0):
    """How tightly packed every tracked person is within its own frame, and how coherently the people around it
    move (lidar_track_crowding_f64; DESIGN.md §3 "Crowding").  people (T, cap, 2), k (T,), prev (T, cap) int32 and
    velocity (T, cap, 2) as track_people / track_stream leave them; radius metres; only the frames t >= first are
    evaluated.  -> CROWDING's eleven, device tensors, nothing synchronised: per row (T - first, cap) neighbours
    int32 (the valid people within the radius, the row itself not counted; -1 at or past K_t), nearest int32 (the
    closest valid person of the whole frame, the lowest row on a tie, -1 without one), spacing float64 (the distance
    to it, inf without one), density float64 ((neighbours + 1) / (pi radius^2), people per m^2), movers int32 (the
    row and its neighbours that have a measured velocity), variance float64 (the variance of their velocities,
    (m/s)^2, 0 with fewer than two) and pressure float64 = density * variance (1/s^2, the crowd pressure of Helbing
    et al., 2007); per frame crowded (T - first, 2) int32 (the people at or above density_limit, at or above
    pressure_limit) and peaks (T - first, 3) float64 (largest density, largest pressure, smallest spacing); with
    x_range / y_range per cell of the venue grid (VenueGrid's binning) cell_peak (nx, ny, 2) float64 (largest density
    and pressure of the people seen in the cell) and cell_crowded (nx, ny) int32 (those at or above density_limit),
    None without an extent.  The defaults, 4.0 people per m^2 (calculate_risk_level's "Critical") and 0.02 1/s^2 (the
    level at which Helbing et al. observed turbulence), are starting points for a venue's own limits, not
    measurements; inf means never.  out: the nine per-row and per-frame arrays preallocated (a None among them is
    allocated); cells = (cell_peak, cell_crowded) preallocated; accumulate=True goes on from what cells hold (a
    stream's calls then give one call's bits), otherwise they start from 0.  Every element is written, none of the
    nine when first == T."""
    what = "track_crowding"
    T, cap = _check_people(what, people, k)
    dev = people.device
    _check_links(what, people, prev)
    _check_tensor(what, "velocity", velocity, dev, torch.float64, (T, cap, 2))
    radius = _positive(what, "radius", radius)
    limits = _limit(what, "density_limit", density_limit), _limit(what, "pressure_limit", pressure_limit)
    if (x_range is None) != (y_range is None):
        raise ValueError(f"{what}: x_range and y_range go together")
    g = _positive(what, "grid_size", grid_size)
    grid = None if x_range is None else venue_grid(x_range, y_range, g)  # (x0, y0, nx, ny)
    first = _integer(what, "first", first, T, "T = ")
    layout = crowding_layout(T - first, cap, grid)
    out = _take(what, "out", out, layout[:9], dev, holes=True)
    if cells is None:
        if accumulate and grid is not None:
            raise ValueError(f"{what}: accumulate needs the cells to go on from")
        with nat.grid_alloc():
            cells = tuple(None if shape is None else torch.zeros(shape, dtype=dtype, device=dev)
                          for _, dtype, shape in layout[9:])
    else:
        cells = _take(what, "cells", cells, layout[9:], dev)
        if not accumulate and T == first:  # no native call below: they start from 0 all the same
            for t in cells:
                if t is not None:
                    t.zero_()
    if T > first:  # an empty tensor has no address to pass
        _crowding(people, k, prev, velocity, first, radius, limits, grid, g, accumulate, out + cells, slot)
    return out + cells


def _crowding_options(what, crowding):
    """PeopleTracker's / analyze_sequence's `crowding`: a radius, or a dict with radius and optionally density_limit
    and pressure_limit -> (radius, (density_limit, pressure_limit))."""
    opts = dict(crowding) if isinstance(crowding, dict) else {"radius": crowding}
    extra = set(opts) - {"radius", "density_limit", "pressure_limit"}
    if extra or "radius" not in opts:
        raise ValueError(f"{what}: crowding is a radius or a dict with radius, density_limit, pressure_limit, got "
                         f"{sorted(opts)}")
    return _positive(what, "crowding radius", opts["radius"]), (
        _limit(what, "density_limit", opts.get("density_limit", DENSITY_LIMIT)),
        _limit(what, "pressure_limit", opts.get("pressure_limit", PRESSURE_LIMIT)))


class PeopleTracker:
    """A sensor's people tracked batch after batch: ids that last across push() calls, tracks stitched over up
    to max_gap missed frames, and (with a venue extent) the flow cells of everything pushed so far.

    push(people, k) takes a batch of any T >= 0 consecutive frames (cap is fixed by the first push).  The
    tracker keeps the last min(max_gap + 1, frames seen) frames on the device in one window (layout(): people, k
    and the five state arrays; held() returns it by name), extends it by the batch, and calls
    lidar_track_stream_f64 with the held frames as the carry; with an extent it then calls
    lidar_flow_cells_acc_f64(first = carry, accumulate = 1) into its own count / vsum.  Whatever the batch sizes,
    the outputs are those of one call over the whole stream, bit for bit.  Nothing is synchronised.  ntracks ()
    int64, matched () int64 (detections with a measured velocity), count (nx, ny) int32 and vsum (nx, ny, 2)
    float64 are device tensors (count / vsum None without an extent); frames is the number of frames seen.

    gates (G, 4) and / or zones (Z, 4), array-likes as check_gates / check_zones take them, are validated here
    and uploaded once, at the first push; push then also calls lidar_track_events_f64(first = carry) and adds the
    new frames' counts into gate_total (G, 2) int64 (forward, backward) and zone_total (Z, 2) int64 (entries,
    exits), device tensors (the attributes G and Z: 0 for an absent kind; occupancy is per frame and not accumulated).
    last_events: track_events' five arrays for the frames of the last push.  However the stream is cut into
    pushes, the concatenated last_events and the totals are those of one call over the whole stream.  Without
    gates and zones the three stay None and push makes no further call.

    history=True: push also calls lidar_track_history_f64(carry = the held frames) after the tracking call, with the
    zones table if one was given, and keeps the history arrays of the held frames beside the association state.
    last_history: track_history's six outputs (age, hits, path, origin, stay, dwell) for the frames of the last push
    (stay and dwell None without zones); dwell_total (Z, 3) int64, with zones: the completed stays of the whole
    stream, their number and summed length added and their largest length maximised across pushes.  However the
    stream is cut, the concatenated last_history and dwell_total are those of one call over the whole stream.
    Without history the two stay None, and push makes exactly the calls it makes without the keyword.

    crowding: a radius in metres, or a dict with radius and optionally density_limit and pressure_limit
    (track_crowding's defaults).  push then also calls lidar_track_crowding_f64(first = the held frames) after the
    tracking call (prev and velocity of the new frames are final once that call returns: later passes only look
    backwards) and keeps the nine per-row and per-frame arrays of the held frames in the window.  last_crowding:
    track_crowding's first nine outputs for the frames of the last push; crowded_total (2,) int64 and peak_total (3,)
    float64 (largest density, largest pressure, smallest spacing) cover the whole stream; with an extent cell_peak
    (nx, ny, 2) and cell_crowded (nx, ny) accumulate on the tracker's venue grid.  However the stream is cut, they are
    those of one call over the whole stream, bit for bit.  Without crowding they all stay None, and push makes
    exactly the calls it makes without the keyword.

    routes=True (needs zones): push also calls lidar_track_routes_f64(carry = the held frames, accumulate = 1) after
    the tracking call, with the zones table, and keeps the six route arrays of the held frames beside history's.
    last_routes: ROUTES' six arrays for the frames of the last push; trips_total (Z, Z, 3) int64, indexed [from][to]:
    the legs of the whole stream, their summed and their longest length in frames, accumulated on the device by the
    call itself.  However the stream is cut, the concatenated last_routes and trips_total are those of one call over
    the whole stream.  Without routes the two stay None, and push makes exactly the calls it makes without the
    keyword."""

    def __init__(self, dt, gate, max_gap=0, x_range=None, y_range=None, grid_size=1.0, slot=0, gates=None,
                 zones=None, history=False, crowding=None, routes=False):
        self.dt, self.gate = _positive("PeopleTracker", "dt", dt), _positive("PeopleTracker", "gate", gate)
        self.max_gap = _integer("PeopleTracker", "max_gap", max_gap, MAX_GAP)
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
        self._tables = (None if gates is None else check_gates(gates), None if zones is None else check_zones(zones))
        self.G, self.Z = (0 if t is None else t.shape[0] for t in self._tables)
        self.events = self.G + self.Z > 0
        self.gate_total = self.zone_total = self.last_events = None
        self.history = bool(history)
        self.last_history = self.dwell_total = None
        self.crowding = None if crowding is None else _crowding_options("PeopleTracker", crowding)
        self.last_crowding = self.crowded_total = self.peak_total = self.cell_peak = self.cell_crowded = None
        self.routes = bool(routes)
        if self.routes and not self.Z:
            raise ValueError("PeopleTracker: routes need zones")
        self.last_routes = self.trips_total = None
        self._window = None  # name -> tensor: the last frames' arrays, layout()'s rows

    def layout(self, T):
        """(name, dtype, shape) of every array held, over T frames: people, k, STATE's five, track_events' arrays with
        gates / zones (no mask of an absent kind), track_history's state arrays with history=True, track_routes' six
        with routes=True, track_crowding's nine per-row and per-frame arrays with crowding.  cap: 1 before the first push."""
        cap = self.cap or 1
        rows = (("people", torch.float64, (T, cap, 2)), ("k", torch.int64, (T,))) + state_layout(T, cap)
        if self.events:
            rows += event_layout(T, cap, self.G, self.Z)
        if self.history:
            rows += history_layout(T, cap, self.Z)
        if self.routes:
            rows += routes_layout(T, cap, self.Z)[:6]
        if self.crowding:
            rows += crowding_layout(T, cap, None)[:9]
        return tuple(row for row in rows if row[2] is not None)

    def held(self):
        """name -> device tensor under layout()'s names: the last min(max_gap + 1, frames) frames as they stand now
        (a later push may set succ in them).  Empty before the first push."""
        return dict(self._window or {})

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
            self._window = {name: torch.empty(shape, dtype=dtype, device=dev) for name, dtype, shape in self.layout(0)}
            if self.events:
                self._tables = tuple(None if t is None else torch.from_numpy(t).to(dev) for t in self._tables)
                self.gate_total = torch.zeros((self.G, 2), dtype=torch.int64, device=dev)
                self.zone_total = torch.zeros((self.Z, 2), dtype=torch.int64, device=dev)
            if self.history and self.Z:
                self.dwell_total = torch.zeros((self.Z, 3), dtype=torch.int64, device=dev)
            if self.routes:
                self.trips_total = torch.zeros((self.Z, self.Z, 3), dtype=torch.int64, device=dev)
            if self.crowding:
                self.crowded_total = torch.zeros(2, dtype=torch.int64, device=dev)
                self.peak_total = torch.tensor([0.0, 0.0, math.inf], dtype=torch.float64, device=dev)
                if self.grid is not None:
                    with nat.grid_alloc():
                        self.cell_peak = torch.zeros(self.grid[2:] + (2,), dtype=torch.float64, device=dev)
                        self.cell_crowded = torch.zeros(self.grid[2:], dtype=torch.int32, device=dev)
        if cap != self.cap or dev != self.ntracks.device:
            raise ValueError(f"PeopleTracker.push: cap and device are fixed by the first push ({self.cap}, "
                             f"{self.ntracks.device}), got {cap}, {dev}")
        if (self.frames + T) * cap >= 1 << 31:  # every row could be a new detection: the ids are int32
            raise ValueError(f"PeopleTracker.push: {self.frames + T} frames of {cap} rows could pass 2^31 track ids")
        # the window extended by the batch: the C held frames, then the T new ones, which the calls below fill in place
        C = self._window["k"].shape[0]
        new = {"people": people, "k": k}
        w = {name: torch.cat([self._window[name],
                              new[name] if name in new else torch.empty(shape, dtype=dtype, device=dev)])
             for name, dtype, shape in self.layout(T)}
        people, k, prev, gap = w["people"], w["k"], w["prev"], w["gap"]
        if T:  # an empty batch links nothing and moves no cell
            track_stream(people, k, self.dt, self.gate, self.max_gap, C, tuple(w[name] for name, _, _ in STATE),
                         self.ntracks, self.slot)
            self.matched += (prev[C:] >= 0).sum()
            if self.grid is not None:
                _flow_cells_acc(people, k, prev, w["velocity"], C, 1, self.grid, self.grid_size, self.count, self.vsum,
                                self.slot)
        # track_events, track_history and track_routes make no native call either when no frame follows the held ones
        if self.events:
            out = tuple(w[name][C:] if name in w else None for name in EVENTS)
            self.last_events = track_events(people, k, prev, gap, *self._tables, first=C, out=out, slot=self.slot)
            self.gate_total += out[0].sum(dim=0, dtype=torch.int64)
            self.zone_total += out[1][:, :, 1:].sum(dim=0, dtype=torch.int64)
        if self.history:
            state = tuple(w[name] for name, _, _ in history_layout(C + T, cap, self.Z))
            out = track_history(people, k, prev, gap, self._tables[1], C, state, self.slot)
            self.last_history = tuple(None if t is None else t[C:] for t in out[:5]) + (out[5],)
            if out[5] is not None:
                self.dwell_total[:, :2] += out[5][:, :, :2].sum(dim=0)
                # the largest of the total and the new frames: no reduction over an empty frame axis at T == 0
                self.dwell_total[:, 2] = torch.cat([self.dwell_total[None, :, 2], out[5][:, :, 2]]).amax(dim=0)
        if self.routes:  # the trips go on in trips_total: no torch add per push
            out = track_routes(people, k, prev, gap, self._tables[1], C, tuple(w[name] for name in ROUTES),
                               self.trips_total, True, self.slot)
            self.last_routes = tuple(t[C:] for t in out[:6])
        if self.crowding:
            out = tuple(w[name][C:] for name in CROWDING[:9])
            if T:
                _crowding(people, k, prev, w["velocity"], C, self.crowding[0], self.crowding[1], self.grid,
                          self.grid_size, True, out + (self.cell_peak, self.cell_crowded), self.slot)
            self.last_crowding = out
            self.crowded_total += out[7].sum(dim=0, dtype=torch.int64)
            # the extremes of the total and the new frames: no reduction over an empty frame axis at T == 0
            self.peak_total[:2] = torch.cat([self.peak_total[None, :2], out[8][:, :2]]).amax(dim=0)
            self.peak_total[2] = torch.cat([self.peak_total[2:], out[8][:, 2]]).amin()
        self.frames += T
        keep = min(self.max_gap + 1, self.frames)
        self._window = {name: t[C + T - keep:] for name, t in w.items()}
        return prev[C:], gap[C:], w["track_id"][C:], w["velocity"][C:]
