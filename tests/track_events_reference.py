"""Host specification of ``lidar_track_events_f64`` / ``people_tracking.track_events`` (plain numpy loops, DESIGN.md
§3 "Gate and zone events"), and the gate / zone tables and the crossing scene the CPU and GPU tests share.

All arithmetic is float64 with one rounding per operation (numpy scalars).  A row (t, j), j < K_t, is linked iff
i = prev[t, j] >= 0, 1 <= g <= 8, g <= t and i < K_(t-g), g = gap[t, j] (1 without gap); P = people[t - g, i],
Q = people[t, j].  A link crosses a gate A -> B iff the four sides (P and Q of A -> B, A and B of P -> Q) are finite
and each pair lies on different sides (>= 0 against < 0); forward iff Q is on the left or on the line.  A zone holds a
point iff x0 <= x < x1 and y0 <= y < y1.
"""
import functools

import numpy as np

import track_stream_reference as sref
from track_reference import DT, JUNK, STEP, clamp_k

MAX_LINK = 8
MAX_TABLE = 64


def side(ax, ay, bx, by, px, py):
    return ((bx - ax) * (py - ay)) - ((by - ay) * (px - ax))


def inside(zone, x, y):
    x0, x1, y0, y1 = zone
    return bool(x0 <= x and x < x1 and y0 <= y and y < y1)


def link_of(people, K, prev, gap, t, j):
    """(t - g, i) of the linked row (t, j), None for an unlinked one."""
    i = int(prev[t, j])
    g = 1 if gap is None else int(gap[t, j])
    if i >= 0 and 1 <= g <= MAX_LINK and g <= t and i < K[t - g]:
        return t - g, i
    return None


def crossing(gate, P, Q):
    """0: the link P -> Q does not cross the gate; +1: forward; -1: backward."""
    ax, ay, bx, by = gate
    with np.errstate(all="ignore"):
        sP, sQ = side(ax, ay, bx, by, P[0], P[1]), side(ax, ay, bx, by, Q[0], Q[1])
        sA, sB = side(P[0], P[1], Q[0], Q[1], ax, ay), side(P[0], P[1], Q[0], Q[1], bx, by)
        if not (np.isfinite(sP) and np.isfinite(sQ) and np.isfinite(sA) and np.isfinite(sB)):
            return 0
        if (sP >= 0) != (sQ >= 0) and (sA >= 0) != (sB >= 0):
            return 1 if sQ >= 0 else -1
    return 0


def events_spec(people, k, prev, gap, gates, zones, first=0):
    """people (T, cap, 2), k (T,), prev (T, cap), gap (T, cap) or None, gates (G, 4) or None, zones (Z, 4) or None ->
    (gate_counts (T - first, G, 2) int32, zone_counts (T - first, Z, 3) int32, gate_fwd, gate_bwd, zone_in
    (T - first, cap) int64)."""
    people = np.asarray(people, dtype=np.float64)
    T, cap, _ = people.shape
    gates = np.zeros((0, 4)) if gates is None else np.asarray(gates, dtype=np.float64).reshape(-1, 4)
    zones = np.zeros((0, 4)) if zones is None else np.asarray(zones, dtype=np.float64).reshape(-1, 4)
    G, Z = len(gates), len(zones)
    assert G <= MAX_TABLE and Z <= MAX_TABLE and G + Z >= 1 and 0 <= first <= T
    K = clamp_k(k, cap)
    n = T - first
    gate_counts = np.zeros((n, G, 2), dtype=np.int32)
    zone_counts = np.zeros((n, Z, 3), dtype=np.int32)
    masks = np.zeros((3, n, cap), dtype=np.uint64)  # fwd, bwd, in
    for t in range(first, T):
        f = t - first
        for j in range(K[t]):
            Q = people[t, j]
            src = link_of(people, K, prev, gap, t, j)
            P = None if src is None else people[src]
            with np.errstate(all="ignore"):
                for z in range(Z):
                    inq = inside(zones[z], Q[0], Q[1])
                    if inq:
                        zone_counts[f, z, 0] += 1
                        masks[2, f, j] |= np.uint64(1) << np.uint64(z)
                    if P is not None:
                        inp = inside(zones[z], P[0], P[1])
                        zone_counts[f, z, 1] += inq and not inp
                        zone_counts[f, z, 2] += inp and not inq
            if P is None:
                continue
            for g in range(G):
                c = crossing(gates[g], P, Q)
                if c:
                    gate_counts[f, g, 0 if c > 0 else 1] += 1
                    masks[0 if c > 0 else 1, f, j] |= np.uint64(1) << np.uint64(g)
    fwd, bwd, zin = (m.view(np.int64) for m in masks)
    return gate_counts, zone_counts, fwd, bwd, zin


NAMES = ("gate_counts", "zone_counts", "gate_fwd", "gate_bwd", "zone_in")
DTYPES = (np.int32, np.int32, np.int64, np.int64, np.int64)


# ------------------------------------------------------------------ the scenes' tables
def lattice_side(n):
    """The lattice nodes per axis of track_stream_reference's gappy sequence of n walkers."""
    return max(4, int(round(0.75 * np.sqrt(n) / STEP)))


def scene_tables(s):
    """(gates (7, 4), zones (3, 4)) for a scene on the 2^-3 m lattice of s nodes per axis: a lattice line, an
    oblique gate with non-dyadic coordinates, a short off-lattice gate, an off-lattice line and its reverse, a
    degenerate gate and a NaN gate; a quadrant, everything, and a zone with non-dyadic edges."""
    L, mid = s * STEP, (s // 2) * STEP
    off = mid + 0.0625
    gates = np.array([(mid, -1.0, mid, L + 1.0),
                      (0.3, -0.7, L - 0.1, L + 0.45),
                      (off, (s // 4) * STEP, off, mid),
                      (off, -1.0, off, L + 1.0),
                      (off, L + 1.0, off, -1.0),
                      (mid, mid, mid, mid),
                      (mid, np.nan, mid, L + 1.0)], dtype=np.float64)
    zones = np.array([(0.0, mid, 0.0, mid),
                      (-1.0, L + 1.0, -1.0, L + 1.0),
                      (0.3, mid + 0.3, 0.2, 0.7 * L)], dtype=np.float64)
    return gates, zones


LATTICE, OBLIQUE, SHORT, OFF, OFF_REVERSED, DEGENERATE, NAN_GATE = range(7)


@functools.lru_cache(maxsize=None)
def gappy_events(T, n, seed, gate, max_gap):
    """events_spec of the gappy sequence's stream_spec under scene_tables, cached and shared."""
    people, k = sref.gappy_sequence(T, n, seed)
    s = sref.gappy_spec(T, n, seed, gate, max_gap)
    gates, zones = scene_tables(lattice_side(n))
    return events_spec(people, k, s["prev"], s["gap"], gates, zones)


# ------------------------------------------------------------------ a scene with many crossings
CROSSING = dict(n=200, T=12, side=96, reach=16, miss=0.12, gate=0.5, max_gap=2, seed=3)


@functools.lru_cache(maxsize=None)
def crossing_scene():
    """(people (12, 203, 2), k (12,), gates, zones), read-only and cached: 200 walkers on a lattice of 96 nodes per
    axis, half of them starting up to 16 nodes left of the middle and drifting +x, half up to 16 nodes right of it
    drifting -x, 1 or 2 nodes per frame (y moves by -1 .. 1), each left out of a frame with probability 0.12; rows
    permuted per frame, junk past K_t."""
    c = CROSSING
    rng = np.random.default_rng(11000 + c["seed"])
    n, T, s = c["n"], c["T"], c["side"]
    half = n // 2
    direction = np.where(np.arange(n) < half, 1, -1)
    reach = c["reach"]
    pos = np.column_stack([np.where(direction > 0, rng.integers(s // 2 - reach, s // 2, n),
                                    rng.integers(s // 2, s // 2 + reach, n)), rng.integers(0, s, n)])
    cap = n + 3
    people = np.empty((T, cap, 2), dtype=np.float64)
    k = np.empty(T, dtype=np.int64)
    for t in range(T):
        if t:
            pos = pos + np.column_stack([direction * rng.integers(1, 3, n), rng.integers(-1, 2, n)])
        rows = np.flatnonzero(rng.random(n) >= c["miss"])
        rows = rows[rng.permutation(len(rows))]
        k[t] = len(rows)
        people[t, :len(rows)] = pos[rows] * STEP
        junk = np.full((cap - len(rows), 2), JUNK)
        junk[::2, rng.integers(0, 2)] = np.nan
        people[t, len(rows):] = junk
    gates, zones = scene_tables(s)
    for a in (people, k, gates, zones):
        a.setflags(write=False)
    return people, k, gates, zones


@functools.lru_cache(maxsize=None)
def crossing_spec(max_gap=CROSSING["max_gap"]):
    """(stream_spec, events_spec) of the crossing scene."""
    people, k, gates, zones = crossing_scene()
    s = sref.stream_spec(people, k, DT, CROSSING["gate"], max_gap)
    return s, events_spec(people, k, s["prev"], s["gap"], gates, zones)
