"""Host specification of ``lidar_track_stream_f64`` / ``lidar_flow_cells_acc_f64`` / ``people_tracking.PeopleTracker``
(plain numpy, DESIGN.md §3 "Continuous people tracking"), and the gappy sequences the CPU and GPU tests share.

The association of ``track_reference`` repeated for frame distances g = 1 .. max_gap + 1 in ascending order, each
pass restricted to the rows still open (ends without a successor, starts without a predecessor), its gate and its
time step multiplied by g; the first ``carry`` frames' state is given, so a stream cut anywhere equals the whole.
"""
import functools

import numpy as np

from track_reference import (DT, JUNK, STEP, bin_right, arange_edges, clamp_k, flow_vectors_spec, pair_nearest,
                             venue_grid)

STATE = ("prev", "gap", "succ", "velocity", "track_id")
MAX_GAP = 7


def empty_state(T, cap):
    return {"prev": np.full((T, cap), -1, dtype=np.int32), "gap": np.zeros((T, cap), dtype=np.int32),
            "succ": np.zeros((T, cap), dtype=np.uint8), "velocity": np.zeros((T, cap, 2), dtype=np.float64),
            "track_id": np.full((T, cap), -1, dtype=np.int32)}


def stream_spec(people, k, dt, gate, max_gap=0, carry=0, state=None, ntracks=0):
    """people (T, cap, 2) float64, k (T,); state: the five arrays whose first `carry` frames are given (the rest
    is ignored); ntracks: the id base -> dict of the five arrays (T, cap, ...) and ntracks (int)."""
    people = np.asarray(people, dtype=np.float64)
    T, cap, _ = people.shape
    M, C = int(max_gap), int(carry)
    assert 0 <= M <= MAX_GAP and 0 <= C <= min(M + 1, T)
    K = clamp_k(k, cap)
    dt, gate = np.float64(dt), np.float64(gate)
    out = empty_state(T, cap)
    for name in STATE:
        if C:
            out[name][:C] = state[name][:C]
    prev, gap, succ, velocity, track_id = (out[name] for name in STATE)
    for g in range(1, M + 2):
        gg, dg = gate * np.float64(g), dt * np.float64(g)  # one fp64 product each; pair_nearest squares gg
        for u in range(max(C, g), T):
            t = u - g
            ia = np.flatnonzero(succ[t, :K[t]] == 0)   # open ends, ascending row index
            jb = np.flatnonzero(prev[u, :K[u]] == -1)  # open starts
            A, B = people[t, ia], people[u, jb]
            fwd, bwd, _, _ = pair_nearest(A, B, gg)
            for b, j in enumerate(jb):
                a = bwd[b]
                if a >= 0 and fwd[a] == b:
                    i = ia[a]
                    prev[u, j], gap[u, j], succ[t, i] = i, g, 1
                    velocity[u, j, 0] = (people[u, j, 0] - people[t, i, 0]) / dg
                    velocity[u, j, 1] = (people[u, j, 1] - people[t, i, 1]) / dg
    ntracks = int(ntracks)
    for u in range(C, T):
        for j in range(K[u]):
            if prev[u, j] < 0:
                track_id[u, j] = ntracks
                ntracks += 1
            else:
                track_id[u, j] = track_id[u - gap[u, j], prev[u, j]]
    out["ntracks"] = ntracks
    return out


def split_spec(people, k, dt, gate, max_gap, cuts):
    """The sequence run in pieces cut at the frames `cuts` (ascending, repeats allowed: an empty piece), every
    piece handed the last min(max_gap + 1, frames seen) frames of what came before -> the whole sequence's dict,
    assembled from the pieces' own frames."""
    T, cap, _ = people.shape
    whole = empty_state(T, cap)
    ntracks, lo = 0, 0
    for hi in list(cuts) + [T]:
        c = min(max_gap + 1, lo)
        sl = slice(lo - c, hi)
        part = stream_spec(people[sl], k[sl], dt, gate, max_gap, c, {n: whole[n][sl] for n in STATE}, ntracks)
        for n in STATE:
            if n != "succ":  # a carried frame changes in succ alone
                assert part[n][:c].tobytes() == whole[n][lo - c:lo].tobytes(), n
            whole[n][sl] = part[n]
        ntracks, lo = part["ntracks"], hi
    whole["ntracks"] = ntracks
    return whole


def matched_rows_from(k, prev, first):
    """[(t, j)] of the matched detections of frames >= first in (t, j) ascending order."""
    T, cap = prev.shape
    K = clamp_k(k, cap)
    return [(t, j) for t in range(first, T) for j in range(K[t]) if prev[t, j] >= 0]


def flow_cells_acc_spec(people, k, prev, velocity, x0, y0, g, nx, ny, first=1, count=None, vsum=None):
    """-> (count, vsum): flow_cells_spec over the frames >= first, continuing from count / vsum when given."""
    xe, ye = arange_edges(x0, g, nx), arange_edges(y0, g, ny)
    count = np.zeros((nx, ny), dtype=np.int32) if count is None else count.copy()
    vsum = np.zeros((nx, ny, 2), dtype=np.float64) if vsum is None else vsum.copy()
    for t, j in matched_rows_from(k, prev, first):
        bx, by = bin_right(xe, people[t, j, 0]), bin_right(ye, people[t, j, 1])
        if bx < 0 or by < 0:
            continue
        count[bx, by] += 1
        vsum[bx, by, 0] = vsum[bx, by, 0] + velocity[t, j, 0]
        vsum[bx, by, 1] = vsum[bx, by, 1] + velocity[t, j, 1]
    return count, vsum


def stream_result_spec(people, k, dt, gate, max_gap, x_range, y_range, grid_size=1.0, min_observations=1):
    """What analyze_sequence(max_gap=...) and analyze_stream owe, bottlenecks apart."""
    s = stream_spec(people, k, dt, gate, max_gap)
    x0, y0, nx, ny, gx, gy = venue_grid(x_range, y_range, grid_size)
    count, vsum = flow_cells_acc_spec(people, k, s["prev"], s["velocity"], x0, y0, grid_size, nx, ny, first=0)
    fv, obs = flow_vectors_spec(count, vsum, gx, gy, min_observations)
    K = clamp_k(k, people.shape[1])
    rows = range(len(K))
    return {"flow_vectors": fv, "observations": obs, "tracks": s["ntracks"],
            "matched": len(matched_rows_from(k, s["prev"], 0)),
            "track_ids": [s["track_id"][t, :K[t]] for t in rows], "velocities": [s["velocity"][t, :K[t]] for t in rows],
            "gaps": [s["gap"][t, :K[t]] for t in rows], "count": count, "vsum": vsum}


# ------------------------------------------------------------------ gappy sequences
GAPPY = [(9, 40, 2), (7, 300, 0), (5, 2100, 0)]  # (T, n, seed); the last crosses the 2 048-row LDS tile
GATES = (0.25, 0.5)
MISS = 0.12


@functools.lru_cache(maxsize=None)
def _gappy(T, n, seed):
    rng = np.random.default_rng(9000 + seed)
    side = max(4, int(round(0.75 * np.sqrt(n) / STEP)))
    pos = rng.integers(0, side, (n, 2))
    alive = rng.random(n) < 0.85
    cap = n + 3
    people = np.empty((T, cap, 2), dtype=np.float64)
    k = np.empty(T, dtype=np.int64)
    steps = np.array([-2, -1, 0, 1, 2])
    for t in range(T):
        if t:
            die = alive & (rng.random(n) < 0.05)
            born = ~alive & (rng.random(n) < 0.30)
            pos = pos + rng.choice(steps, (n, 2), p=[0.1, 0.2, 0.4, 0.2, 0.1])
            alive = (alive & ~die) | born
            pos[born] = rng.integers(0, side, (int(born.sum()), 2))  # a birth lands on a fresh node
        seen = alive & (rng.random(n) >= MISS)  # a missed detection: the walker goes on, the frame lacks it
        rows = np.flatnonzero(seen)
        rows = rows[rng.permutation(len(rows))]
        k[t] = len(rows)
        people[t, :len(rows)] = pos[rows] * STEP
        junk = np.full((cap - len(rows), 2), JUNK)
        junk[::2, rng.integers(0, 2)] = np.nan
        people[t, len(rows):] = junk
    people.setflags(write=False)
    k.setflags(write=False)
    return people, k


def gappy_sequence(T, n, seed=0):
    """(people (T, n + 3, 2) float64, k (T,) int64), read-only and cached: track_reference.planted_sequence's
    walkers, each live walker additionally left out of a frame with probability 0.12, re-births on fresh nodes."""
    return _gappy(T, n, seed)


@functools.lru_cache(maxsize=None)
def gappy_spec(T, n, seed, gate, max_gap):
    people, k = gappy_sequence(T, n, seed)
    return stream_spec(people, k, DT, gate, max_gap)


def dropout_scene(n_side, T, max_gap, gate, seed):
    """Constant-velocity walkers on the 2^-3 m lattice, spaced 4 * gate * (max_gap + 1) apart (rounded up to the
    lattice), all moving one lattice step in x per frame (dt = STEP: 1 m/s); every walker is present in frame 0
    and the last frame and goes missing once for 1 .. max_gap consecutive frames in between (where T allows).
    -> (people (T, n + 2, 2), k, present (T, n) bool, rows (T, n): walker w's row in frame t or -1)."""
    rng = np.random.default_rng(seed)
    n = n_side * n_side
    spacing = np.ceil(4.0 * gate * (max_gap + 1) / STEP) * STEP
    gx, gy = np.meshgrid(np.arange(n_side, dtype=np.float64), np.arange(n_side, dtype=np.float64))
    base = np.column_stack([gx.ravel(), gy.ravel()]) * spacing + 0.25
    present = np.ones((T, n), dtype=bool)
    for w in range(n):
        if max_gap >= 1 and T >= 3:
            length = int(rng.integers(1, min(max_gap, T - 2) + 1))
            start = int(rng.integers(1, T - length))
            present[start:start + length, w] = False
    people = np.full((T, n + 2, 2), np.nan)
    k = np.empty(T, dtype=np.int64)
    rows = np.full((T, n), -1, dtype=np.int64)
    for t in range(T):
        who = np.flatnonzero(present[t])
        who = who[rng.permutation(len(who))]
        k[t] = len(who)
        people[t, :len(who)] = base[who] + np.array([t * STEP, 0.0])
        rows[t, who] = np.arange(len(who))
    return people, k, present, rows
