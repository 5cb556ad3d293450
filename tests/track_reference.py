"""Host specification of ``lidar_track_people_f64`` / ``lidar_flow_cells_f64`` / ``CrowdFlowModel.analyze_sequence``
(plain numpy, DESIGN.md §3 "People tracking"), and the planted sequences the CPU and GPU tests share.

All arithmetic is float64 with one rounding per operation (numpy's elementwise operators).  Per consecutive
pair of frames: d(i, j) = (dx*dx) + (dy*dy), candidates d <= gate*gate, fwd / bwd = the candidate with the
smallest (d, index), matched = mutual; ids number the new detections in (t, j) order; flow cells bin the
matched detections by their own position and add their velocities sequentially in (t, j) order.
"""
import functools

import numpy as np


def clamp_k(k, cap):
    return np.minimum(np.maximum(np.asarray(k, dtype=np.int64), 0), cap)


def pair_nearest(A, B, gate):
    """A (Ka, 2), B (Kb, 2) -> (fwd (Ka,), bwd (Kb,), D (Ka, Kb), cand (Ka, Kb))."""
    g2 = np.float64(gate) * np.float64(gate)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = B[None, :, 0] - A[:, None, 0]
        dy = B[None, :, 1] - A[:, None, 1]
        D = (dx * dx) + (dy * dy)
        cand = D <= g2  # a NaN or infinite d is never a candidate
    Dm = np.where(cand, D, np.inf)
    fwd = np.full(len(A), -1, dtype=np.int64)
    bwd = np.full(len(B), -1, dtype=np.int64)
    if len(A) and len(B):
        f = np.argmin(Dm, axis=1)  # the first minimum: the lowest index on a tie
        fwd = np.where(cand.any(axis=1), f, -1)
        b = np.argmin(Dm, axis=0)
        bwd = np.where(cand.any(axis=0), b, -1)
    return fwd, bwd, D, cand


def track_spec(people, k, dt, gate, details=False):
    """people (T, cap, 2) float64, k (T,) -> dict prev (T, cap) int32, track_id (T, cap) int32, velocity
    (T, cap, 2) float64, ntracks int; with details also per pair the fwd, bwd, D and cand of pair_nearest."""
    people = np.asarray(people, dtype=np.float64)
    T, cap, _ = people.shape
    K = clamp_k(k, cap)
    dt = np.float64(dt)
    prev = np.full((T, cap), -1, dtype=np.int32)
    track_id = np.full((T, cap), -1, dtype=np.int32)
    velocity = np.zeros((T, cap, 2), dtype=np.float64)
    pairs = []
    ntracks = 0
    for t in range(T):
        B = people[t, :K[t]]
        if t >= 1:
            A = people[t - 1, :K[t - 1]]
            fwd, bwd, D, cand = pair_nearest(A, B, gate)
            if details:
                pairs.append({"fwd": fwd, "bwd": bwd, "D": D, "cand": cand})
            for j in range(K[t]):
                i = bwd[j]
                if i >= 0 and fwd[i] == j:
                    prev[t, j] = i
                    velocity[t, j, 0] = (B[j, 0] - A[i, 0]) / dt
                    velocity[t, j, 1] = (B[j, 1] - A[i, 1]) / dt
        for j in range(K[t]):
            if prev[t, j] < 0:
                track_id[t, j] = ntracks
                ntracks += 1
            else:
                track_id[t, j] = track_id[t - 1, prev[t, j]]
    out = {"prev": prev, "track_id": track_id, "velocity": velocity, "ntracks": ntracks}
    if details:
        out["pairs"] = pairs
    return out


def arange_edges(a, g, nb):
    """np.arange(a, ., g)'s first nb + 1 elements: e[0] = a, e[1] = a + g, e[i] = a + i * ((a + g) - a)."""
    a, g = np.float64(a), np.float64(g)
    e = a + np.arange(nb + 1, dtype=np.float64) * ((a + g) - a)
    e[0] = a
    if nb >= 1:
        e[1] = a + g
    return e


def bin_right(edges, v):
    """searchsorted right, the last edge closed: the bin index, or -1 outside."""
    nb = len(edges) - 1
    b = int(np.searchsorted(edges, v, side="right"))
    if v == edges[nb]:
        b -= 1
    return b - 1 if 1 <= b <= nb else -1


def matched_rows(k, prev):
    """[(t, j)] of the matched detections in (t, j) ascending order."""
    T, cap = prev.shape
    K = clamp_k(k, cap)
    return [(t, j) for t in range(1, T) for j in range(K[t]) if prev[t, j] >= 0]


def flow_cells_spec(people, k, prev, velocity, x0, y0, g, nx, ny):
    """-> (count (nx, ny) int32, vsum (nx, ny, 2) float64)."""
    xe, ye = arange_edges(x0, g, nx), arange_edges(y0, g, ny)
    count = np.zeros((nx, ny), dtype=np.int32)
    vsum = np.zeros((nx, ny, 2), dtype=np.float64)
    for t, j in matched_rows(k, prev):
        bx, by = bin_right(xe, people[t, j, 0]), bin_right(ye, people[t, j, 1])
        if bx < 0 or by < 0:
            continue
        count[bx, by] += 1
        vsum[bx, by, 0] = vsum[bx, by, 0] + velocity[t, j, 0]
        vsum[bx, by, 1] = vsum[bx, by, 1] + velocity[t, j, 1]
    return count, vsum


def venue_grid(x_range, y_range, g):
    """(x0, y0, nx, ny, grid_x, grid_y) as global_density.VenueGrid derives them, in numpy alone."""
    g = float(g)
    x0, y0 = float(x_range[0]) - g * 2.0, float(y_range[0]) - g * 2.0
    xe = np.arange(x0, (float(x_range[1]) + g * 2.0) + g, g)
    ye = np.arange(y0, (float(y_range[1]) + g * 2.0) + g, g)
    return x0, y0, len(xe) - 1, len(ye) - 1, (xe[:-1] + xe[1:]) / 2, (ye[:-1] + ye[1:]) / 2


def flow_vectors_spec(count, vsum, grid_x, grid_y, min_observations=1):
    """analyze_sequence's flow_vectors and observations from the cells: y index outer, x index inner."""
    nx, ny = count.shape
    ix, iy = np.meshgrid(np.arange(nx), np.arange(ny))  # (ny, nx)
    ix, iy = ix.ravel(), iy.ravel()
    c = count[ix, iy]
    sel = c >= min_observations
    ix, iy, c = ix[sel], iy[sel], c[sel]
    positions = np.column_stack([grid_x[ix], grid_y[iy]]).reshape(-1, 2)
    vectors = vsum[ix, iy] / c[:, None]
    vx, vy = vectors[:, 0], vectors[:, 1]
    return {"positions": positions, "vectors": vectors, "magnitudes": np.sqrt(vx * vx + vy * vy)}, c.astype(np.int32)


# ------------------------------------------------------------------ planted sequences
STEP = 2.0 ** -3   # the lattice, metres
JUNK = 777.25      # a finite constant past K_t (beside NaN)
DT = 0.1
GATES = (0.25, 0.5)
PLANTED = [(7, 40, 2), (5, 300, 0), (3, 2100, 0)]  # (T, n, seed)


@functools.lru_cache(maxsize=None)
def _planted(T, n, seed):
    rng = np.random.default_rng(7000 + seed)
    side = max(4, int(round(0.75 * np.sqrt(n) / STEP)))  # lattice nodes per axis: the scene is about 0.75 sqrt(n) m
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
            for w in np.flatnonzero(born):  # a birth: a fresh node, or (one in four) the node of a walker that is there
                others = np.flatnonzero(alive & (np.arange(n) != w))
                if len(others) and rng.random() < 0.25:
                    pos[w] = pos[rng.choice(others)]
                else:
                    pos[w] = rng.integers(0, side, 2)
        rows = np.flatnonzero(alive)
        rows = rows[rng.permutation(len(rows))]  # the row order is independent per frame
        k[t] = len(rows)
        people[t, :len(rows)] = pos[rows] * STEP
        junk = np.full((cap - len(rows), 2), JUNK)
        junk[::2, rng.integers(0, 2)] = np.nan
        people[t, len(rows):] = junk
    people.setflags(write=False)
    k.setflags(write=False)
    return people, k


def planted_sequence(T, n, seed=0):
    """(people (T, n + 3, 2) float64, k (T,) int64), read-only and cached: walkers on the 2^-3 m lattice moving
    {-2..2} nodes per axis and frame, about 5 % deaths and 30 % re-births per frame, rows permuted per frame,
    junk (a finite constant and NaN) past K_t."""
    return _planted(T, n, seed)


@functools.lru_cache(maxsize=None)
def planted_spec(T, n, seed, gate):
    people, k = planted_sequence(T, n, seed)
    return track_spec(people, k, DT, gate, details=True)


def planted_cases():
    return [(c, g) for c in PLANTED for g in GATES]


def extent_of(people, k):
    """The xy extent of the live rows: (x_range, y_range)."""
    K = clamp_k(k, people.shape[1])
    live = np.concatenate([people[t, :K[t]] for t in range(len(K))]).reshape(-1, 2)
    live = live[np.isfinite(live).all(axis=1)]
    return (live[:, 0].min(), live[:, 0].max()), (live[:, 1].min(), live[:, 1].max())


def sequence_result_spec(people, k, dt, gate, x_range, y_range, grid_size=1.0, min_observations=1):
    """What analyze_sequence owes, bottlenecks apart (they are the model's own _identify_bottlenecks of the
    flow_vectors here)."""
    s = track_spec(people, k, dt, gate)
    x0, y0, nx, ny, gx, gy = venue_grid(x_range, y_range, grid_size)
    count, vsum = flow_cells_spec(people, k, s["prev"], s["velocity"], x0, y0, grid_size, nx, ny)
    fv, obs = flow_vectors_spec(count, vsum, gx, gy, min_observations)
    K = clamp_k(k, people.shape[1])
    return {"flow_vectors": fv, "observations": obs, "tracks": s["ntracks"],
            "matched": len(matched_rows(k, s["prev"])),
            "track_ids": [s["track_id"][t, :K[t]] for t in range(len(K))],
            "velocities": [s["velocity"][t, :K[t]] for t in range(len(K))], "count": count, "vsum": vsum}
