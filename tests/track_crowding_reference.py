"""Host specification of ``lidar_track_crowding_f64`` / ``people_tracking.track_crowding`` (numpy, DESIGN.md §3
"Crowding"), and the scenes the CPU and GPU tests share.

All arithmetic is float64 with one rounding per operation (numpy's elementwise operators on float64).  Per frame on
its own: d(i, j) = (dx*dx) + (dy*dy) with dx = P[i].x - P[j].x; near(i, j): i != j, both valid, d <= R*R; the nearest
is the first minimum of d over the valid i != j with finite d; the three velocity sums of a row run over its moving
neighbours and itself in ascending i, one addition after the other from +0.0 (plain loops: the order is the
specification).  The cells use track_reference's edges and binning, which are lidar_flow_cells_f64's.
"""
import numpy as np

from track_reference import arange_edges, bin_right, clamp_k

ROWS = ("neighbours", "nearest", "spacing", "density", "movers", "variance", "pressure")
NAMES = ROWS + ("crowded", "peaks", "cell_peak", "cell_crowded")
DTYPES = (np.int32, np.int32, np.float64, np.float64, np.int32, np.float64, np.float64, np.int32, np.float64,
          np.float64, np.int32)
RISK = ("Low", "Moderate", "High", "Critical")


def valid_rows(P):
    """P (K, 2) -> (K,) bool: both coordinates finite."""
    return np.isfinite(P).all(axis=1)


def pair_d(P):
    """P (K, 2) -> D (K, K), D[i, j] = d(i, j)."""
    with np.errstate(invalid="ignore", over="ignore"):
        dx = P[:, None, 0] - P[None, :, 0]
        dy = P[:, None, 1] - P[None, :, 1]
        return (dx * dx) + (dy * dy)


def near_matrix(P, radius):
    """near[i, j] over the K rows of a frame (rows that are not valid: False)."""
    R = np.float64(radius)
    v = valid_rows(P)
    with np.errstate(invalid="ignore"):
        near = pair_d(P) <= R * R
    near &= v[:, None] & v[None, :]
    np.fill_diagonal(near, False)
    return near


def frame_spec(P, link, V, radius):
    """One frame's K live rows: P (K, 2), link (K,) prev, V (K, 2) -> dict of the seven per-row arrays (K,)."""
    K = len(P)
    R = np.float64(radius)
    area = (np.float64(np.pi) * R) * R
    valid = valid_rows(P)
    moving = valid & (np.asarray(link) >= 0) & np.isfinite(V).all(axis=1)
    D = pair_d(P)
    near = near_matrix(P, radius)
    out = {"neighbours": np.zeros(K, dtype=np.int32), "nearest": np.full(K, -1, dtype=np.int32),
           "spacing": np.full(K, np.inf), "density": np.zeros(K), "movers": np.zeros(K, dtype=np.int32),
           "variance": np.zeros(K), "pressure": np.zeros(K)}
    for j in np.flatnonzero(valid):
        out["neighbours"][j] = n = int(near[:, j].sum())
        cand = valid & np.isfinite(D[:, j])
        cand[j] = False
        if cand.any():
            dj = np.where(cand, D[:, j], np.inf)
            i = int(np.argmin(dj))  # the first minimum: the lowest index on a tie
            out["nearest"][j] = i
            out["spacing"][j] = np.sqrt(dj[i])
        out["density"][j] = np.float64(n + 1) / area
        members = near[:, j] & moving
        members[j] = moving[j]
        sx = sy = sq = np.float64(0.0)
        m = 0
        with np.errstate(invalid="ignore", over="ignore"):
            for i in np.flatnonzero(members):  # ascending i, one addition after the other
                vx, vy = V[i, 0], V[i, 1]
                sx = sx + vx
                sy = sy + vy
                sq = sq + ((vx * vx) + (vy * vy))
                m += 1
            out["movers"][j] = m
            var = np.float64(0.0)
            if m >= 2:
                md = np.float64(m)
                mx, my = sx / md, sy / md
                var = (sq / md) - ((mx * mx) + (my * my))
                if not np.isnan(var) and not var > 0.0:
                    var = np.float64(0.0)
            out["variance"][j] = var
            out["pressure"][j] = out["density"][j] * var
    return out, valid


def crowding_spec(people, k, prev, velocity, radius, density_limit=4.0, pressure_limit=0.02, grid=None, first=0,
                  cells=None):
    """people (T, cap, 2), k (T,), prev (T, cap), velocity (T, cap, 2); grid: (x0, y0, g, nx, ny) or None; cells:
    (cell_peak, cell_crowded) to go on from (accumulate) or None (from 0) -> dict of NAMES' arrays over the frames
    >= first (the cell arrays None without a grid), and "valid" (T - first, cap) bool."""
    people = np.asarray(people, dtype=np.float64)
    velocity = np.asarray(velocity, dtype=np.float64)
    T, cap, _ = people.shape
    K = clamp_k(k, cap)
    nf = T - first
    out = {"neighbours": np.full((nf, cap), -1, dtype=np.int32), "nearest": np.full((nf, cap), -1, dtype=np.int32),
           "spacing": np.full((nf, cap), np.inf), "density": np.zeros((nf, cap)),
           "movers": np.zeros((nf, cap), dtype=np.int32), "variance": np.zeros((nf, cap)),
           "pressure": np.zeros((nf, cap)), "crowded": np.zeros((nf, 2), dtype=np.int32),
           "peaks": np.tile(np.array([0.0, 0.0, np.inf]), (nf, 1)), "cell_peak": None, "cell_crowded": None,
           "valid": np.zeros((nf, cap), dtype=bool)}
    if grid is not None:
        x0, y0, g, nx, ny = grid
        xe, ye = arange_edges(x0, g, nx), arange_edges(y0, g, ny)
        out["cell_peak"] = np.zeros((nx, ny, 2)) if cells is None else cells[0].copy()
        out["cell_crowded"] = np.zeros((nx, ny), dtype=np.int32) if cells is None else cells[1].copy()
    for f in range(nf):
        t = first + f
        n = K[t]
        rows, valid = frame_spec(people[t, :n], prev[t, :n], velocity[t, :n], radius)
        for name in ROWS:
            out[name][f, :n] = rows[name]
        out["valid"][f, :n] = valid
        for j in np.flatnonzero(valid):
            d, p, s = rows["density"][j], rows["pressure"][j], rows["spacing"][j]
            out["crowded"][f, 0] += d >= density_limit
            out["crowded"][f, 1] += p >= pressure_limit  # a NaN: False
            if d > out["peaks"][f, 0]:
                out["peaks"][f, 0] = d
            if p > out["peaks"][f, 1]:
                out["peaks"][f, 1] = p
            if s < out["peaks"][f, 2]:
                out["peaks"][f, 2] = s
            if grid is not None:
                bx, by = bin_right(xe, people[t, j, 0]), bin_right(ye, people[t, j, 1])
                if bx < 0 or by < 0:
                    continue
                if d > out["cell_peak"][bx, by, 0]:
                    out["cell_peak"][bx, by, 0] = d
                if p > out["cell_peak"][bx, by, 1]:
                    out["cell_peak"][bx, by, 1] = p
                out["cell_crowded"][bx, by] += d >= density_limit
    return out


def risk_level(density):
    """CrowdDensityModel.calculate_risk_level's classes as an index into RISK."""
    return 0 if density < 1.0 else (1 if density < 2.5 else (2 if density < 4.0 else 3))


def risk_levels(spec):
    """(T, 4) int64: the valid rows of each frame in the four classes of their density."""
    out = np.zeros((len(spec["valid"]), 4), dtype=np.int64)
    for f, valid in enumerate(spec["valid"]):
        for d in spec["density"][f][valid]:
            out[f, risk_level(d)] += 1
    return out


def totals(spec):
    """crowded_total (2,) int64 and peak_total (3,) over the frames of a specification."""
    p = spec["peaks"]
    return spec["crowded"].sum(axis=0, dtype=np.int64), np.array(
        [p[:, 0].max(initial=0.0), p[:, 1].max(initial=0.0), p[:, 2].min(initial=np.inf)])


def same_bits(got, want, what=""):
    """Two arrays of one of NAMES' kinds: dtype, shape, integers equal, doubles equal as uint64 apart from where both
    hold a NaN (its payload and sign are free)."""
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {got.shape}"
    if got.dtype == np.float64:
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaNs differ"
        got, want = np.where(np.isnan(got), 0.0, got), np.where(np.isnan(want), 0.0, want)
        got, want = np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(want).view(np.uint64)
    bad = np.argwhere(got != want)
    assert np.array_equal(got, want), f"{what}: {len(bad)} entries differ, first at {bad[:5].tolist()}"


# ------------------------------------------------------------------ scenes
def lattice_frame(side, step=1.0):
    """side x side people on a square lattice of pitch `step`, row-major: (side * side, 2)."""
    a = np.arange(side, dtype=np.float64) * step
    return np.column_stack([np.repeat(a, side), np.tile(a, side)])


def pack(frames, cap=None, junk=777.25):
    """A list of (K_t, 2) arrays -> (people (T, cap, 2), k): junk (a finite constant, and NaN in every other row)
    past K_t."""
    cap = cap or max(1, max(len(f) for f in frames))
    people = np.full((len(frames), cap, 2), junk)
    people[:, ::2, 0] = np.nan
    for t, f in enumerate(frames):
        people[t, :len(f)] = f
    return people, np.array([len(f) for f in frames], dtype=np.int64)


def random_links(rng, T, cap, speed=1.5, linked=0.8):
    """prev (T, cap) int32 (-1 or a row number: only its sign matters here) and velocity (T, cap, 2) on a 2^-6 m/s
    lattice for the linked rows, junk for the others; every row, live or not, holds something."""
    prev = np.where(rng.random((T, cap)) < linked, rng.integers(0, cap, (T, cap)), -1).astype(np.int32)
    velocity = np.round(rng.uniform(-speed, speed, (T, cap, 2)) * 64) / 64
    return prev, velocity
