"""Inputs and numpy references for the people and density-grid kernels of csrc/density_grid.hip.

Everything is generated from seeds; no torch.  The references are numpy itself and oracle/tier_r.py's
restatements (pinned to the reference by tests/test_oracle.py); every comparison is on bit patterns
(``bits``, ``fhex``), so the sign of a zero counts.

People: ``(xyz (n, 3) float64, labels (n,) int64)`` built by hand, labels dense 0..K-1 plus -1 noise,
coordinates ``standard_normal * 2^e`` with e in -20..20 per point, so the order of a sequential sum shows
in its last bits.  Every cluster of 16 members or more is drawn until its numpy mean changes when its
members are summed in reverse order (``reverse_changes``).

Density: people placed inside chosen cells of the grid that calculate_grid_density lays over an extent,
1 to 6 per cell, so the number of occupied cells is exact and the densities are count / g^2.
"""
import json
import os

import numpy as np

from oracle import tier_r

CHUNK = 960                       # people_kernel: points per chunk (kT - 64)
SEAM_N = (1, 63, 64, 65, 959, 960, 961, 1919, 1920, 1921, 2881, 4807)
MANY_K = (255, 256, 257, 513, 1000)
SPECIAL_SIZES = (1, 2, 16, 17, 18, 33)   # the chain's start, the 16-wide blocks and their tail
OCCUPIED = (1, 7, 8, 9, 127, 128, 129, 130, 136, 1000, 8191, 8192, 8193, 8200, 16385)

GOLDEN_NUMPY = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tier_r.json")))["numpy"]


# ---------------------------------------------------------------------------------------------- comparison
def bits(a):
    """The bit patterns of a float64 array (what every comparison is made on)."""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def fhex(v):
    return float(v).hex()


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype == np.float64 and got.shape == want.shape and np.array_equal(bits(got), bits(want))


def first_diff(got, want):
    """A short description of the first differing element, for assertion messages."""
    g, w = bits(got).reshape(-1), bits(want).reshape(-1)
    if g.shape != w.shape:
        return f"shapes {np.shape(got)} / {np.shape(want)}"
    bad = np.flatnonzero(g != w)
    return "equal" if bad.size == 0 else f"{bad.size} differ, first at {bad[0]}: got {int(g[bad[0]]):#018x}, want {int(w[bad[0]]):#018x}"


# ---------------------------------------------------------------------------------------------- people
def coords(rng, n):
    return rng.standard_normal((n, 3)) * 2.0 ** rng.integers(-20, 21, (n, 1))


def people_ref(xyz, labels):
    """numpy's people of a frame, (K, 2) float64: oracle.tier_r.extract_people_positions."""
    return np.asarray(tier_r.extract_people_positions({"points": xyz, "clusters": labels}), dtype=np.float64).reshape(-1, 2)


def reverse_changes(xyz, labels, c):
    """Whether cluster c's numpy mean (x, y) changes in bits when its members are summed in reverse order."""
    m = xyz[labels == c]
    return not np.array_equal(bits(np.mean(m, axis=0)[:2]), bits(np.mean(m[::-1], axis=0)[:2]))


def make_order_sensitive(rng, xyz, labels, keep_x=()):
    """Redraw the coordinates of every cluster of >= 16 members until reverse_changes holds (clusters in keep_x
    keep their x column)."""
    for c in range(int(labels.max()) + 1 if len(labels) else 0):
        idx = np.flatnonzero(labels == c)
        while len(idx) >= 16 and not reverse_changes(xyz, labels, c):
            new = coords(rng, len(idx))
            if c in keep_x:
                new[:, 0] = xyz[idx, 0]
            xyz[idx] = new
    return xyz


def big_clusters(labels):
    return [c for c in range(int(labels.max()) + 1 if len(labels) else 0) if np.count_nonzero(labels == c) >= 16]


def chunks_of(labels, c):
    return frozenset((np.flatnonzero(labels == c) // CHUNK).tolist())


def seam_frame(n):
    """K = 3 (fewer for n < 3), members interleaved by index: every wave and every chunk feeds every cluster."""
    rng = np.random.default_rng(1000 + n)
    labels = np.arange(n, dtype=np.int64) % 3
    if n >= 64:
        labels[np.arange(n) % 7 == 5] = -1
    xyz = coords(rng, n)
    return make_order_sensitive(rng, xyz, labels), labels


def cluster_sizes(rng, n, K, stride):
    """K sizes >= 1 summing to at most n, very unequal; SPECIAL_SIZES first where they fit; sizes of clusters
    c and c + stride differ while points are left to make them so."""
    sizes = np.ones(K, dtype=np.int64)
    special = K >= len(SPECIAL_SIZES) and K - len(SPECIAL_SIZES) + sum(SPECIAL_SIZES) <= n
    if special:
        sizes[:len(SPECIAL_SIZES)] = SPECIAL_SIZES
    noise = min(n - int(sizes.sum()), max(n // 25, K if K > stride else 0))  # noise, and room for the fix-up below
    extra = n - int(sizes.sum()) - noise
    free = np.arange(len(SPECIAL_SIZES) if special else 0, K)
    if extra > 0 and len(free):
        w = rng.pareto(1.2, len(free)) + 0.01
        sizes[free] += rng.multinomial(extra, w / w.sum())
    left = n - int(sizes.sum())
    for c in range(stride, K):
        if sizes[c] == sizes[c - stride] and left > 0:
            sizes[c] += 1
            left -= 1
    return sizes


def place_clusters(rng, n, sizes, stride):
    """labels (n,) with sizes[c] members of cluster c, the rest -1.  With three chunks or more, cluster c keeps out
    of chunk f(c) = (c + c // stride) % nch and has a member in chunk f(c + stride) where that has room, so clusters
    c and c + stride occupy different sets of chunks."""
    labels = np.full(n, -1, dtype=np.int64)
    nch = -(-n // CHUNK)
    chunk = np.arange(n) // CHUNK
    d = (stride + 1) % nch if nch else 0
    banded = nch >= 3 and d != 0
    K = len(sizes)
    forbid = [(c + c // stride) % nch if banded else -1 for c in range(K)]
    placed = np.zeros(K, dtype=np.int64)
    if banded:
        for c in range(K):
            cand = np.flatnonzero((labels == -1) & (chunk == (forbid[c] + d) % nch))
            if len(cand):
                labels[rng.choice(cand)] = c
                placed[c] = 1
    for c in range(K):
        need = int(sizes[c] - placed[c])
        cand = np.flatnonzero((labels == -1) & (chunk != forbid[c]))
        if len(cand) < need:
            cand = np.flatnonzero(labels == -1)
        labels[rng.choice(cand, need, replace=False)] = c
    return labels


def clustered_frame(seed, n, K, stride=256):
    """n points, K clusters of very different sizes scattered over the chunks, the rest noise."""
    rng = np.random.default_rng(seed)
    if K == 0:
        return coords(rng, n), np.full(n, -1, dtype=np.int64)
    assert K <= n
    labels = place_clusters(rng, n, cluster_sizes(rng, n, K, stride), stride)
    return make_order_sensitive(rng, coords(rng, n), labels), labels


def many_frame(K):
    return clustered_frame(2000 + K, 5000, K)


def placement_frame():
    """Four chunks, the last partial (n = 3 380).  Cluster 0 owns all of chunk 1; cluster 1 is the last point of
    chunk 0 and the first of chunk 2; cluster 2 begins in the last chunk; cluster 3 lives in one wave's 64-point
    slot (wave 5 of chunk 0); cluster 4 is scattered over the rest; what remains is noise."""
    rng = np.random.default_rng(31)
    n = 3 * CHUNK + 500
    labels = np.full(n, -1, dtype=np.int64)
    labels[CHUNK:2 * CHUNK] = 0
    labels[[CHUNK - 1, 2 * CHUNK]] = 1
    labels[3 * CHUNK + 100 + rng.choice(400, 40, replace=False)] = 2
    labels[256 + rng.choice(64, 30, replace=False)] = 3
    rest = np.flatnonzero(labels == -1)
    rest = rest[(rest < 256) | (rest >= 320)]
    labels[rng.choice(rest, 700, replace=False)] = 4
    return make_order_sensitive(rng, coords(rng, n), labels), labels


ZERO_CLUSTERS = {0: "x all -0.0", 1: "the single member (-0.0, -0.0, 1.0)", 2: "x -0.0 then +0.0"}


def zeros_frame():
    """Cluster 0: x all -0.0, y ordinary (20 members); cluster 1: the single member (-0.0, -0.0, 1.0); cluster 2: x
    -0.0 then +0.0; cluster 3: ordinary; noise between them."""
    rng = np.random.default_rng(32)
    n = 300
    labels = np.full(n, -1, dtype=np.int64)
    labels[10:250:12] = 0
    labels[77] = 1
    labels[[5, 260]] = 2
    labels[np.arange(3, 290, 7)] = np.where(labels[np.arange(3, 290, 7)] == -1, 3, labels[np.arange(3, 290, 7)])
    xyz = coords(rng, n)
    xyz[labels == 0, 0] = -0.0
    xyz[77] = (-0.0, -0.0, 1.0)
    xyz[5, 0], xyz[260, 0] = -0.0, 0.0
    return make_order_sensitive(rng, xyz, labels, keep_x=(0,)), labels


def nobody_frame(n):
    return coords(np.random.default_rng(33 + n), n), np.full(n, -1, dtype=np.int64)


def people_cases():
    """name -> builder of (xyz, labels), every single-frame people case."""
    cases = {f"seam_n{n}": (lambda n=n: seam_frame(n)) for n in SEAM_N}
    cases.update({f"many_k{K}": (lambda K=K: many_frame(K)) for K in MANY_K})
    cases.update(placement=placement_frame, zeros=zeros_frame)
    cases.update({f"nobody_n{n}": (lambda n=n: nobody_frame(n)) for n in (1, 2000)})
    return cases


def batch_frames_32():
    """32 frames, sizes from SEAM_N, K from {0, 1, 64, 65, 130} (the largest of them that fits the frame); 64 blocks
    per frame, so K = 65 and 130 give blocks a second and third cluster."""
    ks = (0, 1, 64, 65, 130)
    out = []
    for f in range(32):
        n = SEAM_N[(5 * f + 3) % len(SEAM_N)]
        K = max(k for k in ks if k <= min(n, ks[f % 5]))
        out.append(clustered_frame(4000 + f, n, K, stride=64))
    return out


def batch_frames_3():
    """A failed frame (500 rows of garbage labels >= 0), a frame of K = 300, an ordinary frame."""
    rng = np.random.default_rng(34)
    failed = (coords(rng, 500), rng.integers(0, 500, 500).astype(np.int64))
    return [failed, clustered_frame(4100, 3000, 300), seam_frame(961)], [1.0, 0.0, 0.0]


# ---------------------------------------------------------------------------------------------- density grid
def grid_edges(x_range, y_range, g):
    """calculate_grid_density's np.arange edges."""
    m = g * 2
    return (np.arange(x_range[0] - m, (x_range[1] + m) + g, g), np.arange(y_range[0] - m, (y_range[1] + m) + g, g))


def extent_for(cells, g, start=0.0):
    """A range whose grid has exactly `cells` cells (>= 5: the margin is two cells on either side)."""
    r = (start, start + (cells - 4.5) * g)
    assert len(np.arange(r[0] - 2 * g, (r[1] + 2 * g) + g, g)) - 1 == cells
    return r


def people_in_cells(rng, xe, ye, flat_cells, counts):
    """counts[i] people strictly inside flat cell flat_cells[i] (row-major over (nx, ny)), shuffled."""
    ny = len(ye) - 1
    ci, cj = np.repeat(flat_cells // ny, counts), np.repeat(flat_cells % ny, counts)
    fx, fy = rng.uniform(0.25, 0.75, len(ci)), rng.uniform(0.25, 0.75, len(ci))
    p = np.column_stack([xe[ci] + fx * (xe[ci + 1] - xe[ci]), ye[cj] + fy * (ye[cj + 1] - ye[cj])])
    return np.ascontiguousarray(p[rng.permutation(len(p))])


def analyze_people(people, x_range, y_range, g):
    """oracle.tier_r.analyze over a supplied people array and extent (its body after extract_people_positions) ->
    the pieces the record is compared with."""
    gx, gy, dg = tier_r.calculate_grid_density(people, x_range, y_range, g)
    flat = dg.flatten()
    fx, fy = np.repeat(gx, len(gy)), np.tile(gy, len(gx))
    mx = np.max(flat)
    avg = np.mean(flat[flat > 0]) if np.any(flat > 0) else 0
    thr = max(0.5, avg * 1.5)
    hs = [{"x": fx[i], "y": fy[i], "density": flat[i]} for i in np.where(flat >= thr)[0]]
    hs = sorted(hs, key=lambda h: h["density"], reverse=True)[:5]
    return {"grid_x": gx, "grid_y": gy, "density": dg, "flat_x": fx, "flat_y": fy, "max": mx, "avg": avg, "thr": thr,
            "hotspots": [(fhex(h["x"]), fhex(h["y"]), fhex(h["density"])) for h in hs], "occupied": flat[flat > 0]}


def sequential_sum(a):
    s = 0.0
    for v in a.tolist():
        s += v
    return s


def pairwise_sum(a):
    """numpy's pairwise_sum of a contiguous float64 vector (8-way unrolled leaves of <= 128)."""
    n = len(a)
    if n < 8:
        return sequential_sum(a)
    if n <= 128:
        r = a[:8].tolist()
        i = 8
        while i < n - n % 8:
            for j in range(8):
                r[j] += float(a[i + j])
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for v in a[i:].tolist():
            res += v
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return pairwise_sum(a[:n2]) + pairwise_sum(a[n2:])


def chunked_sum(a):
    """numpy's add.reduce of a contiguous vector: 8192-element buffer chunks, each a pairwise sum, added in order."""
    s = 0.0
    for i in range(0, len(a), 8192):
        s += pairwise_sum(a[i:i + 8192])
    return s


def occupied_case(n_occ, g):
    """(people, x_range, y_range, g) with exactly n_occ occupied cells, 1 to 6 people each, on a grid just large
    enough.  The seed is the first from 5000 + n_occ at which the summation order shows: from 129 cells on a plain
    sequential mean differs from np.mean, above 8192 an unchunked pairwise sum does too."""
    side = max(6, int(np.ceil(np.sqrt(n_occ))) + 1)
    nx = side + (3 if side < 100 else 0)
    xr, yr = extent_for(nx, g, 0.3), extent_for(side, g, -1.1)
    xe, ye = grid_edges(xr, yr, g)
    assert (len(xe) - 1, len(ye) - 1) == (nx, side)
    for seed in range(5000 + n_occ, 5200 + n_occ):
        rng = np.random.default_rng(seed)
        cells = np.sort(rng.choice(nx * side, n_occ, replace=False))
        counts = rng.integers(1, 7, n_occ)
        occ = counts / (g * g)
        if g == 1.0:  # the densities are small integers: every order gives the same sum
            return people_in_cells(rng, xe, ye, cells, counts), xr, yr, g
        if n_occ >= 129 and fhex(sequential_sum(occ) / n_occ) == fhex(np.mean(occ)):
            continue
        if n_occ > 8192 and fhex(pairwise_sum(occ) / n_occ) == fhex(np.mean(occ)):
            continue
        return people_in_cells(rng, xe, ye, cells, counts), xr, yr, g
    raise AssertionError("no seed shows the summation order")


def edge_people(xe, ye):
    """People on the first, an interior and the last edge, one ulp outside either end, and NaN / +-inf, in x with y
    inside and in y with x inside; plus two interior people (so that some cell is occupied)."""
    xin, yin = (xe[2] + xe[3]) / 2, (ye[1] + ye[2]) / 2
    p = [(xin, yin), ((xe[-2] + xe[-1]) / 2, (ye[-2] + ye[-1]) / 2)]
    for e, inside, swap in ((xe, yin, False), (ye, xin, True)):
        for v in (e[0], e[3], e[len(e) // 2], e[-2], e[-1], np.nextafter(e[-1], np.inf), np.nextafter(e[0], -np.inf),
                  np.nan, np.inf, -np.inf):
            p.append((inside, v) if swap else (v, inside))
    p += [(xe[0], ye[0]), (xe[-1], ye[-1]), (xe[3], ye[3]), (np.nan, np.nan), (np.inf, -np.inf)]
    return np.array(p, dtype=np.float64)


def edge_case(g):
    xr, yr = (0.0, 10.0), (0.0, 7.0)
    return edge_people(*grid_edges(xr, yr, g)), xr, yr, g


def far_case(which):
    """Extents where a + i * ((a + g) - a) and naive edges part: one starting at 1e6 + 0.1 with g = 0.1, one at
    -3.2 .. 11.7 with g = 3.7.  People inside seeded cells and on every edge."""
    rng = np.random.default_rng(41)
    xr, yr, g = (((1e6 + 0.1, 1e6 + 0.1 + 3.0), (-0.35, 2.0), 0.1) if which == "far_1e6" else ((-3.2, 11.7), (-3.2, 11.7), 3.7))
    xe, ye = grid_edges(xr, yr, g)
    nx, ny = len(xe) - 1, len(ye) - 1
    n_occ = max(3, nx * ny // 3)
    inside = people_in_cells(rng, xe, ye, np.sort(rng.choice(nx * ny, n_occ, replace=False)), rng.integers(1, 7, n_occ))
    on = np.array([(x, (ye[j] + ye[j + 1]) / 2) for j, x in zip(np.arange(len(xe)) % ny, xe)] +
                  [((xe[i] + xe[i + 1]) / 2, y) for i, y in zip(np.arange(len(ye)) % nx, ye)])
    return np.concatenate([inside, on]), xr, yr, g


def hotspot_case(which):
    """g = 1.0 (densities are the counts) on an 11 x 8 grid, except `below` (g = 3.7: every density under 0.5).
    tie: seven cells at the maximum 6 -> the five lowest flat indices.  five: exactly five cells at or above the
    threshold.  fewer: two.  threshold: counts 3, 1, 2, 2 -> avg 2, thr 3.0 = the largest cell, which is included."""
    rng = np.random.default_rng(42)
    g = 3.7 if which == "below" else 1.0
    xr, yr = extent_for(11, g, 0.5), extent_for(8, g, -2.0)
    xe, ye = grid_edges(xr, yr, g)
    m = 11 * 8
    counts = {"tie": [6] * 7 + [1] * 10, "five": [5, 6, 5, 4, 6] + [1] * 12, "fewer": [6, 5] + [1] * 9,
              "threshold": [3, 1, 2, 2], "below": list(rng.integers(1, 7, 20))}[which]
    cells = rng.choice(m, len(counts), replace=False)
    return people_in_cells(rng, xe, ye, cells, np.array(counts)), xr, yr, g


def density_cases():
    """name -> builder of (people, x_range, y_range, g), every single-frame density case."""
    cases = {f"occ{n}_g{g}": (lambda n=n, g=g: occupied_case(n, g)) for n in OCCUPIED for g in (0.3, 3.7)}
    cases.update({f"occ{n}_g1.0": (lambda n=n: occupied_case(n, 1.0)) for n in (9, 130)})
    cases.update({f"edges_g{g}": (lambda g=g: edge_case(g)) for g in (0.3, 1.0, 3.7)})
    cases.update({w: (lambda w=w: far_case(w)) for w in ("far_1e6", "far_3.7")})
    cases.update({f"hot_{w}": (lambda w=w: hotspot_case(w)) for w in ("tie", "five", "fewer", "threshold", "below")})
    return cases


BATCH_DENSITY = ("occ9_g0.3", "occ130_g3.7", None, "hot_tie", "occ1000_g0.3", "occ8193_g3.7")  # None: a frame of nobody


# ---------------------------------------------------------------------------------------------- cell radius density
CELL_R = 5.0
CELL_K = (0, 1, 255, 256, 257, 600)


def cell_grid():
    """Edges of a 23 x 17-cell grid: 391 cells, no multiple of the kernel's 256-thread block, nx != ny."""
    return np.arange(0.0, 24.0, 1.0), np.arange(0.0, 18.0, 1.0)


def cell_people(k):
    """k people: 3-4-5 offsets from cell centres (distance exactly r = 5, counted) and the same one ulp farther (not
    counted) first, then people all over the grid and a little outside it."""
    rng = np.random.default_rng(50 + k)
    c = np.array([8.5, 7.5])
    # offsets towards larger coordinates: there the person's ulp is at least the difference's, so cx - px is exact
    on = [c + (3, 4), c + (4, 3), c + (5, 0), c + (0, 5)]
    off = [(c[0] + 3, np.nextafter(c[1] + 4, np.inf)), (np.nextafter(c[0] + 4, np.inf), c[1] + 3),
           (np.nextafter(c[0] + 5, np.inf), c[1]), (c[0], np.nextafter(c[1] + 5, np.inf))]
    special = np.array([v for pair in zip(on, off) for v in pair], dtype=np.float64)
    rest = rng.uniform([-3.0, -3.0], [26.0, 20.0], (max(0, k - len(special)), 2))
    return np.ascontiguousarray(np.concatenate([special, rest])[:k].reshape(k, 2))


def cell_radius_ref(people, xg, yg, r, divisor):
    """The brute-force expression of oracle.tier_r.variant_analyze_crowd_density, for any r and divisor."""
    cx, cy = (xg[:-1] + xg[1:]) / 2, (yg[:-1] + yg[1:]) / 2
    dx = cx[None, :, None] - people[None, None, :, 0]
    dy = cy[:, None, None] - people[None, None, :, 1]
    return np.sum(dx * dx + dy * dy <= r * r, axis=2) / divisor


# ---------------------------------------------------------------------------------------------- histogram2d
def hist_cases():
    """name -> (x, y, bins, range): different bin counts per axis both ways round, explicit non-uniform edges,
    samples holding NaN and +-inf, samples on every edge."""
    rng = np.random.default_rng(60)
    n = 5000
    x, y = rng.uniform(-3.0, 9.0, n), rng.normal(2.0, 1.5, n)
    xe = np.concatenate([[-3.5], -3.5 + np.cumsum(rng.uniform(0.05, 4.0, 7))])
    ye = np.concatenate([[-4.0], -4.0 + np.cumsum(rng.exponential(0.25, 50) + 1e-3)])
    bad = np.array([np.nan, np.inf, -np.inf])
    xb, yb = np.concatenate([x[:500], bad, x[:3], bad]), np.concatenate([y[:500], y[:3], bad, bad[::-1]])
    on_x = np.concatenate([np.repeat(xe, len(ye)), np.repeat((xe[:-1] + xe[1:]) / 2, len(ye))])
    on_y = np.concatenate([np.tile(ye, len(xe)), np.tile(ye, len(xe) - 1)])
    return {"bins_7x50": (x, y, (7, 50), None), "bins_50x7": (x, y, (50, 7), None),
            "edges_8x51": (x, y, (xe, ye), None), "edges_51x8": (y, x, (ye, xe), None),
            "nonfinite_edges": (xb, yb, (xe, ye), None),
            "nonfinite_range": (xb, yb, (7, 50), [[-3.0, 9.0], [-2.5, 6.5]]),
            "on_every_edge": (on_x, on_y, (xe, ye), None),
            "on_every_linspace_edge": (np.repeat(np.linspace(-3.0, 9.0, 8), 51), np.tile(np.linspace(-2.5, 6.5, 51), 8),
                                       (7, 50), [[-3.0, 9.0], [-2.5, 6.5]])}
