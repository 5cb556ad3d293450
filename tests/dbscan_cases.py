"""Structured DBSCAN scenes and an independent reference (plain numpy, no GPU, no oracle).

``csrc/dbscan.hip`` is exact only because a handful of tight geometric arguments hold (DESIGN.md §2 names
them).  Random continuous frames never sit on those arguments' edges, so every scene here is built to: pairs
one part in 2^30 either side of eps across each of the 62 cell offsets, lattices whose neighbour distance is
eps itself or one rounding from it, pairs on which a fused multiply-add flips the eps test, a border point
between two clusters, long union chains, a frame of isolated points, frames on the edge of the cell cap, and
the degenerate boxes.

``dbscan_brute`` is the reference: all pairs in float64.  ``grid_kind`` / ``grid_shape`` restate the grid
choice of ``dbscan_setup_kernel`` and serve only to show that a scene lands on the path it is built for
(tests/test_dbscan_cases_cpu.py); a GPU result is judged by the reference alone.

A scene is ``(x float64 (n, 3), eps, min_samples)``; ``SCENES`` maps stable names to builders, and
``scene(name)`` builds one, cached and read-only.
"""
import functools
import itertools
from fractions import Fraction

import numpy as np

BRUTE_MAX = 4096  # dbscan_brute is O(n^2)


def fine_side(eps):
    """The fine cell side s = eps / sqrt(3) * (1 - 2^-20), as dbscan_setup_kernel computes it."""
    return eps / np.sqrt(3.0) * (1.0 - 1.0 / 1048576.0)


# ------------------------------------------------------------------ reference
def dbscan_brute(x, eps, min_samples):
    """sklearn's DBSCAN(eps, min_samples) in its order-independent form -> (labels int64, counts int32).

    neighbours: ((dx*dx + dy*dy) + dz*dz) <= eps*eps in float64, one numpy operation per arithmetic
    operation (nothing can be contracted); counts include the point itself; core: count >= min_samples; core
    labels: the components of the core-core graph numbered by ascending minimum core index; a border point
    takes the smallest label among its adjacent cores; every other point -1."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    n = len(x)
    assert x.shape == (n, 3) and n <= BRUTE_MAX
    eps2 = np.float64(eps) * np.float64(eps)
    adj = np.empty((n, n), dtype=bool)
    for r0 in range(0, n, 512):  # row blocks: the float64 temporaries stay small
        a = x[r0:r0 + 512]
        dx = a[:, None, 0] - x[None, :, 0]
        dy = a[:, None, 1] - x[None, :, 1]
        dz = a[:, None, 2] - x[None, :, 2]
        xx = dx * dx
        yy = dy * dy
        zz = dz * dz
        d = xx + yy
        d = d + zz
        adj[r0:r0 + 512] = d <= eps2
    counts = adj.sum(axis=1).astype(np.int32)
    core = counts >= min_samples
    labels = np.full(n, -1, dtype=np.int64)
    k = 0
    for i in np.flatnonzero(core):  # ascending: a new component starts at its minimum core index
        if labels[i] >= 0:
            continue
        labels[i] = k
        frontier = np.array([i])
        while frontier.size:
            reach = adj[frontier].any(axis=0) & core & (labels < 0)
            labels[reach] = k
            frontier = np.flatnonzero(reach)
        k += 1
    big = np.iinfo(np.int64).max
    for r0 in range(0, n, 512):
        rows = np.arange(r0, min(r0 + 512, n))
        rows = rows[~core[rows]]
        if rows.size:
            best = np.where(adj[rows] & core[None, :], labels[None, :], big).min(axis=1)
            labels[rows] = np.where(best == big, -1, best)
    return labels, counts


# ------------------------------------------------------------------ the grid rule, restated
def grid_shape(x, eps):
    """dbscan_setup_kernel's choice for the points x -> (kind, dims (3,) float64, cell side)."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    lo, hi = x.min(axis=0), x.max(axis=0)
    cap = min(8.0 * n + 64.0, 4194304.0)

    def fits(c):
        with np.errstate(over="ignore"):
            dims = np.floor((hi - lo) / c) + 1.0
            tot = (dims[0] * dims[1]) * dims[2]
        return tot <= cap, dims

    s = fine_side(eps)
    ok, dims = fits(s)
    if ok:
        return "fine", dims, s
    c = eps * (1.0 + 1.0 / 1048576.0)
    for _ in range(256):
        ok, dims = fits(c)
        if ok:
            return "coarse", dims, c
        c *= 1.5
    ok, dims = fits(c)
    if ok:
        return "coarse", dims, c
    return "one_cell", np.ones(3), np.inf


def grid_kind(x, eps):
    """"fine" | "coarse" | "one_cell": the grid dbscan_setup_kernel picks for the points x."""
    return grid_shape(x, eps)[0]


def fine_cell(x, lo, eps):
    """floor((x - lo) / s) per axis: the fine cell of each row of x in a box whose low corner is lo."""
    return np.floor((np.asarray(x, dtype=np.float64) - lo) / fine_side(eps)).astype(np.int64)


# ------------------------------------------------------------------ scenes
# the 62 offsets of [-2, 2]^3 lexicographically after (0, 0, 0)
PAIR_OFFSETS = [o for o in itertools.product(range(-2, 3), repeat=3) if o > (0, 0, 0)]
PAIR_A = (2, 2, 2)
PAIR_CLUMP = 20


def pair_points(o, linked):
    """(pa, pb): the two clump positions of pair(o, linked), in cells A = (2, 2, 2) and B = A + o."""
    eps = 1.0
    s = fine_side(eps)
    o = np.array(o, dtype=np.float64)
    cA = (np.array(PAIR_A, dtype=np.float64) + 0.5) * s
    cB = (np.array(PAIR_A, dtype=np.float64) + o + 0.5) * s
    mid = (cA + cB) / 2
    u = o / np.sqrt((o * o).sum())
    L = eps * (1.0 - 2.0 ** -30) if linked else eps * (1.0 + 2.0 ** -30)
    return mid - u * (L / 2), mid + u * (L / 2)


def pair(o, linked):
    """Two clumps of 20 coincident points, one part in 2^30 inside (linked) or outside eps of one another, in
    the fine cells A and A + o of a 5x5x5 box fixed by two anchor points."""
    eps = 1.0
    s = fine_side(eps)
    pa, pb = pair_points(o, linked)
    top = 5 * s * (1.0 - 2.0 ** -30)
    x = np.concatenate([np.tile(pa, (PAIR_CLUMP, 1)), np.tile(pb, (PAIR_CLUMP, 1)),
                        np.zeros((1, 3)), np.full((1, 3), top)])
    return x, eps, 5


def pair_name(o, linked):
    return "pair_%+d%+d%+d_%s" % (o[0], o[1], o[2], "linked" if linked else "unlinked")


SHIFT = (1e3, -2e2, 7.0)


def lattice(step, eps, min_samples, variant="plain"):
    """The 8x8x8 lattice k * step (the product in float64), k = 0..7 per axis, x slowest.  variant: "plain";
    "shifted": rows permuted (fixed seed) and moved by SHIFT; "far": plain plus two points at -+1e4 eps on the
    main diagonal, which push the frame onto the coarse grid."""
    k = np.arange(8, dtype=np.float64) * np.float64(step)
    x = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3)
    if variant == "shifted":
        x = np.random.default_rng(11).permutation(x) + np.array(SHIFT)
    elif variant == "far":
        x = np.concatenate([x, np.full((1, 3), -1e4 * eps), np.full((1, 3), 1e4 * eps)])
    else:
        assert variant == "plain"
    return x, eps, min_samples


def planar():
    """A 30x30 lattice of step 0.1 in the plane z = 7: a zero-width box axis."""
    k = np.arange(30, dtype=np.float64) * 0.1
    xy = np.stack(np.meshgrid(k, k, indexing="ij"), axis=-1).reshape(-1, 2)
    return np.column_stack([xy, np.full(len(xy), 7.0)]), 0.1, 4


def border_tie(first):
    """Clusters P and Q of six cores each and, last, one border point within eps of cores of both; `first`
    says whose rows come first, that is, which of them is cluster 0: "A" for P, "B" for Q."""
    P = np.array([[-0.5, 0, 0]] * 4 + [[0.0, 0, 0]] * 2)
    Q = np.array([[2.3, 0, 0]] * 4 + [[1.8, 0, 0]] * 2)
    assert first in ("A", "B")
    x = np.concatenate([P, Q] if first == "A" else [Q, P])
    return np.concatenate([x, [[0.9, 0.0, 0.0]]]), 1.0, 6


def chain(n, kind):
    """n points 0.9 apart in a row, rows permuted (fixed seed): one cluster, n - 2 cores of count 3 and the two
    ends as border points of count 2.  "axis": along x (fine grid); "diag": along the main diagonal, whose
    fine grid would need ~ (1.56 n)^3 cells (coarse grid, per-point union)."""
    i = np.arange(n, dtype=np.float64)
    if kind == "axis":
        x = np.column_stack([0.9 * i, np.zeros(n), np.zeros(n)])
    else:
        assert kind == "diag"
        x = np.repeat((i * (0.9 / np.sqrt(3.0)))[:, None], 3, axis=1)
    return np.random.default_rng(n).permutation(x), 1.0, 3


def chain_answer(x):
    """(labels, counts) of a chain scene in closed form: the two ends are the extreme points along x."""
    n = len(x)
    counts = np.full(n, 3, dtype=np.int32)
    counts[[np.argmin(x[:, 0]), np.argmax(x[:, 0])]] = 2
    return np.zeros(n, dtype=np.int64), counts


def isolated(n):
    """n points 3 eps apart with min_samples = 1: every point its own cluster, labels == arange(n)."""
    return np.column_stack([3.0 * np.arange(n, dtype=np.float64), np.zeros(n), np.zeros(n)]), 1.0, 1


def single():
    return np.array([[0.25, -1.5, 3.0]]), 1.0, 1


def four_noise():
    return np.random.default_rng(4).uniform(0.0, 1.0, (4, 3)), 5.0, 5


def duplicates():
    """100 copies of one point: a zero-size box, one cell, the same-cell shortcut."""
    return np.tile(np.array([[1.5, -2.25, 0.125]]), (100, 1)), 0.5, 5


def uniform(eps, min_samples):
    return np.random.default_rng(500).uniform(0.0, 10.0, (500, 3)), eps, min_samples


CAP_EDGE_DIMS = {"at": (12, 9, 8), "over": (12, 9, 9)}  # cap = 8 * 100 + 64 = 864 = 12 * 9 * 8


def cap_edge(side):
    """100 points whose fine grid has exactly the cell cap ("at": 12 x 9 x 8 = 864 cells, fine grid) or
    exceeds it ("over": 12 x 9 x 9 = 972, coarse grid): two anchors fix the box, the other 98 points are a
    7 x 7 x 2 block of a 0.3-step lattice inside it."""
    eps = 1.0
    s = fine_side(eps)
    d = np.array(CAP_EDGE_DIMS[side], dtype=np.float64)
    k7, k2 = np.arange(7, dtype=np.float64) * 0.3, np.arange(2, dtype=np.float64) * 0.3
    block = np.stack(np.meshgrid(k7, k7, k2, indexing="ij"), axis=-1).reshape(-1, 3) + np.array([1.0, 1.0, 1.0])
    x = np.concatenate([np.zeros((1, 3)), block, ((d - 0.5) * s)[None, :]])
    return x, eps, 5


def _fma(a, b, c):
    """fl(a * b + c) with one rounding (exact rational arithmetic, correctly rounded on conversion)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def contracted_forms(d):
    """The squared length of d as the kernel must compute it, then as a compiler could contract it:
    (plain, first add fused, second add fused, both fused)."""
    dx, dy, dz = (float(v) for v in d)
    plain = (dx * dx + dy * dy) + dz * dz
    return plain, _fma(dy, dy, dx * dx) + dz * dz, _fma(dz, dz, dx * dx + dy * dy), _fma(dz, dz, _fma(dy, dy, dx * dx))


CONTRACTION_EPS = 0.37
CONTRACTION_BUCKET = 24  # pairs per (contracted form, side of eps the plain form falls on)


@functools.lru_cache(maxsize=None)
def _contraction_pairs():
    eps = CONTRACTION_EPS
    eps2 = eps * eps
    rng = np.random.default_rng(53)
    have = {(f, side): 0 for f in (1, 2, 3) for side in (True, False)}
    rows = []
    while min(have.values()) < CONTRACTION_BUCKET:
        u = rng.normal(size=3)
        u /= np.sqrt((u * u).sum())
        p = rng.uniform(0.0, 1.0, 3) * np.array([2.0, 2.0, 1.0])
        q = p + u * eps
        v = [t <= eps2 for t in contracted_forms(p - q)]
        hits = [(f, v[0]) for f in (1, 2, 3) if v[f] != v[0]]
        if any(have[h] < CONTRACTION_BUCKET for h in hits):
            for h in hits:
                have[h] += 1
            rows += [p, q]
    x = np.array(rows)
    x.setflags(write=False)
    return x


def contraction(variant="plain"):
    """Pairs (rows 2i, 2i + 1) at distance eps in random directions, kept where fusing a multiply into an add
    changes the verdict of the eps test: for each of the three contracted forms, at least 24 pairs that the
    plain form accepts and the fused one rejects, and 24 the other way round.  The pairs lie among one another,
    so a flipped pair shows in the counts.  "far": plus two distant points (coarse grid)."""
    x, eps = _contraction_pairs(), CONTRACTION_EPS
    if variant == "far":
        x = np.concatenate([x, np.full((1, 3), -1e4 * eps), np.full((1, 3), 1e4 * eps)])
    return x, eps, 5


# (step, eps, min_samples) of the lattice scenes
LATTICES = [(1.0, 1.0, 7), (1.0, 1.0, 6), (0.1, 0.1, 5), (0.3, 0.3, 5), (0.7, 0.7, 5)]
VARIANTS = ("plain", "shifted", "far")
CHAIN_SIZES = (4096, 20000)
ISOLATED_N = 9000


def lattice_name(step, eps, ms, variant):
    return "lattice_%g_ms%d_%s" % (step, ms, variant)


SCENES = {}
for _o in PAIR_OFFSETS:
    for _l in (True, False):
        SCENES[pair_name(_o, _l)] = functools.partial(pair, _o, _l)
for _s, _e, _m in LATTICES:
    for _v in VARIANTS:
        SCENES[lattice_name(_s, _e, _m, _v)] = functools.partial(lattice, _s, _e, _m, _v)
SCENES["planar"] = planar
SCENES["contraction_plain"] = functools.partial(contraction, "plain")
SCENES["contraction_far"] = functools.partial(contraction, "far")
SCENES["border_tie_A"] = functools.partial(border_tie, "A")
SCENES["border_tie_B"] = functools.partial(border_tie, "B")
for _n in CHAIN_SIZES:
    for _k in ("axis", "diag"):
        SCENES["chain_%s_%d" % (_k, _n)] = functools.partial(chain, _n, _k)
SCENES["isolated_%d" % ISOLATED_N] = functools.partial(isolated, ISOLATED_N)
SCENES["single"] = single
SCENES["four_noise"] = four_noise
SCENES["duplicates"] = duplicates
SCENES["uniform_eps0.7_ms1"] = functools.partial(uniform, 0.7, 1)
SCENES["uniform_eps1e-9_ms1"] = functools.partial(uniform, 1e-9, 1)
SCENES["uniform_eps1e6_ms5"] = functools.partial(uniform, 1e6, 5)
SCENES["cap_edge_at"] = functools.partial(cap_edge, "at")
SCENES["cap_edge_over"] = functools.partial(cap_edge, "over")

PAIR_NAMES = [n for n in SCENES if n.startswith("pair_")]
LATTICE_NAMES = [n for n in SCENES if n.startswith("lattice_")] + ["planar", "contraction_plain", "contraction_far"]
CHAIN_NAMES = [n for n in SCENES if n.startswith("chain_")]
CLOSED_FORM = CHAIN_NAMES + ["isolated_%d" % ISOLATED_N]
OTHER_NAMES = [n for n in SCENES if n not in PAIR_NAMES + LATTICE_NAMES + CLOSED_FORM]

# the grid every scene is built to take ("fine" unless listed)
GRID = {n: "fine" for n in SCENES}
GRID.update({n: "coarse" for n in SCENES if n.endswith("_far") or n.startswith("chain_diag")})
GRID.update({"uniform_eps0.7_ms1": "coarse", "uniform_eps1e-9_ms1": "coarse", "cap_edge_over": "coarse"})


@functools.lru_cache(maxsize=None)
def scene(name):
    x, eps, ms = SCENES[name]()
    x = np.ascontiguousarray(x, dtype=np.float64)
    x.setflags(write=False)
    return x, float(eps), int(ms)


@functools.lru_cache(maxsize=None)
def answer(name):
    """(labels, counts) a scene owes: the closed form for the chains and the isolated points, else dbscan_brute."""
    x, eps, ms = scene(name)
    if name.startswith("chain_"):
        out = chain_answer(x)
    elif name.startswith("isolated_"):
        out = np.arange(len(x), dtype=np.int64), np.ones(len(x), dtype=np.int32)
    else:
        out = dbscan_brute(x, eps, ms)
    for a in out:
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------ radius_count and the batched path
def fourfold():
    """2048 points: 512 distinct rows, each four times, shuffled."""
    rng = np.random.default_rng(2048)
    return rng.permutation(np.repeat(rng.uniform(-5.0, 5.0, (512, 3)), 4, axis=0))


# class_people takes one (eps, min_samples) per call: the batch of structured frames is clustered at each of
# the settings its scenes are built for (eps 1 with the chain's, border_tie's and the unit lattice's
# min_samples; eps 0.1 for the float32 0.1-step lattice, whose distances then sit one float32 rounding
# either side of eps)
BATCH_PARAMS = [(1.0, 3), (1.0, 6), (1.0, 7), (0.1, 5)]
BATCH_CLASS = 1


@functools.lru_cache(maxsize=None)
def batch_frames():
    """(xyz (6, N, 3) float32, labels (6, N) int32, names): six scenes stated in float32, each padded to
    N = 1536 rows with points of another class strewn among its own (fixed seed), read-only."""
    k = np.arange(8, dtype=np.float64)
    k01 = (k * 0.1).astype(np.float32)
    grid = lambda v: np.stack(np.meshgrid(v, v, v, indexing="ij"), axis=-1).reshape(-1, 3)
    frames = [("lattice_1", grid(k.astype(np.float32))), ("lattice_0.1_f32", grid(k01)),
              ("border_tie_A", border_tie("A")[0]), ("border_tie_B", border_tie("B")[0]),
              ("chain_axis_1024", chain(1024, "axis")[0]), ("duplicates", duplicates()[0])]
    N = 1536
    rng = np.random.default_rng(6)
    xyz = np.empty((len(frames), N, 3), dtype=np.float32)
    labels = np.empty((len(frames), N), dtype=np.int32)
    for f, (_, pts) in enumerate(frames):
        pts = pts.astype(np.float32)
        assert np.array_equal(pts.astype(np.float64).astype(np.float32), pts)
        where = np.sort(rng.choice(N, len(pts), replace=False))  # the scene keeps its row order
        xyz[f] = rng.uniform(-3.0, 3.0, (N, 3)).astype(np.float32)  # the other classes' points, among the scene's
        labels[f] = rng.choice([0, 2], N)
        xyz[f, where] = pts
        labels[f, where] = BATCH_CLASS
    xyz.setflags(write=False)
    labels.setflags(write=False)
    return xyz, labels, [n for n, _ in frames]


@functools.lru_cache(maxsize=None)
def batch_answer(eps, min_samples):
    """Per frame of batch_frames(): (instance (N,) int32, k, labels and counts of the selected points)."""
    xyz, labels, _ = batch_frames()
    out = []
    for x, l in zip(xyz, labels):
        mask = l == BATCH_CLASS
        lab, cnt = dbscan_brute(x[mask].astype(np.float64), eps, min_samples)
        inst = np.full(len(x), -1, dtype=np.int32)
        inst[mask] = lab
        out.append((inst, int(lab.max()) + 1, lab, cnt))
    return out
