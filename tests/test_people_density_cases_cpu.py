"""The conditions that keep tests/test_gpu_people_density.py from passing vacuously, checked without a GPU: the
cases built by people_density_cases.py have the structure they claim, and the summation orders the kernels must
reproduce are visible in the references' bits."""
import numpy as np
import pytest

import people_density_cases as pdc
from oracle import tier_r

PEOPLE = pdc.people_cases()
DENSITY = pdc.density_cases()


@pytest.fixture(scope="module")
def frames():
    return {name: build() for name, build in PEOPLE.items()}


def test_labels_are_dense(frames):
    all_frames = list(frames.values()) + pdc.batch_frames_32() + pdc.batch_frames_3()[0][1:]
    for xyz, labels in all_frames:
        assert xyz.dtype == np.float64 and xyz.shape == (len(labels), 3) and labels.dtype == np.int64
        ids = np.unique(labels[labels >= 0])
        assert labels.min(initial=0) >= -1 and np.array_equal(ids, np.arange(len(ids)))


@pytest.mark.parametrize("name", sorted(PEOPLE))
def test_people_member_order_shows(frames, name):
    """Every cluster of 16 members or more: its numpy mean changes when the members are summed in reverse order."""
    xyz, labels = frames[name]
    big = pdc.big_clusters(labels)
    if name.startswith(("seam_n", "many_k")) and len(labels) >= 64 or name in ("placement", "zeros"):
        assert big, "the case has no cluster of 16 members"
    for c in big:
        assert pdc.reverse_changes(xyz, labels, c), f"cluster {c}"


def test_seam_frames(frames):
    for n in pdc.SEAM_N:
        xyz, labels = frames[f"seam_n{n}"]
        assert len(labels) == n and labels.max() == min(n, 3) - 1
        for k in range(-(-n // pdc.CHUNK)):  # every chunk, and every full wave slot of it, feeds every cluster
            part = labels[k * pdc.CHUNK:(k + 1) * pdc.CHUNK]
            for w in range(len(part) // 64):
                assert set(part[64 * w:64 * w + 64].tolist()) >= set(range(3))
            assert n < 3 or set(part.tolist()) >= set(range(min(3, len(part))))


@pytest.mark.parametrize("K", pdc.MANY_K)
def test_many_cluster_frames(frames, K):
    """More clusters than the 256 workgroups: the sizes named in the issue occur, the sizes are very unequal, and
    the cluster a workgroup takes next (c + 256) differs from c in size and in the chunks it occupies."""
    xyz, labels = frames[f"many_k{K}"]
    sizes = np.bincount(labels[labels >= 0], minlength=K)
    assert len(labels) == 5000 and labels.max() == K - 1 and (labels == -1).any()
    assert set(pdc.SPECIAL_SIZES) <= set(sizes.tolist())
    assert sizes.max() >= 20 * np.median(sizes) and sizes.min() == 1
    for c in range(K - 256):
        assert sizes[c] != sizes[c + 256], f"clusters {c} and {c + 256} have {sizes[c]} members each"
        assert pdc.chunks_of(labels, c) != pdc.chunks_of(labels, c + 256), f"clusters {c} and {c + 256} occupy the same chunks"


def test_placement_frame(frames):
    xyz, labels = frames["placement"]
    C = pdc.CHUNK
    assert len(labels) % C != 0 and len(labels) // C == 3
    assert np.array_equal(np.flatnonzero(labels == 0), np.arange(C, 2 * C))
    assert np.flatnonzero(labels == 1).tolist() == [C - 1, 2 * C]
    assert np.flatnonzero(labels == 2).min() >= 3 * C
    slot = np.flatnonzero(labels == 3)
    assert len(slot) >= 16 and slot.min() // 64 == slot.max() // 64 and slot.max() < C
    assert len(pdc.chunks_of(labels, 4)) == 3


def test_zero_clusters_have_clear_sign_bits(frames):
    """numpy's axis-0 mean starts from +0.0: a cluster of -0.0 members has the mean +0.0.  What the kernel has to
    reproduce; skipped under another numpy than the one that wrote the fixtures."""
    xyz, labels = frames["zeros"]
    m0, m1, m2 = (xyz[labels == c] for c in (0, 1, 2))
    assert len(m0) >= 16 and np.signbit(m0[:, 0]).all() and (m0[:, 0] == 0).all() and (m0[:, 1] != 0).all()
    assert bytes(m1) == np.array([[-0.0, -0.0, 1.0]]).tobytes()
    assert np.signbit(m2[:, 0]).tolist() == [True, False] and (m2[:, 0] == 0).all()
    if np.__version__ != pdc.GOLDEN_NUMPY:
        pytest.skip(f"numpy {np.__version__} is not the fixtures' {pdc.GOLDEN_NUMPY}: the sign of an all -0.0 mean is that version's")
    want = pdc.people_ref(xyz, labels)
    assert pdc.bits(want[0, 0]) == 0 and pdc.bits(want[2, 0]) == 0
    assert pdc.bits(want[1]).tolist() == [0, 0]
    for m in (1, 2, 5, 9, 200):
        assert not np.signbit(np.mean(np.full((m, 3), -0.0), axis=0)).any()


def test_nobody_frames(frames):
    for n in (1, 2000):
        xyz, labels = frames[f"nobody_n{n}"]
        assert len(labels) == n and (labels == -1).all() and pdc.people_ref(xyz, labels).shape == (0, 2)


def test_batch_frames():
    frames = pdc.batch_frames_32()
    ks = [int(l.max()) + 1 if len(l) else 0 for _, l in frames]
    assert len(frames) == 32 and set(ks) == {0, 1, 64, 65, 130}
    assert {len(l) for _, l in frames} <= set(pdc.SEAM_N) and len({len(l) for _, l in frames}) >= 8
    three, status = pdc.batch_frames_3()
    assert status == [1.0, 0.0, 0.0] and three[1][1].max() == 299
    assert three[0][1].min() >= 0 and three[0][1].max() < len(three[0][1])  # garbage, but inside the frame's rows


# ---------------------------------------------------------------------------------------------- density
@pytest.fixture(scope="module")
def analyzed():
    out = {}
    for name, build in DENSITY.items():
        people, xr, yr, g = build()
        out[name] = (people, xr, yr, g, pdc.analyze_people(people, xr, yr, g))
    return out


def test_analyze_restatement_is_the_oracles(analyzed):
    """analyze_people against oracle.tier_r.analyze itself, on frames whose clusters are single points (the
    centroid of one point is the point)."""
    for name in ("occ130_g0.3", "hot_tie", "hot_threshold", "far_3.7", "hot_below"):
        people, xr, yr, g, a = analyzed[name]
        pd = {"points": np.column_stack([people, np.zeros(len(people))]), "clusters": np.arange(len(people)),
              "dimensions": {"x_range": xr, "y_range": yr}}
        assert pdc.same(tier_r.extract_people_positions(pd), people)
        want = tier_r.analyze(pd, g)
        assert pdc.same(a["density"], want["density_map"]) and pdc.same(a["flat_x"], want["grid_coordinates"][0])
        assert pdc.same(a["flat_y"], want["grid_coordinates"][1])
        assert (pdc.fhex(a["avg"]), pdc.fhex(a["max"])) == (pdc.fhex(want["avg_density"]), pdc.fhex(want["max_density"]))
        assert a["hotspots"] == [(pdc.fhex(h["x"]), pdc.fhex(h["y"]), pdc.fhex(h["density"])) for h in want["hotspots"]]


@pytest.mark.parametrize("g", [0.3, 1.0, 3.7])
@pytest.mark.parametrize("n_occ", pdc.OCCUPIED)
def test_occupied_cells_are_exact(analyzed, n_occ, g):
    if f"occ{n_occ}_g{g}" not in analyzed:
        return
    people, xr, yr, g, a = analyzed[f"occ{n_occ}_g{g}"]
    assert len(a["occupied"]) == n_occ and a["density"].sum() * (g * g) == pytest.approx(len(people), rel=1e-12)
    counts = np.rint(a["occupied"] * (g * g))
    assert counts.min() >= 1 and counts.max() <= 6
    assert a["density"].size < 1.35 * n_occ + 72  # the grid is just large enough
    if n_occ == 16385:
        assert a["density"].shape == (130, 130)


@pytest.mark.parametrize("name", sorted(n for n in DENSITY if n.startswith("occ") and not n.endswith("g1.0")))
def test_density_summation_order_shows(analyzed, name):
    """From 129 occupied cells on a sequential mean is not np.mean's; above 8192 neither is one pairwise sum over the
    whole vector, while numpy's chunked pairwise sum, restated, is np.mean's at every size."""
    occ = analyzed[name][4]["occupied"]
    n = len(occ)
    want = pdc.fhex(np.mean(occ))
    assert pdc.fhex(pdc.chunked_sum(occ) / n) == want == pdc.fhex(analyzed[name][4]["avg"])
    if n >= 129:
        assert pdc.fhex(pdc.sequential_sum(occ) / n) != want
    if n > 8192:
        assert pdc.fhex(pdc.pairwise_sum(occ) / n) != want


@pytest.mark.parametrize("g", [0.3, 1.0, 3.7])
def test_edge_people(analyzed, g):
    """The edge cases hold what they claim; what numpy makes of them is np.histogram2d's business."""
    people, xr, yr, g, a = analyzed[f"edges_g{g}"]
    xe, ye = pdc.grid_edges(xr, yr, g)
    for col, e in ((0, xe), (1, ye)):
        v = people[:, col]
        for want in (e[0], e[3], e[-1], np.nextafter(e[-1], np.inf), np.nextafter(e[0], -np.inf), np.inf, -np.inf):
            assert (v == want).any()
        assert np.isnan(v).any()
    h = np.histogram2d(people[:, 0], people[:, 1], bins=[xe, ye])[0]
    assert pdc.same(a["density"], h / (g * g)) and 0 < h.sum() < len(people)
    assert h[-1, 1] >= 1 and h[0, 1] >= 1 and h[2, -1] >= 1 and h[2, 0] >= 1  # the closed last edge, the first edge


def test_far_extents_part_from_naive_edges(analyzed):
    for name in ("far_1e6", "far_3.7"):
        people, xr, yr, g, a = analyzed[name]
        xe, _ = pdc.grid_edges(xr, yr, g)
        naive = np.array([xe[0] + g * i for i in range(len(xe))])  # a + i * g, not a + i * ((a + g) - a)
        if name == "far_1e6":  # at -10.6 with g = 3.7 the two agree: that extent is the second g = 3.7 grid, with nx = ny
            assert not np.array_equal(naive, xe), name
        assert (people[:, 0][:, None] == xe[None, :]).any(axis=0).all()  # somebody on every x edge


def test_hotspot_cases(analyzed):
    a = analyzed["hot_tie"][4]
    flat = a["density"].flatten()
    top = np.flatnonzero(flat == a["max"])
    assert len(top) > 5 and a["max"] >= a["thr"]
    assert a["hotspots"] == [(pdc.fhex(a["flat_x"][i]), pdc.fhex(a["flat_y"][i]), pdc.fhex(flat[i])) for i in top[:5]]
    a = analyzed["hot_five"][4]
    assert np.count_nonzero(a["density"] >= a["thr"]) == 5 == len(a["hotspots"])
    assert len({h[2] for h in a["hotspots"]}) > 1  # and they are ordered by density, ties by index
    a = analyzed["hot_fewer"][4]
    assert 0 < np.count_nonzero(a["density"] >= a["thr"]) == len(a["hotspots"]) < 5
    a = analyzed["hot_threshold"][4]
    assert a["thr"] == 1.5 * a["avg"] > 0.5 and np.count_nonzero(a["density"] == a["thr"]) == 1 == len(a["hotspots"])
    a = analyzed["hot_below"][4]
    assert 0 < a["max"] < 0.5 and a["thr"] >= 0.5 and a["hotspots"] == []


# ---------------------------------------------------------------------------------------------- neighbours
def test_cell_radius_people():
    xg, yg = pdc.cell_grid()
    assert (len(xg) - 1, len(yg) - 1) == (23, 17)
    for k in pdc.CELL_K:
        p = pdc.cell_people(k)
        assert p.shape == (k, 2)
    p = pdc.cell_people(600)
    on, off = p[0:8:2], p[1:8:2]
    j, i = 7, 8  # the centre (8.5, 7.5)
    assert pdc.cell_radius_ref(on, xg, yg, pdc.CELL_R, 1.0)[j, i] == 4  # exactly at r: counted
    assert pdc.cell_radius_ref(off, xg, yg, pdc.CELL_R, 1.0)[j, i] == 0  # one ulp farther: not
    pd = {"points": np.column_stack([p, np.zeros(600)]), "clusters": np.arange(600),
          "dimensions": {"x_range": (0.0, 23.0), "y_range": (0.0, 17.0), "width": 23.0, "length": 17.0}}
    assert pdc.same(tier_r.variant_analyze_crowd_density(pd)["density_grid"], pdc.cell_radius_ref(p, xg, yg, 2.0, 4.0))


def test_hist_cases():
    cases = pdc.hist_cases()
    shapes = set()
    for name, (x, y, bins, rng) in cases.items():
        H, xe, ye = np.histogram2d(x, y, bins=bins, range=rng)
        shapes.add(H.shape)
        assert H.shape[0] != H.shape[1] and 0 < H.sum() <= len(x)
        if name.startswith("nonfinite"):
            assert np.isnan(x).any() and np.isinf(x).any() and np.isnan(y).any() and np.isinf(y).any() and H.sum() < len(x)
        if name.startswith("on_every"):
            assert all((x == e).any() for e in xe) and all((y == e).any() for e in ye)
    assert {(7, 50), (50, 7)} <= shapes
    xe, ye = cases["edges_8x51"][2]
    assert len(set(np.diff(xe).round(6))) > 1 and len(set(np.diff(ye).round(6))) > 1
