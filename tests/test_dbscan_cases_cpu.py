"""The scenes of tests/dbscan_cases.py are what they claim (CPU only): the brute-force reference, the oracle
and scikit-learn agree on every one, and each scene hits the grid, the cells and the side of eps it is built
for.  tests/test_gpu_dbscan_geometry.py runs the same scenes through the HIP kernels."""
import numpy as np
import pytest

import dbscan_cases as dc
from oracle import tier_r

ALL = list(dc.SCENES)


def parts(name):
    """(x, eps, min_samples, labels, counts, core mask) of a scene and its answer."""
    x, eps, ms = dc.scene(name)
    lab, cnt = dc.answer(name)
    return x, eps, ms, lab, cnt, cnt >= ms


@pytest.mark.parametrize("name", ALL)
def test_reference_oracle_and_sklearn_agree(name):
    x, eps, ms, lab, cnt, _ = parts(name)
    assert lab.dtype == np.int64 and cnt.dtype == np.int32
    olab, ocnt = tier_r.dbscan_labels(x, eps, ms, return_counts=True)
    assert np.array_equal(cnt, ocnt)
    assert np.array_equal(lab, olab)
    if len(x) <= dc.BRUTE_MAX:
        from sklearn.cluster import DBSCAN
        blab, bcnt = dc.dbscan_brute(x, eps, ms)  # also where the answer is a closed form
        assert np.array_equal(blab, lab) and np.array_equal(bcnt, cnt)
        assert np.array_equal(DBSCAN(eps=eps, min_samples=ms).fit(x).labels_, lab)


@pytest.mark.parametrize("name", ALL)
def test_grid_kind(name):
    x, eps, _ = dc.scene(name)
    assert dc.grid_kind(x, eps) == dc.GRID[name]


def test_every_grid_kind_is_taken():
    assert {"fine", "coarse"} <= set(dc.GRID.values())
    assert dc.grid_kind(dc.fourfold(), 1e-300) == "one_cell"  # radius_count's r = 0


def test_pair_scenes_are_the_62_offsets():
    assert len(dc.PAIR_OFFSETS) == 62 and len(set(dc.PAIR_OFFSETS)) == 62 and len(dc.PAIR_NAMES) == 124
    assert sum(max(abs(c) for c in o) == 1 for o in dc.PAIR_OFFSETS) == 13
    assert all(o > (0, 0, 0) and max(abs(c) for c in o) <= 2 for o in dc.PAIR_OFFSETS)
    assert (2, 2, 2) in dc.PAIR_OFFSETS and (0, 0, 1) in dc.PAIR_OFFSETS and (2, -2, -2) in dc.PAIR_OFFSETS


@pytest.mark.parametrize("linked", [True, False], ids=["linked", "unlinked"])
@pytest.mark.parametrize("o", dc.PAIR_OFFSETS, ids=lambda o: "%+d%+d%+d" % o)
def test_pair_targets(o, linked):
    name = dc.pair_name(o, linked)
    x, eps, ms, lab, cnt, core = parts(name)
    assert len(x) == 42 and eps == 1.0 and ms == 5
    kind, dims, _ = dc.grid_shape(x, eps)
    assert kind == "fine" and tuple(dims) == (5.0, 5.0, 5.0)
    lo = x.min(axis=0)
    assert np.array_equal(lo, np.zeros(3))
    pa, pb = dc.pair_points(o, linked)
    n = dc.PAIR_CLUMP
    assert np.array_equal(x[:n], np.tile(pa, (n, 1))) and np.array_equal(x[n:2 * n], np.tile(pb, (n, 1)))
    assert tuple(dc.fine_cell(pa, lo, eps)) == dc.PAIR_A
    assert tuple(dc.fine_cell(pb, lo, eps)) == tuple(a + c for a, c in zip(dc.PAIR_A, o))
    dx, dy, dz = pa - pb
    d2 = (dx * dx + dy * dy) + dz * dz
    assert (d2 <= 1.0) if linked else (d2 > 1.0)
    assert abs(d2 - 1.0) < 2.0 ** -28  # one part in 2^30 of eps: the cell side's 2^-20 window is far wider
    assert core[:2 * n].all() and lab[0] == 0
    assert lab[n] == (0 if linked else 1) and lab.max() == lab[n]


@pytest.mark.parametrize("step,eps,ms", dc.LATTICES)
def test_lattice_targets(step, eps, ms):
    for variant in dc.VARIANTS:
        x, e, m, lab, cnt, core = parts(dc.lattice_name(step, eps, ms, variant))
        assert e == eps and m == ms and len(x) == (514 if variant == "far" else 512)
        assert np.any(core) and np.any(~core)
    x, _, _, lab, cnt, core = parts(dc.lattice_name(step, eps, ms, "plain"))
    assert np.array_equal(x[1], [0.0, 0.0, np.float64(1) * np.float64(step)])
    noise, border, k = int((lab < 0).sum()), int(((lab >= 0) & ~core).sum()), int(lab.max()) + 1
    if step == 1.0:
        # every neighbour distance is eps exactly: the six axis neighbours and the point itself, nothing more
        inner = np.all((x > 0) & (x < 7), axis=1)
        assert np.all(cnt[inner] == 7) and cnt.min() == 4 and k == 1
    elif step == 0.1:
        assert (cnt.min(), cnt.max(), k) == (4, 7, 26)
    else:
        # k * step carries a rounding: a neighbour sits one rounding inside or outside eps, so a count can
        # fall short of the lattice's 4 .. 7 and rounding decides which points are cores
        assert (cnt.min(), cnt.max()) == (1, 7) and cnt.min() < 4 and border >= 1
        assert (k, noise, border) == (13, 232, 104)
    if step == 0.1:
        _, _, _, slab, scnt, _ = parts(dc.lattice_name(step, eps, ms, "shifted"))
        assert (int(slab.max()) + 1, int((slab < 0).sum())) == (18, 304)


def test_far_variant_equals_plain_plus_two_noise_points():
    for step, eps, ms in dc.LATTICES:
        lab, cnt = dc.answer(dc.lattice_name(step, eps, ms, "plain"))
        flab, fcnt = dc.answer(dc.lattice_name(step, eps, ms, "far"))
        assert np.array_equal(flab[:512], lab) and np.array_equal(fcnt[:512], cnt)
        assert np.array_equal(flab[512:], [-1, -1]) and np.array_equal(fcnt[512:], [1, 1])


def test_planar_targets():
    x, eps, ms, lab, cnt, core = parts("planar")
    kind, dims, _ = dc.grid_shape(x, eps)
    assert kind == "fine" and dims[2] == 1.0 and np.all(x[:, 2] == 7.0) and len(x) == 900
    assert (int(lab.max()) + 1, int((lab < 0).sum())) == (39, 559)
    assert np.any((lab >= 0) & ~core)


def test_contraction_targets():
    """Every pair of the contraction scene is decided differently by some fused form of the distance, each
    form flips at least 24 pairs either way, and the reference sides with the plain form."""
    x, eps, ms, lab, cnt, core = parts("contraction_plain")
    eps2 = eps * eps
    n = len(x) // 2
    assert len(x) == 2 * n and n >= 3 * dc.CONTRACTION_BUCKET
    flips = {(f, side): 0 for f in (1, 2, 3) for side in (True, False)}
    for i in range(n):
        v = [t <= eps2 for t in dc.contracted_forms(x[2 * i] - x[2 * i + 1])]
        assert any(v[f] != v[0] for f in (1, 2, 3))
        for f in (1, 2, 3):
            flips[f, v[0]] += v[f] != v[0]
        # the reference's verdict on the pair is the plain form's: one scene with the pair alone
        assert dc.dbscan_brute(x[2 * i:2 * i + 2], eps, 2)[1][0] == (2 if v[0] else 1)
    assert min(flips.values()) >= dc.CONTRACTION_BUCKET
    assert np.any(core) and np.any(~core) and np.any(lab < 0) and np.any((lab >= 0) & ~core)
    fx, _, _, flab, fcnt, _ = parts("contraction_far")
    assert np.array_equal(fx[:-2], x) and np.array_equal(flab[:-2], lab) and np.array_equal(fcnt[:-2], cnt)


@pytest.mark.parametrize("first", ["A", "B"])
def test_border_tie_targets(first):
    x, eps, ms, lab, cnt, core = parts("border_tie_" + first)
    assert len(x) == 13 and ms == 6
    assert cnt[12] == 5 and not core[12] and core[:12].all()
    d = x[:12] - x[12]
    near = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) <= eps * eps
    assert set(lab[:12][near]) == {0, 1}  # adjacent to cores of both clusters
    assert lab[12] == 0
    assert np.array_equal(lab[:12], [0] * 6 + [1] * 6)
    # the cluster that comes first is the one the border point joins
    assert x[0, 0] == (-0.5 if first == "A" else 2.3)


@pytest.mark.parametrize("name", dc.CHAIN_NAMES)
def test_chain_closed_form(name):
    x, eps, ms, lab, cnt, core = parts(name)
    assert (eps, ms) == (1.0, 3)
    assert np.all(lab == 0) and int(core.sum()) == len(x) - 2 and sorted(np.unique(cnt)) == [2, 3]
    assert not np.all(np.diff(x[:, 0]) > 0)  # the rows are permuted
    # neighbours along the chain are within eps, next-but-one are not
    s = x[np.argsort(x[:, 0])]
    d1, d2 = s[1:] - s[:-1], s[2:] - s[:-2]
    assert np.all(((d1[:, 0] * d1[:, 0] + d1[:, 1] * d1[:, 1]) + d1[:, 2] * d1[:, 2]) <= 1.0)
    assert np.all(((d2[:, 0] * d2[:, 0] + d2[:, 1] * d2[:, 1]) + d2[:, 2] * d2[:, 2]) > 1.0)


def test_isolated_closed_form():
    x, eps, ms, lab, cnt, _ = parts("isolated_%d" % dc.ISOLATED_N)
    assert ms == 1 and len(x) == 9000 > 2 * 4096  # more than two scan blocks of roots
    assert np.array_equal(lab, np.arange(len(x))) and np.all(cnt == 1)
    assert np.all(np.diff(x[:, 0]) == 3.0)


def test_small_scene_targets():
    assert len(dc.scene("single")[0]) == 1 and np.array_equal(dc.answer("single")[0], [0])
    assert np.array_equal(dc.answer("four_noise")[0], [-1] * 4) and np.array_equal(dc.answer("four_noise")[1], [4] * 4)
    x, eps, _ = dc.scene("duplicates")
    assert np.all(x == x[0]) and tuple(dc.grid_shape(x, eps)[1]) == (1.0, 1.0, 1.0)
    assert np.all(dc.answer("duplicates")[0] == 0) and np.all(dc.answer("duplicates")[1] == 100)
    assert np.array_equal(dc.answer("uniform_eps1e-9_ms1")[0], np.arange(500))
    x, eps, _ = dc.scene("uniform_eps1e6_ms5")
    assert tuple(dc.grid_shape(x, eps)[1]) == (1.0, 1.0, 1.0)  # one cell, of the fine grid
    assert np.all(dc.answer("uniform_eps1e6_ms5")[0] == 0) and np.all(dc.answer("uniform_eps1e6_ms5")[1] == 500)
    lab, cnt = dc.answer("uniform_eps0.7_ms1")
    assert 1 < lab.max() + 1 < 500 and lab.min() == 0 and cnt.max() > 1


@pytest.mark.parametrize("side", ["at", "over"])
def test_cap_edge_targets(side):
    x, eps, ms, lab, cnt, core = parts("cap_edge_" + side)
    assert len(x) == 100 and 8 * len(x) + 64 == 864
    kind, dims, _ = dc.grid_shape(x, eps)
    fine = np.floor((x.max(axis=0) - x.min(axis=0)) / dc.fine_side(eps)) + 1.0
    assert tuple(fine) == tuple(float(d) for d in dc.CAP_EDGE_DIMS[side])
    assert fine.prod() == (864 if side == "at" else 972)
    assert kind == ("fine" if side == "at" else "coarse")
    assert np.all((x >= x[0]) & (x <= x[-1]))  # the block lies inside the anchors' box
    assert np.array_equal(lab, dc.answer("cap_edge_at")[0]) and lab.max() == 0 and np.array_equal(lab[[0, -1]], [-1, -1])


def test_fourfold_scene():
    from sklearn.neighbors import KDTree
    p = dc.fourfold()
    assert p.shape == (2048, 3) and len(np.unique(p, axis=0)) == 512
    assert np.all(KDTree(p).query_radius(p, r=0.0, count_only=True) == 4)


@pytest.mark.parametrize("eps,ms", dc.BATCH_PARAMS)
def test_batch_frames(eps, ms):
    xyz, labels, names = dc.batch_frames()
    assert xyz.dtype == np.float32 and labels.dtype == np.int32 and xyz.shape == (6, 1536, 3)
    nsel = (labels == dc.BATCH_CLASS).sum(axis=1)
    assert list(nsel) == [512, 512, 13, 13, 1024, 100] and np.all(nsel < xyz.shape[1])
    want = dc.batch_answer(eps, ms)
    for f, (inst, k, lab, cnt) in enumerate(want):
        sel = xyz[f][labels[f] == dc.BATCH_CLASS].astype(np.float64)
        olab, ocnt = tier_r.dbscan_labels(sel, eps, ms, return_counts=True)
        assert np.array_equal(lab, olab) and np.array_equal(cnt, ocnt), names[f]
        assert np.all(inst[labels[f] != dc.BATCH_CLASS] == -1) and k == lab.max() + 1
    by = dict(zip(names, want))
    if (eps, ms) == (1.0, 3):
        assert np.all(by["chain_axis_1024"][2] == 0) and sorted(np.unique(by["chain_axis_1024"][3])) == [2, 3]
    if (eps, ms) == (1.0, 6):
        for n in ("border_tie_A", "border_tie_B"):
            assert by[n][1] == 2 and by[n][2][12] == 0 and by[n][3][12] == 5
    if (eps, ms) == (1.0, 7):
        assert by["lattice_1"][1] == 1 and (by["lattice_1"][2] < 0).sum() == 80
    if (eps, ms) == (0.1, 5):
        # float32(k * 0.1) against the double 0.1: rounding decides the pairs, counts fall below the lattice's 4
        assert by["lattice_0.1_f32"][3].min() < 4 and by["lattice_0.1_f32"][1] > 1
        kinds = {dc.grid_kind(x[l == dc.BATCH_CLASS].astype(np.float64), eps) for x, l in zip(xyz, labels)}
        assert kinds == {"fine", "coarse"}  # grids of both kinds side by side in one call
    assert by["duplicates"][1] == 1
