"""CPU side of the crowding measures: hand cases of the specification (tests/track_crowding_reference.py), its
properties (near is symmetric, any split with accumulate equals the whole, the risk classes cover the valid people),
the conditions on the shared scenes that keep the GPU comparison from passing vacuously, and the argument checks of
lidar_track_crowding_f64 that return before the device is touched (no GPU needed)."""
import ctypes

import numpy as np
import pytest

import track_reference as ref
import track_stream_reference as sref
import track_crowding_reference as cref


def still(people):
    """Nobody linked: prev -1, velocity 0."""
    T, cap, _ = people.shape
    return np.full((T, cap), -1, dtype=np.int32), np.zeros((T, cap, 2))


def one_frame(points, radius, prev=None, velocity=None, **kw):
    people, k = cref.pack([np.asarray(points, dtype=np.float64)])
    p, v = still(people)
    if prev is not None:
        p[0, :len(prev)] = prev
        v[0, :len(velocity)] = velocity
    return cref.crowding_spec(people, k, p, v, radius, **kw)


# ------------------------------------------------------------------ hand cases
def test_triangle_345_and_the_inclusive_edge():
    pts = [(0.0, 0.0), (3.0, 0.0), (0.0, 4.0)]  # sides 3, 4, 5: every square, sum and root exact
    for R, want in ((5.0, [2, 2, 2]), (4.0, [2, 1, 1]), (3.0, [1, 1, 0]), (2.999, [0, 0, 0])):
        s = one_frame(pts, R)
        assert s["neighbours"][0].tolist() == want, R
        assert s["nearest"][0].tolist() == [1, 0, 0] and s["spacing"][0].tolist() == [3.0, 3.0, 4.0]  # whatever R
        area = (np.float64(np.pi) * np.float64(R)) * np.float64(R)
        assert s["density"][0].tolist() == [(n + 1) / area for n in want]
        assert s["movers"][0].tolist() == [0, 0, 0] and not s["variance"].any() and not s["pressure"].any()
        assert s["peaks"][0].tolist() == [(max(want) + 1) / area, 0.0, 3.0]
    assert s["neighbours"].dtype == np.int32 and s["nearest"].dtype == np.int32 and s["spacing"].dtype == np.float64


def test_lattice_ties_take_the_lowest_index():
    pts = cref.lattice_frame(2)  # (0,0) (0,1) (1,0) (1,1)
    s = one_frame(pts, 1.0)
    assert s["nearest"][0].tolist() == [1, 0, 0, 1] and s["spacing"][0].tolist() == [1.0] * 4
    assert s["neighbours"][0].tolist() == [2, 2, 2, 2]
    s = one_frame(pts, np.sqrt(2.0))  # fp64 sqrt(2) squared is above 2: the diagonal is inside
    assert np.float64(np.sqrt(2.0)) * np.float64(np.sqrt(2.0)) > 2.0 and s["neighbours"][0].tolist() == [3, 3, 3, 3]
    s = one_frame(pts, np.nextafter(np.sqrt(2.0), 0.0))
    assert s["neighbours"][0].tolist() == [2, 2, 2, 2]


def test_coincident_people_are_neighbours_at_distance_zero():
    s = one_frame([(1.0, 1.0), (1.0, 1.0), (5.0, 1.0)], 0.5)
    assert s["neighbours"][0].tolist() == [1, 1, 0] and s["nearest"][0].tolist() == [1, 0, 0]
    assert s["spacing"][0].tolist() == [0.0, 0.0, 4.0] and s["peaks"][0, 2] == 0.0


def test_movers_and_the_variance():
    pts = [(0.0, 0.0), (0.5, 0.0), (0.0, 0.5)]
    v = 0.75
    # one mover: no variance
    s = one_frame(pts, 1.0, [0, -1, -1], [(v, 0.0), (9.0, 9.0), (9.0, 9.0)])
    assert s["movers"][0].tolist() == [1, 1, 1] and not s["variance"].any()
    # two movers with opposite velocities: mean 0, variance v^2, pressure density * v^2
    s = one_frame(pts, 1.0, [0, 2, -1], [(v, 0.0), (-v, 0.0), (9.0, 9.0)])
    assert s["movers"][0].tolist() == [2, 2, 2] and s["variance"][0].tolist() == [v * v] * 3
    area = (np.float64(np.pi) * 1.0) * 1.0
    assert s["pressure"][0].tolist() == [(3.0 / area) * (v * v)] * 3 and s["peaks"][0, 1] == (3.0 / area) * (v * v)
    assert s["crowded"][0].tolist() == [0, 3]  # 0.95 per m^2 < 4; 0.54 1/s^2 >= 0.02
    # a row that is not moving itself still sees its neighbours' velocities; a far row sees only itself
    s = one_frame(pts + [(9.0, 9.0)], 1.0, [0, 2, -1, 5], [(v, 0.0), (-v, 0.0), (9.0, 9.0), (1.0, 1.0)])
    assert s["movers"][0].tolist() == [2, 2, 2, 1] and s["variance"][0].tolist() == [v * v] * 3 + [0.0]
    # a non-finite velocity does not move
    s = one_frame(pts, 1.0, [0, 2, 1], [(v, 0.0), (-v, np.inf), (np.nan, 0.0)])
    assert s["movers"][0].tolist() == [1, 1, 1] and not s["variance"].any()


def test_a_variance_that_rounds_below_zero_is_stored_as_plus_zero():
    vx, vy = np.float64(0.7), np.float64(0.1)
    sx = sy = sq = np.float64(0.0)
    for _ in range(5):
        sx, sy, sq = sx + vx, sy + vy, sq + ((vx * vx) + (vy * vy))
    mx, my = sx / 5.0, sy / 5.0
    assert (sq / 5.0) - ((mx * mx) + (my * my)) < 0.0  # five equal velocities: the raw value is a negative rounding error
    pts = [(0.125 * i, 0.0) for i in range(5)]
    s = one_frame(pts, 1.0, [0] * 5, [(vx, vy)] * 5)
    assert s["movers"][0].tolist() == [5] * 5
    assert s["variance"][0].tobytes() == np.zeros(5).tobytes() and s["pressure"][0].tobytes() == np.zeros(5).tobytes()


def test_rows_that_are_not_valid_and_rows_past_k():
    people, k = cref.pack([np.array([(0.0, 0.0), (np.nan, 0.0), (0.5, 0.0), (0.0, np.inf), (1e200, 0.0), (-1e200, 0.0)])],
                          cap=9)
    prev = np.zeros((1, 9), dtype=np.int32)
    vel = np.ones((1, 9, 2))
    s = cref.crowding_spec(people, k, prev, vel, 1.0)
    assert s["valid"][0].tolist() == [True, False, True, False, True, True, False, False, False]
    assert s["neighbours"][0].tolist() == [1, 0, 1, 0, 0, 0, -1, -1, -1]
    # from the two far rows d overflows to inf against every other row: valid, but without a nearest
    assert s["nearest"][0].tolist() == [2, -1, 0, -1, -1, -1, -1, -1, -1]
    assert s["spacing"][0].tolist() == [0.5, np.inf, 0.5] + [np.inf] * 6
    assert s["movers"][0].tolist() == [2, 0, 2, 0, 1, 1, 0, 0, 0]
    assert s["density"][0, 1] == 0.0 and s["density"][0, 6] == 0.0 and s["density"][0, 4] > 0.0
    # k above cap and below 0
    s = cref.crowding_spec(people, [99], prev, vel, 1.0)
    assert (s["neighbours"][0] >= 0).all()
    s = cref.crowding_spec(people, [-3], prev, vel, 1.0)
    assert (s["neighbours"][0] == -1).all() and s["peaks"][0].tolist() == [0.0, 0.0, np.inf]
    assert s["crowded"][0].tolist() == [0, 0]


def test_limits_of_zero_and_infinity():
    pts = cref.lattice_frame(3, 0.5)
    s = one_frame(pts, 1.0, density_limit=0.0, pressure_limit=0.0)
    assert s["crowded"][0].tolist() == [9, 9]  # 0.0 >= 0.0
    s = one_frame(pts, 1.0, density_limit=np.inf, pressure_limit=np.inf)
    assert s["crowded"][0].tolist() == [0, 0]


def test_cells_edges_and_outside():
    # the grid of the extent (0, 2) x (0, 1) at 1 m: x0 = y0 = -2, 6 x 5 cells; its outer edges are at -2 and 4 / 3
    x0, y0, nx, ny, _, _ = ref.venue_grid((0.0, 2.0), (0.0, 1.0), 1.0)
    assert (x0, y0, nx, ny) == (-2.0, -2.0, 6, 5)
    pts = [(-2.0, -2.0), (4.0, 3.0), (4.0, 0.5), (4.0000001, -1.5), (-2.0000001, 0.0), (0.5, 0.5), (0.6, 0.5), (0.0, 3.5)]
    s = one_frame(pts, 1.0, grid=(x0, y0, 1.0, nx, ny), density_limit=0.5)
    area = (np.float64(np.pi) * 1.0) * 1.0
    assert s["cell_crowded"].sum() == 2 and s["cell_crowded"][2, 2] == 2  # the pair at (0.5, 0.5): 2 / pi >= 0.5
    assert s["cell_peak"][0, 0, 0] == 1.0 / area and s["cell_peak"][5, 4, 0] == 1.0 / area  # the closed last edge
    assert s["cell_peak"][5, 2, 0] == 1.0 / area and np.count_nonzero(s["cell_peak"][:, :, 0]) == 4
    assert s["crowded"][0, 0] == 2 and s["cell_peak"].shape == (6, 5, 2) and s["cell_crowded"].dtype == np.int32


# ------------------------------------------------------------------ properties on the shared scenes
def scene(case=sref.GAPPY[1], gate=0.5, max_gap=2):
    people, k = sref.gappy_sequence(*case)
    s = sref.gappy_spec(*case, gate, max_gap)
    return people, k, s["prev"], s["velocity"]


def test_near_is_symmetric_and_neighbours_sum_to_an_even_number():
    people, k, prev, vel = scene()
    K = ref.clamp_k(k, people.shape[1])
    for R in (0.25, 1.0, np.sqrt(2.0)):
        s = cref.crowding_spec(people, k, prev, vel, R)
        for t in range(len(K)):
            near = cref.near_matrix(people[t, :K[t]], R)
            assert np.array_equal(near, near.T)
            assert s["neighbours"][t, :K[t]].sum() % 2 == 0
            assert np.array_equal(s["neighbours"][t, :K[t]], near.sum(axis=0))
    # the scene is not vacuous: ties for the nearest, pairs exactly at the radius, movers and a variance
    s = cref.crowding_spec(people, k, prev, vel, 1.0)
    P = people[1, :K[1]]
    D = cref.pair_d(P)
    assert (D == 1.0).sum() > 10 and (s["movers"] >= 2).sum() > 100 and (s["variance"] > 0).sum() > 100
    np.fill_diagonal(D, np.inf)
    assert ((D == D.min(axis=0)).sum(axis=0) > 1).sum() >= 10  # rows with several nearest: the tie rule decides
    assert (s["crowded"][1:, 1] > 0).all() and (s["peaks"][:, 2] < 1.0).all()
    dense = cref.crowding_spec(people, k, prev, vel, 1.0, 2.0)["crowded"][:, 0]  # the default, 4 per m^2, is never met
    assert not s["crowded"][:, 0].any() and (dense > 0).all() and (dense < K).all()


def test_any_split_with_accumulate_equals_the_whole():
    people, k, prev, vel = scene(sref.GAPPY[0])
    T = len(k)
    xr, yr = ref.extent_of(people, k)
    x0, y0, nx, ny, _, _ = ref.venue_grid(xr, yr, 1.0)
    grid = (x0, y0, 1.0, nx, ny)
    whole = cref.crowding_spec(people, k, prev, vel, 1.0, 2.0, 0.02, grid)
    assert whole["cell_crowded"].sum() > 0 and np.count_nonzero(whole["cell_peak"][:, :, 1]) > 3
    for cut in range(T + 1):
        a = cref.crowding_spec(people[:cut], k[:cut], prev[:cut], vel[:cut], 1.0, 2.0, 0.02, grid)
        b = cref.crowding_spec(people, k, prev, vel, 1.0, 2.0, 0.02, grid, first=cut,
                               cells=(a["cell_peak"], a["cell_crowded"]))
        for name in cref.NAMES[:9]:
            cref.same_bits(np.concatenate([a[name], b[name]]), whole[name], f"cut {cut} {name}")
        cref.same_bits(b["cell_peak"], whole["cell_peak"], f"cut {cut} cell_peak")
        cref.same_bits(b["cell_crowded"], whole["cell_crowded"], f"cut {cut} cell_crowded")


def test_risk_levels_rows_sum_to_the_valid_counts():
    people, k, prev, vel = scene(sref.GAPPY[0])
    people = people.copy()
    people[2, 1] = np.nan
    s = cref.crowding_spec(people, k, prev, vel, 0.5)
    risk = cref.risk_levels(s)
    assert risk.shape == (len(k), 4) and risk.dtype == np.int64
    assert np.array_equal(risk.sum(axis=1), s["valid"].sum(axis=1))
    assert s["valid"][2].sum() == ref.clamp_k(k, people.shape[1])[2] - 1
    assert np.count_nonzero(risk.sum(axis=0)) >= 3  # the classes are populated
    # the classes are CrowdDensityModel.calculate_risk_level's
    from lidar_ai_recommendation_software_amd.crowd_density_model import CrowdDensityModel
    from lidar_ai_recommendation_software_amd.crowd_flow_model import CrowdFlowModel
    level = CrowdDensityModel().calculate_risk_level
    assert CrowdFlowModel.RISK_LEVELS == cref.RISK
    for d in (0.0, 0.99, 1.0, 2.49, 2.5, 3.99, 4.0, 1e9):
        assert cref.RISK[cref.risk_level(d)] == level(d)


# ------------------------------------------------------------------ the package, before the device is touched
def test_layout_and_names():
    torch = pytest.importorskip("torch")
    from lidar_ai_recommendation_software_amd import people_tracking as pt
    assert pt.CROWDING == cref.NAMES
    rows = pt.crowding_layout(5, 43, (0.0, 0.0, 6, 4))
    assert [n for n, _, _ in rows] == list(cref.NAMES)
    assert [s for _, _, s in rows] == [(5, 43)] * 7 + [(5, 2), (5, 3), (6, 4, 2), (6, 4)]
    assert [np.dtype(str(d).split(".")[1]) for _, d, _ in rows] == [np.dtype(d) for d in cref.DTYPES]
    assert [s for _, _, s in pt.crowding_layout(5, 43, None)[9:]] == [None, None]
    t = pt.PeopleTracker(0.1, 0.3, crowding=1.0)
    assert t.crowding == (1.0, (4.0, 0.02)) and t.last_crowding is None and t.crowded_total is None
    assert [n for n, _, _ in t.layout(2)][-9:] == list(cref.NAMES[:9])
    t = pt.PeopleTracker(0.1, 0.3, crowding={"radius": 0.5, "pressure_limit": np.inf})
    assert t.crowding == (0.5, (4.0, np.inf))
    plain = pt.PeopleTracker(0.1, 0.3)
    assert plain.crowding is None and not set(cref.NAMES) & {n for n, _, _ in plain.layout(2)}
    for bad in (0.0, -1.0, np.inf, {"density_limit": 1.0}, {"radius": 1.0, "limit": 2.0},
                {"radius": 1.0, "density_limit": -1.0}, {"radius": 1.0, "pressure_limit": np.nan}):
        with pytest.raises(ValueError, match="^PeopleTracker"):
            pt.PeopleTracker(0.1, 0.3, crowding=bad)
    with pytest.raises(ValueError, match="^track_crowding"):
        pt.track_crowding(np.zeros((1, 4, 2)), np.zeros(1, dtype=np.int64), np.zeros((1, 4), dtype=np.int32),
                          np.zeros((1, 4, 2)), 1.0)
    assert torch.float64 == rows[2][1]


def test_entry_point_rejects_bad_arguments_before_any_launch():
    from lidar_ai_recommendation_software_amd import _native as nat
    lib = nat.load_library()
    n = None
    assert lib.lidar_track_crowding_f64(n, n, n, n, n, 1, 1, 0, 1.0, 4.0, 0.02, 0.0, 0.0, 1.0, 0, 0, 0, n, n, n, n, n, n,
                                        n, n, n, n, n, n) == -1
    assert lib.lidar_last_error().startswith(b"lidar_track_crowding_f64: null pointer")
    # the checks come before the handle is touched: a call that passed them would crash on this dummy handle
    p = ctypes.c_void_p(64)
    T, cap = 7, 43
    outs = ("neighbours", "nearest", "spacing", "density", "movers", "variance", "pressure", "crowded", "peaks")

    def call(frames=T, c=cap, first=T, radius=1.0, dlim=4.0, plim=0.02, x0=0.0, y0=0.0, g=1.0, nx=3, ny=4, acc=0, h=p,
             people=p, k=p, prev=p, velocity=p, cell_peak=p, cell_crowded=p, **out):
        return lib.lidar_track_crowding_f64(h, people, k, prev, velocity, frames, c, first, radius, dlim, plim, x0, y0, g,
                                            nx, ny, acc, *(out.get(name, p) for name in outs), cell_peak, cell_crowded, n)

    inf, nan = float("inf"), float("nan")
    for kw in ([dict(h=n), dict(people=n), dict(k=n), dict(prev=n), dict(velocity=n)] + [{name: n} for name in outs] + [
            dict(frames=-1), dict(frames=65536), dict(c=0), dict(frames=65535, first=65535, c=1 << 16), dict(first=-1),
            dict(first=T + 1), dict(radius=0.0), dict(radius=-1.0), dict(radius=inf), dict(radius=nan), dict(dlim=-1.0),
            dict(dlim=nan), dict(plim=-0.5), dict(plim=nan), dict(acc=2), dict(acc=-1), dict(nx=-1), dict(ny=0),
            dict(g=0.0), dict(g=inf), dict(x0=nan), dict(y0=inf), dict(nx=1 << 16, ny=1 << 15), dict(cell_peak=n),
            dict(cell_crowded=n)]):
        assert call(**kw) == -1, kw
        assert lib.lidar_last_error().startswith(b"lidar_track_crowding_f64: "), kw
    assert call(first=T + 1) == -1 and lib.lidar_last_error().startswith(b"lidar_track_crowding_f64: first")
    assert call(radius=nan) == -1 and lib.lidar_last_error().startswith(b"lidar_track_crowding_f64: radius")
    # nothing to do, whatever the handle: first == frames; +inf limits are allowed; nx == 0: the grid is not looked at
    assert call() == 0 and call(frames=0, first=0) == 0 and call(dlim=inf, plim=inf) == 0 and call(acc=1) == 0
    assert call(nx=0, ny=0, g=nan, x0=nan, cell_peak=n, cell_crowded=n) == 0
