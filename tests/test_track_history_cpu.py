"""CPU side of the track history: hand cases of the specification (tests/track_history_reference.py), its two
properties (any split equals the whole; the batch form equals the stream form with max_gap = 0), the conditions on the
shared scenes that keep the GPU comparison from passing vacuously, the host construction of track_table, and the
checks of people_tracking.track_history and lidar_track_history_f64 that return before the device is touched (no GPU
needed)."""
import ctypes

import numpy as np
import pytest

import track_reference as ref
import track_stream_reference as sref
import track_events_reference as eref
import track_history_reference as href

ROOM = (0.0, 4.0, 0.0, 4.0)  # x0, x1, y0, y1


def chain(points, cap=2):
    """One track through `points`, a frame each, on row 0 -> (people, k, prev)."""
    T = len(points)
    people = np.full((T, cap, 2), np.nan)
    people[:, 0] = points
    prev = np.full((T, cap), -1, dtype=np.int32)
    prev[1:, 0] = 0
    return people, np.ones(T, dtype=np.int64), prev


def same_state(a, b, frames, what=""):
    """The five state arrays of two specifications over the frame slices `frames` = (of a, of b): integers equal,
    path and origin equal as bytes."""
    for name in href.STATE:
        x, y = a[name], b[name]
        assert (x is None) == (y is None), name
        if x is not None:
            x, y = x[frames[0]], y[frames[1]]
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f"{what} {name}"


# ------------------------------------------------------------------ hand cases
def test_one_walker_with_a_known_path():
    # 3-4-5 steps: every square, sum and root is exact
    pts = [(0.0, 0.0), (3.0, 4.0), (3.0, 4.0), (9.0, 12.0), (9.0, 7.0)]
    h = href.history_spec(*chain(pts), None, None)
    assert h["age"][:, 0].tolist() == [0, 1, 2, 3, 4] and h["hits"][:, 0].tolist() == [1, 2, 3, 4, 5]
    assert h["path"][:, 0].tolist() == [0.0, 5.0, 5.0, 15.0, 20.0]
    assert h["origin"][:, 0].tolist() == [[0.0, 0.0]] * 5
    assert h["stay"] is None and h["dwell"] is None and h["heirs"] == h["linked"] == 4
    # the rows at or past K_t hold the defaults
    assert (h["age"][:, 1] == -1).all() and not h["hits"][:, 1].any() and not h["path"][:, 1].any()
    assert not h["origin"][:, 1].any()
    assert h["age"].dtype == np.int32 and h["hits"].dtype == np.int32 and h["path"].dtype == np.float64


def test_a_link_over_a_gap_adds_its_frames():
    people, k, prev = chain([(1.0, 1.0), (np.nan, np.nan), (1.0, 2.0), (1.0, 3.0)])
    k = np.array([1, 0, 1, 1])
    gap = np.array([0, 0, 2, 1], dtype=np.int32).reshape(4, 1).repeat(2, axis=1)
    h = href.history_spec(people, k, prev, gap, [ROOM])
    assert h["age"][:, 0].tolist() == [0, -1, 2, 3] and h["hits"][:, 0].tolist() == [1, 0, 2, 3]
    assert h["stay"][:, 0, 0].tolist() == [0, -1, 2, 3] and h["path"][:, 0].tolist() == [0.0, 0.0, 1.0, 2.0]
    assert not h["dwell"].any() and h["dwell"].shape == (4, 1, 3) and h["dwell"].dtype == np.int64


def test_stays():
    inside, outside = (1.0, 1.0), (5.0, 1.0)
    # a stay of one detection has length 0
    h = href.history_spec(*chain([outside, inside, outside]), None, [ROOM])
    assert h["stay"][:, 0, 0].tolist() == [-1, 0, -1] and h["dwell"][:, 0].tolist() == [[0, 0, 0], [0, 0, 0], [1, 0, 0]]
    # a birth inside: the stay starts at 0 with the history
    h = href.history_spec(*chain([inside, inside, inside, outside]), None, [ROOM])
    assert h["stay"][:, 0, 0].tolist() == [0, 1, 2, -1] and h["dwell"][3, 0].tolist() == [1, 2, 2]
    # leaving and re-entering: two stays, the second counted from its own first detection
    h = href.history_spec(*chain([inside, inside, outside, inside, inside, inside, inside, outside]), None, [ROOM])
    assert h["stay"][:, 0, 0].tolist() == [0, 1, -1, 0, 1, 2, 3, -1]
    assert h["dwell"][:, 0].sum(axis=0)[:2].tolist() == [2, 4] and h["dwell"][:, 0, 2].max() == 3
    assert h["dwell"][2, 0].tolist() == [1, 1, 1] and h["dwell"][7, 0].tolist() == [1, 3, 3]
    # a history that ends inside (lost, then a new one starts outside) is not a completed stay
    people, k, prev = chain([inside, inside, outside, outside])
    prev[2, 0] = -1
    h = href.history_spec(people, k, prev, None, [ROOM])
    assert h["stay"][:, 0, 0].tolist() == [0, 1, -1, -1] and not h["dwell"].any()
    assert h["age"][:, 0].tolist() == [0, 1, 0, 1]
    # half-open edges, and a NaN is outside: it ends the stay
    h = href.history_spec(*chain([(0.0, 0.0), (4.0, 1.0), (1.0, 1.0), (np.nan, 1.0)]), None, [ROOM])
    assert h["stay"][:, 0, 0].tolist() == [0, -1, 0, -1] and h["dwell"][:, 0, 0].tolist() == [0, 1, 0, 1]


def two_heirs():
    """Rows 0 and 1 of frame 1 both name row 0 of frame 0; row 2 of frame 2 and row 0 of frame 2 both name row 1 of
    frame 1 (the second with gap 1 against the first's 1: same source)."""
    people = np.array([[(0.0, 0.0), (9.0, 9.0), (9.0, 9.0)],
                       [(3.0, 4.0), (0.0, 1.0), (9.0, 9.0)],
                       [(0.0, 2.0), (7.0, 7.0), (0.0, 4.0)]])
    k = np.array([1, 2, 3])
    prev = np.array([[-1, -1, -1], [0, 0, -1], [1, -1, 1]], dtype=np.int32)
    gap = np.array([[0, 0, 0], [1, 1, 0], [1, 0, 1]], dtype=np.int32)
    return people, k, prev, gap


def test_two_rows_naming_one_source():
    people, k, prev, gap = two_heirs()
    h = href.history_spec(people, k, prev, gap, [ROOM])
    assert h["linked"] == 4 and h["heirs"] == 2
    # frame 1: row 0 is the heir, row 1 starts with its own origin
    assert h["age"][1].tolist() == [1, 0, -1] and h["hits"][1].tolist() == [2, 1, 0]
    assert h["path"][1].tolist() == [5.0, 0.0, 0.0] and h["origin"][1].tolist() == [[0.0, 0.0], [0.0, 1.0], [0.0, 0.0]]
    # frame 2: row 0 continues (1, 1), row 2 starts at 0 / 1 / 0.0
    assert h["age"][2].tolist() == [1, 0, 0] and h["hits"][2].tolist() == [2, 1, 1]
    assert h["path"][2].tolist() == [1.0, 0.0, 0.0] and h["origin"][2, 2].tolist() == [0.0, 4.0]
    assert h["stay"][2, :, 0].tolist() == [1, -1, -1]  # (0, 4) is on the open edge


def guard_cases():
    """Links the guard rejects, one per row of frame 3 (cap = 8, K = 6 everywhere but frame 1 with K = 2): -5, cap, a
    row >= K_s, gap 0, gap 9, gap > t; the rows are starts."""
    T, cap = 4, 8
    rng = np.random.default_rng(5)
    people = rng.integers(0, 32, (T, cap, 2)) * ref.STEP
    k = np.array([6, 2, 6, 6])
    prev = np.full((T, cap), -1, dtype=np.int32)
    gap = np.zeros((T, cap), dtype=np.int32)
    prev[3, :6] = [-5, cap, 3, 1, 1, 1]
    gap[3, :6] = [1, 1, 2, 0, 9, 4]
    prev[2, 0], gap[2, 0] = 0, 1  # one good link, so that something continues
    return people, k, prev, gap


def test_links_the_guard_rejects_are_starts():
    people, k, prev, gap = guard_cases()
    h = href.history_spec(people, k, prev, gap, [ROOM])
    assert h["linked"] == 1 and h["heirs"] == 1 and h["age"][2, 0] == 1
    assert h["age"][3, :6].tolist() == [0] * 6 and h["hits"][3, :6].tolist() == [1] * 6 and not h["path"][3].any()
    assert np.array_equal(h["origin"][3, :6], people[3, :6])
    # without gap (the batch form) every link spans one frame: -5 and cap are rejected, row 3 of frame 2 is a source,
    # and the three rows that name row 1 of frame 2 have one heir
    h = href.history_spec(people, k, prev, None, None)
    assert h["linked"] == 5 and h["heirs"] == 3 and h["age"][3, :6].tolist() == [0, 0, 1, 1, 0, 0]


def nan_chain():
    return chain([(0.0, 0.0), (3.0, 4.0), (np.nan, 4.0), (3.0, 4.0), (6.0, 8.0)])


def test_a_nan_coordinate_makes_the_path_nan_from_there_on():
    h = href.history_spec(*nan_chain(), None, [(0.0, 5.0, 0.0, 5.0)])
    p = h["path"][:, 0]
    assert p[:2].tolist() == [0.0, 5.0] and np.isnan(p[2:]).all()
    assert h["age"][:, 0].tolist() == [0, 1, 2, 3, 4] and h["stay"][:, 0, 0].tolist() == [0, 1, -1, 0, -1]


# ------------------------------------------------------------------ the two properties, on the shared scenes
def scenes():
    for case in sref.GAPPY:
        people, k = sref.gappy_sequence(*case)
        zones = eref.scene_tables(eref.lattice_side(case[1]))[1]
        for max_gap in (0, 1, 2):
            yield str(case), people, k, zones, max_gap, sref.gappy_spec(*case, 0.5, max_gap), href.gappy_history(
                *case, 0.5, max_gap)
    people, k, _, zones = eref.crossing_scene()
    for max_gap in (0, 1, 2):
        yield "crossing", people, k, zones, max_gap, eref.crossing_spec(max_gap)[0], href.crossing_history(max_gap)


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_any_split_equals_the_whole(which):
    name = (sref.GAPPY + ["crossing"])[which]
    for what, people, k, zones, max_gap, s, whole in scenes():
        if what != str(name):
            continue
        T = len(k)
        for cut in range(T + 1):
            head, tail, c = href.split_history(people, k, s["prev"], s["gap"], zones, max_gap, cut)
            same_state(head, whole, (slice(None), slice(0, cut)), f"{what} head of cut {cut}")
            same_state(tail, whole, (slice(c, None), slice(cut, None)), f"{what} M {max_gap} cut {cut}")
            same_state(tail, head, (slice(0, c), slice(cut - c, cut)), "the carried frames stay")
            assert np.array_equal(tail["dwell"], whole["dwell"][cut:]) and tail["dwell"].shape[0] == T - cut
            assert np.array_equal(head["dwell"], whole["dwell"][:cut])


def test_batch_links_without_gap_equal_stream_links_with_max_gap_0():
    for case in sref.GAPPY[:2]:
        people, k = sref.gappy_sequence(*case)
        zones = eref.scene_tables(eref.lattice_side(case[1]))[1]
        batch = ref.track_spec(people, k, ref.DT, 0.5)  # track_people's specification: prev, no gap
        s = sref.gappy_spec(*case, 0.5, 0)
        assert np.array_equal(batch["prev"], s["prev"])
        a = href.history_spec(people, k, batch["prev"], None, zones)
        b = href.gappy_history(*case, 0.5, 0)
        same_state(a, b, (slice(None), slice(None)))
        assert np.array_equal(a["dwell"], b["dwell"]) and a["heirs"] == b["heirs"]


def test_scenes_are_not_vacuous():
    for what, people, k, zones, max_gap, s, h in scenes():
        href.not_vacuous(h, k, people.shape[1], max_gap, s["gap"])
        # on tracker links the completed stays are track_events' exits
        ev = eref.events_spec(people, k, s["prev"], s["gap"], None, zones)
        assert np.array_equal(h["dwell"][:, :, 0], ev[1][:, :, 2]), what
        if what == "crossing":
            d = h["dwell"]
            assert d[:, 0, 1].sum() > 0 and d[:, 2, 1].sum() > 0 and 4 <= d[:, :, 2].max() <= 10
            print("crossing", max_gap, "dwell frames", d[:, :, 1].sum(axis=0).tolist(), "max", d[:, :, 2].max(axis=0).tolist())


# ------------------------------------------------------------------ the host side of the package
def test_track_table_from_spec_arrays():
    from lidar_ai_recommendation_software_amd.crowd_flow_model import CrowdFlowModel
    case = sref.GAPPY[1]
    people, k = sref.gappy_sequence(*case)
    T, cap, _ = people.shape
    K = ref.clamp_k(k, cap)
    s, h = sref.gappy_spec(*case, 0.5, 2), href.gappy_history(*case, 0.5, 2)
    for lo in (0, T - 3):  # a whole sequence; the held frames of a stream, numbered from its first frame
        sl, frames = slice(lo, T), np.arange(lo, T)
        args = (s["track_id"][sl], h["age"][sl], h["hits"][sl], h["path"][sl], h["origin"][sl], people[sl], K[sl], frames)
        got, want = CrowdFlowModel.track_table(*args, ref.DT), href.track_table(*args, ref.DT)
        assert list(got) == ["track_id", "first_frame", "last_frame", "hits", "path_length", "displacement", "mean_speed"]
        for key in want:
            assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), key
        n = len(got["track_id"])
        assert all(len(v) == n for v in got.values())
        if lo == 0:
            assert got["track_id"].tolist() == list(range(s["ntracks"]))
            assert got["first_frame"].min() == 0 and got["last_frame"].max() == T - 1
            assert (got["first_frame"] >= 0).all() and (got["displacement"] <= got["path_length"] + 1e-12).all()
            assert np.array_equal(got["mean_speed"] == 0.0, (got["last_frame"] == got["first_frame"]) | (got["path_length"] == 0))
        else:
            assert 0 < n < s["ntracks"] and got["last_frame"].min() >= lo
    one = CrowdFlowModel.track_table(*(np.zeros((0, 1) + t, dtype=d) for t, d in (
        ((), np.int32), ((), np.int32), ((), np.int32), ((), np.float64), ((2,), np.float64), ((2,), np.float64))), [], [], 0.1)
    assert all(len(v) == 0 for v in one.values()) and one["first_frame"].dtype == np.int64


def test_wrapper_checks_before_any_device_call(monkeypatch):
    from lidar_ai_recommendation_software_amd import people_tracking as pt
    from test_track_stream_cpu import host_tensors
    torch = pytest.importorskip("torch")
    with monkeypatch.context() as m:
        # the checks the wrappers share, each through every wrapper that uses it and under that wrapper's name
        people, k, prev, velocity, table = host_tensors(m)
        T, cap = prev.shape
        for name, call in (("flow_cells", lambda p, g: pt.flow_cells(people, k, p, velocity, (0.0, 1.0), (0.0, 1.0))),
                           ("track_events", lambda p, g: pt.track_events(people, k, p, g, zones=table)),
                           ("track_history", lambda p, g: pt.track_history(people, k, p, g))):
            with pytest.raises(ValueError, match=f"^{name}: prev must be"):
                call(prev.long(), None)
            if name != "flow_cells":
                with pytest.raises(ValueError, match=f"^{name}: gap must be"):
                    call(prev, prev[:2].contiguous())
        for bad in (torch.zeros((65, 4), dtype=torch.float64), table.float(), torch.zeros((1, 3), dtype=torch.float64),
                    torch.zeros((0, 4), dtype=torch.float64)):
            for name, call in (("track_events: gates", lambda t: pt.track_events(people, k, prev, gates=t)),
                               ("track_events: zones", lambda t: pt.track_events(people, k, prev, zones=t)),
                               ("track_history: zones", lambda t: pt.track_history(people, k, prev, zones=t))):
                with pytest.raises(ValueError, match=f"^{name} must be \\(n, 4\\) float64 with 1 <= n <= 64, got"):
                    call(bad)
        with pytest.raises(ValueError, match="^track_events: needs gates or zones"):
            pt.track_events(people, k, prev)
        # the caller's arrays against the layout tables
        state = tuple(torch.zeros(shape, dtype=dtype) for _, dtype, shape in pt.state_layout(T, cap))
        with pytest.raises(ValueError, match="^track_stream: carried frames need their state"):
            pt.track_stream(people, k, 0.1, 0.3, 1, carry=1)
        with pytest.raises(ValueError, match=r"^track_stream: state is \(prev, gap, succ, velocity, track_id\)$"):
            pt.track_stream(people, k, 0.1, 0.3, 1, 1, state[:4])
        with pytest.raises(ValueError, match="^track_stream: succ must be"):
            pt.track_stream(people, k, 0.1, 0.3, 1, 1, state[:2] + (state[2].int(),) + state[3:])
        out = tuple(None if shape is None else torch.zeros(shape, dtype=dtype)
                    for _, dtype, shape in pt.event_layout(T, cap, 0, 1))
        assert [t is None for t in out] == [False, False, True, True, False]
        with pytest.raises(ValueError, match=r"^track_events: out is \(gate_counts, zone_counts, gate_fwd, gate_bwd, zone_in\)$"):
            pt.track_events(people, k, prev, zones=table, out=out[:4])
        with pytest.raises(ValueError, match="^track_events: out's gate_fwd must be None without its table"):
            pt.track_events(people, k, prev, zones=table, out=out[:2] + (out[4],) + out[3:])
        with pytest.raises(ValueError, match="^track_events: gate_counts must be"):
            pt.track_events(people, k, prev, zones=table, out=out, first=1)
        hstate = tuple(torch.zeros(shape, dtype=dtype) for _, dtype, shape in pt.history_layout(T, cap, 1))
        assert [name for name, _, _ in pt.history_layout(T, cap, 1)] == ["age", "hits", "path", "origin", "stay"]
        with pytest.raises(ValueError, match="^track_history: carried frames need their state"):
            pt.track_history(people, k, prev, carry=1)
        with pytest.raises(ValueError, match=r"^track_history: state is \(age, hits, path, origin, stay\) with zones$"):
            pt.track_history(people, k, prev, zones=table, state=hstate[:4])
        with pytest.raises(ValueError, match=r"^track_history: state is \(age, hits, path, origin\) without zones$"):
            pt.track_history(people, k, prev, state=hstate)
        with pytest.raises(ValueError, match="^track_history: path must be"):
            pt.track_history(people, k, prev, zones=table, state=hstate[:2] + (hstate[2].float(),) + hstate[3:])
    assert [n for n, _, _ in pt.HISTORY] == ["age", "hits", "path", "origin"]
    assert [(d, t) for _, d, t in pt.HISTORY] == [(torch.int32, ()), (torch.int32, ()), (torch.float64, ()),
                                                  (torch.float64, (2,))]
    with pytest.raises(ValueError, match="^track_history"):
        pt.track_history(np.zeros((1, 4, 2)), np.zeros(1, dtype=np.int64), np.zeros((1, 4), dtype=np.int32))
    t = pt.PeopleTracker(0.1, 0.3, history=True)
    assert t.history and t.last_history is None and t.dwell_total is None and not t.events
    plain = pt.PeopleTracker(0.1, 0.3)
    assert not plain.history and plain.last_history is None and plain.dwell_total is None


def test_entry_point_rejects_bad_arguments_before_any_launch():
    from lidar_ai_recommendation_software_amd import _native as nat
    lib = nat.load_library()
    n = None
    assert lib.lidar_track_history_f64(n, n, n, n, n, 1, 1, 0, n, 0, n, n, n, n, n, n, n) == -1
    assert lib.lidar_last_error().startswith(b"lidar_track_history_f64: null pointer")
    # the checks come before the handle is touched: a call that passed them would crash on this dummy handle
    p = ctypes.c_void_p(64)
    T, cap = 7, 43

    def call(frames=T, c=cap, carry=0, Z=3, h=p, people=p, k=p, prev=p, zones=p, age=p, hits=p, path=p, origin=p, stay=p,
             dwell=p):
        return lib.lidar_track_history_f64(h, people, k, prev, n, frames, c, carry, zones, Z, age, hits, path, origin,
                                           stay, dwell, n)

    for kw in (dict(h=n), dict(people=n), dict(k=n), dict(prev=n), dict(age=n), dict(hits=n), dict(path=n),
               dict(origin=n), dict(frames=-1), dict(frames=65536), dict(c=0), dict(frames=65535, c=1 << 16),
               dict(carry=-1), dict(carry=T + 1), dict(Z=-1), dict(Z=65), dict(zones=n), dict(stay=n), dict(dwell=n)):
        assert call(**kw) == -1, kw
        assert lib.lidar_last_error().startswith(b"lidar_track_history_f64: "), kw
    assert call(carry=T + 1) == -1 and lib.lidar_last_error().startswith(b"lidar_track_history_f64: carry")
    # nothing to do, whatever the handle: carry == frames; the zone pointers are not looked at with nzones == 0
    assert call(carry=T) == 0 and call(frames=0) == 0
    assert call(carry=T, Z=0, zones=n, stay=n, dwell=n) == 0
