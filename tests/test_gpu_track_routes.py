"""lidar_track_routes_f64 / people_tracking.track_routes / PeopleTracker(routes=True) / CrowdFlowModel's routes keys on
the GPU: every output equal to the host specification of tests/track_routes_reference.py, integers element for
element, on scenes tests/test_track_routes_cpu.py shows to hold legs off the diagonal, returns, legs over missed
frames and after detections outside every zone, tracks with several legs and positions inside two zones."""
import ctypes

import numpy as np
import pytest

import track_reference as ref
import track_stream_reference as sref
import track_events_reference as eref
import track_routes_reference as rref
import test_track_routes_cpu as hand
from diag_lib import diag_library

torch = pytest.importorskip("torch")
from lidar_ai_recommendation_software_amd import _native as nat  # noqa: E402
from lidar_ai_recommendation_software_amd import people_tracking as pt  # noqa: E402
from lidar_ai_recommendation_software_amd.crowd_flow_model import CrowdFlowModel  # noqa: E402

from track_gpu_helpers import dev, pieces_of  # noqa: E402

pytestmark = pytest.mark.gpu


def same(got, want, what="", frames=slice(None)):
    """track_routes' seven outputs against routes_spec's dict (its state arrays over `frames`): dtype, shape and
    every element."""
    assert len(got) == 7
    for name, dtype, g in zip(rref.NAMES, rref.DTYPES, got):
        w = want[name] if name == "trips" else want[name][frames]
        g = g.cpu().numpy() if isinstance(g, torch.Tensor) else g
        assert g.dtype == dtype and g.shape == w.shape, f"{what} {name}: {g.dtype} {g.shape}"
        bad = np.argwhere(g != w)
        assert np.array_equal(g, w), f"{what} {name}: {len(bad)} entries differ, first at {bad[:5].tolist()}"


def run(cuda, people, k, prev, gap, zones, **kw):
    return pt.track_routes(dev(cuda, people), dev(cuda, np.asarray(k, dtype=np.int64)), dev(cuda, prev), dev(cuda, gap),
                           dev(cuda, np.asarray(zones, dtype=np.float64)), **kw)


def sentinels(cuda, T, cap, value=77):
    return tuple(torch.full(shape, value, dtype=dtype, device=cuda) for _, dtype, shape in pt.routes_layout(T, cap, 1)[:6])


# ------------------------------------------------------------------ against the specification
@pytest.mark.parametrize("case", sref.GAPPY, ids=str)
@pytest.mark.parametrize("gate", sref.GATES)
@pytest.mark.parametrize("max_gap", [0, 1, 2])
def test_vs_spec(cuda, case, gate, max_gap):
    """cap = 43 (one row tile), 303 (two) and 2 103 (nine, and the longest next[] chains), NaN and junk past K_t."""
    people, k, s, zones, want, _ = hand.scene((case, gate, max_gap))
    rref.not_vacuous(want, people, k, s["prev"], s["gap"], zones, max_gap)
    same(run(cuda, people, k, s["prev"], s["gap"], zones), want)


@pytest.mark.parametrize("max_gap", [0, 1, 2])
def test_crossing_scene(cuda, max_gap):
    people, k, s, zones, want, _ = hand.scene(("crossing", max_gap))
    rref.not_vacuous(want, people, k, s["prev"], s["gap"], zones, max_gap)
    same(run(cuda, people, k, s["prev"], s["gap"], zones), want)


def test_hand_cases(cuda):
    """The CPU file's hand cases through the kernel: the table's columns, the heir rule, the link guard, a NaN."""
    rooms = [hand.A, hand.B]
    for xs in ([0.5], [1.5], [1.5, 1.2, 0.5], [0.5, 1.5, 1.6, 2.5, 2.6], [0.5, 2.5], [0.5, 1.5, 0.6, 0.7],
               [0.5, 2.5, 1.5, 1.5, 0.5], [0.5, np.nan, 0.7]):
        people, k, prev, gap = hand.chain(xs)
        same(run(cuda, people, k, prev, gap, rooms), rref.routes_spec(people, k, prev, gap, rooms), str(xs))
        same(run(cuda, people, k, prev, None, rooms), rref.routes_spec(people, k, prev, None, rooms), f"{xs}, no gap")
    people, k, prev, gap = hand.two_heirs()
    want = rref.routes_spec(people, k, prev, gap, rooms)
    assert want["linked"] == 2 and want["heirs"] == 1
    same(run(cuda, people, k, prev, gap, rooms), want, "two heirs")
    people, k, prev, gap = hand.guard_cases()
    for g in (gap, None):
        same(run(cuda, people, k, prev, g, rooms), rref.routes_spec(people, k, prev, g, rooms), "guard")
    people, k, prev, gap = hand.chain([0.5, 9.0, 2.5])  # a link over a missed frame
    k = np.array([1, 0, 1])
    prev[2, 0], gap[2, 0] = 0, 2
    want = rref.routes_spec(people, k, prev, gap, rooms)
    assert want["leg_frames"][2, 0] == 2
    same(run(cuda, people, k, prev, gap, rooms), want, "gap 2")


@pytest.mark.parametrize("case", sref.GAPPY[:2], ids=str)
def test_batch_form_without_gap(cuda, case):
    """gap = None on track_people's prev is gap from track_stream(max_gap = 0), and the specification's."""
    people, k = sref.gappy_sequence(*case)
    zones = rref.gappy_zones(eref.lattice_side(case[1]))
    pd, kd, zd = dev(cuda, people), dev(cuda, k), dev(cuda, zones)
    prev = pt.track_people(pd, kd, ref.DT, 0.5)[0]
    sprev, sgap = pt.track_stream(pd, kd, ref.DT, 0.5, 0)[:2]
    a = pt.track_routes(pd, kd, prev, None, zd)
    b = pt.track_routes(pd, kd, sprev, sgap, zd)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    same(a, rref.gappy_routes(*case, 0.5, 0))


# ------------------------------------------------------------------ zone counts
@pytest.mark.parametrize("which", ["crossing", "gappy"])
def test_one_zone_and_64_zones(cuda, which):
    if which == "crossing":  # cap = 203: one row tile
        people, k, s, zones, _, _ = hand.scene(("crossing", 2))
        side = eref.CROSSING["side"]
    else:  # cap = 303: two row tiles
        people, k, s, zones, _, _ = hand.scene((sref.GAPPY[1], 0.5, 2))
        side = eref.lattice_side(sref.GAPPY[1][1])
    L = side * ref.STEP
    one = zones[1:2]
    want = rref.routes_spec(people, k, s["prev"], s["gap"], one)
    assert want["trips"].shape == (1, 1, 3) and want["trips"][0, 0, 0] > 0  # only returns
    same(run(cuda, people, k, s["prev"], s["gap"], one), want, "Z = 1")
    # tests/test_gpu_track_events.py's table of 64 zones: overlapping strips, and everything as zone 63, which holds
    # whoever no strip holds: the lowest hit is found at every index up to the last
    x = np.linspace(0.05, L - 0.05, 64)
    zones = np.column_stack([x - 0.3, x + 0.4, np.full(64, 0.1), np.linspace(0.5, L, 64)])
    zones[63] = (-1.0, L + 1.0, -1.0, L + 1.0)
    want = rref.routes_spec(people, k, s["prev"], s["gap"], zones)
    K = ref.clamp_k(k, people.shape[1])
    live = np.arange(people.shape[1])[None, :] < K[:, None]
    taken = np.unique(want["last_zone"][live])  # the crossing scene's walkers stay within 3 m of the middle
    assert len(taken) >= 20 and taken[0] >= 0 and taken[-1] == 63 and np.count_nonzero(want["last_zone"][live] == 63) > 500
    assert want["trips"][63, :63, 0].sum() > 0 and want["trips"][:63, 63, 0].sum() > 0
    assert rref.kinds(want, people, k, s["prev"], s["gap"], zones)["positions_in_two_zones"] > 100
    same(run(cuda, people, k, s["prev"], s["gap"], zones), want, "Z = 64")


def test_no_zones_raise_and_launch_nothing(cuda):
    people, k, s, zones, _, _ = hand.scene((sref.GAPPY[0], 0.5, 1))
    T, cap, _ = people.shape
    pd, kd, prev, gap = (dev(cuda, a) for a in (people, k, s["prev"], s["gap"]))
    state = sentinels(cuda, T, cap)
    trips = torch.full((1, 1, 3), 77, dtype=torch.int64, device=cuda)
    with pytest.raises(ValueError, match="^track_routes: needs zones"):
        pt.track_routes(pd, kd, prev, gap, None, state=state, trips=trips)
    with pytest.raises(ValueError, match="^track_routes: zones"):
        pt.track_routes(pd, kd, prev, gap, torch.zeros((0, 4), dtype=torch.float64, device=cuda), state=state, trips=trips)
    # the entry point refuses Z = 0 as well, before any launch
    zd = dev(cuda, zones)
    with pytest.raises(nat.LidarError, match="lidar_track_routes_f64: nzones"):
        nat.call("lidar_track_routes_f64", nat.handle(cuda.index), nat.ptr(pd), nat.ptr(kd), nat.ptr(prev), nat.ptr(gap), T,
                 cap, 0, nat.ptr(zd), 0, *(nat.ptr(t) for t in state), nat.ptr(trips), 0, nat.stream_ptr())
    torch.cuda.synchronize()
    assert all((t == 77).all() for t in state) and (trips == 77).all()


# ------------------------------------------------------------------ carry
@pytest.mark.parametrize("max_gap", [0, 2])
def test_carry_at_every_split_point(cuda, max_gap):
    """Two calls cut at every frame of the crossing scene, the second with the head's last frames as its carry and
    accumulate=True on the head's trips, equal one call."""
    people, k, s, zones, whole, _ = hand.scene(("crossing", max_gap))
    T, cap, _ = people.shape
    pd, kd, prev, gap, zd = (dev(cuda, a) for a in (people, k, s["prev"], s["gap"], zones))
    for cut in range(1, T):
        c = min(max_gap + 1, cut)
        head = pt.track_routes(pd[:cut], kd[:cut], prev[:cut], gap[:cut], zd)
        # the carried frames hold the head's state, the others a sentinel: the call fills those, all of them
        state = sentinels(cuda, T - cut + c, cap)
        for t, h in zip(state, head):
            t[:c] = h[cut - c:]
        sl = slice(cut - c, T)
        got = pt.track_routes(pd[sl], kd[sl], prev[sl], gap[sl], zd, carry=c, state=state, trips=head[6], accumulate=True)
        assert all(g is t for g, t in zip(got, state)) and got[6] is head[6]
        same(got, whole, f"cut {cut}", sl)
    # without accumulate the second call counts its own frames' trips from zero, whatever the array held
    trips = torch.full((len(zones),) * 2 + (3,), 77, dtype=torch.int64, device=cuda)
    got = pt.track_routes(pd[sl], kd[sl], prev[sl], gap[sl], zd, carry=c, state=state, trips=trips)
    own = rref.routes_spec(people[sl], k[sl], s["prev"][sl], s["gap"][sl], zones, c,
                           {n: whole[n][sl] for n in rref.STATE})
    same(got, own, "from zero")


def test_carry_equal_to_T(cuda):
    people, k, s, zones, want, _ = hand.scene((sref.GAPPY[0], 0.5, 1))
    T, cap, _ = people.shape
    Z = len(zones)
    pd, kd, prev, gap, zd = (dev(cuda, a) for a in (people, k, s["prev"], s["gap"], zones))
    state = sentinels(cuda, T, cap)
    trips = torch.full((Z, Z, 3), 77, dtype=torch.int64, device=cuda)
    # no row is written; the trips go on as they are with accumulate, and count from zero without: by the wrapper ...
    got = pt.track_routes(pd, kd, prev, gap, zd, carry=T, state=state, trips=trips, accumulate=True)
    assert got[6] is trips and (trips == 77).all()
    pt.track_routes(pd, kd, prev, gap, zd, carry=T, state=state, trips=trips)
    assert (trips == 0).all() and all((t == 77).all() for t in state)
    # ... and by the entry point
    for accumulate in (1, 0):
        trips.fill_(77)
        nat.call("lidar_track_routes_f64", nat.handle(cuda.index), nat.ptr(pd), nat.ptr(kd), nat.ptr(prev), nat.ptr(gap), T,
                 cap, T, nat.ptr(zd), Z, *(nat.ptr(t) for t in state), nat.ptr(trips), accumulate, nat.stream_ptr())
        torch.cuda.synchronize()
        assert (trips == (77 if accumulate else 0)).all() and all((t == 77).all() for t in state)
    same(pt.track_routes(pd, kd, prev, gap, zd), want, "afterwards")


# ------------------------------------------------------------------ hostile links
def test_hostile_links_are_unlinked_rows(cuda):
    """prev and gap filled with values no tracker writes.  The guard makes such a row an ordinary start: the outputs
    are the specification's, which never follows them either."""
    people, k, s, zones, _, _ = hand.scene(("crossing", 2))
    T, cap, _ = people.shape
    rng = np.random.default_rng(5)
    prev, gap = s["prev"].copy(), s["gap"].copy()
    bad_prev = np.array([-1, -5, -2 ** 31, cap, cap + 1, 2 ** 31 - 1, 10 ** 6], dtype=np.int32)
    bad_gap = np.array([0, -1, 9, 64, 2 ** 31 - 1, -2 ** 31], dtype=np.int32)
    hit = rng.random((T, cap)) < 0.3
    prev[hit] = rng.choice(bad_prev, int(hit.sum()))
    hit = rng.random((T, cap)) < 0.3
    gap[hit] = rng.choice(bad_gap, int(hit.sum()))
    far = rng.random((T, cap)) < 0.1  # a gap that reaches before frame 0, on rows that keep their prev
    gap[far] = (np.arange(T)[:, None] + rng.integers(1, 3, (T, cap)))[far]
    keep = rng.random((T, cap)) < 0.05  # rows past K_(t-g) of the source frame
    prev[keep] = cap - 1
    want = rref.routes_spec(people, k, prev, gap, zones)
    assert 50 < want["linked"] < s["prev"].size and want["trips"][:, :, 0].sum() > 0
    same(run(cuda, people, k, prev, gap, zones), want, "hostile")
    same(run(cuda, people, k, prev, None, zones), rref.routes_spec(people, k, prev, None, zones), "hostile, no gap")


# ------------------------------------------------------------------ a dirty workspace
def test_dirty_workspace_and_outputs(cuda):
    """The handle's workspace (next[]) and every output array filled with 0xFF bytes before the call: the result is
    the specification's, the same as on a clean handle."""
    people, k, s, zones, want, _ = hand.scene((sref.GAPPY[1], 0.5, 2))
    T, cap, _ = people.shape
    Z = len(zones)
    pd, kd, prev, gap, zd = (dev(cuda, a) for a in (people, k, s["prev"], s["gap"], zones))
    with open("/proc/self/maps") as f:  # the HIP runtime this process already runs on, not a second copy of it
        loaded = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert len(loaded) == 1, loaded
    hip = ctypes.CDLL(loaded.pop())
    hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
    with diag_library(device=cuda.index, poison_bytes=1 << 20) as ctx:
        with ctx.clean_handles():
            clean = pt.track_routes(pd, kd, prev, gap, zd)
            torch.cuda.synchronize()
        same(clean, want, "clean handle")
        for c in (0, 2):  # with a carry next[] is initialised from frame max(0, c - 8) on
            ctx.poison(cap, 1)  # the block at its fixed size from here on
            p, b, _ = ctx.info(cap)
            assert p and b >= T * cap * 4
            torch.cuda.synchronize()
            assert hip.hipMemset(p, 0xFF, b) == 0
            state = sentinels(cuda, T, cap, -1)  # 0xFF bytes
            for t, name in zip(state, rref.STATE):
                t[:c] = dev(cuda, want[name][:c])
            trips = torch.full((Z, Z, 3), -1, dtype=torch.int64, device=cuda)
            torch.cuda.synchronize()
            got = pt.track_routes(pd, kd, prev, gap, zd, carry=c, state=state, trips=trips)
            p1, b1, _ = ctx.info(cap)
            assert (p1, b1) == (p, b)
            if c:
                own = rref.routes_spec(people, k, s["prev"], s["gap"], zones, c, {n: want[n] for n in rref.STATE})
                same(got, own, f"dirty, carry {c}")
            else:
                same(got, want, "dirty")
                assert all(torch.equal(a, b) for a, b in zip(got, clean))


# ------------------------------------------------------------------ through the tracker
@pytest.mark.parametrize("case,max_gap", [(sref.GAPPY[0], 0), (sref.GAPPY[0], 2), (sref.GAPPY[1], 1), (sref.GAPPY[2], 2)],
                         ids=str)
def test_split_equals_whole_through_the_tracker(cuda, case, max_gap):
    """Pushed in uneven batches, an empty one and batches of one frame among them."""
    gate = 0.5
    people, k, s, zones, want, _ = hand.scene((case, gate, max_gap))
    T = case[0]
    assert 0 in pieces_of(T) and 1 in pieces_of(T)
    xr, yr = ref.extent_of(people, k)
    pd, kd = dev(cuda, people), dev(cuda, k)
    tracker = pt.PeopleTracker(ref.DT, gate, max_gap, xr, yr, zones=zones, routes=True, history=True)
    bare = pt.PeopleTracker(ref.DT, gate, max_gap, xr, yr, zones=zones, history=True)
    parts, lo = [], 0
    for n in pieces_of(T):
        a = tracker.push(pd[lo:lo + n], kd[lo:lo + n])
        b = bare.push(pd[lo:lo + n], kd[lo:lo + n])
        assert all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a, b))
        assert len(tracker.last_routes) == 6 and all(t.shape[0] == n for t in tracker.last_routes)
        parts.append(tracker.last_routes)
        lo += n
        keep = min(max_gap + 1, lo)
        held = tracker.held()
        assert set(held) == set(bare.held()) | set(pt.ROUTES) and tracker.frames == lo
        assert [name for name, _, _ in tracker.layout(keep)] == list(held)
        for name in pt.ROUTES:
            g = held[name].cpu().numpy()
            assert g.dtype == np.int32 and np.array_equal(g, want[name][lo - keep:lo]), (lo, name)
        for name, t in bare.held().items():
            assert t.cpu().numpy().tobytes() == held[name].cpu().numpy().tobytes(), (lo, name)  # people holds NaN
        # the trips so far: those of the frames pushed, which no later frame changes
        so_far = rref.routes_spec(people[:lo], k[:lo], s["prev"][:lo], s["gap"][:lo], zones)["trips"] if lo in (1, T) \
            else None
        if so_far is not None:
            assert np.array_equal(tracker.trips_total.cpu().numpy(), so_far), lo
    got = tuple(torch.cat([p[i] for p in parts]) for i in range(6)) + (tracker.trips_total,)
    same(got, want, "last_routes and trips_total")
    assert bare.last_routes is None and bare.trips_total is None and not set(pt.ROUTES) & set(bare.held())
    assert torch.equal(tracker.dwell_total, bare.dwell_total) and int(tracker.ntracks) == int(bare.ntracks)


def test_tracker_needs_zones(cuda):
    with pytest.raises(ValueError, match="^PeopleTracker: routes need zones"):
        pt.PeopleTracker(ref.DT, 0.5, 1, routes=True)
    with pytest.raises(ValueError, match="^PeopleTracker: routes need zones"):
        pt.PeopleTracker(ref.DT, 0.5, 1, gates=[(0.0, 0.0, 1.0, 1.0)], routes=True)
    t = pt.PeopleTracker(ref.DT, 0.5, 1, zones=[hand.A], routes=True)
    assert t.routes and t.held() == {} and t.trips_total is None
    assert [name for name, _, _ in t.layout(3)][-6:] == list(pt.ROUTES)
    assert not pt.PeopleTracker(ref.DT, 0.5, 1, zones=[hand.A]).routes


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize("case,gate,max_gap", [(sref.GAPPY[0], 0.5, 2), (sref.GAPPY[1], 0.5, 0), (sref.GAPPY[2], 0.25, 1)],
                         ids=str)
def test_analyze_sequence_and_stream(cuda, case, gate, max_gap):
    people, k, s, zones, want, _ = hand.scene((case, gate, max_gap))
    T, cap, _ = people.shape
    K = ref.clamp_k(k, cap)
    xr, yr = ref.extent_of(people, k)
    model = CrowdFlowModel()
    pd, kd = dev(cuda, people), dev(cuda, k)
    kw = dict(dt=ref.DT, x_range=xr, y_range=yr, gate=gate, max_gap=max_gap)
    today = {"flow_vectors", "avg_speed", "dominant_direction", "bottlenecks", "tracks", "matched", "observations",
             "track_ids", "velocities", "gate_counts", "gate_series", "zone_occupancy", "zone_entries", "zone_exits",
             "gate_events", "zone_membership"} | ({"gaps"} if max_gap else set())
    assert set(model.analyze_sequence(pd, kd, zones=zones, **kw)) == today
    assert set(model.analyze_sequence(pd, kd, zones=zones, routes=False, **kw)) == today
    with pytest.raises(ValueError, match="^analyze_sequence: routes need zones"):
        model.analyze_sequence(pd, kd, routes=True, **kw)
    got = model.analyze_sequence(pd, kd, zones=zones, routes=True, **kw)
    assert set(got) == today | rref.ROUTE_KEYS
    keys = rref.route_keys(s["track_id"], want, K, want["trips"], ref.DT)
    assert hand.same_keys(got, keys)
    assert got["route_table"]["track_id"].tolist() == list(range(got["tracks"]))
    assert got["od_matrix"].sum() == np.count_nonzero(got["route_table"]["first_zone"] >= 0) > 0
    assert np.isnan(got["zone_trip_mean_s"]).any() and np.isfinite(got["zone_trip_mean_s"]).any()
    # the same stream pushed in pieces: the trips of the whole, the arrays and the tables of the held frames
    tracker = pt.PeopleTracker(ref.DT, gate, max_gap, xr, yr, zones=zones, routes=True)
    bare = pt.PeopleTracker(ref.DT, gate, max_gap, xr, yr, zones=zones)
    lo = 0
    for n in pieces_of(T):
        tracker.push(pd[lo:lo + n], kd[lo:lo + n])
        bare.push(pd[lo:lo + n], kd[lo:lo + n])
        lo += n
    held = slice(T - min(max_gap + 1, T), T)
    res = model.analyze_stream(tracker)
    assert set(res) == today | rref.ROUTE_KEYS | {"gaps"} and set(model.analyze_stream(bare)) == today | {"gaps"}
    keys = rref.route_keys(s["track_id"][held], {n: want[n][held] for n in rref.STATE}, K[held], want["trips"], ref.DT)
    assert hand.same_keys(res, keys)


def test_analyze_stream_on_an_empty_tracker(cuda):
    tracker = pt.PeopleTracker(ref.DT, 0.25, 1, (0.0, 4.0), (0.0, 4.0), zones=[(0, 1, 0, 1), (1, 2, 0, 1)], routes=True)
    res = CrowdFlowModel().analyze_stream(tracker)
    assert rref.ROUTE_KEYS <= set(res) and res["legs"] == [] and res["first_zones"] == []
    assert res["zone_trips"].tolist() == [[0, 0], [0, 0]] and np.isnan(res["zone_trip_mean_s"]).all()
    assert all(len(a) == 0 for a in res["route_table"].values()) and res["od_matrix"].tolist() == [[0, 0], [0, 0]]


# ------------------------------------------------------------------ argument checks
def test_argument_checks(cuda):
    people, k, s, zones, want, _ = hand.scene((sref.GAPPY[0], 0.5, 1))
    T, cap, _ = people.shape
    Z = len(zones)
    pd, kd, prev, gap, zd = (dev(cuda, a) for a in (people, k, s["prev"], s["gap"], zones))
    state = sentinels(cuda, T, cap)
    trips = torch.zeros((Z, Z, 3), dtype=torch.int64, device=cuda)
    for kw in (dict(carry=-1), dict(carry=T + 1), dict(carry=1.5), dict(carry=1), dict(state=state[:5]),
               dict(state=sentinels(cuda, T - 1, cap)), dict(state=sentinels(cuda, T, cap + 1)),
               dict(state=tuple(t.long() for t in state)), dict(state=tuple(t.cpu() for t in state)),
               dict(trips=trips.int()), dict(trips=trips[:, :, :2].contiguous()), dict(trips=trips.cpu()),
               dict(trips=torch.zeros((Z + 1, Z + 1, 3), dtype=torch.int64, device=cuda)), dict(accumulate=True)):
        with pytest.raises(ValueError, match="^track_routes"):
            pt.track_routes(pd, kd, prev, gap, zd, **kw)
    with pytest.raises(ValueError, match="^track_routes: carried frames need their state"):
        pt.track_routes(pd, kd, prev, gap, zd, carry=2)
    with pytest.raises(ValueError, match="^track_routes: zones"):
        pt.track_routes(pd, kd, prev, gap, torch.zeros((65, 4), dtype=torch.float64, device=cuda))
    with pytest.raises(ValueError, match="^track_routes: zones"):
        pt.track_routes(pd, kd, prev, gap, zd.float())
    with pytest.raises(ValueError, match="^track_routes: zones"):
        pt.track_routes(pd, kd, prev, gap, zd.cpu())
    with pytest.raises(ValueError, match="^track_routes: gap"):
        pt.track_routes(pd, kd, prev, gap.long(), zd)
    with pytest.raises(ValueError, match="^track_routes: prev"):
        pt.track_routes(pd, kd, prev[:, :-1].contiguous(), gap, zd)
    with pytest.raises(ValueError, match="^track_routes: people"):
        pt.track_routes(pd.float(), kd, prev, gap, zd)
    with pytest.raises(ValueError, match="^track_routes: k"):
        pt.track_routes(pd, kd.int(), prev, gap, zd)
    # what the entry point rejects with a real handle
    args = lambda carry, nz, acc: (nat.handle(cuda.index), nat.ptr(pd), nat.ptr(kd), nat.ptr(prev), nat.ptr(gap), T, cap, carry,
                                   nat.ptr(zd), nz, *(nat.ptr(t) for t in state), nat.ptr(trips), acc, nat.stream_ptr())
    for bad, what in ((args(T + 1, Z, 0), "carry"), (args(0, 65, 0), "nzones"), (args(0, Z, 2), "accumulate")):
        with pytest.raises(nat.LidarError, match=f"lidar_track_routes_f64: {what}"):
            nat.call("lidar_track_routes_f64", *bad)
    with pytest.raises(nat.LidarError, match="lidar_track_routes_f64: null pointer"):
        nat.call("lidar_track_routes_f64", nat.handle(cuda.index), nat.ptr(pd), nat.ptr(kd), nat.ptr(prev), nat.ptr(gap), T,
                 cap, 0, None, Z, *(nat.ptr(t) for t in state), nat.ptr(trips), 0, nat.stream_ptr())
    torch.cuda.synchronize()
    assert all((t == 77).all() for t in state) and not trips.any()
    same(pt.track_routes(pd, kd, prev, gap, zd), want, "after errors")
