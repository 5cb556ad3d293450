"""lidar_track_stream_f64 / lidar_flow_cells_acc_f64 / people_tracking.PeopleTracker / CrowdFlowModel.analyze_stream on
the GPU: every output equal, bit for bit, to the host specification of tests/track_stream_reference.py, whose gappy
sequences tests/test_track_stream_cpu.py shows to be stitched (13-19 % of the matched rows have gap >= 2)."""
import numpy as np
import pytest

import track_reference as ref
import track_stream_reference as sref

torch = pytest.importorskip("torch")
from lidar_ai_recommendation_software_amd import _native as nat  # noqa: E402
from lidar_ai_recommendation_software_amd import people_tracking as pt  # noqa: E402
from lidar_ai_recommendation_software_amd.crowd_flow_model import CrowdFlowModel  # noqa: E402

from track_gpu_helpers import dev, pieces_of  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = {"prev": np.int32, "gap": np.int32, "succ": np.uint8, "velocity": np.float64, "track_id": np.int32}


def run(cuda, people, k, dt, gate, max_gap):
    out = pt.track_stream(dev(cuda, people), dev(cuda, np.asarray(k, dtype=np.int64)), dt, gate, max_gap)
    got = dict(zip(sref.STATE + ("ntracks",), (t.cpu().numpy() for t in out)))
    got["ntracks"] = int(got["ntracks"])
    return got


def check(got, want, what=""):
    """The five state arrays over the full (T, cap) arrays, and ntracks."""
    for name in sref.STATE:
        assert got[name].dtype == DTYPES[name] and got[name].shape == want[name].shape, f"{what} {name}"
        if name == "velocity":
            assert got[name].tobytes() == want[name].tobytes(), f"{what} velocity"
        else:
            bad = np.argwhere(got[name] != want[name])
            assert bad.size == 0, f"{what} {name}: {len(bad)} entries differ, first at {bad[:5].tolist()}"
    assert got["ntracks"] == want["ntracks"], f"{what} ntracks {got['ntracks']} != {want['ntracks']}"


@pytest.mark.parametrize("case", sref.GAPPY, ids=str)
@pytest.mark.parametrize("gate", sref.GATES)
@pytest.mark.parametrize("max_gap", [0, 1, 2])
def test_vs_spec(cuda, case, gate, max_gap):
    people, k = sref.gappy_sequence(*case)
    check(run(cuda, people, k, ref.DT, gate, max_gap), sref.gappy_spec(*case, gate, max_gap))


@pytest.mark.parametrize("case", sref.GAPPY + ref.PLANTED[:1], ids=str)
def test_max_gap_0_equals_track_people(cuda, case):
    people, k = sref.gappy_sequence(*case) if case in sref.GAPPY else ref.planted_sequence(*case)
    pd, kd = dev(cuda, people), dev(cuda, k)
    for gate in sref.GATES:
        prev, tid, vel, nt = pt.track_people(pd, kd, ref.DT, gate)
        sprev, sgap, ssucc, svel, stid, snt = pt.track_stream(pd, kd, ref.DT, gate, 0)
        assert torch.equal(prev, sprev) and torch.equal(tid, stid) and int(nt) == int(snt)
        assert vel.cpu().numpy().tobytes() == svel.cpu().numpy().tobytes()
        assert torch.equal(sgap, (prev >= 0).to(torch.int32))
        assert int(ssucc.sum()) == int((prev >= 0).sum())


@pytest.mark.parametrize("case", sref.GAPPY, ids=str)
@pytest.mark.parametrize("max_gap", [0, 1, 2])
def test_split_equals_whole_through_the_tracker(cuda, case, max_gap):
    people, k = sref.gappy_sequence(*case)
    T, gate, grid = case[0], 0.25, 1.0
    want = sref.gappy_spec(*case, gate, max_gap)
    xr, yr = ref.extent_of(people, k)
    x0, y0, nx, ny, _, _ = ref.venue_grid(xr, yr, grid)
    wc, wv = sref.flow_cells_acc_spec(people, k, want["prev"], want["velocity"], x0, y0, grid, nx, ny, first=0)
    assert wc.sum() > 0 and np.any(wv != 0.0)
    pd, kd = dev(cuda, people), dev(cuda, k)
    pieces = pieces_of(T)
    assert 0 in pieces and pieces[0] < max_gap + 1 or max_gap == 0
    tracker = pt.PeopleTracker(ref.DT, gate, max_gap, xr, yr, grid)
    outs, lo = [], 0
    for n in pieces:
        o = tracker.push(pd[lo:lo + n], kd[lo:lo + n])
        assert all(t.shape[0] == n for t in o)
        outs.append(o)
        lo += n
        assert tracker.frames == lo
    assert lo == T
    prev, gap, tid, vel = (torch.cat([o[i] for o in outs]).cpu().numpy() for i in range(4))
    assert np.array_equal(prev, want["prev"]) and np.array_equal(gap, want["gap"])
    assert np.array_equal(tid, want["track_id"]) and vel.tobytes() == want["velocity"].tobytes()
    assert prev.dtype == np.int32 and gap.dtype == np.int32 and tid.dtype == np.int32
    assert int(tracker.ntracks) == want["ntracks"]
    assert int(tracker.matched) == int(np.sum(want["prev"] >= 0))
    assert np.array_equal(tracker.count.cpu().numpy(), wc)
    assert tracker.vsum.cpu().numpy().tobytes() == wv.tobytes()
    # the frames the tracker holds: the whole's last min(max_gap + 1, T), succ included
    keep = min(max_gap + 1, T)
    held = {name: t.cpu().numpy() for name, t in tracker.held().items()}
    for name in sref.STATE:
        assert held[name].tobytes() == want[name][T - keep:].tobytes(), name


def test_carry_through_the_wrapper(cuda):
    """track_stream with an explicit carry: the head's last frames, state and ntracks handed to a second call."""
    case, gate, M = sref.GAPPY[1], 0.5, 2
    people, k = sref.gappy_sequence(*case)
    want = sref.gappy_spec(*case, gate, M)
    pd, kd = dev(cuda, people), dev(cuda, k)
    for cut in (1, 2, 4, case[0]):
        head = pt.track_stream(pd[:cut].contiguous(), kd[:cut].contiguous(), ref.DT, gate, M)
        c = min(M + 1, cut)
        T2 = case[0] - (cut - c)
        state = tuple(torch.cat([h[cut - c:], torch.full((T2 - c,) + tuple(h.shape[1:]), 77, dtype=h.dtype, device=cuda)])
                      for h in head[:5])
        out = pt.track_stream(pd[cut - c:].contiguous(), kd[cut - c:].contiguous(), ref.DT, gate, M, c, state, head[5])
        got = dict(zip(sref.STATE, (t.cpu().numpy() for t in out[:5])))
        for name in sref.STATE:
            assert got[name].tobytes() == want[name][cut - c:].tobytes(), (cut, name)
        assert int(out[5]) == want["ntracks"] and out[5] is head[5]


# ------------------------------------------------------------------ edges
def test_hand_made_gaps(cuda):
    """tests/test_track_stream_cpu.py::test_spec_on_a_hand_made_gap's scene: an empty frame inside a gap, an exact
    tie at gap 2 (the lowest row), an end with candidates at gap 2 and gap 3 (the smaller gap), a match at gap 3;
    and a candidate exactly at gate * g (inclusive) beside one an ulp past it."""
    nan = np.nan
    people = np.full((4, 4, 2), nan)
    people[0, :3] = [(0.0, 0.0), (10.0, 0.0), (20.0, 0.0)]
    people[2, :3] = [(0.75, 0.0), (10.5, 0.0), (9.5, 0.0)]
    people[3, :2] = [(0.0, 0.0), (21.0, 0.0)]
    k = np.array([3, 0, 3, 2])
    got = run(cuda, people, k, 0.5, 0.5, 2)
    check(got, sref.stream_spec(people, k, 0.5, 0.5, 2))
    assert got["prev"][2].tolist() == [0, 1, -1, -1] and got["gap"][2].tolist() == [2, 2, 0, 0]
    assert got["prev"][3].tolist() == [-1, 2, -1, -1] and got["gap"][3].tolist() == [0, 3, 0, 0]
    assert got["track_id"][3].tolist() == [4, 2, -1, -1] and got["ntracks"] == 5
    for g in (2, 3):  # pass g: gate * g = 0.5 g from (10, 0)
        p = np.full((g + 1, 2, 2), nan)
        p[0, :2] = [(10.0, 0.0), (10.0, 50.0)]
        p[g, :2] = [(10.0 + 0.5 * g, 0.0), (10.0, float(np.nextafter(50.0 + 0.5 * g, 99.0)))]
        kk = np.array([2] + [0] * (g - 1) + [2])
        got = run(cuda, p, kk, 0.5, 0.5, g - 1)
        check(got, sref.stream_spec(p, kk, 0.5, 0.5, g - 1), f"gate * {g}")
        assert got["prev"][g].tolist() == [0, -1] and got["gap"][g].tolist() == [g, 0] and got["ntracks"] == 3


def test_k_above_cap_junk_and_non_finite_rows(cuda):
    case, gate, M = sref.GAPPY[1], 0.5, 2
    people, k = sref.gappy_sequence(*case)
    want = sref.gappy_spec(*case, gate, M)
    # junk past K_t: the same bits out, whatever it is (a live row's position, -inf)
    a = run(cuda, people, k, ref.DT, gate, M)
    other = people.copy()
    for t in range(len(k)):
        other[t, k[t]:] = other[t, 0]
    other[-1, k[-1]:] = -np.inf
    b = run(cuda, other, k, ref.DT, gate, M)
    for name in sref.STATE:
        assert a[name].tobytes() == b[name].tobytes(), name
    check(a, want, "junk")
    # k above cap (and below 0) on arrays cut at the smallest K_t
    cut = int(k.min())
    p2, k2 = np.ascontiguousarray(people[:, :cut]), k.copy()
    k2[0], k2[3] = 1 << 40, -3
    check(run(cuda, p2, k2, ref.DT, gate, M), sref.stream_spec(p2, k2, ref.DT, gate, M), "k > cap")
    # NaN / inf in rows the clean sequence stitches: never a candidate in any pass
    bad = people.copy()
    hit = np.zeros(people.shape[:2], dtype=bool)
    vals = [(np.nan, 0), (np.inf, 1), (-np.inf, 0), (np.nan, 1)]
    for t in range(len(k)):
        rows = np.flatnonzero(want["gap"][t] >= 2)[:2].tolist()  # stitched starts ...
        rows += [r for r in np.flatnonzero((want["succ"][t] == 1) & (want["gap"][t] == 0))[:2].tolist()]  # ... and roots
        for n, r in enumerate(rows):
            v, c = vals[(n + t) % len(vals)]
            bad[t, r, c] = v
            hit[t, r] = True
    assert hit.sum() >= 8
    wb = sref.stream_spec(bad, k, ref.DT, gate, M)
    gb = run(cuda, bad, k, ref.DT, gate, M)
    check(gb, wb, "non-finite")
    assert np.all(gb["prev"][hit] == -1) and np.all(gb["succ"][hit] == 0)


def test_frames_without_an_open_row(cuda):
    """Nobody moves and nobody is missed: pass 1 closes every row, the later passes find no open query (every
    workgroup leaves at its first barrier) and no open candidate; and frames with K_t = 0 in between."""
    rng = np.random.default_rng(5)
    n, cap = 300, 301
    base = rng.permutation(40 * 40)[:n]
    pos = np.column_stack([base % 40, base // 40]) * 1.0
    people = np.full((6, cap, 2), ref.JUNK)
    k = np.array([n, n, n, 0, n, n])
    for t in range(6):
        people[t, :n] = pos[rng.permutation(n)]
    want = sref.stream_spec(people, k, ref.DT, 0.25, 2)
    assert np.all(want["gap"][1:3, :n] == 1) and np.all(want["gap"][4, :n] == 2) and want["ntracks"] == n
    check(run(cuda, people, k, ref.DT, 0.25, 2), want)


@pytest.mark.parametrize("K", [255, 256, 257, 2047, 2048, 2049])
def test_block_and_tile_edges(cuda, K):
    """Three frames of K walkers one metre apart; the walkers on the rows around the block (256) and tile (2 048)
    edges are missing from frame 1 and sit on those rows, in another order, in frame 2: the open rows of pass 2
    lie on both sides of every edge.  cap = K for the block edges, K + 2 for the tile edges."""
    rng = np.random.default_rng(K)
    cap = K if K < 300 else K + 2
    side = int(np.ceil(np.sqrt(K)))
    node = rng.permutation(side * side)[:K]
    pos = np.column_stack([node % side, node // side]) * 1.0
    edge = sorted({r for r in (0, 1, 254, 255, 256, 2046, 2047, 2048, K - 2, K - 1) if 0 <= r < K})
    rest = np.setdiff1d(np.arange(K), edge)
    people = np.full((3, cap, 2), ref.JUNK)
    people[0, :K] = pos
    people[1, :len(rest)] = pos[rest[rng.permutation(len(rest))]] + np.array([ref.STEP, 0.0])
    order = np.arange(K)
    order[edge] = edge[::-1]  # walker edge[-1-i] on row edge[i]
    order[rest] = rest[rng.permutation(len(rest))]
    people[2, :K] = pos[order] + np.array([2 * ref.STEP, 0.0])
    k = np.array([K, len(rest), K])
    want = sref.stream_spec(people, k, ref.DT, 0.25, 1)
    assert np.flatnonzero(want["gap"][2] == 2).tolist() == edge and np.all(want["gap"][2, rest] == 1)
    assert want["prev"][2, edge].tolist() == edge[::-1] and want["ntracks"] == K
    check(run(cuda, people, k, ref.DT, 0.25, 1), want)


@pytest.mark.parametrize("max_gap", [1, 2])
def test_constant_velocity_with_dropouts(cuda, max_gap):
    """Well separated walkers at 1 m/s, each missing for 1 .. max_gap frames: one id per walker over the whole
    sequence, every velocity the true one, ntracks the number of walkers; in one call and through the tracker."""
    gate, T, n_side = 0.25, 9, 6
    people, k, present, rows = sref.dropout_scene(n_side, T, max_gap, gate, 17 + max_gap)
    n = n_side * n_side
    one = run(cuda, people, k, ref.STEP, gate, max_gap)
    tracker = pt.PeopleTracker(ref.STEP, gate, max_gap)
    pd, kd = dev(cuda, people), dev(cuda, k)
    outs = [tracker.push(pd[lo:hi], kd[lo:hi]) for lo, hi in ((0, 2), (2, 3), (3, 7), (7, 9))]
    via = {"prev": 0, "gap": 1, "track_id": 2, "velocity": 3}
    via = {name: torch.cat([o[i] for o in outs]).cpu().numpy() for name, i in via.items()}
    via["ntracks"] = int(tracker.ntracks)
    for what, got in (("one call", one), ("tracker", via)):
        assert got["ntracks"] == n, what
        ids = np.full((T, n), -1)
        for t in range(T):
            w = np.flatnonzero(present[t])
            ids[t, w] = got["track_id"][t, rows[t, w]]
            later = w[[present[:t, x].any() for x in w]] if t else w[:0]
            assert np.all(got["velocity"][t, rows[t, later]] == np.array([1.0, 0.0])), (what, t)
            assert np.all(got["prev"][t, rows[t, later]] >= 0), (what, t)
        for w in range(n):
            assert len(set(ids[present[:, w], w].tolist())) == 1, (what, w)
        assert int(np.sum(got["gap"] >= 2)) == n and got["gap"].max() == max_gap + 1
    check(one, sref.stream_spec(people, k, ref.STEP, gate, max_gap))


# ------------------------------------------------------------------ flow cells
def call_acc(cuda, pd, kd, prev, vel, first, accumulate, grid4, g, count, vsum):
    x0, y0, nx, ny = grid4
    T, cap = prev.shape
    nat.call("lidar_flow_cells_acc_f64", nat.handle(cuda.index), nat.ptr(pd), nat.ptr(kd), nat.ptr(prev), nat.ptr(vel),
             T, cap, first, accumulate, x0, y0, g, nx, ny, nat.ptr(count), nat.ptr(vsum), nat.stream_ptr())


def test_flow_cells_acc(cuda):
    case, gate, M, g = sref.GAPPY[1], 0.25, 1, 1.0
    people, k = sref.gappy_sequence(*case)
    s = sref.gappy_spec(*case, gate, M)
    T = case[0]
    xr, yr = ref.extent_of(people, k)
    x0, y0, nx, ny, _, _ = ref.venue_grid(xr, yr, g)
    pd, kd, prev, vel = dev(cuda, people), dev(cuda, k), dev(cuda, s["prev"]), dev(cuda, s["velocity"])

    def fresh(fill):
        return (torch.full((nx, ny), fill, dtype=torch.int32, device=cuda),
                torch.full((nx, ny, 2), float(fill), dtype=torch.float64, device=cuda))

    # first = 1, accumulate = 0 is lidar_flow_cells_f64 (which overwrites whatever was there)
    c0, v0, grid4 = pt.flow_cells(pd, kd, prev, vel, xr, yr, g)
    assert grid4 == (x0, y0, nx, ny)
    c1, v1 = fresh(77)
    call_acc(cuda, pd, kd, prev, vel, 1, 0, grid4, g, c1, v1)
    assert torch.equal(c0, c1) and v0.cpu().numpy().tobytes() == v1.cpu().numpy().tobytes()
    wc, wv = sref.flow_cells_acc_spec(people, k, s["prev"], s["velocity"], x0, y0, g, nx, ny, first=1)
    assert np.array_equal(c1.cpu().numpy(), wc) and v1.cpu().numpy().tobytes() == wv.tobytes()
    # accumulation over overlapping windows equals the whole: [0, 3) from 0, then [1, 5) from 3, then [4, T) from 5
    c2, v2 = fresh(0)
    for lo, first, hi in ((0, 0, 3), (1, 3, 5), (4, 5, T)):
        call_acc(cuda, pd[lo:hi], kd[lo:hi], prev[lo:hi], vel[lo:hi], first - lo, 1, grid4, g, c2, v2)
    assert torch.equal(c0, c2) and v0.cpu().numpy().tobytes() == v2.cpu().numpy().tobytes()
    # a frame-0 matched row (its predecessor is in a carry) is counted iff first = 0
    tail = slice(2, T)
    for first in (0, 1):
        c3, v3 = fresh(77)
        call_acc(cuda, pd[tail], kd[tail], prev[tail], vel[tail], first, 0, grid4, g, c3, v3)
        wc3, wv3 = sref.flow_cells_acc_spec(people[tail], k[tail], s["prev"][tail], s["velocity"][tail], x0, y0, g, nx, ny,
                                            first=first)
        assert np.array_equal(c3.cpu().numpy(), wc3) and v3.cpu().numpy().tobytes() == wv3.tobytes(), first
    inside = sref.flow_cells_acc_spec(people[2:3], k[2:3], s["prev"][2:3], s["velocity"][2:3], x0, y0, g, nx, ny, first=0)
    assert inside[0].sum() > 0  # frame 2 has matched rows inside the grid: first = 0 and first = 1 differ above
    # first = frames: nothing is counted; accumulate = 1 then leaves the cells as they are
    c4, v4 = c2.clone(), v2.clone()
    call_acc(cuda, pd, kd, prev, vel, T, 1, grid4, g, c4, v4)
    assert torch.equal(c4, c2) and torch.equal(v4, v2)


# ------------------------------------------------------------------ the model
def same_flow(got, want, frames, what):
    for key in ("positions", "vectors", "magnitudes"):
        g, w = got["flow_vectors"][key], want["flow_vectors"][key]
        assert g.dtype == np.float64 and g.shape == w.shape and g.tobytes() == w.tobytes(), f"{what}.{key}"
    assert got["observations"].dtype == np.int32 and np.array_equal(got["observations"], want["observations"])
    assert got["tracks"] == want["tracks"] and got["matched"] == want["matched"]
    assert type(got["tracks"]) is int and type(got["matched"]) is int
    for key in ("track_ids", "velocities", "gaps"):
        assert len(got[key]) == len(frames)
        for g, t in zip(got[key], frames):
            w = want[key][t]
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), f"{what}.{key}[{t}]"


@pytest.mark.parametrize("case,gate,max_gap,grid,min_obs", [(sref.GAPPY[0], 0.25, 2, 1.0, 1), (sref.GAPPY[1], 0.5, 1, 1.0, 3),
                                                            (sref.GAPPY[2], 0.25, 1, 2.0, 1)], ids=str)
def test_analyze_sequence_and_stream(cuda, case, gate, max_gap, grid, min_obs):
    people, k = sref.gappy_sequence(*case)
    T = case[0]
    xr, yr = ref.extent_of(people, k)
    want = sref.stream_result_spec(people, k, ref.DT, gate, max_gap, xr, yr, grid, min_obs)
    assert len(want["observations"]) >= 5 and any(np.any(g >= 2) for g in want["gaps"])
    model = CrowdFlowModel()
    pd, kd = dev(cuda, people), dev(cuda, k)
    got = model.analyze_sequence(pd, kd, dt=ref.DT, x_range=xr, y_range=yr, gate=gate, grid_size=grid,
                                 min_observations=min_obs, max_gap=max_gap)
    keys = {"flow_vectors", "avg_speed", "dominant_direction", "bottlenecks", "tracks", "matched", "observations",
            "track_ids", "velocities", "gaps"}
    assert set(got) == keys
    same_flow(got, want, range(T), "sequence")
    fv = want["flow_vectors"]
    assert float(got["avg_speed"]).hex() == float(np.mean(fv["magnitudes"])).hex()
    assert got["dominant_direction"] == CrowdFlowModel._dominant_direction(fv["vectors"])
    assert got["bottlenecks"] == model._identify_bottlenecks(fv, None)
    # the default keeps its keys: no gaps
    plain = model.analyze_sequence(pd, kd, dt=ref.DT, x_range=xr, y_range=yr, gate=gate, grid_size=grid)
    assert set(plain) == keys - {"gaps"} and plain["tracks"] > got["tracks"]
    # the same stream pushed in pieces
    tracker = pt.PeopleTracker(ref.DT, gate, max_gap, xr, yr, grid)
    lo = 0
    for n in pieces_of(T):
        tracker.push(pd[lo:lo + n], kd[lo:lo + n])
        lo += n
    res = model.analyze_stream(tracker, min_observations=min_obs)
    assert set(res) == keys
    same_flow(res, want, range(T - min(max_gap + 1, T), T), "stream")
    assert float(res["avg_speed"]).hex() == float(got["avg_speed"]).hex()
    assert res["dominant_direction"] == got["dominant_direction"] and res["bottlenecks"] == got["bottlenecks"]


def test_tracker_and_wrapper_edges(cuda):
    people, k = sref.gappy_sequence(*sref.GAPPY[0])
    pd, kd = dev(cuda, people), dev(cuda, k)
    T, cap, _ = people.shape
    # an empty tracker, and one that saw only an empty push
    model = CrowdFlowModel()
    tracker = pt.PeopleTracker(ref.DT, 0.25, 1, (0.0, 4.0), (0.0, 4.0))
    assert model.analyze_stream(tracker)["tracks"] == 0
    out = tracker.push(pd[:0], kd[:0])
    assert [tuple(t.shape) for t in out] == [(0, cap), (0, cap), (0, cap), (0, cap, 2)] and tracker.frames == 0
    res = model.analyze_stream(tracker)
    assert res["tracks"] == 0 and res["matched"] == 0 and res["dominant_direction"] == "N/A" and res["gaps"] == []
    tracker.push(pd[:1], kd[:1])
    assert int(tracker.ntracks) == int(k[0]) and int(tracker.count.sum()) == 0
    with pytest.raises(ValueError, match="cap"):
        tracker.push(pd[:1, :cap - 1].contiguous(), kd[:1])
    # empty pushes through a tracker with a gate, a zone and history, the first of them before any frame: every
    # output has its dtype and trailing shape and no frame, the totals stay what they were
    full = pt.PeopleTracker(ref.DT, 0.5, 1, (0.0, 4.0), (0.0, 4.0), gates=[(2.0, 4.0, 2.0, 0.0)],
                            zones=[(0.0, 2.0, 0.0, 4.0)], history=True)
    p5 = np.full((3, 5, 2), np.nan)
    p5[:, :2, 0] = [[1.5, 3.0], [1.9, 3.0], [2.25, 3.0]]  # row 0 walks east through the gate and out of the zone
    p5[:, :2, 1] = 1.0
    p5d, k5d = dev(cuda, p5), dev(cuda, np.array([2, 2, 2]))
    i32, i64, f64 = torch.int32, torch.int64, torch.float64
    totals = None
    for lo, hi, frames in ((0, 0, 0), (0, 3, 3), (3, 3, 3)):
        n = hi - lo
        out = full.push(p5d[lo:hi], k5d[lo:hi])
        assert [(t.dtype, tuple(t.shape)) for t in out] == [(i32, (n, 5)), (i32, (n, 5)), (i32, (n, 5)), (f64, (n, 5, 2))]
        assert [(t.dtype, tuple(t.shape)) for t in full.last_events] == [
            (i32, (n, 1, 2)), (i32, (n, 1, 3)), (i64, (n, 5)), (i64, (n, 5)), (i64, (n, 5))]
        assert [(t.dtype, tuple(t.shape)) for t in full.last_history] == [
            (i32, (n, 5)), (i32, (n, 5)), (f64, (n, 5)), (f64, (n, 5, 2)), (i32, (n, 5, 1)), (i64, (n, 1, 3))]
        assert full.frames == frames
        now = [t.cpu().numpy().copy() for t in (full.ntracks, full.matched, full.count, full.vsum, full.gate_total,
                                                full.zone_total, full.dwell_total)]
        if n == 0:
            assert all(np.array_equal(a, b) if totals else not a.any() for a, b in zip(now, totals or now))
        totals = now
    assert int(full.ntracks) == 2 and full.gate_total.tolist() == [[1, 0]] and full.zone_total.tolist() == [[0, 1]]
    assert full.dwell_total.tolist() == [[1, 1, 1]] and int(full.matched) == 4
    # the id bound is the host's: frames * cap, no read-back
    big = pt.PeopleTracker(ref.DT, 0.25)
    big.push(pd[:1], kd[:1])
    big.frames = (1 << 31) // cap
    with pytest.raises(ValueError, match="2\\^31"):
        big.push(pd[:1], kd[:1])
    # the wrapper's own checks
    for kw in (dict(max_gap=8), dict(max_gap=-1), dict(max_gap=1, carry=3), dict(max_gap=1, carry=1)):
        with pytest.raises(ValueError):
            pt.track_stream(pd, kd, ref.DT, 0.25, **kw)
    state = pt.track_stream(pd, kd, ref.DT, 0.25, 1)
    with pytest.raises(ValueError, match="succ"):
        pt.track_stream(pd, kd, ref.DT, 0.25, 1, 1, state[:2] + (state[2].int(),) + state[3:5], state[5])
    with pytest.raises(ValueError, match="ntracks"):
        pt.track_stream(pd, kd, ref.DT, 0.25, 1, 1, state[:5], state[5].int())
    # what the entry point rejects with a real handle (tests/test_track_stream_cpu.py: each returns before a launch)
    ptrs = [nat.ptr(t) for t in state]
    for frames, carry, max_gap in ((T, 0, 8), (T, 3, 1), (T, -1, 1), (1, 2, 3), (65536, 0, 0)):
        with pytest.raises(nat.LidarError, match="lidar_track_stream_f64"):
            nat.call("lidar_track_stream_f64", nat.handle(cuda.index), nat.ptr(pd), nat.ptr(kd), frames, cap, carry, ref.DT,
                     0.25, max_gap, *ptrs, nat.stream_ptr())
    # frames == carry: nothing is written, ntracks stays
    before = [t.clone() for t in state]
    nat.call("lidar_track_stream_f64", nat.handle(cuda.index), nat.ptr(pd), nat.ptr(kd), 2, cap, 2, ref.DT, 0.25, 1, *ptrs,
             nat.stream_ptr())
    assert all(torch.equal(a, b) for a, b in zip(before, state))
    check(run(cuda, people, k, ref.DT, 0.25, 1), sref.gappy_spec(*sref.GAPPY[0], 0.25, 1), "after errors")
