"""lidar_track_history_f64 / people_tracking.track_history / PeopleTracker(history=True) / CrowdFlowModel's history keys
on the GPU: every output equal to the host specification of tests/track_history_reference.py, integers element for
element and path / origin byte for byte, on scenes tests/test_track_history_cpu.py shows to hold links over missed
frames, stays of several frames, completed stays and paths whose square roots round."""
import numpy as np
import pytest

import track_reference as ref
import track_stream_reference as sref
import track_events_reference as eref
import track_history_reference as href
import test_track_history_cpu as hand

torch = pytest.importorskip("torch")
from lidar_ai_recommendation_software_amd import _native as nat  # noqa: E402
from lidar_ai_recommendation_software_amd import people_tracking as pt  # noqa: E402
from lidar_ai_recommendation_software_amd.crowd_flow_model import CrowdFlowModel  # noqa: E402

from track_gpu_helpers import dev, pieces_of  # noqa: E402

pytestmark = pytest.mark.gpu


def same(got, want, what="", frames=slice(None)):
    """track_history's six outputs against history_spec's dict (its state arrays over `frames`): dtypes, shapes,
    integers equal, path and origin equal as bytes apart from the payload of a NaN; None without zones."""
    assert len(got) == 6
    for name, dtype, g in zip(href.NAMES, href.DTYPES, got):
        w = want[name]
        if w is None:
            assert g is None, f"{what} {name}"
            continue
        w = w if name == "dwell" else w[frames]
        g = g.cpu().numpy() if isinstance(g, torch.Tensor) else g
        assert g.dtype == dtype and g.shape == w.shape, f"{what} {name}: {g.dtype} {g.shape}"
        if dtype == np.float64:  # a NaN's payload and sign are free: compare where it is, then the bytes without it
            assert np.array_equal(np.isnan(g), np.isnan(w)), f"{what} {name}: NaNs differ"
            g, w = np.nan_to_num(g, nan=0.0), np.nan_to_num(w, nan=0.0)
            bad = np.argwhere(g.view(np.int64) != w.view(np.int64))
            assert g.tobytes() == w.tobytes(), f"{what} {name}: {len(bad)} entries differ in bits, first at {bad[:5].tolist()}"
        else:
            bad = np.argwhere(g != w)
            assert np.array_equal(g, w), f"{what} {name}: {len(bad)} entries differ, first at {bad[:5].tolist()}"


def run(cuda, people, k, prev, gap, zones, **kw):
    return pt.track_history(dev(cuda, people), dev(cuda, np.asarray(k, dtype=np.int64)), dev(cuda, prev), dev(cuda, gap),
                            dev(cuda, zones), **kw)


# ------------------------------------------------------------------ against the specification
@pytest.mark.parametrize("case", sref.GAPPY, ids=str)
@pytest.mark.parametrize("gate", sref.GATES)
@pytest.mark.parametrize("max_gap", [0, 1, 2])
def test_vs_spec(cuda, case, gate, max_gap):
    """cap = 43 (one row tile), 303 (two) and 2 103 (crosses the 2 048-row tile), NaN and junk past K_t."""
    people, k = sref.gappy_sequence(*case)
    s = sref.gappy_spec(*case, gate, max_gap)
    zones = eref.scene_tables(eref.lattice_side(case[1]))[1]
    want = href.gappy_history(*case, gate, max_gap)
    href.not_vacuous(want, k, people.shape[1], max_gap, s["gap"])
    same(run(cuda, people, k, s["prev"], s["gap"], zones), want)


@pytest.mark.parametrize("max_gap", [0, 1, 2])
def test_crossing_scene(cuda, max_gap):
    people, k, _, zones = eref.crossing_scene()
    s = eref.crossing_spec(max_gap)[0]
    want = href.crossing_history(max_gap)
    href.not_vacuous(want, k, people.shape[1], max_gap, s["gap"])
    assert want["dwell"][:, 0, 1].sum() > 0 and 4 <= want["dwell"][:, :, 2].max() <= 10
    same(run(cuda, people, k, s["prev"], s["gap"], zones), want)


@pytest.mark.parametrize("case", sref.GAPPY[:2], ids=str)
def test_batch_form_without_gap(cuda, case):
    """gap = None on track_people's prev is gap from track_stream(max_gap = 0), and the specification's."""
    people, k = sref.gappy_sequence(*case)
    zones = eref.scene_tables(eref.lattice_side(case[1]))[1]
    pd, kd, zd = dev(cuda, people), dev(cuda, k), dev(cuda, zones)
    prev = pt.track_people(pd, kd, ref.DT, 0.5)[0]
    sprev, sgap = pt.track_stream(pd, kd, ref.DT, 0.5, 0)[:2]
    a = pt.track_history(pd, kd, prev, None, zd)
    b = pt.track_history(pd, kd, sprev, sgap, zd)
    assert all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a, b))
    same(a, href.gappy_history(*case, 0.5, 0))


# ------------------------------------------------------------------ shapes
def scene(which):
    if which == "crossing":  # cap = 203: one row tile
        people, k, _, _ = eref.crossing_scene()
        return people, k, eref.crossing_spec()[0], eref.CROSSING["side"]
    case = sref.GAPPY[1]  # cap = 303: two row tiles
    return sref.gappy_sequence(*case) + (sref.gappy_spec(*case, 0.5, 2), eref.lattice_side(case[1]))


@pytest.mark.parametrize("which", ["crossing", "gappy"])
def test_no_zone_one_zone_and_64_zones(cuda, which):
    people, k, s, side = scene(which)
    L = side * ref.STEP
    want = href.history_spec(people, k, s["prev"], s["gap"], None)
    got = run(cuda, people, k, s["prev"], s["gap"], None)
    assert got[4] is None and got[5] is None
    same(got, want, "Z = 0")
    zones = eref.scene_tables(side)[1]
    want = href.history_spec(people, k, s["prev"], s["gap"], zones[2:3])
    assert want["dwell"][:, 0, 0].sum() > 0 and (want["stay"] >= 2).sum() > 20
    same(run(cuda, people, k, s["prev"], s["gap"], zones[2:3]), want, "Z = 1")
    # tests/test_gpu_track_events.py's table of 64 zones: overlapping strips, and everything as zone 63
    x = np.linspace(0.05, L - 0.05, 64)
    zones = np.column_stack([x - 0.3, x + 0.4, np.full(64, 0.1), np.linspace(0.5, L, 64)])
    zones[63] = (-1.0, L + 1.0, -1.0, L + 1.0)
    want = href.history_spec(people, k, s["prev"], s["gap"], zones)
    assert np.count_nonzero(want["dwell"][:, :, 0].sum(axis=0)) >= 20 and not want["dwell"][:, 63].any()
    assert want["stay"][:, :, 63].max() == len(k) - 1
    same(run(cuda, people, k, s["prev"], s["gap"], zones), want, "Z = 64")


def test_one_frame_and_one_row(cuda):
    people, k, s, side = scene("gappy")
    zones = eref.scene_tables(side)[1]
    # T = 1: every live row starts
    p1, k1 = people[:1], k[:1]
    prev = np.full((1, people.shape[1]), -1, dtype=np.int32)
    gap = np.zeros_like(prev)
    want = href.history_spec(p1, k1, prev, gap, zones)
    assert want["linked"] == 0 and want["hits"].sum() == k[0] and not want["dwell"].any()
    same(run(cuda, p1, k1, prev, gap, zones), want, "T = 1")
    same(run(cuda, p1, k1, prev, None, zones), want, "T = 1, no gap")
    # cap = 1: one walker back and forth, missing from frame 3 (gap 2 into frame 4), k = 0 there
    x = np.array([1.0, -1.0, 0.0, np.nan, 2.0, -0.5])
    pc = np.column_stack([x, np.full(6, 5.0)]).reshape(6, 1, 2)
    kc = np.array([1, 1, 1, 0, 1, 7])
    prevc = np.array([-1, 0, 0, 0, 0, 0], dtype=np.int32).reshape(6, 1)
    gapc = np.array([0, 1, 1, 1, 2, 1], dtype=np.int32).reshape(6, 1)
    z1 = [(-2.0, 0.0, 0.0, 10.0)]
    want = href.history_spec(pc, kc, prevc, gapc, z1)
    assert want["age"][:, 0].tolist() == [0, 1, 2, -1, 4, 5] and want["hits"][:, 0].tolist() == [1, 2, 3, 0, 4, 5]
    assert want["path"][:, 0].tolist() == [0.0, 2.0, 3.0, 0.0, 5.0, 7.5]
    assert want["stay"][:, 0, 0].tolist() == [-1, 0, -1, -1, -1, 0] and want["dwell"][:, 0].tolist() == [
        [0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]]
    same(run(cuda, pc, kc, prevc, gapc, z1), want, "cap = 1")


def test_hand_cases_of_the_heir_rule_and_the_link_guard(cuda):
    """Links no tracker makes have defined results: the lowest (t, j) continues a source named twice, a link the
    guard rejects is a start and nothing is read or written outside the arrays, a NaN poisons the path."""
    people, k, prev, gap = hand.two_heirs()
    want = href.history_spec(people, k, prev, gap, [hand.ROOM])
    assert want["linked"] == 4 and want["heirs"] == 2
    same(run(cuda, people, k, prev, gap, [hand.ROOM]), want, "two heirs")
    people, k, prev, gap = hand.guard_cases()
    for g in (gap, None):
        want = href.history_spec(people, k, prev, g, [hand.ROOM])
        same(run(cuda, people, k, prev, g, [hand.ROOM]), want, "guard")
    people, k, prev = hand.nan_chain()
    want = href.history_spec(people, k, prev, None, [(0.0, 5.0, 0.0, 5.0)])
    assert np.isnan(want["path"][2:, 0]).all()
    same(run(cuda, people, k, prev, None, [(0.0, 5.0, 0.0, 5.0)]), want, "NaN")


# ------------------------------------------------------------------ carry
def sentinels(cuda, T, cap, Z):
    return tuple(torch.full(shape, 77, dtype=dtype, device=cuda) for _, dtype, shape in pt.history_layout(T, cap, Z))


@pytest.mark.parametrize("max_gap", [0, 2])
def test_carry(cuda, max_gap):
    case = sref.GAPPY[1]
    people, k = sref.gappy_sequence(*case)
    T, cap, _ = people.shape
    s = sref.gappy_spec(*case, 0.5, max_gap)
    zones = eref.scene_tables(eref.lattice_side(case[1]))[1]
    Z = len(zones)
    whole = href.gappy_history(*case, 0.5, max_gap)
    pd, kd, prev, gap, zd = (dev(cuda, a) for a in (people, k, s["prev"], s["gap"], zones))
    for cut in (1, 3, T - 1):
        c = min(max_gap + 1, cut)
        sl = slice(cut - c, T)
        # the carried frames hold the whole's state, the others a sentinel: the call fills those, all of them
        state = sentinels(cuda, T - cut + c, cap, Z)
        for t, name in zip(state, href.STATE):
            t[:c] = dev(cuda, whole[name][cut - c:cut])
        got = pt.track_history(pd[sl].contiguous(), kd[sl].contiguous(), prev[sl].contiguous(), gap[sl].contiguous(), zd,
                               carry=c, state=state)
        assert all(g is t for g, t in zip(got, state)) and tuple(got[5].shape) == (T - cut, Z, 3)
        same(got, {**{n: whole[n] for n in href.STATE}, "dwell": whole["dwell"][cut:]}, f"cut {cut}", slice(cut - c, T))
        # carried frames that hold a sentinel: they stay untouched, every other element is written, and the heirs of
        # carried rows go on from the sentinel as the specification does
        given = {n: np.full(whole[n].shape, 77, dtype=whole[n].dtype) for n in href.STATE}
        want = href.history_spec(people, k, s["prev"], s["gap"], zones, cut, given)
        assert want["hits"].max() >= 78 and all((want[n][:cut] == 77).all() for n in href.STATE)
        state = sentinels(cuda, T, cap, Z)
        got = pt.track_history(pd, kd, prev, gap, zd, carry=cut, state=state)
        same(got, want, f"carry {cut} of sentinels")
        assert not (got[0][cut:] == 77).any() and not (got[1][cut:] == 77).any()


def test_carry_equal_to_T_and_the_argument_checks(cuda):
    case = sref.GAPPY[0]
    people, k = sref.gappy_sequence(*case)
    T, cap, _ = people.shape
    s = sref.gappy_spec(*case, 0.5, 1)
    zones = eref.scene_tables(eref.lattice_side(case[1]))[1]
    Z = len(zones)
    pd, kd, prev, gap, zd = (dev(cuda, a) for a in (people, k, s["prev"], s["gap"], zones))
    # carry == T: nothing is written, by the wrapper ...
    state = sentinels(cuda, T, cap, Z)
    got = pt.track_history(pd, kd, prev, gap, zd, carry=T, state=state)
    assert tuple(got[5].shape) == (0, Z, 3)
    # ... and by the entry point, handed sentinel-filled arrays
    dwell = torch.full((T, Z, 3), 77, dtype=torch.int64, device=cuda)
    nat.call("lidar_track_history_f64", nat.handle(cuda.index), nat.ptr(pd), nat.ptr(kd), nat.ptr(prev), nat.ptr(gap), T, cap,
             T, nat.ptr(zd), Z, *(nat.ptr(t) for t in state), nat.ptr(dwell), nat.stream_ptr())
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(state, sentinels(cuda, T, cap, Z))) and (dwell == 77).all()
    # the wrapper's own checks
    for kw in (dict(carry=-1), dict(carry=T + 1), dict(carry=1.5), dict(carry=1), dict(state=state[:4]),
               dict(state=sentinels(cuda, T - 1, cap, Z)), dict(state=sentinels(cuda, T, cap, Z + 1)),
               dict(state=tuple(t.long() for t in state))):
        with pytest.raises(ValueError, match="^track_history"):
            pt.track_history(pd, kd, prev, gap, zd, **kw)
    with pytest.raises(ValueError, match="^track_history: state"):
        pt.track_history(pd, kd, prev, gap, None, state=state)  # stay without zones
    with pytest.raises(ValueError, match="^track_history: zones"):
        pt.track_history(pd, kd, prev, gap, torch.zeros((65, 4), dtype=torch.float64, device=cuda))
    with pytest.raises(ValueError, match="^track_history: zones"):
        pt.track_history(pd, kd, prev, gap, zd.float())
    with pytest.raises(ValueError, match="^track_history: gap"):
        pt.track_history(pd, kd, prev, gap.long(), zd)
    with pytest.raises(ValueError, match="^track_history: prev"):
        pt.track_history(pd, kd, prev[:, :-1].contiguous(), gap, zd)
    # what the entry point rejects with a real handle
    with pytest.raises(nat.LidarError, match="lidar_track_history_f64: carry"):
        nat.call("lidar_track_history_f64", nat.handle(cuda.index), nat.ptr(pd), nat.ptr(kd), nat.ptr(prev), nat.ptr(gap), T,
                 cap, T + 1, nat.ptr(zd), Z, *(nat.ptr(t) for t in state), nat.ptr(dwell), nat.stream_ptr())
    same(pt.track_history(pd, kd, prev, gap, zd), href.gappy_history(*case, 0.5, 1), "after errors")


# ------------------------------------------------------------------ through the tracker
@pytest.mark.parametrize("case", sref.GAPPY, ids=str)
@pytest.mark.parametrize("max_gap", [0, 1, 2])
def test_split_equals_whole_through_the_tracker(cuda, case, max_gap):
    people, k = sref.gappy_sequence(*case)
    T, gate, grid = case[0], 0.5, 1.0
    gates, zones = eref.scene_tables(eref.lattice_side(case[1]))
    gates = gates[:5]
    want = href.gappy_history(*case, gate, max_gap)
    assert want["dwell"][:, :, 0].sum() > 0
    xr, yr = ref.extent_of(people, k)
    pd, kd = dev(cuda, people), dev(cuda, k)
    tracker = pt.PeopleTracker(ref.DT, gate, max_gap, xr, yr, grid, gates=gates, zones=zones, history=True)
    bare = pt.PeopleTracker(ref.DT, gate, max_gap, xr, yr, grid, gates=gates, zones=zones)
    hist, lo = [], 0
    seen = {name: [] for name in ("prev", "gap", "track_id", "velocity") + eref.NAMES + href.STATE}
    for n in pieces_of(T):
        a = tracker.push(pd[lo:lo + n], kd[lo:lo + n])
        b = bare.push(pd[lo:lo + n], kd[lo:lo + n])
        # prev, gap, track_id, velocity: what the tracker returns without history, byte for byte
        assert all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a, b))
        assert len(tracker.last_history) == 6 and all(t.shape[0] == n for t in tracker.last_history)
        hist.append(tracker.last_history)
        lo += n
        # the window: the last min(max_gap + 1, frames so far) frames of everything pushed, returned or left so far
        for name, t in zip(seen, a + tracker.last_events + tracker.last_history[:5]):
            seen[name].append(t.cpu().numpy())
        so_far = {name: np.concatenate(parts) for name, parts in seen.items()}
        so_far.update(people=people[:lo], k=k[:lo], succ=np.zeros((lo, people.shape[1]), dtype=np.uint8))
        t, j = np.nonzero(so_far["prev"] >= 0)  # a linked row marks its source, so_far["gap"] frames back
        so_far["succ"][t - so_far["gap"][t, j], so_far["prev"][t, j]] = 1
        keep = min(max_gap + 1, lo)
        held = tracker.held()
        assert set(held) == set(so_far) and tracker.frames == lo
        for name, t in held.items():
            g, w = t.cpu().numpy(), so_far[name][lo - keep:]
            assert g.shape[0] == keep and g.dtype == w.dtype and g.tobytes() == w.tobytes(), (lo, name)
    same(tuple(torch.cat([h[i] for h in hist]) for i in range(6)), want, "last_history")
    total = tracker.dwell_total.cpu().numpy()
    d = want["dwell"]
    assert total.dtype == np.int64 and total.shape == (3, 3)
    assert np.array_equal(total[:, :2], d[:, :, :2].sum(axis=0)) and np.array_equal(total[:, 2], d[:, :, 2].max(axis=0))
    assert bare.last_history is None and bare.dwell_total is None and not set(href.STATE) & set(bare.held())
    assert int(tracker.ntracks) == int(bare.ntracks) and int(tracker.matched) == int(bare.matched)
    assert torch.equal(tracker.count, bare.count) and tracker.vsum.cpu().numpy().tobytes() == bare.vsum.cpu().numpy().tobytes()
    assert torch.equal(tracker.gate_total, bare.gate_total) and torch.equal(tracker.zone_total, bare.zone_total)
    assert np.array_equal(total[:, 0], tracker.zone_total[:, 1].cpu().numpy())  # completed stays are exits


def test_tracker_without_zones(cuda):
    case = sref.GAPPY[0]
    people, k = sref.gappy_sequence(*case)
    s = sref.gappy_spec(*case, 0.5, 1)
    want = href.history_spec(people, k, s["prev"], s["gap"], None)
    pd, kd = dev(cuda, people), dev(cuda, k)
    tracker = pt.PeopleTracker(ref.DT, 0.5, 1, history=True)
    hist = []
    for lo, hi in ((0, 4), (4, 4), (4, len(k))):
        tracker.push(pd[lo:hi], kd[lo:hi])
        assert tracker.last_history[4] is None and tracker.last_history[5] is None
        assert all(t.shape[0] == hi - lo for t in tracker.last_history[:4])
        hist.append(tracker.last_history)
    same(tuple(torch.cat([h[i] for h in hist]) for i in range(4)) + (None, None), want, "no zones")
    assert tracker.dwell_total is None and tracker.last_events is None


# ------------------------------------------------------------------ the model
HISTORY_KEYS = {"ages", "hits", "path_lengths", "origins", "track_table"}
DWELL_KEYS = {"zone_stays", "zone_dwell_count", "zone_dwell_frames", "zone_dwell_max", "zone_dwell_mean_s"}
EVENT_KEYS = {"gate_counts", "gate_series", "zone_occupancy", "zone_entries", "zone_exits", "gate_events",
              "zone_membership"}


def same_keys(got, want, s, people, K, frames, first, dwell, zoned, what):
    """The model's history keys against history_spec's arrays over the frames `frames` (numbered from `first` in
    track_table); dwell: the whole stream's (T, Z, 3)."""
    for key, name, dtype in (("ages", "age", np.int32), ("hits", "hits", np.int32), ("path_lengths", "path", np.float64),
                             ("origins", "origin", np.float64)) + ((("zone_stays", "stay", np.int32),) if zoned else ()):
        assert len(got[key]) == len(frames), f"{what}.{key}"
        for a, t in zip(got[key], frames):
            assert a.dtype == dtype and a.tobytes() == want[name][t, :K[t]].tobytes(), f"{what}.{key}[{t}]"
    sl = slice(frames[0], frames[-1] + 1)
    table = href.track_table(s["track_id"][sl], want["age"][sl], want["hits"][sl], want["path"][sl], want["origin"][sl],
                             people[sl], K[sl], np.arange(frames[0], frames[-1] + 1) - first, ref.DT)
    assert list(got["track_table"]) == list(table)
    for key in table:
        g, w = got["track_table"][key], table[key]
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), f"{what}.track_table.{key}"
    if zoned:
        count, total, longest = dwell[:, :, 0].sum(axis=0), dwell[:, :, 1].sum(axis=0), dwell[:, :, 2].max(axis=0)
        for key, w in (("zone_dwell_count", count), ("zone_dwell_frames", total), ("zone_dwell_max", longest)):
            assert got[key].dtype == np.int64 and np.array_equal(got[key], w), f"{what}.{key}"
        mean = got["zone_dwell_mean_s"]
        assert mean.dtype == np.float64 and np.array_equal(np.isnan(mean), count == 0)
        assert np.array_equal(mean[count > 0], (np.float64(ref.DT) * total / np.maximum(count, 1))[count > 0])


@pytest.mark.parametrize("case,gate,max_gap", [(sref.GAPPY[0], 0.5, 2), (sref.GAPPY[1], 0.5, 0), (sref.GAPPY[2], 0.25, 1)],
                         ids=str)
def test_analyze_sequence_and_stream(cuda, case, gate, max_gap):
    people, k = sref.gappy_sequence(*case)
    T, cap, _ = people.shape
    K = ref.clamp_k(k, cap)
    zones = eref.scene_tables(eref.lattice_side(case[1]))[1]
    s = sref.gappy_spec(*case, gate, max_gap)
    want = href.gappy_history(*case, gate, max_gap)
    assert want["dwell"][:, 2, 0].sum() > 0 and want["dwell"][:, 1, 0].sum() == 0
    xr, yr = ref.extent_of(people, k)
    model = CrowdFlowModel()
    pd, kd = dev(cuda, people), dev(cuda, k)
    kw = dict(dt=ref.DT, x_range=xr, y_range=yr, gate=gate, max_gap=max_gap)
    keys = {"flow_vectors", "avg_speed", "dominant_direction", "bottlenecks", "tracks", "matched", "observations",
            "track_ids", "velocities"} | ({"gaps"} if max_gap else set())
    assert set(model.analyze_sequence(pd, kd, **kw)) == keys
    assert set(model.analyze_sequence(pd, kd, zones=zones, **kw)) == keys | EVENT_KEYS
    got = model.analyze_sequence(pd, kd, history=True, **kw)
    assert set(got) == keys | HISTORY_KEYS
    same_keys(got, want, s, people, K, range(T), 0, None, False, "sequence")
    assert got["track_table"]["track_id"].tolist() == list(range(got["tracks"]))
    got = model.analyze_sequence(pd, kd, zones=zones, history=True, **kw)
    assert set(got) == keys | EVENT_KEYS | HISTORY_KEYS | DWELL_KEYS
    same_keys(got, want, s, people, K, range(T), 0, want["dwell"], True, "sequence with zones")
    assert np.array_equal(got["zone_dwell_count"], got["zone_exits"])
    # the same stream pushed in pieces: the totals of the whole, the arrays of the held frames
    tracker = pt.PeopleTracker(ref.DT, gate, max_gap, xr, yr, zones=zones, history=True)
    bare = pt.PeopleTracker(ref.DT, gate, max_gap, xr, yr, zones=zones)
    unzoned = pt.PeopleTracker(ref.DT, gate, max_gap, xr, yr, history=True)
    lo = 0
    for n in pieces_of(T):
        for t in (tracker, bare, unzoned):
            t.push(pd[lo:lo + n], kd[lo:lo + n])
        lo += n
    held = range(T - min(max_gap + 1, T), T)
    res = model.analyze_stream(tracker)
    assert set(res) == keys | EVENT_KEYS | HISTORY_KEYS | DWELL_KEYS | {"gaps"}
    assert set(model.analyze_stream(bare)) == keys | EVENT_KEYS | {"gaps"}
    same_keys(res, want, s, people, K, held, 0, want["dwell"], True, "stream")
    res = model.analyze_stream(unzoned)
    assert set(res) == keys | HISTORY_KEYS | {"gaps"}
    same_keys(res, want, s, people, K, held, 0, None, False, "stream without zones")


def test_analyze_stream_on_an_empty_tracker(cuda):
    model = CrowdFlowModel()
    tracker = pt.PeopleTracker(ref.DT, 0.25, 1, (0.0, 4.0), (0.0, 4.0), zones=[(0, 1, 0, 1), (1, 2, 0, 1)], history=True)
    res = model.analyze_stream(tracker)
    assert res["ages"] == [] and res["hits"] == [] and res["path_lengths"] == [] and res["origins"] == []
    assert res["zone_stays"] == [] and all(len(v) == 0 for v in res["track_table"].values())
    assert len(res["track_table"]) == 7
    for key in ("zone_dwell_count", "zone_dwell_frames", "zone_dwell_max"):
        assert res[key].dtype == np.int64 and res[key].tolist() == [0, 0]
    assert np.isnan(res["zone_dwell_mean_s"]).all() and res["zone_dwell_mean_s"].shape == (2,)
    plain = model.analyze_stream(pt.PeopleTracker(ref.DT, 0.25, 1, (0.0, 4.0), (0.0, 4.0), history=True))
    assert HISTORY_KEYS <= set(plain) and not DWELL_KEYS & set(plain)
