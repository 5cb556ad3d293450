"""lidar_track_events_f64 / people_tracking.track_events / PeopleTracker(gates=, zones=) / CrowdFlowModel's gate and zone
keys on the GPU: every output equal, element for element, to the host specification of tests/track_events_reference.py,
on scenes tests/test_track_events_cpu.py shows to hold crossings of every kind (detections on a gate's line, links
over missed frames, rows that cross several gates)."""
import numpy as np
import pytest

import track_reference as ref
import track_stream_reference as sref
import track_events_reference as eref

torch = pytest.importorskip("torch")
from lidar_ai_recommendation_software_amd import _native as nat  # noqa: E402
from lidar_ai_recommendation_software_amd import people_tracking as pt  # noqa: E402
from lidar_ai_recommendation_software_amd.crowd_flow_model import CrowdFlowModel  # noqa: E402

from track_gpu_helpers import dev, pieces_of  # noqa: E402

pytestmark = pytest.mark.gpu


def same(got, want, what=""):
    """track_events' five outputs against events_spec's: dtypes, shapes, every element; None for an absent kind."""
    G, Z = want[0].shape[1], want[1].shape[1]
    assert len(got) == 5
    for name, dtype, g, w, present in zip(eref.NAMES, eref.DTYPES, got, want, (True, True, G, G, Z)):
        if not present:
            assert g is None and not w.any(), f"{what} {name}"
            continue
        g = g.cpu().numpy() if isinstance(g, torch.Tensor) else g
        assert g.dtype == dtype and g.shape == w.shape, f"{what} {name}: {g.dtype} {g.shape}"
        bad = np.argwhere(g != w)
        assert np.array_equal(g, w), f"{what} {name}: {len(bad)} entries differ, first at {bad[:5].tolist()}"


def run(cuda, people, k, prev, gap, gates, zones, **kw):
    return pt.track_events(dev(cuda, people), dev(cuda, np.asarray(k, dtype=np.int64)), dev(cuda, prev), dev(cuda, gap),
                           dev(cuda, gates), dev(cuda, zones), **kw)


def subset(events, gates, zones):
    """events_spec's arrays for the first `gates` gates and `zones` zones of its tables."""
    gc, zc, fwd, bwd, zin = events
    mg, mz = np.int64((1 << gates) - 1), np.int64((1 << zones) - 1)
    return gc[:, :gates], zc[:, :zones], fwd & mg, bwd & mg, zin & mz


# ------------------------------------------------------------------ against the specification
@pytest.mark.parametrize("case", sref.GAPPY, ids=str)
@pytest.mark.parametrize("gate", sref.GATES)
@pytest.mark.parametrize("max_gap", [0, 1, 2])
def test_vs_spec(cuda, case, gate, max_gap):
    """cap = 43 (one row tile: the counters are stored), 303 and 2 103 (several: they are added), NaN and junk past
    K_t, the degenerate and the NaN gate in the table."""
    people, k = sref.gappy_sequence(*case)
    s = sref.gappy_spec(*case, gate, max_gap)
    gates, zones = eref.scene_tables(eref.lattice_side(case[1]))
    same(run(cuda, people, k, s["prev"], s["gap"], gates, zones), eref.gappy_events(*case, gate, max_gap))


@pytest.mark.parametrize("max_gap", [0, 1, 2])
def test_crossing_scene(cuda, max_gap):
    people, k, gates, zones = eref.crossing_scene()
    s, want = eref.crossing_spec(max_gap)
    same(run(cuda, people, k, s["prev"], s["gap"], gates, zones), want)


@pytest.mark.parametrize("case", sref.GAPPY[:2], ids=str)
def test_batch_form_without_gap(cuda, case):
    """gap = None on track_people's prev is gap from track_stream(max_gap = 0), and the specification's."""
    people, k = sref.gappy_sequence(*case)
    gates, zones = eref.scene_tables(eref.lattice_side(case[1]))
    pd, kd, gd, zd = dev(cuda, people), dev(cuda, k), dev(cuda, gates), dev(cuda, zones)
    prev = pt.track_people(pd, kd, ref.DT, 0.5)[0]
    sprev, sgap = pt.track_stream(pd, kd, ref.DT, 0.5, 0)[:2]
    a = pt.track_events(pd, kd, prev, None, gd, zd)
    b = pt.track_events(pd, kd, sprev, sgap, gd, zd)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    s = sref.gappy_spec(*case, 0.5, 0)
    want = eref.events_spec(people, k, s["prev"], None, gates, zones)
    same(a, want)
    same(want, eref.gappy_events(*case, 0.5, 0), "the specification with and without gap")


# ------------------------------------------------------------------ shapes
def scene(which):
    if which == "crossing":  # cap = 203: one row tile
        people, k, _, _ = eref.crossing_scene()
        return people, k, eref.crossing_spec()[0], eref.CROSSING["side"]
    case = sref.GAPPY[1]  # cap = 303: two row tiles
    return sref.gappy_sequence(*case) + (sref.gappy_spec(*case, 0.5, 2), eref.lattice_side(case[1]))


@pytest.mark.parametrize("which", ["crossing", "gappy"])
def test_64_gates_or_64_zones(cuda, which):
    people, k, s, side = scene(which)
    L, mid = side * ref.STEP, (side // 2) * ref.STEP
    x = np.linspace(0.05, L - 0.05, 64)
    gates = np.column_stack([x, np.full(64, -1.0), x + 0.3, np.full(64, L + 1.0)])
    gates[63] = (mid, -1.0, mid, L + 1.0)
    want = eref.events_spec(people, k, s["prev"], s["gap"], gates, None)
    assert (want[2] < 0).any() and (want[3] < 0).any()  # bit 63: the int64 sign
    assert np.count_nonzero(want[0].sum(axis=(0, 2))) >= 20  # the gates with crossings
    got = run(cuda, people, k, s["prev"], s["gap"], gates, None)
    same(got, want, "G = 64, Z = 0")
    assert tuple(got[1].shape) == (len(k), 0, 3) and got[4] is None
    assert (got[2] < 0).any() and np.array_equal(got[2].cpu().numpy() < 0, want[2] < 0)
    zones = np.column_stack([x - 0.3, x + 0.4, np.full(64, 0.1), np.linspace(0.5, L, 64)])
    zones[63] = (-1.0, L + 1.0, -1.0, L + 1.0)
    want = eref.events_spec(people, k, s["prev"], s["gap"], None, zones)
    K = ref.clamp_k(k, people.shape[1])
    assert all(np.all(want[4][t, :K[t]] < 0) for t in range(len(K)))  # everyone is in zone 63
    assert np.count_nonzero(want[1][:, :, 1].sum(axis=0)) >= 20 and np.count_nonzero(want[1][:, :, 2].sum(axis=0)) >= 20
    got = run(cuda, people, k, s["prev"], s["gap"], None, zones)
    same(got, want, "G = 0, Z = 64")
    assert tuple(got[0].shape) == (len(k), 0, 2) and got[2] is None and got[3] is None


@pytest.mark.parametrize("which", ["crossing", "gappy"])
def test_one_gate_and_one_zone(cuda, which):
    people, k, s, side = scene(which)
    gates, zones = eref.scene_tables(side)
    want = eref.events_spec(people, k, s["prev"], s["gap"], gates[1:2], zones[2:3])
    assert want[0].any() and want[1][:, :, 1:].any()
    same(run(cuda, people, k, s["prev"], s["gap"], gates[1:2], zones[2:3]), want)


def test_one_frame_and_one_row(cuda):
    people, k, s, side = scene("gappy")
    gates, zones = eref.scene_tables(side)
    # T = 1: no links
    p1, k1 = people[:1], k[:1]
    prev = np.full((1, people.shape[1]), -1, dtype=np.int32)
    gap = np.zeros_like(prev)
    want = eref.events_spec(p1, k1, prev, gap, gates, zones)
    assert not want[0].any() and not want[1][:, :, 1:].any() and want[1][0, 1, 0] == k[0]
    same(run(cuda, p1, k1, prev, gap, gates, zones), want, "T = 1")
    same(run(cuda, p1, k1, prev, None, gates, zones), want, "T = 1, no gap")
    # cap = 1: one walker back and forth over the gate, missing from frame 3 (gap 2 into frame 4), k = 0 there
    x = np.array([1.0, -1.0, 0.0, np.nan, 2.0, -0.5])
    pc = np.column_stack([x, np.full(6, 5.0)]).reshape(6, 1, 2)
    kc = np.array([1, 1, 1, 0, 1, 7])
    prevc = np.array([-1, 0, 0, 0, 0, 0], dtype=np.int32).reshape(6, 1)
    gapc = np.array([0, 1, 1, 1, 2, 1], dtype=np.int32).reshape(6, 1)
    g1, z1 = [(0.0, 0.0, 0.0, 10.0)], [(-2.0, 0.0, 0.0, 10.0)]
    want = eref.events_spec(pc, kc, prevc, gapc, g1, z1)
    assert want[0][:, 0].tolist() == [[0, 0], [1, 0], [0, 0], [0, 0], [0, 1], [1, 0]]
    assert want[1][:, 0].tolist() == [[0, 0, 0], [1, 1, 0], [0, 0, 1], [0, 0, 0], [0, 0, 0], [1, 1, 0]]
    same(run(cuda, pc, kc, prevc, gapc, g1, z1), want, "cap = 1")


def test_first_and_out(cuda):
    case = sref.GAPPY[1]
    people, k = sref.gappy_sequence(*case)
    T, cap, _ = people.shape
    s = sref.gappy_spec(*case, 0.5, 2)
    whole = eref.gappy_events(*case, 0.5, 2)
    gates, zones = eref.scene_tables(eref.lattice_side(case[1]))
    G, Z = len(gates), len(zones)

    def sentinels(n):
        return (torch.full((n, G, 2), 77, dtype=torch.int32, device=cuda), torch.full((n, Z, 3), 77, dtype=torch.int32, device=cuda),
                *(torch.full((n, cap), -77, dtype=torch.int64, device=cuda) for _ in range(3)))

    # first = 2: every element of out= is written, and they are the whole's frames from 2 on
    out = sentinels(T - 2)
    got = run(cuda, people, k, s["prev"], s["gap"], gates, zones, first=2, out=out)
    assert all(g is o for g, o in zip(got, out))
    same(got, tuple(a[2:] for a in whole), "first = 2")
    # first = T: nothing is written, by the wrapper ...
    empty = run(cuda, people, k, s["prev"], s["gap"], gates, zones, first=T)
    assert [tuple(t.shape) for t in empty] == [(0, G, 2), (0, Z, 3), (0, cap), (0, cap), (0, cap)]
    # ... and by the entry point, handed sentinel-filled arrays
    out = sentinels(T)
    pd, kd, prev, gap, gd, zd = (dev(cuda, a) for a in (people, k, s["prev"], s["gap"], gates, zones))
    nat.call("lidar_track_events_f64", nat.handle(cuda.index), nat.ptr(pd), nat.ptr(kd), nat.ptr(prev), nat.ptr(gap), T, cap,
             T, nat.ptr(gd), G, nat.ptr(zd), Z, *(nat.ptr(t) for t in out), nat.stream_ptr())
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, sentinels(T)))
    # the wrapper's own checks, and what the entry point rejects with a real handle
    for kw in (dict(first=-1), dict(first=T + 1), dict(first=1.5), dict(out=out[:4]), dict(out=sentinels(T - 1))):
        with pytest.raises(ValueError, match="track_events"):
            pt.track_events(pd, kd, prev, gap, gd, zd, **kw)
    with pytest.raises(ValueError, match="gates or zones"):
        pt.track_events(pd, kd, prev, gap)
    with pytest.raises(ValueError, match="gates"):
        pt.track_events(pd, kd, prev, gap, gd.float(), zd)
    with pytest.raises(ValueError, match="zones"):
        pt.track_events(pd, kd, prev, gap, gd, torch.zeros((65, 4), dtype=torch.float64, device=cuda))
    with pytest.raises(ValueError, match="gap"):
        pt.track_events(pd, kd, prev, gap.long(), gd, zd)
    with pytest.raises(ValueError, match="gate_fwd"):
        pt.track_events(pd, kd, prev, gap, None, zd, out=(None, None, out[2], None, None))
    with pytest.raises(nat.LidarError, match="lidar_track_events_f64: first"):
        nat.call("lidar_track_events_f64", nat.handle(cuda.index), nat.ptr(pd), nat.ptr(kd), nat.ptr(prev), nat.ptr(gap), T, cap,
                 T + 1, nat.ptr(gd), G, nat.ptr(zd), Z, *(nat.ptr(t) for t in out), nat.stream_ptr())
    same(run(cuda, people, k, s["prev"], s["gap"], gates, zones), whole, "after errors")


# ------------------------------------------------------------------ through the tracker
@pytest.mark.parametrize("case", sref.GAPPY, ids=str)
@pytest.mark.parametrize("max_gap", [0, 1, 2])
def test_split_equals_whole_through_the_tracker(cuda, case, max_gap):
    people, k = sref.gappy_sequence(*case)
    T, gate, grid = case[0], 0.25, 1.0
    s = sref.gappy_spec(*case, gate, max_gap)
    gates, zones = eref.scene_tables(eref.lattice_side(case[1]))
    gates = gates[:5]  # what check_gates accepts: without the degenerate and the NaN gate
    want = subset(eref.gappy_events(*case, gate, max_gap), 5, 3)
    assert want[0].any() and want[1][:, :, 1:].any()
    xr, yr = ref.extent_of(people, k)
    x0, y0, nx, ny, _, _ = ref.venue_grid(xr, yr, grid)
    wc, wv = sref.flow_cells_acc_spec(people, k, s["prev"], s["velocity"], x0, y0, grid, nx, ny, first=0)
    pd, kd = dev(cuda, people), dev(cuda, k)
    tracker = pt.PeopleTracker(ref.DT, gate, max_gap, xr, yr, grid, gates=gates, zones=zones)
    outs, events, lo = [], [], 0
    for n in pieces_of(T):
        outs.append(tracker.push(pd[lo:lo + n], kd[lo:lo + n]))
        assert all(t.shape[0] == n for t in tracker.last_events)
        events.append(tracker.last_events)
        lo += n
    same(tuple(torch.cat([e[i] for e in events]) for i in range(5)), want, "last_events")
    gt, zt = tracker.gate_total.cpu().numpy(), tracker.zone_total.cpu().numpy()
    assert gt.dtype == np.int64 and zt.dtype == np.int64
    assert np.array_equal(gt, want[0].sum(axis=0)) and np.array_equal(zt, want[1][:, :, 1:].sum(axis=0))
    # the tracker's outputs stay what they are without gates and zones
    prev, gap, tid, vel = (torch.cat([o[i] for o in outs]).cpu().numpy() for i in range(4))
    assert np.array_equal(prev, s["prev"]) and np.array_equal(gap, s["gap"])
    assert np.array_equal(tid, s["track_id"]) and vel.tobytes() == s["velocity"].tobytes()
    assert int(tracker.ntracks) == s["ntracks"] and int(tracker.matched) == int(np.sum(s["prev"] >= 0))
    assert np.array_equal(tracker.count.cpu().numpy(), wc) and tracker.vsum.cpu().numpy().tobytes() == wv.tobytes()


def test_tracker_with_one_kind_and_without(cuda):
    case = sref.GAPPY[0]
    people, k = sref.gappy_sequence(*case)
    gates, zones = eref.scene_tables(eref.lattice_side(case[1]))
    want = eref.gappy_events(*case, 0.5, 1)
    pd, kd = dev(cuda, people), dev(cuda, k)
    only_gates = pt.PeopleTracker(ref.DT, 0.5, 1, gates=gates[:5])
    only_zones = pt.PeopleTracker(ref.DT, 0.5, 1, zones=zones)
    plain = pt.PeopleTracker(ref.DT, 0.5, 1)
    for t in (only_gates, only_zones, plain):
        t.push(pd[:4], kd[:4])
        t.push(pd[4:4], kd[4:4])
        assert t.last_events is None or all(e is None or e.shape[0] == 0 for e in t.last_events)
        t.push(pd[4:], kd[4:])
    assert np.array_equal(only_gates.gate_total.cpu().numpy(), want[0][:, :5].sum(axis=0))
    assert tuple(only_gates.zone_total.shape) == (0, 2) and only_gates.last_events[4] is None
    assert np.array_equal(only_zones.zone_total.cpu().numpy(), want[1][:, :, 1:].sum(axis=0))
    assert tuple(only_zones.gate_total.shape) == (0, 2) and only_zones.last_events[2] is None
    assert np.array_equal(only_zones.last_events[4].cpu().numpy(), want[4][4:])
    assert plain.gate_total is None and plain.zone_total is None and plain.last_events is None


# ------------------------------------------------------------------ the model
EVENT_KEYS = {"gate_counts", "gate_series", "zone_occupancy", "zone_entries", "zone_exits", "gate_events",
              "zone_membership"}


def same_keys(got, want, K, frames, totals, what):
    """The model's gate and zone keys against events_spec's arrays `want` over the frames `frames`; the totals
    (gate (G, 2), entries (Z,), exits (Z,)) are given: a stream's cover more than the held frames."""
    gc, zc, fwd, bwd, zin = want
    for key, g, w in (("gate_counts", got["gate_counts"], totals[0]), ("zone_entries", got["zone_entries"], totals[1]),
                      ("zone_exits", got["zone_exits"], totals[2])):
        assert g.dtype == np.int64 and np.array_equal(g, w), f"{what}.{key}"
    assert got["gate_series"].dtype == np.int32 and np.array_equal(got["gate_series"], gc[frames]), what
    assert got["zone_occupancy"].dtype == np.int32 and np.array_equal(got["zone_occupancy"], zc[frames, :, 0]), what
    assert set(got["gate_events"]) == {"forward", "backward"}
    for name, g, w in (("forward", got["gate_events"]["forward"], fwd), ("backward", got["gate_events"]["backward"], bwd),
                       ("zone_membership", got["zone_membership"], zin)):
        assert len(g) == len(frames), f"{what}.{name}"
        for a, t in zip(g, frames):
            assert a.dtype == np.int64 and np.array_equal(a, w[t, :K[t]]), f"{what}.{name}[{t}]"


@pytest.mark.parametrize("case,gate,max_gap", [(sref.GAPPY[0], 0.25, 2), (sref.GAPPY[1], 0.5, 0), (sref.GAPPY[2], 0.25, 1)],
                         ids=str)
def test_analyze_sequence_and_stream(cuda, case, gate, max_gap):
    people, k = sref.gappy_sequence(*case)
    T, cap, _ = people.shape
    K = ref.clamp_k(k, cap)
    gates, zones = eref.scene_tables(eref.lattice_side(case[1]))
    gates = gates[:5]
    want = subset(eref.gappy_events(*case, gate, max_gap), 5, 3)
    totals = (want[0].sum(axis=0), want[1][:, :, 1].sum(axis=0), want[1][:, :, 2].sum(axis=0))
    assert totals[0].any() and totals[1].any() and totals[2].any()
    xr, yr = ref.extent_of(people, k)
    model = CrowdFlowModel()
    pd, kd = dev(cuda, people), dev(cuda, k)
    kw = dict(dt=ref.DT, x_range=xr, y_range=yr, gate=gate, max_gap=max_gap)
    plain = model.analyze_sequence(pd, kd, **kw)
    keys = {"flow_vectors", "avg_speed", "dominant_direction", "bottlenecks", "tracks", "matched", "observations",
            "track_ids", "velocities"} | ({"gaps"} if max_gap else set())
    assert set(plain) == keys  # without tables: exactly the keys it has without this feature
    got = model.analyze_sequence(pd, kd, gates=gates, zones=zones, **kw)
    assert set(got) == keys | EVENT_KEYS
    same_keys(got, want, K, range(T), totals, "sequence")
    for key in ("tracks", "matched"):
        assert got[key] == plain[key]
    for a, b in zip(got["track_ids"], plain["track_ids"]):
        assert np.array_equal(a, b)
    assert got["flow_vectors"]["vectors"].tobytes() == plain["flow_vectors"]["vectors"].tobytes()
    # the list-of-host-arrays form: cap = the largest K_t, zeros past K_t
    if case[1] <= 300:
        listed = model.analyze_sequence([people[t, :K[t]] for t in range(T)], gates=gates.tolist(), zones=zones, **kw)
        assert set(listed) == keys | EVENT_KEYS
        same_keys(listed, want, K, range(T), totals, "list")
    # one kind alone: the other is empty
    g_only = model.analyze_sequence(pd, kd, gates=gates, **kw)
    assert set(g_only) == keys | EVENT_KEYS and np.array_equal(g_only["gate_series"], want[0])
    assert g_only["zone_occupancy"].shape == (T, 0) and g_only["zone_entries"].shape == (0,)
    assert all(a.shape == (K[t],) and not a.any() for t, a in enumerate(g_only["zone_membership"]))
    # the same stream pushed in pieces: the totals of the whole, the arrays of the held frames
    tracker = pt.PeopleTracker(ref.DT, gate, max_gap, xr, yr, gates=gates, zones=zones)
    bare = pt.PeopleTracker(ref.DT, gate, max_gap, xr, yr)
    lo = 0
    for n in pieces_of(T):
        tracker.push(pd[lo:lo + n], kd[lo:lo + n])
        bare.push(pd[lo:lo + n], kd[lo:lo + n])
        lo += n
    res = model.analyze_stream(tracker)
    assert set(res) == keys | EVENT_KEYS | {"gaps"}
    assert set(model.analyze_stream(bare)) == keys | {"gaps"}
    same_keys(res, want, K, range(T - min(max_gap + 1, T), T), totals, "stream")
    assert res["tracks"] == got["tracks"] and res["matched"] == got["matched"]


def test_analyze_stream_on_an_empty_tracker(cuda):
    model = CrowdFlowModel()
    tracker = pt.PeopleTracker(ref.DT, 0.25, 1, (0.0, 4.0), (0.0, 4.0), gates=[(0, 0, 0, 1), (1, 0, 1, 1)])
    res = model.analyze_stream(tracker)
    assert res["gate_counts"].tolist() == [[0, 0], [0, 0]] and res["zone_entries"].shape == (0,)
    assert res["gate_series"].shape == (0, 2, 2) and res["zone_membership"] == [] and res["gate_events"] == {
        "forward": [], "backward": []}
