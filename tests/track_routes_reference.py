"""Host specification of ``lidar_track_routes_f64`` / ``people_tracking.track_routes`` (plain numpy and Python, row by
row in (t, j) order, DESIGN.md §3 "Routes"), the host construction of ``CrowdFlowModel``'s routes keys, the zone
tables of the scenes the tracking tests share (``track_stream_reference.GAPPY`` and
``track_events_reference.crossing_scene``) and cached specifications over them.

Integers only.  The link guard and the zone predicate are ``track_events_reference``'s; the heirs are
``track_history_reference``'s: among the rows of frames >= carry that are linked to the same source, the lowest in
(t, j) order continues the source's route; every other row starts one.  zone_of(p) is the lowest zone that holds p.
"""
import functools

import numpy as np

import track_stream_reference as sref
import track_events_reference as eref
from track_reference import STEP, clamp_k

NAMES = ("first_zone", "last_zone", "away", "legs", "leg_from", "leg_frames", "trips")
DTYPES = (np.int32,) * 6 + (np.int64,)
STATE = NAMES[:6]  # the arrays with T frames


def zone_of(zones, x, y):
    for z in range(len(zones)):
        if eref.inside(zones[z], x, y):
            return z
    return -1


def routes_spec(people, k, prev, gap, zones, carry=0, state=None, trips=None):
    """people (T, cap, 2), k (T,), prev (T, cap), gap (T, cap) or None, zones (Z, 4), 1 <= Z <= 64; state: dict of
    the six arrays whose first `carry` frames are given; trips (Z, Z, 3): what the count goes on from (None: zero)
    -> dict of NAMES' arrays, (T, cap) int32 and trips (Z, Z, 3) int64, and heirs, linked: the numbers of continuing
    and of linked rows among the frames >= carry."""
    people = np.asarray(people, dtype=np.float64)
    T, cap, _ = people.shape
    zones = np.asarray(zones, dtype=np.float64).reshape(-1, 4)
    Z, C = len(zones), int(carry)
    assert 1 <= Z <= eref.MAX_TABLE and 0 <= C <= T
    K = clamp_k(k, cap)
    out = {name: np.full((T, cap), fill, dtype=np.int32) for name, fill in zip(STATE, (-1, -1, -1, 0, -1, 0))}
    if C:
        for name in STATE:
            out[name][:C] = state[name][:C]
    first_zone, last_zone, away, legs, leg_from, leg_frames = (out[name] for name in STATE)
    trips = np.zeros((Z, Z, 3), dtype=np.int64) if trips is None else np.array(trips, dtype=np.int64)
    assert trips.shape == (Z, Z, 3)
    claimed = set()  # the sources that have their heir
    heirs = linked = 0
    for t in range(C, T):
        for j in range(K[t]):
            c = zone_of(zones, people[t, j, 0], people[t, j, 1])
            src = eref.link_of(people, K, prev, gap, t, j)
            linked += src is not None
            if src is None or src in claimed:  # starts
                first_zone[t, j] = last_zone[t, j] = c
                away[t, j] = 0 if c >= 0 else -1
                continue  # legs 0, leg_from -1, leg_frames 0
            claimed.add(src)  # (t, j) ascending: the first to name a source is its heir
            heirs += 1
            g = t - src[0]
            F, L, A, N = (int(a[src]) for a in (first_zone, last_zone, away, legs))
            if c < 0:
                first_zone[t, j], last_zone[t, j], legs[t, j] = F, L, N
                away[t, j] = A + g if L >= 0 else -1
                continue
            leg = L >= 0 and (L != c or A > 0)
            first_zone[t, j] = F if F >= 0 else c
            last_zone[t, j] = c
            away[t, j] = 0
            legs[t, j] = N + leg
            if leg:
                leg_from[t, j] = L
                leg_frames[t, j] = A + g
                if L < Z:  # a carried last_zone that is no zone of this table adds no trip
                    trips[L, c, 0] += 1
                    trips[L, c, 1] += A + g
                    trips[L, c, 2] = max(trips[L, c, 2], A + g)
    return {**out, "trips": trips, "heirs": heirs, "linked": linked}


def split_routes(people, k, prev, gap, zones, max_gap, cut):
    """The sequence's routes in two calls cut at frame `cut`: the head's last min(max_gap + 1, cut) frames are handed
    to the second call as its carry, and the head's trips as what it goes on from -> (head's dict over the frames
    < cut, second call's dict, c)."""
    c = min(max_gap + 1, cut)
    g = (lambda sl: None) if gap is None else (lambda sl: gap[sl])
    head = routes_spec(people[:cut], k[:cut], prev[:cut], g(slice(0, cut)), zones)
    sl = slice(cut - c, None)
    T = people.shape[0]
    state = {name: np.concatenate([head[name][cut - c:], np.full((T - cut,) + head[name].shape[1:], 77, dtype=np.int32)])
             for name in STATE}
    tail = routes_spec(people[sl], k[sl], prev[sl], g(sl), zones, c, state, head["trips"])
    return head, tail, c


def route_keys(track_id, r, K, trips, dt):
    """CrowdFlowModel's routes keys from host arrays over the frames read back: r, routes_spec's dict sliced to
    them; trips (Z, Z, 3), the whole stream's."""
    last = {}
    for t in range(len(K)):
        for j in range(int(K[t])):
            last[int(track_id[t, j])] = (t, j)
    ids = sorted(last)
    table = {"track_id": np.array(ids, dtype=np.int32)}
    for name in ("first_zone", "last_zone", "legs"):
        table[name] = np.array([r[name][last[i]] for i in ids], dtype=np.int32)
    Z = trips.shape[0]
    od = np.zeros((Z, Z), dtype=np.int64)
    for f, l in zip(table["first_zone"], table["last_zone"]):
        if f >= 0:
            od[f, l] += 1
    count, total = trips[:, :, 0], trips[:, :, 1]
    mean = np.full((Z, Z), np.nan)
    for a in range(Z):
        for b in range(Z):
            if count[a, b]:
                mean[a, b] = np.float64(dt) * total[a, b] / count[a, b]
    out = {key: [r[name][t, :K[t]] for t in range(len(K))] for key, name in (
        ("first_zones", "first_zone"), ("last_zones", "last_zone"), ("away", "away"), ("legs", "legs"),
        ("leg_from", "leg_from"), ("leg_frames", "leg_frames"))}
    out.update(zone_trips=count.astype(np.int64), zone_trip_frames=total.astype(np.int64),
               zone_trip_max=trips[:, :, 2].astype(np.int64), zone_trip_mean_s=mean, route_table=table, od_matrix=od)
    return out


ROUTE_KEYS = {"zone_trips", "zone_trip_frames", "zone_trip_max", "zone_trip_mean_s", "first_zones", "last_zones", "away",
              "legs", "leg_from", "leg_frames", "route_table", "od_matrix"}


# ------------------------------------------------------------------ the scenes' zone tables
def crossing_zones():
    """Eight zones for the crossing scene (96 nodes of 2^-3 m per axis, the middle at 6 m; the walkers start within
    2 m of it and drift 1 or 2 nodes per frame across it, y moving by -1 .. 1 nodes): 0 and 2, strips of 4 nodes in x
    left and right of the middle, and 1, a strip of 3 nodes across it, with 3 nodes between neighbours, so that a
    walker leaves one, is seen outside all of them and reaches the next within a few frames; the strips are cut in y
    at edges the walkers' y steps cross back and forth (a return); 3 lies against zone 0's outer edge and overlaps
    it (the overlap belongs to 0, and 0 <-> 3 are direct legs); 4 is 2's mirror for the walkers coming the other
    way; 5 holds everything right of them; 6 is a zone nobody enters; 7 is a NaN zone."""
    n = STEP
    return np.array([(41 * n, 45 * n, 0.0, 40.5 * n),
                     (48 * n, 51 * n, -1.0, 13.0),
                     (54 * n, 58 * n, 55.5 * n, 13.0),
                     (37 * n, 43 * n, -1.0, 13.0),
                     (54 * n, 58 * n, -1.0, 30.5 * n),
                     (61 * n, 80 * n, -1.0, 13.0),
                     (20.0, 21.0, 0.0, 12.0),
                     (np.nan, 1.0, 0.0, 1.0)], dtype=np.float64)


def gappy_zones(s):
    """Zones for a gappy sequence on the lattice of s nodes per axis (the walkers step -2 .. 2 nodes per axis and
    frame): min(s // 4, 60) strips in x, 2 nodes wide with 2 nodes between neighbours, cut in y above the middle;
    then a box in the lower left corner, three eighths of the side wide and high, which overlaps the strips and holds the nodes between them there; then everything
    from 2 nodes above the strips' upper edge as one zone."""
    L, mid = s * STEP, (s // 2) * STEP
    strips = [((4 * i) * STEP, (4 * i + 2) * STEP, -1.0, mid + 0.5 * STEP) for i in range(min(s // 4, 60))]
    return np.array(strips + [(0.0, 0.75 * mid, 0.0, 0.75 * mid), (-1.0, L + 1.0, mid + 2.5 * STEP, L + 1.0)], dtype=np.float64)


# ------------------------------------------------------------------ the scenes, cached and shared
def _frozen(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def gappy_routes(T, n, seed, gate, max_gap):
    """routes_spec of the gappy sequence's stream_spec under gappy_zones."""
    people, k = sref.gappy_sequence(T, n, seed)
    s = sref.gappy_spec(T, n, seed, gate, max_gap)
    return _frozen(routes_spec(people, k, s["prev"], s["gap"], gappy_zones(eref.lattice_side(n))))


@functools.lru_cache(maxsize=None)
def crossing_routes(max_gap=eref.CROSSING["max_gap"]):
    people, k, _, _ = eref.crossing_scene()
    s = eref.crossing_spec(max_gap)[0]
    return _frozen(routes_spec(people, k, s["prev"], s["gap"], crossing_zones()))


def kinds(r, people, k, prev, gap, zones):
    """How often each kind of row a comparison has to see occurs in the specification r of a scene: dict of counts."""
    T, cap = r["legs"].shape
    K = clamp_k(k, cap)
    off = back = far = waited = two = 0
    for t in range(T):
        for j in range(K[t]):
            if r["leg_from"][t, j] >= 0:
                src = eref.link_of(people, K, prev, gap, t, j)
                off += r["leg_from"][t, j] != r["last_zone"][t, j]
                back += r["leg_from"][t, j] == r["last_zone"][t, j]
                far += t - src[0] > 1
                waited += r["away"][src] > 0
            x, y = people[t, j]
            two += sum(eref.inside(z, x, y) for z in zones) >= 2
    live = np.arange(cap)[None, :] < K[:, None]
    return {"off_diagonal": int(off), "returns": int(back), "legs_over_a_gap": int(far), "legs_after_away": int(waited),
            "rows_with_two_legs": int(np.count_nonzero(r["legs"][live] >= 2)),
            "rows_first_differs_from_last": int(np.count_nonzero((r["first_zone"] != r["last_zone"])[live])),
            "positions_in_two_zones": int(two), "longest_trip": int(r["trips"][:, :, 2].max())}


def not_vacuous(r, people, k, prev, gap, zones, max_gap):
    """The conditions a scene's specification has to meet for a comparison against it to mean something -> the
    counts."""
    n = kinds(r, people, k, prev, gap, zones)
    assert r["heirs"] == r["linked"] > 0
    for name, count in n.items():
        if name == "legs_over_a_gap":
            assert count >= 1 or max_gap == 0, n  # max_gap = 0 links over one frame only
        elif name == "longest_trip":
            assert count > 1, n
        else:
            assert count >= 1, n
    return n
