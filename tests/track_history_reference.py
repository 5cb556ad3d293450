"""Host specification of ``lidar_track_history_f64`` / ``people_tracking.track_history`` (plain numpy loops, DESIGN.md
§3 "Track history"), the host construction of ``CrowdFlowModel``'s ``track_table``, and cached specifications over
the scenes the tracking tests share (``track_stream_reference.GAPPY`` with ``track_events_reference.scene_tables``,
and ``track_events_reference.crossing_scene``).

All arithmetic is float64 with one rounding per operation (numpy scalars); the link guard and the zone predicate
are ``track_events_reference``'s.  Among the rows of frames >= carry that are linked to the same source, the lowest
in (t, j) order is the heir and continues the source's history; every other row starts one.
"""
import functools

import numpy as np

import track_stream_reference as sref
import track_events_reference as eref
from track_reference import DT, clamp_k

NAMES = ("age", "hits", "path", "origin", "stay", "dwell")
DTYPES = (np.int32, np.int32, np.float64, np.float64, np.int32, np.int64)
STATE = NAMES[:5]  # the arrays with T frames; stay only with zones


def history_spec(people, k, prev, gap, zones, carry=0, state=None):
    """people (T, cap, 2), k (T,), prev (T, cap), gap (T, cap) or None, zones (Z, 4) or None (Z = 0); state: dict
    of the arrays age, hits, path, origin (and stay with zones) whose first `carry` frames are given ->
    dict of age, hits (T, cap) int32, path (T, cap), origin (T, cap, 2) float64, stay (T, cap, Z) int32,
    dwell (T - carry, Z, 3) int64 (stay and dwell None without zones), and heirs, linked: the numbers of
    continuing and of linked rows among the frames >= carry."""
    people = np.asarray(people, dtype=np.float64)
    T, cap, _ = people.shape
    zones = np.zeros((0, 4)) if zones is None else np.asarray(zones, dtype=np.float64).reshape(-1, 4)
    Z, C = len(zones), int(carry)
    assert Z <= eref.MAX_TABLE and 0 <= C <= T
    K = clamp_k(k, cap)
    age = np.full((T, cap), -1, dtype=np.int32)
    hits = np.zeros((T, cap), dtype=np.int32)
    path = np.zeros((T, cap), dtype=np.float64)
    origin = np.zeros((T, cap, 2), dtype=np.float64)
    stay = np.full((T, cap, Z), -1, dtype=np.int32)
    dwell = np.zeros((T - C, Z, 3), dtype=np.int64)
    if C:
        for name, a in (("age", age), ("hits", hits), ("path", path), ("origin", origin)) + ((("stay", stay),) if Z else ()):
            a[:C] = state[name][:C]
    claimed = set()  # the sources that have their heir
    heirs = linked = 0
    for t in range(C, T):
        for j in range(K[t]):
            Q = people[t, j]
            src = eref.link_of(people, K, prev, gap, t, j)
            linked += src is not None
            if src is not None and src not in claimed:  # (t, j) ascending: the first to name a source is its heir
                claimed.add(src)
                heirs += 1
                s, i = src
                g = t - s
                P = people[s, i]
                with np.errstate(all="ignore"):
                    dx, dy = Q[0] - P[0], Q[1] - P[1]
                    path[t, j] = path[s, i] + np.sqrt((dx * dx) + (dy * dy))
                age[t, j] = age[s, i] + g
                hits[t, j] = hits[s, i] + 1
                origin[t, j] = origin[s, i]
                for z in range(Z):
                    inq, was = eref.inside(zones[z], Q[0], Q[1]), int(stay[s, i, z])
                    stay[t, j, z] = (was + g if was >= 0 else 0) if inq else -1
                    if was >= 0 and not inq:
                        d = dwell[t - C, z]
                        d[0] += 1
                        d[1] += was
                        d[2] = max(d[2], was)
            else:
                age[t, j], hits[t, j], path[t, j] = 0, 1, 0.0
                origin[t, j] = Q
                for z in range(Z):
                    stay[t, j, z] = 0 if eref.inside(zones[z], Q[0], Q[1]) else -1
    return {"age": age, "hits": hits, "path": path, "origin": origin, "stay": stay if Z else None,
            "dwell": dwell if Z else None, "heirs": heirs, "linked": linked}


def split_history(people, k, prev, gap, zones, max_gap, cut):
    """The sequence's history in two calls cut at frame `cut`: the head's last min(max_gap + 1, cut) frames are
    handed to the second call as its carry -> (head's dict over frames < cut, second call's dict, c)."""
    c = min(max_gap + 1, cut)
    g = (lambda sl: None) if gap is None else (lambda sl: gap[sl])
    head = history_spec(people[:cut], k[:cut], prev[:cut], g(slice(0, cut)), zones)
    sl = slice(cut - c, None)
    T = people.shape[0]
    state = {}
    for name in STATE:
        if head[name] is not None:
            a = head[name][cut - c:]
            state[name] = np.concatenate([a, np.full((T - cut,) + a.shape[1:], 77, dtype=a.dtype)])
    tail = history_spec(people[sl], k[sl], prev[sl], g(sl), zones, c, state)
    return head, tail, c


def track_table(track_id, age, hits, path, origin, people, K, frames, dt):
    """CrowdFlowModel's track_table from host arrays over the frames read back (frames[r]: the frame number of
    row r of the arrays): per track id, ascending, its last row in (t, j) order."""
    last = {}
    for r in range(len(K)):
        for j in range(int(K[r])):
            last[int(track_id[r, j])] = (r, j)
    ids = sorted(last)
    rows = [last[i] for i in ids]
    r = np.array([a for a, _ in rows], dtype=np.int64)
    j = np.array([b for _, b in rows], dtype=np.int64)
    frames = np.asarray(frames, dtype=np.int64)
    a = age[r, j].astype(np.int64) if len(ids) else np.zeros(0, dtype=np.int64)
    last_frame = frames[r] if len(ids) else np.zeros(0, dtype=np.int64)
    if len(ids):
        d = people[r, j] - origin[r, j]
        disp = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
        pl = path[r, j]
        h = hits[r, j]
    else:
        disp, pl, h = np.zeros(0), np.zeros(0), np.zeros(0, dtype=np.int32)
    speed = np.zeros(len(ids), dtype=np.float64)
    moving = a > 0
    speed[moving] = pl[moving] / (a[moving] * np.float64(dt))
    return {"track_id": np.array(ids, dtype=np.int32), "first_frame": last_frame - a, "last_frame": last_frame,
            "hits": h.astype(np.int32), "path_length": pl.astype(np.float64), "displacement": disp, "mean_speed": speed}


# ------------------------------------------------------------------ the scenes, cached and shared
def _frozen(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def gappy_history(T, n, seed, gate, max_gap):
    """history_spec of the gappy sequence's stream_spec under scene_tables' three zones."""
    people, k = sref.gappy_sequence(T, n, seed)
    s = sref.gappy_spec(T, n, seed, gate, max_gap)
    zones = eref.scene_tables(eref.lattice_side(n))[1]
    return _frozen(history_spec(people, k, s["prev"], s["gap"], zones))


@functools.lru_cache(maxsize=None)
def crossing_history(max_gap=eref.CROSSING["max_gap"]):
    people, k, _, zones = eref.crossing_scene()
    s = eref.crossing_spec(max_gap)[0]
    return _frozen(history_spec(people, k, s["prev"], s["gap"], zones))


def not_vacuous(h, k, cap, max_gap, gap):
    """The conditions a scene's specification has to meet for a comparison against it to mean something."""
    T = len(k)
    K = clamp_k(k, cap)
    live = np.arange(cap)[None, :] < K[:, None]
    assert h["heirs"] == h["linked"] > 0
    if max_gap == 2:
        assert np.count_nonzero(gap[live] > 1) >= 20
    assert np.count_nonzero(h["stay"][live] >= 2) >= 100
    pos = h["path"][live]
    pos = pos[pos > 0]
    assert np.count_nonzero(pos * 2.0 ** 20 != np.floor(pos * 2.0 ** 20)) > len(pos) / 4  # sqrt's rounding shows
    assert h["age"][live].max() == T - 1 and h["hits"][live].max() == T
    assert h["dwell"][:, 1].sum() == 0  # zone 1 holds everyone: nobody leaves it
    assert h["dwell"][:, 2, 1].sum() > 0
