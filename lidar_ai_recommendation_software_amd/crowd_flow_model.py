"""Drop-in for the reference's ``models/crowd_flow_model.py``.

``CrowdFlowModel().analyze(processed_data)`` returns the reference's dict — flow vectors on
the 1 m grid of the frame's extent, average speed, dominant direction and up to five
bottlenecks — bit for bit (``tests/test_flow.py``, ``tests/golden/flow.json`` captured from
the reference itself).  People positions come from the GPU path
(``data_processing.extract_people_positions``); the flow field and the bottleneck search run
in the library's native host code (``csrc/flow.hip``): every deciding operation there is a
glibc ``sin`` / ``cos`` / ``pow`` call or an sklearn KD-tree traversal that only the host C
library reproduces exactly, on a few thousand grid nodes.
"""
import ctypes

import numpy as np

from . import _native as nat
from .data_processing import extract_people_positions


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _read_back(named, device):
    """name -> device tensor or None  ->  name -> host ndarray, the None entries left out: every copy queued, then
    the one synchronise of analyze_sequence / analyze_stream."""
    import torch
    host = {name: t.to("cpu", non_blocking=True) for name, t in named.items() if t is not None}
    torch.cuda.current_stream(device).synchronize()
    return {name: t.numpy() for name, t in host.items()}


class CrowdFlowModel:
    """``models/crowd_flow_model.py:6-279``: same attributes, methods and outputs."""

    def __init__(self):
        self.prev_positions = None
        self.flow_vectors = None
        self.simulation_params = {
            "flow_field_complexity": 2,
            "bottleneck_count": 3,
            "flow_speed_range": (0.2, 1.5),
            "random_seed": 42,
        }

    def analyze(self, processed_data):
        """``crowd_flow_model.py:28-86``."""
        people_positions = extract_people_positions(processed_data)
        if len(people_positions) == 0:
            return {"flow_vectors": {"positions": np.zeros((0, 2)), "vectors": np.zeros((0, 2)),
                                     "magnitudes": np.zeros(0)},
                    "avg_speed": 0.0, "dominant_direction": "N/A", "bottlenecks": []}
        flow_vectors = self._generate_simulated_flow(people_positions, processed_data)
        magnitudes = flow_vectors["magnitudes"]
        vectors = flow_vectors["vectors"]
        avg_speed = np.mean(magnitudes)
        dominant_direction = self._dominant_direction(vectors)
        bottlenecks = self._identify_bottlenecks(flow_vectors, processed_data)
        return {"flow_vectors": flow_vectors, "avg_speed": avg_speed,
                "dominant_direction": dominant_direction, "bottlenecks": bottlenecks}

    @staticmethod
    def _track_keys(K, host, matched):
        """tracks, matched and the per-frame lists of both analyses over the frames K, from the host copies in `host`."""
        rows = range(len(K))
        out = {"tracks": int(host["ntracks"]), "matched": matched,
               "track_ids": [host["track_id"][t, :K[t]] for t in rows],
               "velocities": [host["velocity"][t, :K[t]] for t in rows]}
        if "gap" in host:
            out["gaps"] = [host["gap"][t, :K[t]] for t in rows]
        return out

    @staticmethod
    def _event_keys(K, host, gate_total, zone_total):
        """The gate and zone keys of analyze_sequence / analyze_stream from the host copies of the totals
        (G, 2) and (Z, 2) and, in `host` under track_events' names, of its arrays over the frames K (a mask that
        is missing: that kind is absent)."""
        rows = range(len(K))

        def sliced(name):
            return [np.zeros(K[t], dtype=np.int64) if name not in host else host[name][t, :K[t]] for t in rows]

        return {"gate_counts": gate_total.astype(np.int64), "gate_series": host["gate_counts"],
                "zone_occupancy": host["zone_counts"][:, :, 0], "zone_entries": zone_total[:, 0].astype(np.int64),
                "zone_exits": zone_total[:, 1].astype(np.int64),
                "gate_events": {"forward": sliced("gate_fwd"), "backward": sliced("gate_bwd")},
                "zone_membership": sliced("zone_in")}

    @staticmethod
    def _last_rows(track_id, K):
        """(ids, r, j): the tracks present among the live rows of track_id (n, cap) with K live rows per frame,
        ascending, and each one's last row in (t, j) order: the selection track_table and route_table share."""
        K = np.asarray(K, dtype=np.int64)
        live = np.arange(track_id.shape[1] if len(K) else 0)[None, :] < K[:, None]
        r, j = np.nonzero(live) if len(K) else (np.zeros(0, dtype=np.int64),) * 2  # (t, j) ascending
        ids, back = np.unique(track_id[r, j][::-1], return_index=True)  # the first from the back: the last row
        return ids, r[::-1][back], j[::-1][back]

    @classmethod
    def track_table(cls, track_id, age, hits, path, origin, people, K, frames, dt):
        """One entry per track present in the rows read back, from each track's last row in (t, j) order: host
        arrays (n, cap[, 2]) over n frames with K live rows each, frames (n,) their frame numbers -> dict of equally
        long arrays, ascending in track_id: track_id int32, first_frame = last_frame - age and last_frame int64,
        hits int32, path_length, displacement (|last position - origin|) and mean_speed (path_length / (age * dt),
        0.0 where age is 0) float64."""
        ids, r, j = cls._last_rows(track_id, K)
        a = age[r, j].astype(np.int64)
        last_frame = np.asarray(frames, dtype=np.int64)[r]
        d = people[r, j] - origin[r, j]
        path_length = path[r, j].astype(np.float64)
        speed = np.zeros(len(ids), dtype=np.float64)
        moving = a > 0
        speed[moving] = path_length[moving] / (a[moving] * np.float64(dt))
        return {"track_id": ids.astype(np.int32), "first_frame": last_frame - a, "last_frame": last_frame,
                "hits": hits[r, j].astype(np.int32), "path_length": path_length,
                "displacement": np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]), "mean_speed": speed}

    @classmethod
    def _history_keys(cls, K, frames, host, dwell_total, dt):
        """The history keys of analyze_sequence / analyze_stream from host copies: in `host`, under their names,
        people, track_id and track_history's age, hits, path, origin and (with zones) stay over the frames K,
        numbered `frames`; dwell_total (Z, 3) or None."""
        age, hits, path, origin = (host[name] for name in ("age", "hits", "path", "origin"))
        rows = range(len(K))
        out = {"ages": [age[t, :K[t]] for t in rows], "hits": [hits[t, :K[t]] for t in rows],
               "path_lengths": [path[t, :K[t]] for t in rows], "origins": [origin[t, :K[t]] for t in rows],
               "track_table": cls.track_table(host["track_id"], age, hits, path, origin, host["people"], K, frames,
                                              dt)}
        if dwell_total is not None:
            count, total = dwell_total[:, 0].astype(np.int64), dwell_total[:, 1].astype(np.int64)
            with np.errstate(all="ignore"):
                mean = np.where(count > 0, np.float64(dt) * total / count, np.nan)
            out.update({"zone_stays": [host["stay"][t, :K[t]] for t in rows], "zone_dwell_count": count,
                        "zone_dwell_frames": total, "zone_dwell_max": dwell_total[:, 2].astype(np.int64),
                        "zone_dwell_mean_s": mean})
        return out

    @classmethod
    def route_table(cls, track_id, first_zone, last_zone, legs, K):
        """One entry per track present in the rows read back, from each track's last row in (t, j) order
        (track_table's selection): host arrays (n, cap) over n frames with K live rows each -> dict of equally long
        int32 arrays, ascending in track_id: track_id, first_zone, last_zone (-1: never in a zone) and legs."""
        ids, r, j = cls._last_rows(track_id, K)
        return {"track_id": ids.astype(np.int32), "first_zone": first_zone[r, j].astype(np.int32),
                "last_zone": last_zone[r, j].astype(np.int32), "legs": legs[r, j].astype(np.int32)}

    @classmethod
    def _route_keys(cls, K, host, trips, dt):
        """The routes keys of analyze_sequence / analyze_stream from host copies: in `host`, under their names,
        track_id and track_routes' six arrays over the frames K; trips (Z, Z, 3): the whole stream's."""
        rows = range(len(K))
        count, total = trips[:, :, 0].astype(np.int64), trips[:, :, 1].astype(np.int64)
        with np.errstate(all="ignore"):
            mean = np.where(count > 0, np.float64(dt) * total / count, np.nan)
        table = cls.route_table(host["track_id"], host["first_zone"], host["last_zone"], host["legs"], K)
        Z = trips.shape[0]
        od = np.zeros((Z, Z), dtype=np.int64)
        first, last = table["first_zone"], table["last_zone"]
        seen = (first >= 0) & (first < Z) & (last >= 0) & (last < Z)  # a track that was never in a zone is left out
        np.add.at(od, (first[seen], last[seen]), 1)
        out = {key: [host[name][t, :K[t]] for t in rows] for key, name in (
            ("first_zones", "first_zone"), ("last_zones", "last_zone"), ("away", "away"), ("legs", "legs"),
            ("leg_from", "leg_from"), ("leg_frames", "leg_frames"))}
        out.update({"zone_trips": count, "zone_trip_frames": total, "zone_trip_max": trips[:, :, 2].astype(np.int64),
                    "zone_trip_mean_s": mean, "route_table": table, "od_matrix": od})
        return out

    RISK_LEVELS = ("Low", "Moderate", "High", "Critical")  # calculate_risk_level's classes, risk_levels' columns

    @classmethod
    def _crowding_keys(cls, K, host, crowded_total, peak_total):
        """The crowding keys of analyze_sequence / analyze_stream from host copies: in `host`, under their names,
        people and track_crowding's nine per-row and per-frame arrays over the frames K, and the two cell arrays of
        the venue grid; crowded_total (2,) and peak_total (3,) of the whole stream."""
        from .crowd_density_model import CrowdDensityModel

        rows = range(len(K))
        level = CrowdDensityModel().calculate_risk_level
        risk = np.zeros((len(K), len(cls.RISK_LEVELS)), dtype=np.int64)
        for t in rows:
            valid = np.isfinite(host["people"][t, :K[t]]).all(axis=1)
            for d in host["density"][t, :K[t]][valid]:
                risk[t, cls.RISK_LEVELS.index(level(d))] += 1
        out = {key: [host[name][t, :K[t]] for t in rows] for key, name in (
            ("neighbours", "neighbours"), ("nearest", "nearest"), ("spacings", "spacing"),
            ("local_density", "density"), ("velocity_variance", "variance"), ("pressure", "pressure"))}
        out.update({"crowded_series": host["crowded"], "peak_series": host["peaks"],
                    "crowded_total": crowded_total.astype(np.int64), "peak_density": float(peak_total[0]),
                    "peak_pressure": float(peak_total[1]), "min_spacing": float(peak_total[2]),
                    "crowd_peak_cells": {"density": host["cell_peak"][:, :, 0], "pressure": host["cell_peak"][:, :, 1]},
                    "crowded_cells": host["cell_crowded"], "risk_levels": risk})
        return out

    def analyze_sequence(self, people, k=None, *, dt, x_range, y_range, gate=None, max_speed=3.0, grid_size=1.0,
                         min_observations=1, max_gap=0, gates=None, zones=None, history=False, crowding=None,
                         density_limit=4.0, pressure_limit=0.02, routes=False):
        """Measured flow of T consecutive frames (no reference counterpart: its flow field is simulated).

        people: the device tensor (T, cap, 2) float64 with k (T,) int64 (``pointnet2.class_people``'s outputs),
        or a list of T host arrays (K_t, 2) (``analyze_frames``' ``"people_positions"``).  dt: seconds between
        frames; gate: the largest displacement accepted between two frames, metres (default max_speed * dt);
        x_range / y_range: the venue's extent, whose ``VenueGrid`` grid the flow lives on.  People are
        associated across frames by mutual nearest neighbour and every matched detection's velocity added into
        the cell of its position (``people_tracking``; csrc/track.hip), with one read-back at the end.

        Returns ``analyze``'s keys — flow_vectors (positions: the centres of the cells with at least
        min_observations matched detections, y index outer and x index inner as the reference's meshgrid ravel;
        vectors: the cells' mean velocity; magnitudes), avg_speed, dominant_direction, bottlenecks — and tracks
        (identities seen), matched (detections with a measured velocity), observations (m,) int32 per position,
        track_ids / velocities: per frame (K_t,) int32 and (K_t, 2) float64.

        max_gap > 0 (at most 7) stitches a track over that many consecutive frames without a detection
        (``people_tracking.track_stream``, DESIGN.md §3 "Continuous people tracking"): a detection is also
        associated with the open detections up to max_gap + 1 frames back, and its velocity is the displacement
        over that many dt.  The result then also holds gaps: per frame (K_t,) int32, the frame distance to each
        row's predecessor (0: none).

        gates (G, 4) rows (ax, ay, bx, by) and / or zones (Z, 4) rows (x0, x1, y0, y1), array-likes as
        ``people_tracking.check_gates`` / ``check_zones`` take them (at most 64 each): the tracks' crossings of
        the gate lines and their presence in the zones (``people_tracking.track_events``, DESIGN.md §3 "Gate and
        zone events"), in the same read-back.  The result then also holds gate_counts (G, 2) int64, the forward
        and backward crossings (forward: from the right of A -> B to its left); gate_series (T, G, 2) int32 per
        frame; zone_occupancy (T, Z) int32; zone_entries / zone_exits (Z,) int64; gate_events {"forward",
        "backward"} and zone_membership: per frame (K_t,) int64, bit g / z set for the gates the row crossed
        and the zones that hold it.  An absent kind has G or Z = 0 and zero masks.

        history=True adds every track's history (``people_tracking.track_history``, DESIGN.md §3 "Track history"),
        in the same read-back: ages and hits, per frame (K_t,) int32 (frames since the track's first detection,
        detections so far); path_lengths per frame (K_t,) float64 and origins per frame (K_t, 2) (metres walked,
        the first detection's position); track_table, ``track_table``'s dict with one entry per track, ids
        0 .. tracks - 1, frames counted from 0.  With zones also zone_stays, per frame (K_t, Z) int32 (frames since
        the row's present stay in the zone began, -1 outside); zone_dwell_count, zone_dwell_frames and
        zone_dwell_max (Z,) int64 (the completed stays, their summed and largest length in frames) and
        zone_dwell_mean_s (Z,) float64 = dt * frames / count, NaN without a completed stay.

        crowding=R, a radius in metres, adds how tightly packed every person is and how coherently the people around
        it move (``people_tracking.track_crowding``, DESIGN.md §3 "Crowding"), in the same read-back: neighbours and
        nearest per frame (K_t,) int32 (the people within R, the row of the closest person of the frame or -1);
        spacings, local_density, velocity_variance and pressure per frame (K_t,) float64 (metres to the nearest
        person, (neighbours + 1) / (pi R^2) people per m^2, the variance of the measured velocities of the person and
        its neighbours, and their product, the crowd pressure of Helbing et al. 2007); crowded_series (T, 2) int32
        (the people at or above density_limit, at or above pressure_limit) and peak_series (T, 3) float64 (largest
        density, largest pressure, smallest spacing) per frame; crowded_total (2,) int64, peak_density,
        peak_pressure and min_spacing over the sequence; crowd_peak_cells {"density", "pressure"} (nx, ny) float64 and
        crowded_cells (nx, ny) int32 on the venue grid; risk_levels (T, 4) int64, the people of each frame in
        ``CrowdDensityModel.calculate_risk_level``'s classes Low / Moderate / High / Critical of their local
        density.  density_limit 4.0 people per m^2 is that function's "Critical" edge and pressure_limit 0.02 1/s^2
        the turbulence level Helbing et al. report: defaults to override per venue, not measurements.

        routes=True (needs zones) adds where people go next (``people_tracking.track_routes``, DESIGN.md §3
        "Routes"), in the same read-back; a position belongs to the lowest zone that holds it.  zone_trips,
        zone_trip_frames and zone_trip_max (Z, Z) int64, indexed [from][to]: the legs of the sequence (an arrival in
        a zone from another one, or a return into the same one after a detection outside every zone, on the
        diagonal), their summed and their longest length in frames; zone_trip_mean_s (Z, Z) float64 =
        dt * frames / count, NaN without a trip; first_zones, last_zones, away, legs, leg_from and leg_frames: per
        frame (K_t,) int32 (the first zone of the row's track and the zone it was last seen in, -1 for none; the
        frames since; the legs so far; on a row that completes a leg the zone left and the frames it took, -1 and 0
        otherwise); route_table, ``route_table``'s dict with one entry per track of the sequence; od_matrix (Z, Z)
        int64, route_table's tracks counted by [first_zone][last_zone], those never in a zone left out."""
        import torch
        from . import people_tracking as pt

        def extent(name, r):
            r = tuple(float(v) for v in r)
            if len(r) != 2 or not np.all(np.isfinite(r)) or r[0] > r[1]:
                raise ValueError(f"analyze_sequence: {name} must be a finite (min, max) with min <= max, got {r}")
            return r

        what = "analyze_sequence"  # people_tracking's checks and messages, under this name
        dt = pt._positive(what, "dt", dt)
        gate = pt._positive(what, "gate", float(max_speed) * dt if gate is None else gate)
        grid_size = pt._positive(what, "grid_size", grid_size)
        x_range, y_range = extent("x_range", x_range), extent("y_range", y_range)
        if int(min_observations) != min_observations or min_observations < 1:
            raise ValueError(f"analyze_sequence: min_observations must be an integer >= 1, got {min_observations}")
        max_gap = pt._integer(what, "max_gap", max_gap, pt.MAX_GAP)
        gates = None if gates is None else pt.check_gates(gates)
        zones = None if zones is None else pt.check_zones(zones)
        if routes and zones is None:
            raise ValueError("analyze_sequence: routes need zones")
        if crowding is not None:
            crowding = pt._crowding_options(what, {"radius": crowding, "density_limit": density_limit,
                                                   "pressure_limit": pressure_limit})
        if isinstance(people, torch.Tensor):
            if k is None:
                raise ValueError("analyze_sequence: a people tensor needs k")
        else:
            if k is not None:
                raise ValueError("analyze_sequence: k goes with a people tensor; a list carries its own counts")
            rows = [np.asarray(p, dtype=np.float64) for p in people]
            for t, p in enumerate(rows):
                if p.ndim != 2 or p.shape[1] != 2:
                    raise ValueError(f"analyze_sequence: frame {t} must be (K, 2), got {p.shape}")
            packed = np.zeros((len(rows), max([1] + [len(p) for p in rows]), 2), dtype=np.float64)
            for t, p in enumerate(rows):
                packed[t, :len(p)] = p
            people = torch.from_numpy(packed).cuda()
            k = torch.tensor([len(p) for p in rows], dtype=torch.int64).to(people.device)

        if max_gap == 0:
            prev, track_id, velocity, ntracks = pt.track_people(people, k, dt, gate)
            gap = None
        else:
            prev, gap, _, velocity, track_id, ntracks = pt.track_stream(people, k, dt, gate, max_gap)
        count, vsum, _ = pt.flow_cells(people, k, prev, velocity, x_range, y_range, grid_size)
        named = {"k": k, "prev": prev, "gap": gap, "track_id": track_id, "velocity": velocity, "ntracks": ntracks,
                 "count": count, "vsum": vsum}
        tables = [None, None]
        if gates is not None or zones is not None:
            tables = [None if t is None else torch.from_numpy(t).to(people.device) for t in (gates, zones)]
            named.update(zip(pt.EVENTS, pt.track_events(people, k, prev, gap, *tables)))
        if history:
            named["people"] = people
            named.update(zip([name for name, _, _ in pt.HISTORY] + ["stay", "dwell"],
                             pt.track_history(people, k, prev, gap, tables[1])))
        if routes:
            named.update(zip(pt.ROUTES + ("trips",), pt.track_routes(people, k, prev, gap, tables[1])))
        if crowding is not None:
            named["people"] = people
            named.update(zip(pt.CROWDING, pt.track_crowding(people, k, prev, velocity, crowding[0], *crowding[1],
                                                            x_range, y_range, grid_size)))
        host = _read_back(named, people.device)  # the one read-back
        K = np.minimum(np.maximum(host["k"], 0), people.shape[1])
        extras = self._track_keys(K, host, int(np.sum(host["prev"] >= 0)))
        if "gate_counts" in host:
            extras.update(self._event_keys(K, host, host["gate_counts"].sum(axis=0),
                                           host["zone_counts"][:, :, 1:].sum(axis=0)))
        if history:
            dwell = host.get("dwell")
            total = None if dwell is None else np.concatenate(
                [dwell[:, :, :2].sum(axis=0), dwell[:, :, 2].max(axis=0, initial=0)[:, None]], axis=1)
            extras.update(self._history_keys(K, np.arange(len(K)), host, total, dt))
        if routes:
            extras.update(self._route_keys(K, host, host["trips"], dt))
        if crowding is not None:
            peaks = host["peaks"]
            extras.update(self._crowding_keys(K, host, host["crowded"].sum(axis=0), np.array(
                [peaks[:, 0].max(initial=0.0), peaks[:, 1].max(initial=0.0), peaks[:, 2].min(initial=np.inf)])))
        return self._measured_flow(host["count"], host["vsum"], x_range, y_range, grid_size, min_observations, extras)

    def analyze_stream(self, tracker, min_observations=1):
        """Measured flow of everything pushed into a ``people_tracking.PeopleTracker`` that was given a venue
        extent: ``analyze_sequence``'s keys (``gaps`` included) from the tracker's accumulated cells, with one
        read-back.  tracks / matched count the whole stream; track_ids / velocities / gaps are per frame for
        the frames the tracker still holds, its last min(max_gap + 1, frames) ones (the rows of earlier frames
        were returned by ``push``).  A tracker built with gates / zones adds ``analyze_sequence``'s gate and zone
        keys, in the same read-back: gate_counts, zone_entries and zone_exits total the whole stream;
        gate_series, zone_occupancy, gate_events and zone_membership cover the held frames.  A tracker built with
        history=True adds ``analyze_sequence``'s history keys, in the same read-back: the per-frame lists cover the
        held frames, track_table the tracks present in them (frames counted from the first pushed frame), and the
        zone_dwell keys total the whole stream.  A tracker built with crowding adds ``analyze_sequence``'s crowding
        keys, in the same read-back: the per-frame lists, crowded_series, peak_series and risk_levels cover the held
        frames; crowded_total, peak_density, peak_pressure, min_spacing and the two cell maps the whole stream.  A
        tracker built with routes=True adds ``analyze_sequence``'s routes keys, in the same read-back: the per-frame
        lists cover the held frames, route_table and od_matrix the tracks present in them, and the zone_trip keys
        total the whole stream."""
        import torch

        if int(min_observations) != min_observations or min_observations < 1:
            raise ValueError(f"analyze_stream: min_observations must be an integer >= 1, got {min_observations}")
        if tracker.grid is None:
            raise ValueError("analyze_stream: the tracker was built without x_range / y_range: it holds no flow cells")
        if tracker.frames == 0:  # nothing to read back: the held arrays without a frame, and zero totals
            host = {name: torch.empty(shape, dtype=dtype).numpy() for name, dtype, shape in tracker.layout(0)}
            host.update(ntracks=0, matched=0, gate_total=np.zeros((tracker.G, 2), dtype=np.int64),
                        zone_total=np.zeros((tracker.Z, 2), dtype=np.int64))
            if tracker.history and tracker.Z:
                host["dwell_total"] = np.zeros((tracker.Z, 3), dtype=np.int64)
            if tracker.routes:
                host["trips_total"] = np.zeros((tracker.Z, tracker.Z, 3), dtype=np.int64)
            if tracker.crowding:
                host.update(crowded_total=np.zeros(2, dtype=np.int64), peak_total=np.array([0.0, 0.0, np.inf]),
                            cell_peak=np.zeros(tracker.grid[2:] + (2,)),
                            cell_crowded=np.zeros(tracker.grid[2:], dtype=np.int32))
        else:
            held = tracker.held()
            for name in ("prev", "succ") + (() if tracker.history or tracker.crowding else ("people",)):
                del held[name]  # no key needs them (the positions: only the history and crowding keys)
            host = _read_back({**held, "ntracks": tracker.ntracks, "matched": tracker.matched, "count": tracker.count,
                               "vsum": tracker.vsum, "gate_total": tracker.gate_total,
                               "zone_total": tracker.zone_total, "dwell_total": tracker.dwell_total,
                               "trips_total": tracker.trips_total,
                               "crowded_total": tracker.crowded_total, "peak_total": tracker.peak_total,
                               "cell_peak": tracker.cell_peak, "cell_crowded": tracker.cell_crowded},
                              tracker.ntracks.device)  # the one read-back
        K = np.minimum(np.maximum(host["k"], 0), tracker.cap or 1)
        extras = self._track_keys(K, host, int(host["matched"]))
        if tracker.events:
            extras.update(self._event_keys(K, host, host["gate_total"], host["zone_total"]))
        if tracker.history:
            extras.update(self._history_keys(K, np.arange(tracker.frames - len(K), tracker.frames), host,
                                             host.get("dwell_total"), tracker.dt))
        if tracker.routes:
            extras.update(self._route_keys(K, host, host["trips_total"], tracker.dt))
        if tracker.crowding:
            extras.update(self._crowding_keys(K, host, host["crowded_total"], host["peak_total"]))
        return self._measured_flow(host.get("count"), host.get("vsum"), tracker.x_range, tracker.y_range,
                                   tracker.grid_size, min_observations, extras)

    def _measured_flow(self, count, vsum, x_range, y_range, grid_size, min_observations, extras):
        """analyze's keys from the flow cells (count, vsum) on the host."""
        from .global_density import venue_centres

        if extras["matched"] == 0:
            return {"flow_vectors": {"positions": np.zeros((0, 2)), "vectors": np.zeros((0, 2)),
                                     "magnitudes": np.zeros(0)},
                    "avg_speed": 0.0, "dominant_direction": "N/A", "bottlenecks": [],
                    "observations": np.zeros(0, dtype=np.int32), **extras}
        grid_x, grid_y = venue_centres(x_range, y_range, grid_size)  # VenueGrid.centres()
        iy, ix = np.nonzero(count.T >= min_observations)  # y index outer, x index inner
        observations = count[ix, iy]
        vectors = vsum[ix, iy] / observations[:, None]
        vx, vy = vectors[:, 0], vectors[:, 1]
        flow_vectors = {"positions": np.column_stack([grid_x[ix], grid_y[iy]]).reshape(-1, 2), "vectors": vectors,
                        "magnitudes": np.sqrt(vx * vx + vy * vy)}
        if len(observations) == 0:  # matched, but no cell reaches min_observations
            avg_speed = 0.0
        else:
            avg_speed = np.mean(flow_vectors["magnitudes"])
        return {"flow_vectors": flow_vectors, "avg_speed": avg_speed,
                "dominant_direction": self._dominant_direction(vectors),
                "bottlenecks": self._identify_bottlenecks(flow_vectors, None),
                "observations": observations.astype(np.int32), **extras}

    @staticmethod
    def _dominant_direction(vectors):
        """``crowd_flow_model.py:66-79``: the compass octant of the mean vector."""
        if len(vectors) > 0:  # the reference's scalar epilogue, same numpy calls
            avg_vector = np.mean(vectors, axis=0)
            angle = np.arctan2(avg_vector[1], avg_vector[0]) * 180 / np.pi
            directions = ["E", "NE", "N", "NW", "W", "SW", "S", "SE", "E"]
            return directions[int((angle + 22.5) % 360 / 45)]
        return "N/A"

    def _generate_simulated_flow(self, people_positions, processed_data):
        """``crowd_flow_model.py:88-184``.  Seeds and draws the GLOBAL legacy NumPy RNG
        exactly as the reference does (seed 42, then two uniforms per bottleneck)."""
        np.random.seed(self.simulation_params["random_seed"])
        x_range = processed_data["dimensions"]["x_range"]
        y_range = processed_data["dimensions"]["y_range"]
        grid_size = 1.0
        x_grid = np.ascontiguousarray(np.arange(x_range[0], x_range[1] + grid_size, grid_size), dtype=np.float64)
        y_grid = np.ascontiguousarray(np.arange(y_range[0], y_range[1] + grid_size, grid_size), dtype=np.float64)
        exit_x = x_range[1]
        exit_y = (y_range[0] + y_range[1]) / 2
        nb = self.simulation_params["bottleneck_count"]
        bn = np.empty((nb, 2), dtype=np.float64)
        for k in range(nb):
            bn[k, 0] = np.random.uniform(x_range[0] + 1, x_range[1] - 1)
            bn[k, 1] = np.random.uniform(y_range[0] + 1, y_range[1] - 1)
        m = len(x_grid) * len(y_grid)
        positions = np.empty((m, 2), dtype=np.float64)
        vectors = np.empty((m, 2), dtype=np.float64)
        magnitudes = np.empty(m, dtype=np.float64)
        lo, hi = self.simulation_params["flow_speed_range"]
        nat.check(nat.load_library().lidar_flow_field_f64(
            _p(x_grid), len(x_grid), _p(y_grid), len(y_grid), float(exit_x), float(exit_y),
            int(self.simulation_params["flow_field_complexity"]), _p(bn), nb, float(lo), float(hi),
            _p(positions), _p(vectors), _p(magnitudes)), "lidar_flow_field_f64")
        return {"positions": positions, "vectors": vectors, "magnitudes": magnitudes}

    def _identify_bottlenecks(self, flow_vectors, processed_data):
        """``crowd_flow_model.py:186-279``: nodes slower than 0.5 m/s with >= 5 neighbours
        within 3 m and >= 3 more within 5 m; severity from the speed gradient and the flow
        convergence; top 5 by severity (stable)."""
        positions = np.ascontiguousarray(flow_vectors["positions"], dtype=np.float64)
        vectors = np.ascontiguousarray(flow_vectors["vectors"], dtype=np.float64)
        magnitudes = np.ascontiguousarray(flow_vectors["magnitudes"], dtype=np.float64)
        m = len(positions)
        if m == 0:
            return []
        cap = m
        ox, oy = np.empty(cap), np.empty(cap)
        osev = np.empty(cap, dtype=np.int64)
        n = nat.I64(0)
        nat.check(nat.load_library().lidar_flow_bottlenecks_f64(
            _p(positions), _p(vectors), _p(magnitudes), m, 0.5, 3.0, 5.0, 5, 3, _p(ox), _p(oy), _p(osev), None,
            cap, ctypes.byref(n)), "lidar_flow_bottlenecks_f64")
        n = n.value
        cand = [{"x": positions[0, 0].dtype.type(ox[i]), "y": positions[0, 0].dtype.type(oy[i]),
                 "severity": int(osev[i])} for i in range(n)]
        return sorted(cand, key=lambda b: b["severity"], reverse=True)[:5]
