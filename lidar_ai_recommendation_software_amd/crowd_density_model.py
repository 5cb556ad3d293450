"""Drop-in for the reference's ``models/crowd_density_model.py`` on MI355X.

``CrowdDensityModel(grid_size=1.0).analyze(processed_data)`` returns the reference's
result dict (``models/crowd_density_model.py:23-98``) bit for bit: people positions,
density grid, statistics and hotspots come from the gfx950 kernels behind
``data_processing.extract_people_positions`` / ``lidar_density_grid_f64`` (the numpy
pairwise mean of the occupied cells and the stable top-5 ordering are restated on the
device).  The optional ``backbone`` ("ssg" / "msg") adds a PointNet++ global feature of
the frame, computed with ``backbone_weights`` when given (trained weights: the
nested [level][branch][layer] = (W, b) lists of ``pointnet2.init_weights``'s layout, or an ``.npz``
written by ``pointnet2.save_weights``) and with the deterministic random init otherwise; the result
says which (``backbone_weights``: "supplied" / "random-init").  The default ``None`` keeps the
reference behaviour exactly.

``segmenter`` (any object with ``segment(xyz (B, N, 3) float32 CUDA) -> (B, N) int32 CUDA``, such as
``pointnet2.PointNet2Segmenter``) adds ``analyze_frames``: people from the per-point labels of a trained
"person" class instead of the reference's heuristic chain (the points of ``person_class``, DBSCAN with
``cluster_eps`` metres on the unscaled coordinates, cluster centroids), then the reference's density
result.  ``analyze()`` does not use it.
"""
import numpy as np

from . import data_processing as dp
from . import density_abi as abi


class CrowdDensityModel:
    """Model for analyzing crowd density from LiDAR point cloud data."""

    def __init__(self, grid_size=1.0, backbone=None, backbone_weights=None, segmenter=None, person_class=1,
                 cluster_eps=0.3, min_samples=5):
        """grid_size as the reference (models/crowd_density_model.py:14-22); backbone None / "ssg" / "msg";
        backbone_weights: the backbone's weights (validated against its configuration here, so a
        mismatched set fails at construction), or None for the seed-0 random init.  segmenter: the
        per-point labeller of analyze_frames (None: analyze_frames raises); person_class: the label of a
        person's points; cluster_eps (metres; 0.3 is what the reference's standalone app clusters unscaled
        points with, app_simplified.py:107) and min_samples: the DBSCAN of those points."""
        if segmenter is not None and not callable(getattr(segmenter, "segment", None)):
            raise ValueError("segmenter must have a segment(xyz) method")
        if isinstance(person_class, bool) or not isinstance(person_class, (int, np.integer)):
            raise ValueError(f"person_class must be an integer, got {person_class!r}")
        if not (np.isfinite(cluster_eps) and cluster_eps > 0):
            raise ValueError(f"cluster_eps must be positive and finite, got {cluster_eps!r}")
        if isinstance(min_samples, bool) or not isinstance(min_samples, (int, np.integer)) or min_samples < 1:
            raise ValueError(f"min_samples must be an integer >= 1, got {min_samples!r}")
        self.grid_size = grid_size
        self.segmenter = segmenter
        self.person_class = int(person_class)
        self.cluster_eps = float(cluster_eps)
        self.min_samples = int(min_samples)
        self.backbone = backbone
        self._net = None
        self._weights = None
        if backbone_weights is not None:
            from . import pointnet2 as pn
            if backbone is None:
                raise ValueError("backbone_weights given without a backbone")
            cfg = pn.CONFIGS[backbone]
            if isinstance(backbone_weights, (str, bytes)) or hasattr(backbone_weights, "__fspath__"):
                self._weights = pn.load_weights(backbone_weights, cfg)
            else:
                self._weights = pn.check_weights(cfg, backbone_weights)

    def analyze(self, processed_data):
        people = dp.extract_people_positions(processed_data)
        if len(people) == 0:
            return abi.empty_result()
        dims = processed_data["dimensions"]
        rec = dp._grid(people, dims["x_range"], dims["y_range"], self.grid_size)
        res = abi.analyze_result(len(people), *rec[2:])
        if self.backbone is not None:
            res["backbone_feature"] = self.encode(processed_data["points"])
            res["backbone_weights"] = "supplied" if self._weights is not None else "random-init"
        return res

    def analyze_frames(self, frames):
        """frames (B, N, 3) array-like in metres -> a list of B result dicts.  Every frame is normalised
        as normalise() does and labelled by the segmenter; the points of person_class are clustered on
        their metric float32 coordinates (pointnet2.class_people) and the clusters' centroids are the
        people; the density grid spans the extent of the frame's finite points.  A frame without people
        gives the reference's empty result; the others analyze()'s keys plus "people_positions" (K, 2)
        float64.  One read-back of the counts and extents, one density launch for the whole batch."""
        if self.segmenter is None:
            raise ValueError("analyze_frames needs a segmenter (CrowdDensityModel(segmenter=...))")
        import torch
        from . import _native as nat
        from . import pointnet2 as pn
        frames = np.asarray(frames)
        if frames.ndim != 3 or frames.shape[2] != 3 or frames.shape[1] < 1:
            raise ValueError(f"analyze_frames: frames must be (B, N, 3) with N >= 1, got {frames.shape}")
        B, N, _ = frames.shape
        if B == 0:
            return []
        dev = torch.device("cuda", torch.cuda.current_device())
        unit = np.stack([self.normalise(f) for f in frames])
        metric = torch.from_numpy(np.array(frames, dtype=np.float32)).to(dev)
        labels = self.segmenter.segment(torch.from_numpy(unit).to(dev))
        _, people, kdev, _, extent = pn.class_people(metric, labels.contiguous(), self.person_class, self.cluster_eps,
                                                      self.min_samples)
        head = torch.cat([kdev.double()[:, None], extent], dim=1).cpu().numpy()  # the one read-back before the grid
        counts, ext = head[:, 0].astype(np.int64).tolist(), head[:, 1:]
        jobs = np.zeros((B, 8), dtype=np.float64)
        out_off = scr_off = 0
        dims = [None] * B
        for f in range(B):
            if counts[f] <= 0:
                continue
            x_min, x_max, y_min, y_max = ext[f]
            nx, ny = nat.grid_dims(x_min, x_max, y_min, y_max, self.grid_size)
            jobs[f] = abi.job_row(x_min, y_min, self.grid_size, nx, ny, out_off, scr_off)
            dims[f] = (nx, ny, out_off)
            out_off += abi.record_doubles(nx, ny, True)
            scr_off += abi.scratch_doubles(nx, ny)
        if out_off:
            offs = torch.arange(B + 1, dtype=torch.int64, device=dev) * N  # people rows of frame f: cap = N each
            jd = torch.from_numpy(jobs).to(dev)
            with nat.grid_alloc():
                out = torch.empty(out_off, dtype=torch.float64, device=dev)
            nat.call("lidar_density_batch_f64", nat.handle(dev.index), nat.ptr(people), nat.ptr(offs), nat.ptr(kdev), B,
                     nat.ptr(jd), nat.ptr(out), scr_off, nat.stream_ptr())
            ob = out.cpu().numpy()
            ph = people[:, :max(counts)].cpu().numpy()
        res = []
        for f in range(B):
            if dims[f] is None:
                res.append(abi.empty_result())
                continue
            nx, ny, off = dims[f]
            r = abi.analyze_result(counts[f], *abi.decode_record(ob, nx, ny, True, off)[2:])
            r["people_positions"] = ph[f, :counts[f]].copy()
            res.append(r)
        return res

    @staticmethod
    def normalise(points):
        """The backbone's input: the frame centred on its bounding box and scaled so that the
        box's longest side spans [-1, 1] (fp32; the SA radii 0.2 / 0.4 are in these units)."""
        p = np.asarray(points, dtype=np.float64)
        lo, hi = p.min(axis=0), p.max(axis=0)
        return ((p - (lo + hi) / 2) / max(float((hi - lo).max()) / 2, 1e-9)).astype(np.float32)

    def encode(self, points):
        """PointNet++ (SSG/MSG) global feature of one frame over ALL its points (1 <= N <= 4 194 304:
        the FPS kernel's limit, lidar_fps_ex_f32; frames above 262 144 points run it on buckets of
        64 x PPL points; a larger frame raises LidarError naming the limit).  SA levels take
        max(1, N/16) and max(1, N/64) centres.  Not part of the reference."""
        import torch
        from . import pointnet2 as pn
        if self._net is None:
            self._net = pn.PointNet2Backbone(pn.CONFIGS[self.backbone], weights=self._weights, device="cuda")
        unit = self.normalise(points)
        g, _ = self._net.forward(torch.from_numpy(np.ascontiguousarray(unit))[None].cuda())
        return g[0].cpu().numpy()

    def calculate_risk_level(self, density):
        """models/crowd_density_model.py:100-117."""
        if density < 1.0:
            return "Low"
        elif density < 2.5:
            return "Moderate"
        elif density < 4.0:
            return "High"
        else:
            return "Critical"
