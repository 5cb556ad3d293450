"""Throughput executor for the reference density path (Tier R) on device-resident frames.

The drop-in API (``data_processing`` + ``CrowdDensityModel``) takes and returns host
NumPy arrays, one frame at a time, exactly like the reference.  A LiDAR feed wants
frames already in HBM and many of them in flight: the per-frame chain (preprocess ->
DBSCAN -> people -> density grid, ``utils/data_processing.py:127-328`` +
``models/crowd_density_model.py:23-98``) has three small host read-backs (the scalars
that size the next step, K, the grid), so one frame alone leaves the GPU idle between
them.  ``DensityStream.run`` runs ``workers`` frames concurrently, each worker thread on its
own HIP stream with its own library handle (workspace).  ``DensityStream.run_batch``
processes a whole batch of frames with one launch per phase instead (frames in CSR
layout: ``lidar_preprocess_batch_f64`` / ``lidar_people_batch_f64`` /
``lidar_density_batch_f64``), three small host read-backs per batch.  Both
return per frame the reference's ``analyze`` result (the big per-point arrays stay on
the device).  Results are the drop-in path's, bit for bit (same kernels).
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _native as nat
from . import density_abi as abi
from .streams import side_streams


class DensityStream:
    def __init__(self, device="cuda", workers=4, grid_size=1.0):
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.workers = workers
        self.grid_size = float(grid_size)
        self._streams = side_streams(self.device, workers)
        self._bufs = [{} for _ in range(workers)]
        # one persistent host thread per lane: the library's handles (workspaces) are per thread,
        # so a lane keeps its handles from call to call instead of creating them per call
        self._lanes = []
        self._last_people = None

    def _lane(self, j):
        while len(self._lanes) <= j:
            self._lanes.append(ThreadPoolExecutor(max_workers=1, thread_name_prefix=f"density-lane{len(self._lanes)}"))
        return self._lanes[j]

    def close(self):
        """Stop the lane threads (their handles are destroyed with them)."""
        for ex in self._lanes:
            ex.shutdown(wait=True)
        self._lanes = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _buffers(self, w, n):
        b = self._bufs[w]
        if b.get("n", 0) < n:
            b.update(abi.preprocess_outputs(n, self.device), n=n,
                     people=torch.empty((n, 2), dtype=torch.float64, device=self.device))
        return b

    def analyze_frame(self, x, w=0):
        """x: (n, 3) float64 CUDA tensor -> (result dict of CrowdDensityModel.analyze,
        device tensors {points, colors, normals, clusters} of the preprocessed frame)."""
        n = x.shape[0]
        if n == 0:  # decided before any launch
            abi.raise_for_status(abi.STATUS_EMPTY)
        b = self._buffers(w, n)
        s = self._streams[w]
        h = nat.handle(self.device.index, slot=8 + w)
        sp = s.cuda_stream
        abi.preprocess(h, x, None, 1, n, None, b, sp)
        S = np.empty(abi.SCALARS)
        with torch.cuda.stream(s):
            S[:] = b["scal"].cpu().numpy()
        abi.raise_for_status(S[abi.S_STATUS])
        nin = int(S[abi.S_N_IN])
        frame = {"points": b["comp"][:nin], "colors": b["colors"][:nin], "normals": b["normals"][:nin],
                 "clusters": b["labels"][:nin]}
        _, k = abi.people(h, b["comp"], b["labels"], nin, sp, out=b["people"])
        if k == 0:
            return abi.empty_result(), frame
        x_min, x_max, y_min, y_max = abi.xy_extent(S)
        nx, ny = nat.grid_dims(x_min, x_max, y_min, y_max, self.grid_size)
        with torch.cuda.stream(s), nat.grid_alloc():
            gx = torch.empty(nx, dtype=torch.float64, device=self.device)
            gy = torch.empty(ny, dtype=torch.float64, device=self.device)
            buf = torch.empty(abi.record_doubles(nx, ny, edges=False), dtype=torch.float64, device=self.device)
        nat.call("lidar_density_grid_f64", h, nat.ptr(b["people"]), k, float(x_min), float(x_max), float(y_min),
                 float(y_max), self.grid_size, nx, ny, nat.ptr(gx), nat.ptr(gy), nat.ptr(buf), sp)
        with torch.cuda.stream(s):
            hb = buf.cpu().numpy()
        return abi.analyze_result(k, *abi.decode_record(hb, nx, ny, edges=False)[2:]), frame

    def run(self, frames):
        """frames: list of (n_i, 3) float64 CUDA tensors -> list of analyze results, in order.
        Worker w takes frames w, w + workers, ...; exceptions are re-raised in order."""
        out = [None] * len(frames)

        def work(w):
            torch.cuda.set_device(self.device)
            for i in range(w, len(frames), self.workers):
                try:
                    out[i] = self.analyze_frame(frames[i], w)[0]
                except Exception as e:  # reported per frame, like the reference per call
                    out[i] = e
            self._streams[w].synchronize()
            nat.trim(self.device.index)  # this lane's work is done: free retired workspaces

        for f in [self._lane(w).submit(work, w) for w in range(min(self.workers, len(frames)))]:
            f.result()
        for r in out:
            if isinstance(r, Exception):
                raise r
        return out

    # ------------------------------------------------------------------ batched mode
    BATCH_SLOT = 7  # run_batch's library handle slot

    def profile(self, enable):
        """Per-phase HIP-event timing of run_batch's launches (lidar_profile): phases preprocess,
        dbscan_grid, dbscan_count, dbscan_union, dbscan_labels, label_scatter, people, density_grid."""
        nat.profile(nat.handle(self.device.index, slot=self.BATCH_SLOT), enable)

    def profile_read(self):
        """{phase: (launches, total ms)} since the last read (waits for the events)."""
        out = {}
        for name, ms in nat.profile_read(nat.handle(self.device.index, slot=self.BATCH_SLOT)):
            n, t = out.get(name, (0, 0.0))
            out[name] = (n + 1, t + ms)
        return out

    def run_batches(self, batches, lanes=3):
        """batches: list of frame lists -> list of per-batch result lists, in order, with `lanes`
        batches in flight: each lane is a host thread with its own HIP stream and library handle
        (handles are per thread), so one lane's host read-backs and latency-bound phases (the
        sequential preprocess / people chains run one workgroup per frame) overlap the other
        lanes' kernels.  Three lanes measured best (a process has 4 hardware queues; 32 x 65 536-point
        batches: 663-704 M points/s vs 602-650 with four).  Results equal run_batch's batch by batch; the first failing batch's
        exception (in batch order) is raised."""
        out = [None] * len(batches)
        lanes = max(1, min(int(lanes), len(batches)))
        caller = torch.cuda.current_stream(self.device)
        streams = side_streams(self.device, lanes)
        for st in streams:
            st.wait_stream(caller)  # the frames exist on the caller's stream

        people = [None] * len(batches)

        def work(j):
            torch.cuda.set_device(self.device)
            with torch.cuda.stream(streams[j]):
                for i in range(j, len(batches), lanes):
                    try:
                        out[i] = self._run_batch(batches[i])
                        people[i] = out[i][1]
                        out[i] = out[i][0]
                    except Exception as e:  # reported in batch order below
                        out[i] = e
            streams[j].synchronize()
            nat.trim(self.device.index)  # this lane's work is done: free retired workspaces

        for f in [self._lane(j).submit(work, j) for j in range(lanes)]:
            f.result()
        for r in out:
            if isinstance(r, Exception):
                raise r
        if batches and people[-1] is not None:  # the last batch in batch order (an empty one keeps the previous)
            self._last_people = people[-1]
        return out

    def people_of_last_batch(self):
        """The people positions of every frame of the last batch of run_batch / run_batches (in
        batch order), concatenated in frame order: a (sum K_f, 2) float64 CUDA tensor (what
        extract_people_positions returns per frame)."""
        if self._last_people is None:
            return torch.empty((0, 2), dtype=torch.float64, device=self.device)
        people, offs, K = self._last_people
        rows = [people[int(o):int(o) + int(k)] for o, k in zip(offs[:-1], K) if k > 0]
        return torch.cat(rows) if rows else people[:0]

    def run_batch(self, frames):
        """frames: list of (n_i, 3) float64 CUDA tensors -> list of analyze results, one
        launch per phase for the whole list.  Raises the reference's exception of the first
        failing frame (ValueError empty, IndexError no inlier), like `run`."""
        res, people = self._run_batch(frames)
        if people is not None:
            self._last_people = people
        torch.cuda.current_stream(self.device).synchronize()
        nat.trim(self.device.index)
        return res

    def _run_batch(self, frames):
        """run_batch's work -> (results, (people, offsets, K) or None); no shared state is
        written, so lanes of run_batches may call it concurrently."""
        F = len(frames)
        if F == 0:
            return [], None
        dev = self.device
        sizes = [int(x.shape[0]) for x in frames]
        offs_h = np.zeros(F + 1, dtype=np.int64)
        offs_h[1:] = np.cumsum(sizes)
        total, max_n = int(offs_h[-1]), max(1, max(sizes))
        x = torch.cat([t.reshape(-1, 3) for t in frames]) if F > 1 else frames[0].reshape(-1, 3)
        x = x.contiguous()
        rows = max(1, total)
        f64 = dict(dtype=torch.float64, device=dev)
        offs = torch.from_numpy(offs_h).to(dev)
        o = abi.preprocess_outputs(rows, dev, frames=F)
        h = nat.handle(self.device.index, slot=self.BATCH_SLOT)
        sp = torch.cuda.current_stream(dev).cuda_stream
        abi.preprocess(h, x, offs, F, max_n, None, o, sp)
        people = torch.empty((rows, 2), **f64)
        kdev = torch.empty(F, dtype=torch.int64, device=dev)
        nat.call("lidar_people_batch_f64", h, nat.ptr(o["comp"]), nat.ptr(o["labels"]), nat.ptr(offs), F, max_n,
                 nat.ptr(o["scal"]), nat.ptr(people), nat.ptr(kdev), sp)
        S = o["scal"].cpu().numpy()  # read-back 1 (also waits for people)
        status = S[:, abi.S_STATUS]
        for bad in status[status != abi.STATUS_OK]:  # the first failing frame's exception
            abi.raise_for_status(bad)
        K = kdev.cpu().numpy()  # read-back 2
        last_people = (people, offs_h, K)
        counts = K.tolist()
        jobs = np.zeros((F, 8), dtype=np.float64)
        out_off = scr_off = 0
        dims = [None] * F
        for f in range(F):
            if counts[f] <= 0:
                continue
            x_min, x_max, y_min, y_max = abi.xy_extent(S[f])
            nx, ny = nat.grid_dims(x_min, x_max, y_min, y_max, self.grid_size)
            jobs[f] = abi.job_row(x_min, y_min, self.grid_size, nx, ny, out_off, scr_off)
            dims[f] = (nx, ny, out_off)
            out_off += abi.record_doubles(nx, ny, True)
            scr_off += abi.scratch_doubles(nx, ny)
        res = [None] * F
        if out_off:
            jd = torch.from_numpy(jobs).to(dev)
            with nat.grid_alloc():
                out = torch.empty(out_off, **f64)
            nat.call("lidar_density_batch_f64", h, nat.ptr(people), nat.ptr(offs), nat.ptr(kdev), F, nat.ptr(jd),
                     nat.ptr(out), scr_off, sp)
            ob = out.cpu().numpy()  # read-back 3
        for f in range(F):
            if dims[f] is None:
                res[f] = abi.empty_result()
                continue
            nx, ny, off = dims[f]
            res[f] = abi.analyze_result(counts[f], *abi.decode_record(ob, nx, ny, True, off)[2:])
        return res, last_people
