"""numpy restatement of the feature-propagation spec (DESIGN.md §3 "Feature propagation"): three_nn,
the inverse-distance weights, three_interpolate and a float64 FP level.  float32 with one rounding per
operation, as the kernels of csrc/feature_prop.hip; no GPU, no product code."""
import numpy as np

F32 = np.float32
INF = F32(np.inf)


def dist2(unknown, known):
    """(n, 3), (m, 3) float32 -> (n, m) float32: (dx*dx + dy*dy) + dz*dz, one rounding per operation."""
    u = np.asarray(unknown, F32)
    k = np.asarray(known, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = u[:, None, 0] - k[None, :, 0]
        dy = u[:, None, 1] - k[None, :, 1]
        dz = u[:, None, 2] - k[None, :, 2]
        return (dx * dx + dy * dy) + dz * dz


def three_nn_ref(unknown, known, fourth=False, chunk=1024):
    """Vectorised three_nn of one frame: a stable argsort of key = where(d < inf, d, inf) (a NaN or +inf
    distance never wins; ties keep the lowest index), unfilled slots mapped to (+inf, 0).  Only the columns
    that can be among a row's first four are sorted: those with key <= the row's fourth-smallest key, kept
    in ascending column order, so the stable order is that of the full row.  -> (dist2 (n, 3) float32,
    idx (n, 3) int32[, the fourth-smallest key (n,), +inf when there is none])."""
    unknown = np.asarray(unknown, F32)
    n, m = len(unknown), len(known)
    d3 = np.empty((n, 3), F32)
    i3 = np.empty((n, 3), np.int32)
    d4 = np.empty(n, F32)
    kth = min(3, m - 1)
    for r0 in range(0, n, chunk):
        d = dist2(unknown[r0:r0 + chunk], known)
        with np.errstate(invalid="ignore"):
            key = np.where(d < INF, d, INF)
        t = np.partition(key, kth, axis=1)[:, kth]
        cand = (key <= t[:, None]) & (key < INF)
        cnt = cand.sum(axis=1)
        r, c = np.nonzero(cand)  # row-major: a row's candidates in ascending column order
        pos = np.arange(len(r)) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        cols = np.zeros((len(key), max(4, int(cnt.max(initial=0)))), np.int64)
        vals = np.full(cols.shape, INF, F32)
        cols[r, pos], vals[r, pos] = c, key[r, c]
        order = np.argsort(vals, axis=1, kind="stable")[:, :4]
        srt = np.take_along_axis(vals, order, axis=1)
        d3[r0:r0 + chunk] = srt[:, :3]
        i3[r0:r0 + chunk] = np.where(srt[:, :3] < INF, np.take_along_axis(cols, order[:, :3], axis=1), 0)
        d4[r0:r0 + chunk] = srt[:, 3]
    return (d3, i3, d4) if fourth else (d3, i3)


def three_nn_scan(unknown, known):
    """The sequential statement: scan j ascending with three slots (d2, idx) = (+inf, 0); insert with strict
    <: d < best0, else d < best1, else d < best2 (vectorised over the unknown points only)."""
    unknown = np.asarray(unknown, F32)
    n = len(unknown)
    b = [np.full(n, INF, F32) for _ in range(3)]
    i = [np.zeros(n, np.int32) for _ in range(3)]
    d = dist2(unknown, known)
    for j in range(len(known)):
        dj = d[:, j]
        with np.errstate(invalid="ignore"):
            lt0 = dj < b[0]
            lt1 = ~lt0 & (dj < b[1])
            lt2 = ~lt0 & ~lt1 & (dj < b[2])
        s01 = lt0 | lt1
        b[2], i[2] = np.where(s01, b[1], np.where(lt2, dj, b[2])), np.where(s01, i[1], np.where(lt2, j, i[2]))
        b[1], i[1] = np.where(lt0, b[0], np.where(lt1, dj, b[1])), np.where(lt0, i[0], np.where(lt1, j, i[1]))
        b[0], i[0] = np.where(lt0, dj, b[0]), np.where(lt0, j, i[0])
    return np.stack(b, 1).astype(F32), np.stack(i, 1).astype(np.int32)


def weights_ref(d3):
    """(n, 3) squared distances -> (n, 3) float32 weights r_i / ((r_0 + r_1) + r_2), r_i = 1 / (sqrt(d2_i) +
    1e-8f): an unfilled slot (+inf) gives 0, three of them 0 / 0 = NaN."""
    d3 = np.asarray(d3, F32)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = F32(1.0) / (np.sqrt(d3) + F32(1e-8))
        return (r / ((r[:, 0] + r[:, 1]) + r[:, 2])[:, None]).astype(F32)


def interpolate_ref(feats, idx, w, skip=None):
    """feats (m, c2), idx / w (n, 3), skip (n, c1) or None -> (n, c2 + c1) float32:
    [(w0 f[i0] + w1 f[i1]) + w2 f[i2] | skip]."""
    f = np.asarray(feats, F32)
    w = np.asarray(w, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        out = (w[:, 0:1] * f[idx[:, 0]] + w[:, 1:2] * f[idx[:, 1]]) + w[:, 2:3] * f[idx[:, 2]]
    out = out.astype(F32)
    return out if skip is None else np.concatenate([out, np.asarray(skip, F32)], axis=1)


def fp_rows_ref(uxyz, kxyz, kfeat, skip=None):
    """One frame's FP-level rows from the spec: three_nn_ref, weights_ref, interpolate_ref."""
    d3, i3 = three_nn_ref(uxyz, kxyz)
    return interpolate_ref(kfeat, i3, weights_ref(d3), skip), i3


def fp_level_exact(rows, layers, last_relu=True):
    """relu(x W + b) per layer in float64 on float32 rows (last_relu=False: a final linear layer)."""
    h = np.asarray(rows, F32).astype(np.float64)
    for j, (W, b) in enumerate(layers):
        h = h @ np.asarray(W, np.float64) + np.asarray(b, np.float64)
        if last_relu or j + 1 < len(layers):
            h = np.maximum(h, 0.0)
    return h
