// voxel_batch.hip — voxel downsampling of a batch of frames over the whole chip.
//
// Spec (voxel_grid.hpp): the voxel key of a point is calculate_grid_density's grid hash
// (utils/data_processing.py:305-319: np.arange edges over the frame's extent with the 2-cell margin, histogram2d's
// searchsorted-right binning with the last edge closed) per axis, key = (bx*ny + by)*nz + bz; voxels in ascending key
// order, voxel id = rank of the key (-1 for a point outside every bin), centroid = sequential fp32 sum of the voxel's
// points in point order / count.
//
// Round 5: a two-level sort in two launches (round 4: an 8-bit LSD radix sort over global memory, 13 launches and ~284
// B of memory traffic per point):
//
//   keys     grid (8192-point tiles, frames; a frame's tiles on one XCD, dispatched together): each tile loads its
//            points once, publishes its extent as self-tagged 8-byte granules and polls its frame's other tiles' (an
//            in-launch hand-off instead of a bbox launch), builds the frame's grid (float64, every workgroup alike),
//            bins every point in float against per-axis LDS tables of the float64 edges' float thresholds (float64
//            beyond 8192 edges per axis; a point outside every bin takes nx ny nz, one past the last voxel), and
//            publishes its histogram over 4096 coarse bins (key >> hs, the top 12 bits of the range) as tagged granules
//            too; then, from the frame's histograms (polled), the exclusive scan over the coarse bins plus the counts
//            of the tiles before it, and it scatters its (key, index) pairs from registers to their coarse bins (LDS
//            atomics: order inside a bin is free, the buckets sort by (key, index) anyway); tile 0 also writes the
//            bucket table (bucket b = the coarse bins whose start s has min(s NB / n, NB - 1) = b, ~2 048 points
//            uniform).  Frames of more than 16 tiles (more than an XCD co-schedules with margin) split this into an
//            extent launch, a keys launch that writes the keys, and a scatter launch.  The granules live in the
//            handle's tag block: every tag there is an earlier call's epoch (no memset).
//   bucket   grid (buckets, frames; 4 workgroups per CU, the bench shape's 1 024 buckets in one round): each bucket
//            loads its pairs and counting-sorts them in LDS over its own key range — one counter per key, whose
//            exclusive scan of (count | occupied << 16) also gives every key its voxel rank; or, for a sparse grid (a
//            range past 4096 keys), counters over the keys' high bits with each run ordered by (key low bits, index)
//            words and the voxel ranks from a scan of first-point flags — equal-key runs ranked by index in parallel;
//            runs past 128: bitonic in LDS, or a stable LSD radix in global memory above 2048 pairs.  Its voxel count
//            goes out at once for the decoupled look-back (every wait is on a lower workgroup index, i.e. one
//            dispatched earlier), then every point's voxel id from registers and, one thread per voxel summing its
//            points' xyz (gathered) in index order, the centroids and counts.
//
// Memory-side bytes per point: xyz 12 (keys) + pair 8 + 8 + id 4 + the xyz gather 12 (+16 per voxel out; 62.9 measured
// by PMC at the bench shape); no host synchronisation: nvox[f] lands on the device (-1: the frame's extent is not
// finite, or its grid has 2^32 - 1 keys or more).
#include <algorithm>

#include "voxel_batch.hpp"
using namespace lidar::vx;

namespace {
// the workspace of a call on (batch, n): its arrays' offsets (Ws) and their total
struct VoxelCarve { uint64_t key, bstart, pairs, scratch, flags, bytes; };
VoxelCarve carve_voxel(int64_t batch, int64_t n)
{
    const int64_t nb = n_buckets(n);
    lidar::Carver cv;  // (a braced list is evaluated in order)
    VoxelCarve o{cv.take<uint32_t>(batch * n), cv.take<uint32_t>(batch * (nb + 1)), cv.take<uint64_t>(batch * n),
                 cv.take<uint64_t>(batch * n), cv.take<uint64_t>(batch * nb),       0};
    o.bytes = cv.off;
    return o;
}

// the handle's tag block of at least `bytes` (granules + meta words), and this call's epoch.  The block is written by
// voxel calls only, so every tag in it is an earlier call's epoch or 0: no per-call reset.  A larger block replaces a
// smaller one (the old one retired like a workspace: queued calls may still use it) and starts zeroed; so does the
// block when the epoch wraps.
void *vx_tags(lidar_handle *h, uint64_t bytes, hipStream_t s, uint32_t *epoch)
{
    if (bytes > h->vx_tags_bytes) {
        const uint64_t want = lidar::align_up(std::max(bytes + bytes / 4, 2 * h->vx_tags_bytes), 1 << 16);
        void *fresh = nullptr;
        const hipError_t e = hipMalloc(&fresh, want);
        if (e != hipSuccess) {
            lidar::set_error(std::string("voxel tag block hipMalloc(") + std::to_string(want) + "): " +
                             hipGetErrorString(e));
            return nullptr;
        }
        if (hipMemsetAsync(fresh, 0, want, s) != hipSuccess) {
            (void)hipFree(fresh);
            lidar::set_error("voxel tag block: hipMemsetAsync failed");
            return nullptr;
        }
        if (h->vx_tags) {
            h->retired.push_back(h->vx_tags);
            h->retired_bytes += h->vx_tags_bytes;
        }
        h->vx_tags = fresh;
        h->vx_tags_bytes = want;
    }
    if (++h->epoch == 0) {  // wrapped: no tag may equal a new epoch
        if (hipMemsetAsync(h->vx_tags, 0, h->vx_tags_bytes, s) != hipSuccess) {
            lidar::set_error("voxel tag block: hipMemsetAsync failed");
            return nullptr;
        }
        h->epoch = 1;
    }
    *epoch = h->epoch;
    return h->vx_tags;
}
}  // namespace

// workspace bytes of lidar_voxel_downsample_batch_f32 for (batch, n) (the granules and meta words live in the handle's
// own tag block, beside it)
LIDAR_EXPORT uint64_t lidar_voxel_batch_workspace_bytes(int64_t batch, int64_t n)
{
    return carve_voxel(batch, n).bytes;
}

// Voxel downsampling of `batch` frames of n points (xyz (batch, n, 3) fp32), all on the device: voxel_id (batch, n)
// int32, centroids (batch, n, 3) and counts (batch, n) with the first nvox[f] rows of frame f valid, nvox (batch,)
// int32 (-1: the frame's extent is not finite or its voxel grid has 2^32 - 1 keys or more; voxel_id -1: a point outside
// every bin).
LIDAR_EXPORT int lidar_voxel_downsample_batch_f32(lidar_handle *h, const float *xyz, int64_t batch, int64_t n,
                                                  double voxel, int32_t *voxel_id, float *centroids, int32_t *counts,
                                                  int32_t *nvox, void *stream)
{
    REQUIRE(h && xyz && voxel_id && centroids && counts && nvox, "lidar_voxel_downsample_batch_f32: null pointer");
    REQUIRE(batch >= 0 && batch <= 65535 && n >= 1 && n < 0x7fffffff,
            "lidar_voxel_downsample_batch_f32: batch in [0, 65535], n >= 1");
    REQUIRE(voxel > 0.0 && voxel < INFINITY, "lidar_voxel_downsample_batch_f32: voxel size must be finite and > 0");
    if (batch == 0) return LIDAR_OK;
    ON_DEVICE(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int ntiles = n_tiles(n);
    REQUIRE((int64_t)frame_grid(batch, std::max<int64_t>(ntiles, n_buckets(n))) < 0x7fffffff,
            "lidar_voxel_downsample_batch_f32: batch * n too large");
    // the in-launch hand-offs' granules (extents, then histograms) and the meta words: the tag block
    lidar::Carver ct;
    const uint64_t ogran = ct.take<unsigned long long>(batch * ntiles * (6 + NBIN / 2));
    const uint64_t ometa = ct.take<uint32_t>(batch * MW);
    uint32_t epoch = 0;
    char *tags = static_cast<char *>(vx_tags(h, ct.off, s, &epoch));
    if (!tags) return LIDAR_ENOMEM;
    const VoxelCarve o = carve_voxel(batch, n);
    char *base = static_cast<char *>(lidar::workspace(h, o.bytes));
    if (!base) return LIDAR_ENOMEM;
    Ws w;
    w.gran = reinterpret_cast<unsigned long long *>(tags + ogran);
    w.meta = reinterpret_cast<uint32_t *>(tags + ometa);
    w.key = reinterpret_cast<uint32_t *>(base + o.key);
    w.hgran = w.gran + batch * ntiles * 6;
    w.bstart = reinterpret_cast<uint32_t *>(base + o.bstart);
    w.pairs = reinterpret_cast<uint64_t *>(base + o.pairs);
    w.scratch = reinterpret_cast<uint64_t *>(base + o.scratch);
    w.flags = reinterpret_cast<uint64_t *>(base + o.flags);
    launch_keys(xyz, batch, n, voxel, w, epoch, s VX_KEYS_DIAG(centroids));
    launch_buckets(xyz, batch, n, w, voxel_id, centroids, counts, nvox, epoch, s);
    LAUNCH_CHECK();
    return LIDAR_OK;
}
