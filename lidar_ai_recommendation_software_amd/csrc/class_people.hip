// class_people.hip — people from per-point class labels: the bridge from a segmenter's (batch, n)
// labels to the Tier R machinery (dbscan.hip's run_dbscan, density_grid.hip's people_kernel).
//
// Per frame: the points of one class with finite coordinates, widened to fp64 and kept in index
// order (flags -> exclusive scan -> scatter: a stable compaction in which no workgroup waits for
// another), DBSCAN(eps, min_samples) over them with one workspace slice per frame, the labels
// scattered back to the frame's points, the clusters' (x, y) centroids and the frame's xy extent.
// Nothing is staged through the host and nothing synchronises: every frame's DBSCAN parameter
// block (point count, eps, bbox of the selected points) is written by a kernel.
#include <cmath>

#include "tier_r.hpp"

namespace {

using namespace lidar::tier_r;

constexpr int kB = 256;        // threads of the per-point kernels
constexpr int kPart = 10;      // doubles per workgroup of flag_kernel's partial record
// partial record: extent x_min, x_max, y_min, y_max over the finite points; lo (3), hi (3) of the selected
enum : int { R_EXT = 0, R_LO = 4, R_HI = 7 };

struct ClassWs {
    int32_t *pos;      // per point of the frame: its row among the selected, -1 when not selected
    int64_t *lab;      // run_dbscan's labels of the selected points
    double *xs;        // the selected points (the slice's DbscanWs::x)
    double *part;      // flag_kernel's per-workgroup partial records
    // outside the per-frame slices, rows of frame f from row f * n on (people_kernel's CSR layout)
    double *xall;      // selected points
    int64_t *laball;   // their labels
    double *ptmp;      // every cluster's centroid (a frame has at most n clusters)
    double *scal;      // (batch, S_COUNT): status 0 and the selected count, people_kernel's per-frame n
    int64_t *offs;     // batch + 1 row offsets: f * n
};

__device__ __forceinline__ double wave_min_d(double v)
{
    for (int m = 32; m >= 1; m >>= 1) v = fmin(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ __forceinline__ double wave_max_d(double v)
{
    for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
    return v;
}

// One read of xyz and labels: the selection flags (the scan's input, DbscanWs::flag), and per workgroup
// the extent of the finite points and the bbox of the selected ones.  A point with a non-finite
// coordinate contributes to neither.
__global__ __launch_bounds__(kB) void flag_kernel(const float *__restrict__ xyz, const int32_t *__restrict__ labels,
                                                  int64_t n, int32_t cls, DbscanWs w, ClassWs c, FrameMap fm)
{
    w = w.frame(fm);
    const float *x = xyz + (int64_t)blockIdx.y * n * 3;
    const int32_t *l = labels + (int64_t)blockIdx.y * n;
    double lo[kPart];  // minima at even R_EXT slots and R_LO, maxima at odd R_EXT slots and R_HI
    for (int k = 0; k < kPart; ++k) lo[k] = (k < R_LO ? (k & 1) : k >= R_HI) ? -INFINITY : INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x; i < n; i += (int64_t)gridDim.x * kB) {
        const float px = x[3 * i], py = x[3 * i + 1], pz = x[3 * i + 2];
        const bool finite = isfinite(px) && isfinite(py) && isfinite(pz);
        const bool sel = finite && l[i] == cls;
        w.flag[i] = sel ? 1u : 0u;
        if (finite) {
            lo[R_EXT] = fmin(lo[R_EXT], (double)px);
            lo[R_EXT + 1] = fmax(lo[R_EXT + 1], (double)px);
            lo[R_EXT + 2] = fmin(lo[R_EXT + 2], (double)py);
            lo[R_EXT + 3] = fmax(lo[R_EXT + 3], (double)py);
        }
        if (sel) {
            const double p[3] = {(double)px, (double)py, (double)pz};
            for (int k = 0; k < 3; ++k) {
                lo[R_LO + k] = fmin(lo[R_LO + k], p[k]);
                lo[R_HI + k] = fmax(lo[R_HI + k], p[k]);
            }
        }
    }
    __shared__ double red[kB / 64][kPart];
    for (int k = 0; k < kPart; ++k) {
        const bool is_max = k < R_LO ? (k & 1) : k >= R_HI;
        const double v = is_max ? wave_max_d(lo[k]) : wave_min_d(lo[k]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < kPart) {
        const int k = threadIdx.x;
        const bool is_max = k < R_LO ? (k & 1) : k >= R_HI;
        double v = red[0][k];
        for (int q = 1; q < kB / 64; ++q) v = is_max ? fmax(v, red[q][k]) : fmin(v, red[q][k]);
        fm.ws(c.part)[(int64_t)blockIdx.x * kPart + k] = v;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) w.P[P_NALL] = (double)n;  // the scan's length
}

// rank = the exclusive scan of the flags: the selected points, widened, to row rank[i] of the slice's
// x (DBSCAN) and of the frame's rows of xall (people_kernel); pos for the way back
__global__ __launch_bounds__(kB) void scatter_kernel(const float *__restrict__ xyz, int64_t n, DbscanWs w, ClassWs c,
                                                     FrameMap fm)
{
    w = w.frame(fm);
    const float *x = xyz + (int64_t)blockIdx.y * n * 3;
    int32_t *pos = fm.ws(c.pos);
    double *xs = fm.ws(c.xs), *xa = c.xall + (int64_t)blockIdx.y * n * 3;
    for (int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x; i < n; i += (int64_t)gridDim.x * kB) {
        const bool sel = w.flag[i] != 0;
        const int64_t r = w.rank[i];
        pos[i] = sel ? (int32_t)r : -1;
        if (sel)
            for (int k = 0; k < 3; ++k) {
                const double v = (double)x[3 * i + k];
                xs[3 * r + k] = v;
                xa[3 * r + k] = v;
            }
    }
}

// One wave per frame: the partial records reduced (min and max: any order gives the same result) into the
// frame's extent and its DBSCAN parameter block; the selected count; people_kernel's scalars and offsets.
__global__ __launch_bounds__(64) void params_kernel(int64_t n, int nparts, double eps, DbscanWs w, ClassWs c,
                                                    double *extent, int64_t *nsel_out, FrameMap fm)
{
    w = w.frame(fm);
    const double *part = fm.ws(c.part);
    double r[kPart];
    for (int k = 0; k < kPart; ++k) {
        const bool is_max = k < R_LO ? (k & 1) : k >= R_HI;
        double v = is_max ? -INFINITY : INFINITY;
        for (int b = threadIdx.x; b < nparts; b += 64) v = is_max ? fmax(v, part[b * kPart + k]) : fmin(v, part[b * kPart + k]);
        r[k] = is_max ? wave_max_d(v) : wave_min_d(v);
    }
    if (threadIdx.x) return;
    const int f = blockIdx.y;
    const int64_t nsel = w.rank[n];
    for (int k = 0; k < 4; ++k) extent[4 * f + k] = r[R_EXT + k];
    nsel_out[f] = nsel;
    for (int k = 0; k < P_COUNT; ++k) w.P[k] = 0.0;
    w.P[P_N] = (double)nsel;
    w.P[P_EPS] = eps;
    // a frame without a selected point stays inactive: no grid over an empty box, zero clusters
    w.P[P_ACTIVE] = nsel > 0 ? 1.0 : 0.0;
    for (int k = 0; k < 3; ++k) {
        w.P[P_LO + k] = nsel > 0 ? r[R_LO + k] : 0.0;
        w.P[P_HI + k] = nsel > 0 ? r[R_HI + k] : 0.0;
    }
    double *S = fm.scal(c.scal);
    S[S_STATUS] = 0.0;
    S[S_NIN] = (double)nsel;
    c.offs[f] = (int64_t)f * n;
    if (f == (int)gridDim.y - 1) c.offs[f + 1] = (int64_t)(f + 1) * n;
}

// DBSCAN's labels back to the frame's points (-1: not selected, or noise), the labels into the frame's
// rows of laball, and the cluster count
__global__ __launch_bounds__(kB) void instance_kernel(int64_t n, DbscanWs w, ClassWs c, int32_t *instance, int64_t *k_out,
                                                      FrameMap fm)
{
    w = w.frame(fm);
    const int32_t *pos = fm.ws(c.pos);
    const int64_t *lab = fm.ws(c.lab);
    int32_t *inst = instance + (int64_t)blockIdx.y * n;
    int64_t *la = c.laball + (int64_t)blockIdx.y * n;
    const int64_t nsel = (int64_t)w.P[P_N];
    for (int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x; i < n; i += (int64_t)gridDim.x * kB) {
        const int32_t p = pos[i];
        inst[i] = p >= 0 ? (int32_t)lab[p] : -1;
        if (i < nsel) la[i] = lab[i];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) k_out[blockIdx.y] = (int64_t)w.P[P_NCLUST];
}

// the first min(k, cap) centroids of every frame to the caller's (batch, cap, 2) array
__global__ __launch_bounds__(kB) void people_out_kernel(int64_t n, int64_t cap, const double *__restrict__ ptmp,
                                                        const int64_t *__restrict__ k, double *__restrict__ people)
{
    const int f = blockIdx.y;
    const int64_t m = 2 * (k[f] < cap ? k[f] : cap);
    const double *src = ptmp + (int64_t)f * n * 2;
    double *dst = people + (int64_t)f * cap * 2;
    for (int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x; i < m; i += (int64_t)gridDim.x * kB) dst[i] = src[i];
}

}  // namespace

// ====================================================================== C-ABI
LIDAR_EXPORT int lidar_class_people_f32(lidar_handle *h, const float *xyz, const int32_t *labels, int64_t batch,
                                        int64_t n, int32_t cls, double eps, int32_t min_samples, int64_t cap,
                                        int32_t *instance, double *people, int64_t *k, int64_t *nsel, double *extent,
                                        void *stream)
{
    REQUIRE(h && xyz && labels && instance && people && k && nsel && extent, "lidar_class_people_f32: null pointer");
    REQUIRE(batch >= 0 && batch <= 65535, "lidar_class_people_f32: batch out of range");
    REQUIRE(n >= 1 && n < 0x80000000ll, "lidar_class_people_f32: n out of range");
    REQUIRE(eps > 0.0 && eps < INFINITY, "lidar_class_people_f32: eps must be positive and finite");
    REQUIRE(min_samples >= 1, "lidar_class_people_f32: min_samples must be >= 1");
    REQUIRE(cap >= 1, "lidar_class_people_f32: cap must be >= 1");
    if (batch == 0) return LIDAR_OK;
    ON_DEVICE(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int frames = (int)batch;
    const unsigned gp = point_blocks(n, frames);

    // one slice per frame, sized for a frame whose every point is selected, then the frame-major rows
    lidar::Carver cv;
    const uint64_t o_pos = cv.take<int32_t>(n), o_lab = cv.take<int64_t>(n), o_xs = cv.take<double>(3 * n);
    const uint64_t o_part = cv.take<double>((uint64_t)gp * kPart);
    lidar::Carver at = cv;  // where the DBSCAN sub-buffers start
    carve_dbscan(cv, n, nullptr);
    const uint64_t wss = lidar::align_up(cv.off, 256);
    lidar::Carver tail;
    tail.off = wss * (uint64_t)frames;
    const uint64_t rows = (uint64_t)frames * (uint64_t)n;
    const uint64_t o_xall = tail.take<double>(3 * rows), o_laball = tail.take<int64_t>(rows);
    const uint64_t o_ptmp = tail.take<double>(2 * rows), o_scal = tail.take<double>((uint64_t)frames * S_COUNT);
    const uint64_t o_offs = tail.take<int64_t>((uint64_t)frames + 1);
    char *base = static_cast<char *>(lidar::workspace(h, tail.off));
    if (!base) return LIDAR_ENOMEM;
    ClassWs c;
    c.pos = reinterpret_cast<int32_t *>(base + o_pos);
    c.lab = reinterpret_cast<int64_t *>(base + o_lab);
    c.xs = reinterpret_cast<double *>(base + o_xs);
    c.part = reinterpret_cast<double *>(base + o_part);
    c.xall = reinterpret_cast<double *>(base + o_xall);
    c.laball = reinterpret_cast<int64_t *>(base + o_laball);
    c.ptmp = reinterpret_cast<double *>(base + o_ptmp);
    c.scal = reinterpret_cast<double *>(base + o_scal);
    c.offs = reinterpret_cast<int64_t *>(base + o_offs);
    DbscanWs w = carve_dbscan(at, n, base);
    w.x = c.xs;
    FrameMap fm;
    fm.wss = (int64_t)wss;

    const dim3 FP(gp, frames), F1(1, frames);
    {
        lidar::Span sp(h, "class_select", s);  // flags, scan, scatter, parameter blocks
        hipLaunchKernelGGL(flag_kernel, FP, dim3(kB), 0, s, xyz, labels, n, cls, w, c, fm);
        int rc = scan_u32(w, w.flag, w.rank, P_NALL, 0, w.nblk_pts, s, fm, frames);
        if (rc) return rc;
        hipLaunchKernelGGL(scatter_kernel, FP, dim3(kB), 0, s, xyz, n, w, c, fm);
        hipLaunchKernelGGL(params_kernel, F1, dim3(64), 0, s, n, (int)gp, eps, w, c, extent, nsel, fm);
    }
    int rc = run_dbscan(h, n, min_samples, w, c.lab, s, fm, frames);
    if (rc) return rc;
    {
        lidar::Span sp(h, "class_instance", s);
        hipLaunchKernelGGL(instance_kernel, FP, dim3(kB), 0, s, n, w, c, instance, k, fm);
    }
    FrameMap rows_of;
    rows_of.offs = c.offs;
    rc = people_of_frames(h, c.xall, c.laball, n, k, c.ptmp, c.scal, s, rows_of, frames);
    if (rc) return rc;
    hipLaunchKernelGGL(people_out_kernel, dim3(std::min<unsigned>(gp, 64), frames), dim3(kB), 0, s, n, cap, c.ptmp, k,
                       people);
    LAUNCH_CHECK();
    return LIDAR_OK;
}
