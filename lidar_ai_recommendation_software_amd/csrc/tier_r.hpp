// tier_r.hpp — what two of preprocess.hip, dbscan.hip and density_grid.hip share: sizes, the scalars slots,
// the frame map, fp64 rounding wrappers, workgroup min / max / scan, the DBSCAN parameter block and workspace,
// the venue grid's binning (density_grid.hip, track.hip), the u32 scan's device code (dbscan.hip, track.hip),
// readlane_d (preprocess.hip, track.hip),
// and the host entry points of dbscan.hip and density_grid.hip for preprocess.hip and class_people.hip.  Kernels stay local to their translation unit.
#pragma once
#include <algorithm>
#include <cmath>

#include "common.hpp"

namespace lidar {
namespace tier_r {

constexpr int kT = 1024;  // threads of the one-workgroup-per-frame kernels
constexpr int kW = kT / 64;

// ------------------------------------------------------------------ scalars layout
// the public slots are lidar_amd.h's LIDAR_S_*; the rest are Tier R's own (and a LIDAR_PRE_DIAG
// build's stamps at 48..57)
enum : int {
    S_NIN = LIDAR_S_N_IN, S_NGROUND = LIDAR_S_N_GROUND, S_NNG = LIDAR_S_N_NONGROUND, S_ZT = LIDAR_S_Z_THRESHOLD,
    S_EPS = LIDAR_S_EPS, S_DIMS = LIDAR_S_DIMS, S_PLANE = LIDAR_S_PLANE, S_STATUS = LIDAR_S_STATUS,
    S_MEAN = LIDAR_S_MEAN, S_STD = LIDAR_S_STD, S_SMEAN = LIDAR_S_SCALER_MEAN, S_SSCALE = LIDAR_S_SCALER_SCALE,
    S_SLO = LIDAR_S_SCALED_BBOX, S_SHI = LIDAR_S_SCALED_BBOX + 3, S_NCLUST = LIDAR_S_N_CLUSTERS,
    S_PLANE_KIND = LIDAR_S_PLANE_KIND, S_COUNT = LIDAR_SCALARS,
    S_CELL = 34, S_CDIM = 35, S_NCELL = 38, S_N = 41, S_MINPTS = 42
};

// ------------------------------------------------------------------ frame batching
// Every Tier R kernel runs one frame per blockIdx.y.  Frame f's scratch lives at
// f * wss bytes into one workspace allocation (same sub-buffer offsets in every frame),
// its rows of the caller's arrays start at row offs[f] (CSR; offs == nullptr: a single
// frame of the given n), and its scalars at S + f * S_COUNT.
struct FrameMap {
    int64_t wss = 0;
    const int64_t *offs = nullptr;
    template <class T> __device__ __forceinline__ T *ws(T *p) const
    {
        return reinterpret_cast<T *>(reinterpret_cast<uintptr_t>(p) + (uintptr_t)((int64_t)blockIdx.y * wss));
    }
    template <class T> __device__ __forceinline__ T *rows(T *p, int width) const
    {
        return offs ? p + offs[blockIdx.y] * width : p;
    }
    __device__ __forceinline__ int64_t n(int64_t single) const
    {
        return offs ? offs[blockIdx.y + 1] - offs[blockIdx.y] : single;
    }
    template <class T> __device__ __forceinline__ T *scal(T *S) const { return S + (int64_t)blockIdx.y * S_COUNT; }
};

__device__ __forceinline__ double dadd(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double dsub(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ double dmul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double ddiv(double a, double b) { return __ddiv_rn(a, b); }

// ---- the venue grid's binning (density_grid.hip's venue_counts_kernel, track.hip's cell_kernel):
// calculate_grid_density's np.arange edges (e[0] = a, e[1] = a + g, e[i] = a + i * ((a + g) - a), numpy's
// DOUBLE_fill), searchsorted right with the last edge closed
__device__ __forceinline__ double arange_edge(double a, double g, int64_t i)
{
    return i == 0 ? a : (i == 1 ? dadd(a, g) : dadd(a, dmul((double)i, dsub(dadd(a, g), a))));
}
__device__ __forceinline__ int64_t arange_bin(double a, double g, int64_t nb, double v)
{
    int64_t lo = 0, hi = nb + 1;  // first edge index with e[idx] > v
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (arange_edge(a, g, mid) <= v) lo = mid + 1;
        else hi = mid;
    }
    if (v == arange_edge(a, g, nb)) --lo;  // the last edge is closed
    return lo;                             // bin lo - 1 when 1 <= lo <= nb
}

// ---- workgroup helpers (1024 threads)
struct BlockScratch {
    double d[6][kW];
    uint32_t i[kW];
    double chain[3];  // preprocess.hip's emulated chains: the result of column c
};

// workgroup reduction of v with op (fmin, fmax, or preprocess.hip's dadd; through row `SLOT` of s.d) in a fixed
// order (the xor butterfly within a wave, then the waves' results in wave order): every thread gets the result
template <int SLOT, class Op>
__device__ __forceinline__ double block_reduce(BlockScratch &s, double v, Op op)
{
    for (int m = 32; m >= 1; m >>= 1) v = op(v, __shfl_xor(v, m, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s.d[SLOT][threadIdx.x >> 6] = v;
    __syncthreads();
    double r = s.d[SLOT][0];
    for (int w = 1; w < kW; ++w) r = op(r, s.d[SLOT][w]);
    return r;
}
__device__ __forceinline__ double block_min(BlockScratch &s, double v)
{
    return block_reduce<0>(s, v, [](double a, double b) { return fmin(a, b); });
}
__device__ __forceinline__ double block_max(BlockScratch &s, double v)
{
    return block_reduce<1>(s, v, [](double a, double b) { return fmax(a, b); });
}
// bounding box of the rows [0, n) of a row-major (n, 3) array, stored to lo_out[0..2] / hi_out[0..2]
__device__ __forceinline__ void block_bbox(BlockScratch &s, const double *x, int64_t n, double *lo_out, double *hi_out)
{
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = threadIdx.x; i < n; i += kT)
        for (int c = 0; c < 3; ++c) {
            lo[c] = fmin(lo[c], x[3 * i + c]);
            hi[c] = fmax(hi[c], x[3 * i + c]);
        }
    for (int c = 0; c < 3; ++c) {
        const double a = block_min(s, lo[c]), b = block_max(s, hi[c]);
        if (threadIdx.x == 0) {
            lo_out[c] = a;
            hi_out[c] = b;
        }
    }
}
// exclusive scan of one 32-bit count per thread over the workgroup's waves from w0 on (0: the whole
// workgroup): the sum of v over the threads of waves w0 .. this one that come before the caller.
// wtot: kW words of LDS, free again after the caller's next barrier.
__device__ __forceinline__ uint32_t block_excl_scan_u32(uint32_t v, uint32_t *wtot, int w0 = 0)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t incl = (uint32_t)wave_incl_scan_i32((int)v);
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    uint32_t base = 0;
    for (int w = w0; w < wave; ++w) base += wtot[w];
    return base + incl - v;
}

// ---- the device code of the three-launch exclusive u32 scan (per-workgroup sums, a scan of the sums, the
// final pass); dbscan.hip and track.hip wrap it in __global__ kernels over their own arguments.
constexpr int kScanPer = 4 * kT;  // entries per workgroup, 4 per thread
// *total = the sum of the kScanPer entries of `in` from b0 on, entries from n on counting 0.  ws: kW words of LDS.
__device__ __forceinline__ void scan_block_sum(const uint32_t *in, int64_t n, int64_t b0, uint32_t *ws, uint32_t *total)
{
    uint32_t v = 0;
    for (int u = 0; u < 4; ++u) {
        const int64_t i = b0 + threadIdx.x * 4 + u;
        v += i < n ? in[i] : 0;
    }
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < kW; ++w) t += ws[w];
        *total = t;
    }
}
// kScanPer entries from b0 on: out[i] = base + the sum of in[b0 .. i) for i < nout, entries from nin on
// counting 0; returns base + the sum of the thread's own and all earlier entries.  in == out is fine: a thread
// reads its four before it writes them.  ws: kW words of LDS, free again after the caller's next barrier.
__device__ __forceinline__ uint32_t scan_block(const uint32_t *in, int64_t nin, uint32_t *out, int64_t nout,
                                               int64_t b0, uint32_t base, uint32_t *ws)
{
    uint32_t v[4], s = 0;
    for (int u = 0; u < 4; ++u) {
        const int64_t i = b0 + threadIdx.x * 4 + u;
        v[u] = i < nin ? in[i] : 0;
        s += v[u];
    }
    uint32_t e = base + block_excl_scan_u32(s, ws);
    for (int u = 0; u < 4; ++u) {
        const int64_t i = b0 + threadIdx.x * 4 + u;
        if (i < nout) out[i] = e;
        e += v[u];
    }
    return e;
}

// lane l's value of v in every lane (l wave-uniform: the result lives in scalar registers)
__device__ __forceinline__ double readlane_d(double v, int l)
{
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), l);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

// ------------------------------------------------------------------ DBSCAN parameter block
// params (double) P: [0] n, [1] eps, [2..4] lo, [5..7] hi, [8] cell, [9..11] dims,
// [12] ncell, [13] clusters, [14] active (n > 10 for the preprocess path), [15] stencil radius
// R in cells (1 or 2), [16] same-cell shortcut (1: cells of side eps/sqrt(3), see dbscan_setup),
// [17] class_people.hip's point count of the whole frame (the length of its selection scan)
enum : int { P_N = 0, P_EPS = 1, P_LO = 2, P_HI = 5, P_CELL = 8, P_DIM = 9, P_NCELL = 12,
             P_NCLUST = 13, P_ACTIVE = 14, P_R = 15, P_INTRA = 16, P_NALL = 17, P_COUNT = 20 };

// ------------------------------------------------------------------ DBSCAN workspace
// One frame's DBSCAN buffers (carve_dbscan names, types and sizes them) and the points x they
// cluster: the preprocess path's scaled cloud inside the same workspace, or the caller's own array
// (a single frame, wss == 0).  Passed to every DBSCAN kernel by value.
struct DbscanWs {
    const double *x;
    double *P;
    uint32_t *cid, *cellcnt, *cellstart, *fill, *order, *flag, *rank, *partial;
    double *sxyz;
    int32_t *cnt, *parent;
    uint8_t *core;  // per sorted slot; `fill` doubles as the cells' smallest core index after the scatter
    int64_t max_cells, nblk_cells, nblk_pts;
    // frame blockIdx.y's view: every buffer at the same offset of that frame's wss bytes
    __device__ __forceinline__ DbscanWs frame(const FrameMap &fm) const
    {
        DbscanWs f = *this;
        f.x = fm.ws(x);
        f.P = fm.ws(P);
        f.cid = fm.ws(cid);
        f.cellcnt = fm.ws(cellcnt);
        f.cellstart = fm.ws(cellstart);
        f.fill = fm.ws(fill);
        f.order = fm.ws(order);
        f.flag = fm.ws(flag);
        f.rank = fm.ws(rank);
        f.partial = fm.ws(partial);
        f.sxyz = fm.ws(sxyz);
        f.cnt = fm.ws(cnt);
        f.parent = fm.ws(parent);
        f.core = fm.ws(core);
        return f;
    }
};

inline int64_t max_cells_for(int64_t n) { return std::min<int64_t>(8 * n + 64, 1 << 22); }

// blocks per frame of a per-point kernel: enough to fill the chip across all frames
inline unsigned point_blocks(int64_t nmax, int frames)
{
    const int64_t cap = std::max<int64_t>(8, 4096 / std::max(1, frames));
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((nmax + 255) / 256, cap));
}

// ---- dbscan.hip, for the preprocess path
// The DBSCAN workspace of one frame of n points, in carve order.  Called twice from the same carver
// position: with base == nullptr to size the allocation (cv.off afterwards), then with the
// allocation for the pointers.  w.x is the caller's to set.
DbscanWs carve_dbscan(Carver &cv, int64_t n, char *base);
// every frame's parameter block P from its preprocess scalars (point count, eps, scaled bbox)
void dbscan_params_from_scalars(const double *scalars, const DbscanWs &w, hipStream_t s, FrameMap fm, int frames);
// the DBSCAN pipeline on w.x (P[P_N] points, eps P[P_EPS], bbox in P) -> labels, for every frame
// exact_counts: cnt[i] is the full eps-neighbour count (radius counts, the standalone API's
// counts output); otherwise counting stops at min_samples.  h: profiling spans (may be null).
int run_dbscan(lidar_handle *h, int64_t nmax, int32_t min_samples, const DbscanWs &w, int64_t *labels, hipStream_t s,
               FrameMap fm, int frames, bool count_only = false, bool exact_counts = false);
// every frame's cluster count, from P into its scalars
void dbscan_nclust_to_scalars(const DbscanWs &w, double *scalars, hipStream_t s, FrameMap fm, int frames);
// exclusive scan of every frame's P[idx] (+extra) entries of src into dst (dst[count] = the total), src
// and dst unshifted pointers into the workspace; nblk: w.nblk_pts / w.nblk_cells, whichever bounds the count
int scan_u32(const DbscanWs &w, const uint32_t *src, uint32_t *dst, int idx, int64_t extra, int64_t nblk, hipStream_t s,
             FrameMap fm, int frames);

// ---- density_grid.hip, for class_people.hip
// people_kernel over `frames` frames: frame f's rows of xyz (3), labels (1) and people (2) start at row
// fm.offs[f], its point count is scalars[f][S_NIN] (status slot 0), its cluster count kdev[f]
int people_of_frames(lidar_handle *h, const double *xyz, const int64_t *labels, int64_t max_n, const int64_t *kdev,
                     double *people, const double *scalars, hipStream_t s, FrameMap fm, int frames);

}  // namespace tier_r
}  // namespace lidar
