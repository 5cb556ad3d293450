// dbscan.hip — sklearn DBSCAN(eps, min_samples) of the reference density path (Tier R), exact.
//
//   dbscan_*           data_processing.py:197 sklearn DBSCAN(eps, min_samples=5):
//                      counting-sort voxel hash (cells > eps, 27-cell stencil), fp64
//                      ((dx*dx+dy*dy)+dz*dz) <= eps*eps counts, union-find over core-core
//                      edges (root = min index), rank by min core index, border = min
//                      adjacent label.  Order-independent: identical to dbscan_inner's DFS.
#include <cmath>
#include <type_traits>

#include "tier_r.hpp"

namespace {

using namespace lidar::tier_r;

// ------------------------------------------------------------------ DBSCAN
__global__ void dbscan_params_from_preprocess(const double *S_in, DbscanWs w, FrameMap fm)
{
    if (threadIdx.x) return;
    const double *S = fm.scal(S_in);
    double *P = w.frame(fm).P;
    const double nng = S[S_NNG];
    P[P_N] = nng;
    P[P_EPS] = S[S_EPS];
    P[P_ACTIVE] = (S[S_STATUS] == 0.0 && nng > 10.0) ? 1.0 : 0.0;
    // dbscan_labels_kernel counts the clusters of an active frame only, and this block lives in the handle's
    // workspace: a frame DBSCAN skips must not report what an earlier call left in the slot.  Its non-ground
    // points (1 .. 10 of them) all take label 0 (cluster_label_scatter_kernel): one cluster; a failed frame has none.
    P[P_NCLUST] = (S[S_STATUS] == 0.0 && nng >= 1.0) ? 1.0 : 0.0;
    for (int c = 0; c < 3; ++c) {
        P[P_LO + c] = S[S_SLO + c];
        P[P_HI + c] = S[S_SHI + c];
    }
}

__global__ __launch_bounds__(kT) void dbscan_bbox_kernel(DbscanWs w, FrameMap fm)
{
    w = w.frame(fm);
    __shared__ BlockScratch s;
    block_bbox(s, w.x, (int64_t)w.P[P_N], w.P + P_LO, w.P + P_HI);
}

// Cell side.  Preferred: s = eps / sqrt(3) * (1 - 2^-20) ("fine" cells).  Any two points of one
// fine cell are eps-neighbours under the fp64 test: the cell coordinate floor((v - lo) / s) of a
// point inside the bbox carries < 2^-29 relative rounding at < 2^22 cells per axis, so the per-axis
// gaps inside a cell stay below s (1 + 2^-29), and the computed ((dx*dx + dy*dy) + dz*dz) below
// 3 s^2 (1 + 2^-26) < eps*eps (1 - 2^-20); a neighbour lies at most ceil(eps / s) = 2 cells away
// per axis (R = 2).  When the fine grid exceeds the cell cap: cells strictly larger than eps
// (R = 1, no same-cell shortcut), grown by 1.5 until they fit.
__global__ void dbscan_setup_kernel(DbscanWs w, FrameMap fm)
{
    if (threadIdx.x) return;
    double *P = w.frame(fm).P;
    const double n = P[P_N], eps = P[P_EPS];
    const double cap = fmin(8.0 * n + 64.0, (double)w.max_cells);
    double dims[3] = {1.0, 1.0, 1.0}, tot = 1.0, cell = 1.0, R = 1.0, intra = 0.0;
    auto fits = [&](double c) {
        tot = 1.0;
        for (int k = 0; k < 3; ++k) {
            dims[k] = floor((P[P_HI + k] - P[P_LO + k]) / c) + 1.0;
            tot *= dims[k];
        }
        return tot <= cap;  // a non-finite box never fits
    };
    const double fine = eps / sqrt(3.0) * (1.0 - 1.0 / 1048576.0);
    if (P[P_ACTIVE] == 0.0 || !(eps > 0.0) || !(eps < INFINITY)) {
        P[P_ACTIVE] = 0.0;
    } else if (fits(fine)) {
        cell = fine;
        R = 2.0;
        intra = 1.0;
    } else {
        // cells strictly larger than eps: a 27-cell stencil sees every pair the fp64 test accepts
        cell = eps * (1.0 + 1.0 / 1048576.0);
        bool fit = false;
        for (int it = 0; it < 256 && !(fit = fits(cell)); ++it) cell *= 1.5;  // bounded: 1.5^256
        if (!fit) {  // non-finite box: one cell (still exact, only slower)
            dims[0] = dims[1] = dims[2] = 1.0;
            tot = 1.0;
            cell = INFINITY;
        }
    }
    P[P_CELL] = cell;
    for (int c = 0; c < 3; ++c) P[P_DIM + c] = dims[c];
    P[P_NCELL] = tot;
    P[P_R] = R;
    P[P_INTRA] = intra;
}

__device__ __forceinline__ int64_t cell_coord(double v, double lo, double cell, int64_t dim)
{
    int64_t c = (int64_t)floor((v - lo) / cell);
    return c < 0 ? 0 : (c >= dim ? dim - 1 : c);
}

struct Grid {
    double lo[3], cell, eps2;
    int64_t dim[3], n;
    int R;       // stencil radius in cells per axis
    bool intra;  // fine cells: any two points of one cell are neighbours
    __device__ void load(const double *P)
    {
        for (int c = 0; c < 3; ++c) {
            lo[c] = P[P_LO + c];
            dim[c] = (int64_t)P[P_DIM + c];
        }
        cell = P[P_CELL];
        eps2 = dmul(P[P_EPS], P[P_EPS]);
        n = (int64_t)P[P_N];
        R = (int)P[P_R];
        intra = P[P_INTRA] != 0.0;
    }
    __device__ int64_t cid(const double *p) const
    {
        return (cell_coord(p[0], lo[0], cell, dim[0]) * dim[1] + cell_coord(p[1], lo[1], cell, dim[1])) * dim[2] +
               cell_coord(p[2], lo[2], cell, dim[2]);
    }
};

// The generic kernels below (fill, copy, scan) take the workspace for the element count P[idx] (+extra)
// and their operands, which differ per call, as explicit unshifted pointers into it.
__global__ void fill_u32_kernel(DbscanWs w, uint32_t *dst, int idx, int64_t extra, uint32_t v, FrameMap fm)
{
    uint32_t *a = fm.ws(dst);
    const int64_t n = (int64_t)w.frame(fm).P[idx] + extra;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        a[i] = v;
}

__global__ void dbscan_cells_kernel(DbscanWs w, FrameMap fm)
{
    w = w.frame(fm);
    if (w.P[P_ACTIVE] == 0.0) return;
    Grid g;
    g.load(w.P);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < g.n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t c = (uint32_t)g.cid(w.x + 3 * i);
        w.cid[i] = c;
        w.parent[i] = (int32_t)i;
        atomicAdd(&w.cellcnt[c], 1u);
    }
}

// --- exclusive scan of u32 over count = P[idx] (+extra) entries; out[count] = total (tier_r.hpp's
// scan_block_sum and scan_block, one frame per blockIdx.y)
__global__ __launch_bounds__(kT) void scan_partial_kernel(DbscanWs w, const uint32_t *src, int idx, int64_t extra,
                                                          FrameMap fm)
{
    __shared__ uint32_t ws[kW];
    w = w.frame(fm);
    scan_block_sum(fm.ws(src), (int64_t)w.P[idx] + extra, (int64_t)blockIdx.x * kScanPer, ws, &w.partial[blockIdx.x]);
}
__global__ __launch_bounds__(kT) void scan_top_kernel(DbscanWs w, int64_t nblk, FrameMap fm)
{
    __shared__ uint32_t ws[kW];
    uint32_t *partial = w.frame(fm).partial;
    scan_block(partial, nblk, partial, nblk, 0, 0u, ws);  // nblk <= kScanPer
}
__global__ __launch_bounds__(kT) void scan_final_kernel(DbscanWs w, const uint32_t *src, uint32_t *dst, int idx,
                                                        int64_t extra, FrameMap fm)
{
    __shared__ uint32_t ws[kW];
    w = w.frame(fm);
    const int64_t n = (int64_t)w.P[idx] + extra;
    const int64_t b0 = (int64_t)blockIdx.x * kScanPer;
    if (b0 > n) return;
    scan_block(fm.ws(src), n, fm.ws(dst), n + 1, b0, w.partial[blockIdx.x], ws);  // out[n] = total
}

__global__ void dbscan_scatter_kernel(DbscanWs w, FrameMap fm)
{
    w = w.frame(fm);
    if (w.P[P_ACTIVE] == 0.0) return;
    const int64_t n = (int64_t)w.P[P_N];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t pos = atomicAdd(&w.fill[w.cid[i]], 1u);
        w.order[pos] = (uint32_t)i;
        w.sxyz[3 * pos] = w.x[3 * i];
        w.sxyz[3 * pos + 1] = w.x[3 * i + 1];
        w.sxyz[3 * pos + 2] = w.x[3 * i + 2];
    }
}

__global__ void copy_u32_kernel(DbscanWs w, uint32_t *dst, const uint32_t *src, int idx, int64_t extra, FrameMap fm)
{
    uint32_t *d = fm.ws(dst);
    const uint32_t *a = fm.ws(src);
    const int64_t n = (int64_t)w.frame(fm).P[idx] + extra;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        d[i] = a[i];
}

// visit every sorted slot u whose point is within eps of point (px,py,pz) in cell c: the
// (2R+1)^2 columns around c, each a contiguous z-run of 2R+1 cells in the sorted order
template <class F>
__device__ __forceinline__ void for_neighbours(const Grid &g, const uint32_t *start, const double *sxyz,
                                               double px, double py, double pz, uint32_t c, F &&f)
{
    const int64_t cz = c % g.dim[2], cy = (c / g.dim[2]) % g.dim[1], cx = c / (g.dim[2] * g.dim[1]);
    const int64_t z0 = cz - g.R > 0 ? cz - g.R : 0, z1 = cz + g.R < g.dim[2] ? cz + g.R : g.dim[2] - 1;
    for (int64_t X = cx - g.R; X <= cx + g.R; ++X) {
        if (X < 0 || X >= g.dim[0]) continue;
        for (int64_t Y = cy - g.R; Y <= cy + g.R; ++Y) {
            if (Y < 0 || Y >= g.dim[1]) continue;
            const int64_t col = (X * g.dim[1] + Y) * g.dim[2];
            const uint32_t u0 = start[col + z0], u1 = start[col + z1 + 1];
            for (uint32_t u = u0; u < u1; ++u) {
                const double d = lidar::dist2d(px, py, pz, sxyz[3 * u], sxyz[3 * u + 1], sxyz[3 * u + 2]);
                if (d <= g.eps2) f(u);
            }
        }
    }
}

// eps-neighbour count of a point, stopping once it reaches `limit`: DBSCAN only asks whether
// cnt >= min_samples, and a standardized dense frame (eps 0.5 on unit-variance data) has hundreds
// of neighbours per point among thousands of candidates
__device__ __forceinline__ int32_t count_neighbours(const Grid &g, const uint32_t *start, const double *sxyz,
                                                    double px, double py, double pz, uint32_t c, int32_t limit)
{
    const int64_t cz = c % g.dim[2], cy = (c / g.dim[2]) % g.dim[1], cx = c / (g.dim[2] * g.dim[1]);
    const int64_t z0 = cz - g.R > 0 ? cz - g.R : 0, z1 = cz + g.R < g.dim[2] ? cz + g.R : g.dim[2] - 1;
    const int W = 2 * g.R + 1, centre = g.R * W + g.R;
    int32_t k = 0;
    // the point's own (X, Y) column first: the likeliest place to find `limit` hits
    for (int r = 0; r < W * W; ++r) {
        const int q = r == 0 ? centre : (r <= centre ? r - 1 : r);  // row-major columns, centre moved first
        const int64_t X = cx + q / W - g.R, Y = cy + q % W - g.R;
        if (X < 0 || X >= g.dim[0] || Y < 0 || Y >= g.dim[1]) continue;
        const int64_t col = (X * g.dim[1] + Y) * g.dim[2];
        const uint32_t u0 = start[col + z0], u1 = start[col + z1 + 1];
        for (uint32_t u = u0; u < u1; ++u) {
            const double d = lidar::dist2d(px, py, pz, sxyz[3 * u], sxyz[3 * u + 1], sxyz[3 * u + 2]);
            if (d <= g.eps2 && ++k >= limit) return k;
        }
    }
    return k;
}

constexpr uint32_t kNoCore = 0xffffffffu;

// eps-neighbour counts (stopping at `limit`); with `cores` also the core flag of every sorted slot
// and rep[c] = the smallest core index of cell c (rep = fill, initialised to kNoCore).  Fine cells:
// every point of a cell is a neighbour, so a cell of >= limit points settles its points' counts
// without a distance test.
__global__ void dbscan_count_kernel(DbscanWs w, int32_t limit, int32_t min_samples, bool cores, FrameMap fm)
{
    w = w.frame(fm);
    if (w.P[P_ACTIVE] == 0.0) return;
    Grid g;
    g.load(w.P);
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < g.n; t += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t i = w.order[t], c = w.cid[i];
        const int64_t in_cell = (int64_t)w.cellstart[c + 1] - w.cellstart[c];
        const int32_t k = g.intra && in_cell >= limit
                              ? (int32_t)in_cell
                              : count_neighbours(g, w.cellstart, w.sxyz, w.sxyz[3 * t], w.sxyz[3 * t + 1], w.sxyz[3 * t + 2], c, limit);
        w.cnt[i] = k;
        if (cores) {
            const bool is_core = k >= min_samples;
            w.core[t] = is_core ? 1 : 0;
            if (is_core) atomicMin(w.fill + c, i);
        }
    }
}

__device__ __forceinline__ int32_t ld(const int32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st(int32_t *p, int32_t v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// find with path halving.  Invariant: parent[x] <= x (roots hook under smaller roots), so
// every pointer moves toward the component minimum and the halving stores (x's parent
// becomes its grandparent, an ancestor in the same component) are benign under races.
__device__ int32_t uf_find(int32_t *parent, int32_t x)
{
    int32_t p = ld(parent + x);
    while (p != x) {
        const int32_t gp = ld(parent + p);
        if (gp != p) st(parent + x, gp);
        x = p;
        p = gp;
    }
    return x;
}
// read-only find: the roots pass publishes parent[i] = root for the labels pass, and a
// halving store racing behind that publish would leave a non-root there
__device__ int32_t uf_find_ro(const int32_t *parent, int32_t x)
{
    int32_t p = ld(parent + x);
    while (p != x) {
        x = p;
        p = ld(parent + x);
    }
    return x;
}
// join the components of roots-or-members a and b; returns the (current) smaller root
__device__ int32_t uf_unite(int32_t *parent, int32_t a, int32_t b)
{
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return a;
        if (a < b) {
            const int32_t t = a;
            a = b;
            b = t;
        }
        // hook the larger root under the smaller: the final root is the component minimum
        const int32_t old = atomicCAS(parent + a, a, b);
        if (old == a) return b;
        a = old;
    }
}

__global__ void dbscan_union_kernel(DbscanWs w, int32_t min_samples, FrameMap fm)
{
    w = w.frame(fm);
    if (w.P[P_ACTIVE] == 0.0 || w.P[P_INTRA] != 0.0) return;  // fine cells: dbscan_intra + dbscan_cross
    Grid g;
    g.load(w.P);
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < g.n; t += (int64_t)gridDim.x * blockDim.x) {
        const int32_t i = (int32_t)w.order[t];
        if (w.cnt[i] < min_samples) continue;
        // i's root is cached across its neighbours: a neighbour already in the same
        // component costs one (halving) find, not two
        int32_t ri = uf_find(w.parent, i);
        for_neighbours(g, w.cellstart, w.sxyz, w.sxyz[3 * t], w.sxyz[3 * t + 1], w.sxyz[3 * t + 2], w.cid[i], [&](uint32_t u) {
            const int32_t j = (int32_t)w.order[u];
            if (j < i && w.cnt[j] >= min_samples) {
                if (ld(w.parent + j) == ri) return;  // already hooked straight under i's root
                const int32_t rj = uf_find(w.parent, j);
                if (rj != ri) ri = uf_unite(w.parent, ri, rj);
            }
        });
    }
}

// Fine cells, step 1: every core point of a cell hooks straight under the cell's smallest core
// index (all of a cell's points are mutually eps-neighbours; parent[i] <= i holds, and no other
// kernel writes parent meanwhile).
__global__ void dbscan_intra_kernel(DbscanWs w, FrameMap fm)
{
    w = w.frame(fm);
    if (w.P[P_ACTIVE] == 0.0 || w.P[P_INTRA] == 0.0) return;
    const uint32_t *rep = w.fill;  // the cells' smallest core index
    const int64_t n = (int64_t)w.P[P_N];
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        if (!w.core[t]) continue;
        const uint32_t i = w.order[t], r = rep[w.cid[i]];
        if (r != i) w.parent[i] = (int32_t)r;
    }
}

// Fine cells, step 2: one thread per (cell A, offset o) over the 62 offsets of [-2, 2]^3 that come
// lexicographically after (0, 0, 0) — every pair of cells within the stencil once.  If A and B =
// A + o both hold core points that are not yet one component, any core of A within eps of any
// core of B links them.  Each cell's cores are one component (step 1), so the components after
// this pass are exactly those of the core-core eps graph.
//
// The 62 offsets run in two launches: first the 13 touching cells (Chebyshev distance 1), which in
// a dense frame link almost every pair at the first core tested and merge nearly everything into
// few components; then the 49 offsets two cells out, most of whose pairs are by then already one
// component (two finds and out) instead of a full core x core scan that finds no link.  Union-find
// yields the connected components whatever the order of the unions, so the split is exact.
// A core u of A whose gap to B's cell box exceeds eps is skipped: the box is taken one part in 2^10
// of a cell larger on every side, far beyond the rounding of floor((v - lo) / s), so it contains
// every point binned into B, and the gap never overstates a true distance.
constexpr int kPairOffsets = 62, kNearOffsets = 13;
struct PairOffsets {
    int o[kPairOffsets];
    constexpr PairOffsets() : o{}
    {
        int k = 0;
        for (int pass = 0; pass < 2; ++pass)
            for (int v = 63; v < 125; ++v) {  // 5x5x5 row-major; (0,0,0) is 62, after it come the 62
                const int dx = v / 25 - 2, dy = (v / 5) % 5 - 2, dz = v % 5 - 2;
                const bool near = dx >= -1 && dx <= 1 && dy >= -1 && dy <= 1 && dz >= -1 && dz <= 1;
                if (near == (pass == 0)) o[k++] = v;
            }
    }
};
__constant__ PairOffsets kOffsets = PairOffsets();

__device__ __forceinline__ double box_gap(double v, double lo, double hi)
{
    const double a = lo - v, b = v - hi;
    return a > 0.0 ? a : (b > 0.0 ? b : 0.0);
}

__global__ void dbscan_cross_kernel(DbscanWs w, int o0, int no, FrameMap fm)
{
    w = w.frame(fm);
    if (w.P[P_ACTIVE] == 0.0 || w.P[P_INTRA] == 0.0) return;
    Grid g;
    g.load(w.P);
    const double slack = g.cell * (1.0 / 1024.0);
    const int64_t work = (int64_t)w.P[P_NCELL] * no;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < work; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t A = j / no;
        const uint32_t ra0 = w.fill[A];  // fill: the cells' smallest core index
        if (ra0 == kNoCore) continue;
        const int o = kOffsets.o[o0 + (int)(j - A * no)];
        const int64_t ax = A / (g.dim[1] * g.dim[2]), ay = (A / g.dim[2]) % g.dim[1], az = A % g.dim[2];
        const int64_t bx = ax + o / 25 - 2, by = ay + (o / 5) % 5 - 2, bz = az + o % 5 - 2;
        if (bx < 0 || bx >= g.dim[0] || by < 0 || by >= g.dim[1] || bz < 0 || bz >= g.dim[2]) continue;
        const int64_t B = (bx * g.dim[1] + by) * g.dim[2] + bz;
        const uint32_t rb0 = w.fill[B];
        if (rb0 == kNoCore) continue;
        const int32_t ra = uf_find(w.parent, (int32_t)ra0), rb = uf_find(w.parent, (int32_t)rb0);
        if (ra == rb) continue;
        double blo[3], bhi[3];
        const int64_t bc[3] = {bx, by, bz};
        for (int k = 0; k < 3; ++k) {
            blo[k] = g.lo[k] + (double)bc[k] * g.cell - slack;
            bhi[k] = g.lo[k] + (double)(bc[k] + 1) * g.cell + slack;
        }
        bool linked = false;
        const uint32_t b0 = w.cellstart[B], b1 = w.cellstart[B + 1];
        for (uint32_t u = w.cellstart[A], u1 = w.cellstart[A + 1]; u < u1 && !linked; ++u) {
            if (!w.core[u]) continue;
            const double px = w.sxyz[3 * u], py = w.sxyz[3 * u + 1], pz = w.sxyz[3 * u + 2];
            const double gx = box_gap(px, blo[0], bhi[0]), gy = box_gap(py, blo[1], bhi[1]),
                         gz = box_gap(pz, blo[2], bhi[2]);
            if ((gx * gx + gy * gy) + gz * gz > g.eps2) continue;
            for (uint32_t v = b0; v < b1; ++v)
                if (w.core[v] && lidar::dist2d(px, py, pz, w.sxyz[3 * v], w.sxyz[3 * v + 1], w.sxyz[3 * v + 2]) <= g.eps2) {
                    linked = true;
                    break;
                }
        }
        if (linked) uf_unite(w.parent, ra, rb);
    }
}

__global__ void dbscan_roots_kernel(DbscanWs w, int32_t min_samples, FrameMap fm)
{
    w = w.frame(fm);
    const int64_t n = (int64_t)w.P[P_N];
    const bool active = w.P[P_ACTIVE] != 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        uint32_t f = 0;
        if (active && w.cnt[i] >= min_samples) {
            const int32_t r = uf_find_ro(w.parent, (int32_t)i);
            w.parent[i] = r;
            f = r == (int32_t)i ? 1u : 0u;
        }
        w.flag[i] = f;
    }
}

// labels: the caller's array (a single frame) or a workspace buffer at the same offset in every frame
__global__ void dbscan_labels_kernel(DbscanWs w, int32_t min_samples, int64_t *labels_in, FrameMap fm)
{
    w = w.frame(fm);
    int64_t *labels = fm.ws(labels_in);
    if (w.P[P_ACTIVE] == 0.0) return;
    Grid g;
    g.load(w.P);
    if (blockIdx.x == 0 && threadIdx.x == 0) w.P[P_NCLUST] = (double)w.rank[g.n];
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < g.n; t += (int64_t)gridDim.x * blockDim.x) {
        const int32_t i = (int32_t)w.order[t];
        int64_t lab;
        if (w.cnt[i] >= min_samples) {
            lab = w.rank[w.parent[i]];
        } else {
            int64_t best = -1;
            for_neighbours(g, w.cellstart, w.sxyz, w.sxyz[3 * t], w.sxyz[3 * t + 1], w.sxyz[3 * t + 2], w.cid[i], [&](uint32_t u) {
                if (w.core[u]) {
                    const int64_t l = w.rank[w.parent[w.order[u]]];
                    if (best < 0 || l < best) best = l;
                }
            });
            lab = best;
        }
        labels[i] = lab;
    }
}

__global__ void nclust_kernel(DbscanWs w, double *S_in, FrameMap fm)
{
    if (threadIdx.x == 0) fm.scal(S_in)[S_NCLUST] = w.frame(fm).P[P_NCLUST];
}

// exclusive scan of P[idx] (+extra) entries of src into dst (dst[count] = the total), through w.partial
int run_scan(const DbscanWs &w, const uint32_t *src, uint32_t *dst, int idx, int64_t extra, int64_t nblk, hipStream_t s,
             FrameMap fm, int frames)
{
    hipLaunchKernelGGL(scan_partial_kernel, dim3((unsigned)nblk, frames), dim3(kT), 0, s, w, src, idx, extra, fm);
    hipLaunchKernelGGL(scan_top_kernel, dim3(1, frames), dim3(kT), 0, s, w, nblk, fm);
    hipLaunchKernelGGL(scan_final_kernel, dim3((unsigned)nblk, frames), dim3(kT), 0, s, w, src, dst, idx, extra, fm);
    LAUNCH_CHECK();
    return LIDAR_OK;
}

}  // namespace

namespace lidar {
namespace tier_r {

// every sub-buffer is named, typed and sized here, in carve order
DbscanWs carve_dbscan(Carver &cv, int64_t n, char *base)
{
    DbscanWs w;
    auto part = [&](auto *&p, uint64_t count) {
        using T = std::remove_reference_t<decltype(*p)>;
        p = reinterpret_cast<T *>(reinterpret_cast<uintptr_t>(base) + cv.take<T>(count));
    };
    w.x = nullptr;
    w.max_cells = max_cells_for(n);
    w.nblk_cells = (w.max_cells + 1 + kScanPer - 1) / kScanPer;
    w.nblk_pts = (n + 1 + kScanPer - 1) / kScanPer;
    part(w.P, P_COUNT);
    part(w.cid, n);
    part(w.cellcnt, w.max_cells + 1);
    part(w.cellstart, w.max_cells + 1);
    part(w.fill, w.max_cells + 1);
    part(w.order, n + 1);
    part(w.flag, n + 1);
    part(w.rank, n + 1);
    part(w.partial, 4 * kT);
    part(w.sxyz, 3 * n);
    part(w.cnt, n);
    part(w.parent, n);
    part(w.core, n);
    return w;
}

void dbscan_params_from_scalars(const double *scalars, const DbscanWs &w, hipStream_t s, FrameMap fm, int frames)
{
    hipLaunchKernelGGL(dbscan_params_from_preprocess, dim3(1, frames), dim3(64), 0, s, scalars, w, fm);
}

void dbscan_nclust_to_scalars(const DbscanWs &w, double *scalars, hipStream_t s, FrameMap fm, int frames)
{
    hipLaunchKernelGGL(nclust_kernel, dim3(1, frames), dim3(64), 0, s, w, scalars, fm);
}

int scan_u32(const DbscanWs &w, const uint32_t *src, uint32_t *dst, int idx, int64_t extra, int64_t nblk, hipStream_t s,
             FrameMap fm, int frames)
{
    return run_scan(w, src, dst, idx, extra, nblk, s, fm, frames);
}

int run_dbscan(lidar_handle *h, int64_t nmax, int32_t min_samples, const DbscanWs &w, int64_t *labels, hipStream_t s,
               FrameMap fm, int frames, bool count_only, bool exact_counts)
{
    const int32_t limit = (count_only || exact_counts) ? 0x7fffffff : min_samples;
    const unsigned gp = point_blocks(nmax, frames);
    const unsigned gc = point_blocks(w.max_cells, frames);
    const unsigned gx = point_blocks(w.max_cells * (kPairOffsets - kNearOffsets), frames);
    const unsigned gn = point_blocks(w.max_cells * kNearOffsets, frames);
    const dim3 F1(1, frames), FP(gp, frames), FC(gc, frames), FX(gx, frames), FN(gn, frames);
    {
        lidar::Span sp(h, "dbscan_grid", s);  // cell sizes, counting sort by cell
        hipLaunchKernelGGL(dbscan_setup_kernel, F1, dim3(64), 0, s, w, fm);
        hipLaunchKernelGGL(fill_u32_kernel, FC, dim3(256), 0, s, w, w.cellcnt, P_NCELL, 1, 0u, fm);
        hipLaunchKernelGGL(dbscan_cells_kernel, FP, dim3(256), 0, s, w, fm);
        int rc = run_scan(w, w.cellcnt, w.cellstart, P_NCELL, 0, w.nblk_cells, s, fm, frames);
        if (rc) return rc;
        hipLaunchKernelGGL(copy_u32_kernel, FC, dim3(256), 0, s, w, w.fill, w.cellstart, P_NCELL, 1, fm);
        hipLaunchKernelGGL(dbscan_scatter_kernel, FP, dim3(256), 0, s, w, fm);
        if (!count_only)  // `fill` is free after the scatter: the cells' smallest core index
            hipLaunchKernelGGL(fill_u32_kernel, FC, dim3(256), 0, s, w, w.fill, P_NCELL, 1, kNoCore, fm);
    }
    {
        lidar::Span sp(h, "dbscan_count", s);
        hipLaunchKernelGGL(dbscan_count_kernel, FP, dim3(256), 0, s, w, limit, min_samples, !count_only, fm);
    }
    if (count_only) {
        LAUNCH_CHECK();
        return LIDAR_OK;
    }
    {
        lidar::Span sp(h, "dbscan_union", s);  // fine cells: intra + cross; coarse cells: per-point union
        hipLaunchKernelGGL(dbscan_intra_kernel, FP, dim3(256), 0, s, w, fm);
        hipLaunchKernelGGL(dbscan_cross_kernel, FN, dim3(256), 0, s, w, 0, kNearOffsets, fm);
        hipLaunchKernelGGL(dbscan_cross_kernel, FX, dim3(256), 0, s, w, kNearOffsets, kPairOffsets - kNearOffsets, fm);
        hipLaunchKernelGGL(dbscan_union_kernel, FP, dim3(256), 0, s, w, min_samples, fm);
    }
    {
        lidar::Span sp(h, "dbscan_labels", s);  // roots, rank scan, labels
        hipLaunchKernelGGL(dbscan_roots_kernel, FP, dim3(256), 0, s, w, min_samples, fm);
        int rc = run_scan(w, w.flag, w.rank, P_N, 0, w.nblk_pts, s, fm, frames);
        if (rc) return rc;
        hipLaunchKernelGGL(dbscan_labels_kernel, FP, dim3(256), 0, s, w, min_samples, labels, fm);
    }
    LAUNCH_CHECK();
    return LIDAR_OK;
}

}  // namespace tier_r
}  // namespace lidar

namespace {

// DBSCAN on the caller's own points (lidar_dbscan_f64, lidar_radius_count_f64): the workspace of one
// frame, its parameter block and bounding box, then run_dbscan.  The block is staged in the
// handle's pinned buffer, which the next call reuses: the caller synchronises s before it returns.
int run_dbscan_on(lidar_handle *h, const double *x, int64_t n, double eps, int32_t min_samples, int64_t *labels,
                  hipStream_t s, bool count_only, bool exact_counts, DbscanWs &w)
{
    lidar::Carver size, cv;
    carve_dbscan(size, n, nullptr);
    char *base = static_cast<char *>(lidar::workspace(h, size.off));
    if (!base) return LIDAR_ENOMEM;
    w = carve_dbscan(cv, n, base);
    w.x = x;
    double *hp = static_cast<double *>(h->host_pinned);
    for (int i = 0; i < P_COUNT; ++i) hp[i] = 0.0;
    hp[P_N] = (double)n;
    hp[P_EPS] = eps;
    hp[P_ACTIVE] = 1.0;
    HIP_TRY(hipMemcpyAsync(w.P, hp, sizeof(double) * P_COUNT, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(dbscan_bbox_kernel, dim3(1), dim3(kT), 0, s, w, FrameMap{});
    return run_dbscan(h, n, min_samples, w, labels, s, FrameMap{}, 1, count_only, exact_counts);
}

}  // namespace

// ====================================================================== C-ABI
LIDAR_EXPORT int lidar_dbscan_f64(lidar_handle *h, const double *x, int64_t n, double eps,
                                  int32_t min_samples, int64_t *labels, int32_t *counts, void *stream)
{
    REQUIRE(h && x && labels, "lidar_dbscan_f64: null pointer");
    REQUIRE(n >= 0 && n < 0x7fffffff, "lidar_dbscan_f64: n out of range");
    REQUIRE(eps > 0.0, "lidar_dbscan_f64: eps must be > 0");
    REQUIRE(min_samples >= 1, "lidar_dbscan_f64: min_samples must be >= 1");
    if (n == 0) return LIDAR_OK;
    ON_DEVICE(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    DbscanWs w;
    int rc = run_dbscan_on(h, x, n, eps, min_samples, labels, s, false, counts != nullptr, w);
    if (rc) return rc;
    if (counts) HIP_TRY(hipMemcpyAsync(counts, w.cnt, sizeof(int32_t) * n, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));  // the pinned parameter block is reused by the next call
    return LIDAR_OK;
}

__global__ void widen_counts_kernel(const int32_t *c, int64_t n, int64_t *out)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = c[i];
}

// KDTree(x).query_radius(x, r, count_only=True) (the reference's density colouring,
// utils/visualization.py:41-48 and :165-168, app_simplified.py:156-159): per point the
// number of points (itself included) with ((dx*dx + dy*dy) + dz*dz) <= r*r in fp64 —
// sklearn's rdist test, the one DBSCAN's neighbour count uses.  2-D data: z = 0.
LIDAR_EXPORT int lidar_radius_count_f64(lidar_handle *h, const double *x, int64_t n, double r, int64_t *counts,
                                        void *stream)
{
    REQUIRE(h && x && counts, "lidar_radius_count_f64: null pointer");
    REQUIRE(n >= 0 && n < 0x7fffffff, "lidar_radius_count_f64: n out of range");
    REQUIRE(r >= 0.0, "lidar_radius_count_f64: r must be >= 0");
    if (n == 0) return LIDAR_OK;
    ON_DEVICE(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    DbscanWs w;
    // r = 0: a tiny positive cell size keeps the grid finite; only exact duplicates count
    int rc = run_dbscan_on(h, x, n, r > 0.0 ? r : 1e-300, 1, nullptr, s, true, false, w);
    if (rc) return rc;
    hipLaunchKernelGGL(widen_counts_kernel, dim3(point_blocks(n, 1)), dim3(256), 0, s, w.cnt, n, counts);
    LAUNCH_CHECK();
    HIP_TRY(hipStreamSynchronize(s));  // the pinned parameter block is reused by the next call
    return LIDAR_OK;
}
