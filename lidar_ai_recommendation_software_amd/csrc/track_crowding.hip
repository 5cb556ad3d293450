// track_crowding.hip — per-person spacing, local density and crowd pressure (DESIGN.md §3 "Crowding", §4.15): how
// tightly packed every tracked person is within its own frame, and whether the people around it move coherently:
// the same-frame pair sweep, where track.hip sweeps a frame against the previous one.
//
// Contract (include/lidar_amd.h repeats it).  All arithmetic fp64, one rounding per operation, square root and
// division correctly rounded.
//   people (T, cap, 2), k (T,), K_t = min(max(k[t], 0), cap), prev (T, cap) int32 and velocity (T, cap, 2) as
//   lidar_track_people_f64 / lidar_track_stream_f64 leave them; only the frames t >= first are evaluated, each on
//   its own.  valid(j): j < K_t and both coordinates finite.  moving(j): valid(j), prev[t][j] >= 0 and both velocity
//   components finite.  d(i, j) = (dx*dx) + (dy*dy), dx = P[i].x - P[j].x, dy = P[i].y - P[j].y.  near(i, j): i != j,
//   valid(i) and d <= R*R (inclusive, R*R one product).  d(i, j) and d(j, i) have the same bits: near is symmetric.
//   Per valid row j (arrays (T - first, cap), indexed by t - first, every element written):
//     neighbours int32   #{i : near(i, j)}
//     nearest int32      the valid i != j with finite d and the smallest (d, i), over the whole frame; -1 without one
//     spacing fp64       sqrt(d(nearest, j)); +inf where nearest == -1
//     density fp64       (double)(neighbours + 1) / ((pi * R) * R)
//     movers int32       m = |M_j|, M_j = {i : moving(i) and (i == j or near(i, j))}
//     variance fp64      sx, sy, sq = the sums of vx, vy, (vx*vx) + (vy*vy) over M_j, added sequentially in ascending
//                        i from +0.0; m >= 2: mx = sx / m, my = sy / m, var = (sq / m) - ((mx*mx) + (my*my)), a
//                        non-NaN var that is not > 0.0 becomes +0.0; m < 2: +0.0
//     pressure fp64      density * variance
//   A row j < K_t that is not valid: neighbours 0, nearest -1, spacing +inf, movers 0, 0.0 for the other doubles, and
//   it is counted nowhere below; a row at or past K_t the same with neighbours -1.
//   crowded (T - first, 2) int32: the valid rows with density >= density_limit, with pressure >= pressure_limit.
//   peaks (T - first, 3) fp64: the largest density, the largest pressure (from +0.0 under >: a NaN never wins), the
//   smallest spacing (from +inf under <) over the valid rows.
//   Cells (nx > 0; tier_r.hpp's arange_bin, rows outside the grid dropped): cell_peak (nx, ny, 2) fp64 the largest
//   density and pressure, cell_crowded (nx, ny) int32 the rows with density >= density_limit, of the valid rows of
//   the frames >= first binned by their own position; accumulate = 0 starts from 0, 1 goes on from what is stored.
//   Every result is an integer, a maximum / minimum over values that are not NaN, or a value one thread computes in
//   a fixed order: the same bits under every schedule.  No floating-point atomic adds.
//
// Kernels: init_kernel (the per-frame summary of a frame with several row tiles, and the cells without accumulate)
// and crowding_kernel, nearest_kernel's form (track.hip): a thread per query row, the grid (row tile, frame), the
// frame's own rows staged through LDS in ascending tiles of kTile and read as broadcasts.  A candidate is
// (x, y, vx, vy): a row that is not valid is staged with a NaN position (its d is NaN: not near, never the
// nearest), a row that is not moving with a NaN velocity, so the inner loop loads nothing beside the tile.  The
// count, the three sums and the running best live in registers; the conditional adds happen while i ascends, which
// is the order of the specification; strict < on ascending i is the tie rule; i == j is skipped by index (two
// people may coincide).  The summary: a ballot or a wave maximum of the bit patterns (the candidates are
// non-negative and not NaN, so the unsigned order of the bits is the order of the values), one LDS atomic per wave,
// then one global atomic per workgroup and non-trivial value; a frame with one row tile stores instead.  A row's
// cell takes an integer atomicMax of the bits and an atomicAdd.
#include <cmath>

#include "track_links.hpp"

namespace {

using namespace lidar::tier_r;
using namespace lidar::track;

constexpr int kB = 256;      // threads of crowding_kernel: one query row each
constexpr int kTile = 1024;  // candidate rows staged in LDS (32 B each: 32 KiB)
constexpr unsigned long long kInfBits = 0x7ff0000000000000ull;

__device__ __forceinline__ bool finite2(double a, double b) { return fabs(a) < INFINITY && fabs(b) < INFINITY; }

__device__ __forceinline__ unsigned long long bits_of(double v) { return (unsigned long long)__double_as_longlong(v); }

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = __shfl_xor(v, m, 64);
        v = o < v ? o : v;
    }
    return v;
}

// crowded (nc int32) = 0; peaks (np / 3 rows of 3 patterns) = (+0.0, +0.0, +inf); cell_peak (ncp patterns) = +0.0;
// cell_crowded (ncc int32) = 0.  A count of 0 leaves its array alone.
__global__ __launch_bounds__(kB) void init_kernel(int32_t *__restrict__ crowded, int64_t nc,
                                                  unsigned long long *__restrict__ peaks, int64_t np,
                                                  unsigned long long *__restrict__ cell_peak, int64_t ncp,
                                                  int32_t *__restrict__ cell_crowded, int64_t ncc)
{
    const int64_t n = nc + np + ncp + ncc;
    for (int64_t e = (int64_t)blockIdx.x * kB + threadIdx.x; e < n; e += (int64_t)gridDim.x * kB) {
        if (e < nc) crowded[e] = 0;
        else if (e < nc + np) peaks[e - nc] = (e - nc) % 3 == 2 ? kInfBits : 0ull;
        else if (e < nc + np + ncp) cell_peak[e - nc - np] = 0ull;
        else cell_crowded[e - nc - np - ncp] = 0;
    }
}

struct Out {
    int32_t *neighbours, *nearest, *movers;
    double *spacing, *density, *variance, *pressure;
    int32_t *crowded;
    unsigned long long *peaks;  // (T - first, 3) fp64 as bit patterns
    unsigned long long *cell_peak;
    int32_t *cell_crowded;
};

// blockIdx.y = t - first; blockIdx.x and gridDim.x stride over the frame's row tiles, every thread of a workgroup
// making the same number of rounds (the ballots, shuffles and barriers are uniform).  gridDim.x == 1: the workgroup
// is the only one of its frame and stores the frame's summary; otherwise it raises what init_kernel set.
// r2 = R*R, area = (pi * R) * R, products of the host (built without contraction, as the device code).
__global__ __launch_bounds__(kB) void crowding_kernel(const double *__restrict__ people, const int64_t *__restrict__ k,
                                                      const int32_t *__restrict__ prev,
                                                      const double *__restrict__ velocity, int64_t cap, int64_t first,
                                                      double r2, double area, double dlim, double plim, double x0,
                                                      double y0, double grid, int64_t nx, int64_t ny, Out o)
{
    __shared__ double2 sp[kTile];  // a candidate's position, NaN for a row that is not valid
    __shared__ double2 sv[kTile];  // its velocity, NaN for a row that is not moving
    __shared__ int32_t cnt[2];
    __shared__ unsigned long long pk[3];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t f = blockIdx.y, t = first + f;
    const int64_t K = clamp_k(k, t, cap);
    const double qnan = __builtin_nan("");
    const double *P = people + t * cap * 2, *V = velocity + t * cap * 2;
    const int32_t *L = prev + t * cap;
    if (tid < 2) cnt[tid] = 0;
    if (tid < 3) pk[tid] = tid == 2 ? kInfBits : 0ull;
    __syncthreads();
    for (int64_t j0 = (int64_t)blockIdx.x * kB; j0 < cap; j0 += (int64_t)gridDim.x * kB) {
        const int64_t j = j0 + tid;
        if (j0 >= K) {  // the whole tile is past the frame's rows: the defaults, no sweep
            if (j < cap) {
                const int64_t e = f * cap + j;
                o.neighbours[e] = -1;
                o.nearest[e] = -1;
                o.movers[e] = 0;
                o.spacing[e] = INFINITY;
                o.density[e] = 0.0;
                o.variance[e] = 0.0;
                o.pressure[e] = 0.0;
            }
            continue;
        }
        double qx = qnan, qy = qnan;  // a thread without a valid row keeps NaN: no pair passes a comparison
        if (j < K) {
            qx = P[2 * j];
            qy = P[2 * j + 1];
        }
        const bool valid = finite2(qx, qy);
        const int32_t self = (int32_t)j;
        int32_t nb = 0, m = 0, bi = -1;
        double best = INFINITY, sx = 0.0, sy = 0.0, sq = 0.0;
        for (int64_t c0 = 0; c0 < K; c0 += kTile) {  // ascending: the order of the sums and the tie rule
            const int n = (int)(K - c0 < kTile ? K - c0 : kTile), n4 = (n + 3) & ~3;
            __syncthreads();  // the previous tile has been read by every wave
            for (int i = tid; i < n4; i += kB) {
                double2 p = make_double2(qnan, qnan), v = make_double2(qnan, qnan);
                if (i < n) {
                    const int64_t c = c0 + i;  // < K <= cap
                    const double x = P[2 * c], y = P[2 * c + 1], vx = V[2 * c], vy = V[2 * c + 1];
                    if (finite2(x, y)) {
                        p = make_double2(x, y);
                        if (L[c] >= 0 && finite2(vx, vy)) v = make_double2(vx, vy);
                    }
                }
                sp[i] = p;
                sv[i] = v;
            }
            __syncthreads();
            const int32_t ibase = (int32_t)c0;
            for (int i = 0; i < n4; i += 4) {
                const double2 p4[4] = {sp[i], sp[i + 1], sp[i + 2], sp[i + 3]};
                const double2 v4[4] = {sv[i], sv[i + 1], sv[i + 2], sv[i + 3]};
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const double dx = dsub(p4[w].x, qx), dy = dsub(p4[w].y, qy);
                    const double d = dadd(dmul(dx, dx), dmul(dy, dy));
                    const bool other = ibase + i + w != self;
                    const bool near = other && d <= r2;  // a NaN on either side: false
                    nb += near;
                    if (other && d < best) {  // d is finite: below a best that starts at +inf
                        best = d;
                        bi = ibase + i + w;
                    }
                    // the row itself takes its place in the ascending order (valid: an invalid row's own staged
                    // velocity is NaN already)
                    if ((near || !other) && v4[w].x == v4[w].x) {
                        sx = dadd(sx, v4[w].x);
                        sy = dadd(sy, v4[w].y);
                        sq = dadd(sq, dadd(dmul(v4[w].x, v4[w].x), dmul(v4[w].y, v4[w].y)));
                        ++m;
                    }
                }
            }
        }
        double spacing = INFINITY, density = 0.0, var = 0.0, pressure = 0.0;
        if (valid) {
            if (bi >= 0) spacing = __dsqrt_rn(best);
            density = ddiv((double)(nb + 1), area);
            if (m >= 2) {
                const double md = (double)m, mx = ddiv(sx, md), my = ddiv(sy, md);
                var = dsub(ddiv(sq, md), dadd(dmul(mx, mx), dmul(my, my)));
                if (var == var && !(var > 0.0)) var = 0.0;  // neither a negative value nor -0.0 is stored
            }
            pressure = dmul(density, var);
        } else {
            nb = j < K ? 0 : -1;
            m = 0;
            bi = -1;
        }
        if (j < cap) {
            const int64_t e = f * cap + j;
            o.neighbours[e] = nb;
            o.nearest[e] = bi;
            o.movers[e] = m;
            o.spacing[e] = spacing;
            o.density[e] = density;
            o.variance[e] = var;
            o.pressure[e] = pressure;
        }
        // the frame's summary: candidates that are > 0.0 (never a NaN) as bit patterns
        const bool cd = valid && density >= dlim, cp = valid && pressure >= plim;
        const unsigned long long bd = density > 0.0 ? bits_of(density) : 0ull;
        const unsigned long long bp = pressure > 0.0 ? bits_of(pressure) : 0ull;
        const uint64_t md = __ballot(cd), mp = __ballot(cp);
        const unsigned long long wd = lidar::wave_max_u64(bd), wp = lidar::wave_max_u64(bp);
        const unsigned long long wsp = wave_min_u64(bits_of(spacing));  // >= +0.0 or +inf, never a NaN
        if (lane == 0) {
            if (md) atomicAdd(&cnt[0], __popcll(md));
            if (mp) atomicAdd(&cnt[1], __popcll(mp));
            if (wd) atomicMax(&pk[0], wd);
            if (wp) atomicMax(&pk[1], wp);
            if (wsp != kInfBits) atomicMin(&pk[2], wsp);
        }
        if (nx > 0 && valid) {
            const int64_t bx = arange_bin(x0, grid, nx, qx), by = arange_bin(y0, grid, ny, qy);
            if (bx >= 1 && bx <= nx && by >= 1 && by <= ny) {
                const int64_t c = (bx - 1) * ny + (by - 1);  // < nx * ny
                if (bd) atomicMax(&o.cell_peak[2 * c], bd);
                if (bp) atomicMax(&o.cell_peak[2 * c + 1], bp);
                if (cd) atomicAdd(&o.cell_crowded[c], 1);
            }
        }
    }
    __syncthreads();
    const bool only = gridDim.x == 1;
    if (tid < 2) {
        int32_t *dst = o.crowded + f * 2 + tid;
        if (only) *dst = cnt[tid];
        else if (cnt[tid]) atomicAdd(dst, cnt[tid]);
    }
    if (tid < 3) {
        unsigned long long *dst = o.peaks + f * 3 + tid;
        if (only) *dst = pk[tid];
        else if (tid < 2 && pk[tid]) atomicMax(dst, pk[tid]);
        else if (tid == 2 && pk[2] != kInfBits) atomicMin(dst, pk[2]);
    }
}

inline bool pos_finite(double v) { return v > 0.0 && v < INFINITY; }

}  // namespace

// ====================================================================== C-ABI
LIDAR_EXPORT int lidar_track_crowding_f64(lidar_handle *h, const double *people, const int64_t *k, const int32_t *prev,
                                          const double *velocity, int64_t frames, int64_t cap, int64_t first,
                                          double radius, double density_limit, double pressure_limit, double x0,
                                          double y0, double grid, int64_t nx, int64_t ny, int32_t accumulate,
                                          int32_t *neighbours, int32_t *nearest, double *spacing, double *density,
                                          int32_t *movers, double *variance, double *pressure, int32_t *crowded,
                                          double *peaks, double *cell_peak, int32_t *cell_crowded, void *stream)
{
    const std::string f("lidar_track_crowding_f64");
    if (int rc = check_frames(f, h && people && k && prev && velocity && neighbours && nearest && spacing && density &&
                                     movers && variance && pressure && crowded && peaks,
                              frames, cap))
        return rc;
    REQUIRE(first >= 0 && first <= frames, f + ": first must be in 0 .. frames");
    REQUIRE(pos_finite(radius), f + ": radius must be positive and finite");
    REQUIRE(density_limit >= 0.0 && pressure_limit >= 0.0, f + ": density_limit and pressure_limit must be >= 0");
    REQUIRE(accumulate == 0 || accumulate == 1, f + ": accumulate must be 0 or 1");
    REQUIRE(nx >= 0, f + ": nx must be >= 0 (0: no cells)");
    if (nx > 0) {
        REQUIRE(pos_finite(grid), f + ": grid must be positive and finite");
        REQUIRE(ny >= 1, f + ": nx and ny must be >= 1");
        REQUIRE(nx < 0x80000000ll && ny < 0x80000000ll && nx * ny < 0x80000000ll, f + ": nx * ny must be below 2^31");
        REQUIRE(std::isfinite(x0) && std::isfinite(y0), f + ": x0 and y0 must be finite");
        REQUIRE(cell_peak && cell_crowded, f + ": null cell output");
    }
    if (frames == first) return LIDAR_OK;  // no frame to evaluate (frames == 0 among them): nothing is written
    ON_DEVICE(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t nf = frames - first;
    const unsigned tiles = (unsigned)std::min<int64_t>((cap + kB - 1) / kB, 4096);
    const double r2 = radius * radius, area = (M_PI * radius) * radius;  // one rounding per product
    Out o{neighbours, nearest, movers, spacing, density, variance, pressure, crowded,
          reinterpret_cast<unsigned long long *>(peaks), reinterpret_cast<unsigned long long *>(cell_peak), cell_crowded};

    lidar::Span sp(h, "track_crowding", s);
    // a frame with one row tile stores its summary; the cells go on from what is stored with accumulate
    const int64_t nc = tiles > 1 ? nf * 2 : 0, np = tiles > 1 ? nf * 3 : 0;
    const int64_t ncell = nx > 0 && !accumulate ? nx * ny : 0;
    if (nc + ncell > 0) {
        const int64_t n = nc + np + 3 * ncell;
        const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + kB - 1) / kB, 4096));
        hipLaunchKernelGGL(init_kernel, dim3(blocks), dim3(kB), 0, s, crowded, nc, o.peaks, np, o.cell_peak, 2 * ncell,
                           cell_crowded, ncell);
    }
    hipLaunchKernelGGL(crowding_kernel, dim3(tiles, (unsigned)nf), dim3(kB), 0, s, people, k, prev, velocity, cap, first,
                       r2, area, density_limit, pressure_limit, x0, y0, grid, nx, ny, o);
    LAUNCH_CHECK();
    return LIDAR_OK;
}
