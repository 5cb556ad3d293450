// density_grid.hip — people, the density grid and the UI helpers of the reference density path
// (Tier R) on gfx950, bit-exact with the CPU path.
//
//   people_kernel      data_processing.py:251-280 per-cluster mean, sequential index-order sums
//   density_kernel     data_processing.py:282-328 + crowd_density_model.py:56-82: np.arange
//                      edges, histogram2d binning, /g^2, cell centres, max, numpy pairwise
//                      mean of the occupied cells, hotspot threshold, stable top-5.
//   histogram2d, cell radius density and venue counts: the reference's heatmaps and grids.
#include <cmath>

#include "tier_r.hpp"

namespace {

using namespace lidar::tier_r;

// ------------------------------------------------------------------ people
// One workgroup per cluster: waves 1..15 compact the cluster's members of a 960-point chunk
// (wave w owns points [64(w-1), 64w) of every chunk) into LDS contiguously in index order
// (double-buffered rows, triple-buffered per-wave counts), and lanes 0 / 1 of wave 0 run the
// x / y chains over the chunk's members in one run, as np.mean of the member rows does
// (sequential axis-0 sums starting from the identity +0.0).  Per chunk: the staging waves place
// chunk k+1 (its counts were published a phase earlier) and count chunk k+2 while wave 0 adds
// chunk k; one barrier per chunk.
__global__ __launch_bounds__(kT) void people_kernel(const double *xyz_in, const int64_t *labels_in, int64_t n_in,
                                                    const int64_t *kdev_in, double *out_in, const double *S_in,
                                                    FrameMap fm)
{
    // a batch frame's rows are its inliers: n = scalars[S_NIN] (0 for a failed frame)
    const int64_t n = S_in ? (fm.scal(S_in)[S_STATUS] == 0.0 ? (int64_t)fm.scal(S_in)[S_NIN] : 0) : n_in;
    const double *xyz = fm.rows(xyz_in, 3);
    const int64_t *labels = fm.rows(labels_in, 1);
    const int64_t *kdev = kdev_in + blockIdx.y;
    double *out = fm.rows(out_in, 2);
    constexpr int kChunk = kT - 64;
    __shared__ double mem[2][kChunk * 2];
    __shared__ int wcnt[3][kW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t K = *kdev;
    const int64_t nch = (n + kChunk - 1) / kChunk;
    for (int64_t c = blockIdx.x; c < K; c += gridDim.x) {
        // members of this wave's 64 points of chunk k (0 for wave 0 and past the end), published
        // as the wave's count of chunk k
        auto count = [&](int64_t k) -> uint64_t {
            if (wave == 0) return 0;
            const int64_t i = k * kChunk + (tid - 64);
            const uint64_t m = __ballot(k < nch && i < n && labels[i] == c);
            if (lane == 0) wcnt[k % 3][wave] = __popcll(m);
            return m;
        };
        auto place = [&](int64_t k, uint64_t m) {
            if (wave == 0 || k >= nch || !((m >> lane) & 1)) return;
            int base = 0;
            for (int w = 1; w < wave; ++w) base += wcnt[k % 3][w];
            const int64_t i = k * kChunk + (tid - 64);
            const int r = base + __popcll(m & ((1ull << lane) - 1));
            mem[k & 1][2 * r] = xyz[3 * i];
            mem[k & 1][2 * r + 1] = xyz[3 * i + 1];
        };
        double acc = 0.0;
        int64_t cnt = 0;
        uint64_t m_next = count(0);
        __syncthreads();
        place(0, m_next);
        m_next = count(1);
        __syncthreads();
        for (int64_t k = 0; k < nch; ++k) {
            if (wave != 0) {
                place(k + 1, m_next);
                m_next = count(k + 2);
            } else if (tid < 2) {
                int tot = 0;
                for (int w = 1; w < kW; ++w) tot += wcnt[k % 3][w];
                const double *b = mem[k & 1] + tid;
                int j = 0;  // acc starts at +0.0, np.add.reduce's identity: members that are all -0.0 sum to +0.0
                for (; j + 16 <= tot; j += 16) {  // reads first, then the dependent adds
                    double v[16];
#pragma unroll
                    for (int u = 0; u < 16; ++u) v[u] = b[2 * (j + u)];
#pragma unroll
                    for (int u = 0; u < 16; ++u) acc = dadd(acc, v[u]);
                }
                for (; j < tot; ++j) acc = dadd(acc, b[2 * j]);
                cnt += tot;
            }
            __syncthreads();
        }
        if (tid < 2) out[2 * c + tid] = ddiv(acc, (double)cnt);
        __syncthreads();  // the next cluster's first counts reuse wcnt[0..1]
    }
}

__global__ void max_label_kernel(const int64_t *labels_in, int64_t n_in, int64_t *kout_in, const double *S_in,
                                 FrameMap fm)
{
    const int64_t n = S_in ? (fm.scal(S_in)[S_STATUS] == 0.0 ? (int64_t)fm.scal(S_in)[S_NIN] : 0) : n_in;
    const int64_t *labels = fm.rows(labels_in, 1);
    int64_t *kout = kout_in + blockIdx.y;
    // K = number of distinct labels >= 0 = max + 1 (labels are dense ranks)
    int64_t m = -1;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        m = labels[i] > m ? labels[i] : m;
    for (int o = 32; o >= 1; o >>= 1) {
        const int64_t t = __shfl_xor(m, o, 64);
        m = t > m ? t : m;
    }
    if ((threadIdx.x & 63) == 0) atomicMax((unsigned long long *)kout, (unsigned long long)(m + 1));
}

// ------------------------------------------------------------------ density grid
// numpy float64 add.reduce of a contiguous 1-D array: 8192-element buffer chunks,
// each summed by pairwise_sum (8-way unrolled leaves of <= 128), chunks added in order
__device__ double np_pairwise(const double *a, int64_t n)
{
    if (n < 8) {
        double r = 0.0;
        for (int64_t i = 0; i < n; ++i) r = dadd(r, a[i]);
        return r;
    }
    if (n <= 128) {
        double r[8];
        for (int j = 0; j < 8; ++j) r[j] = a[j];
        int64_t i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; ++j) r[j] = dadd(r[j], a[i + j]);
        double res = dadd(dadd(dadd(r[0], r[1]), dadd(r[2], r[3])), dadd(dadd(r[4], r[5]), dadd(r[6], r[7])));
        for (; i < n; ++i) res = dadd(res, a[i]);
        return res;
    }
    int64_t n2 = n / 2;
    n2 -= n2 % 8;
    return dadd(np_pairwise(a, n2), np_pairwise(a + n2, n - n2));
}
__device__ double np_sum(const double *a, int64_t n)
{
    double out = 0.0;
    for (int64_t i = 0; i < n; i += 8192) out = dadd(out, np_pairwise(a + i, n - i < 8192 ? n - i : 8192));
    return out;
}

__device__ int64_t searchsorted_right(const double *e, int64_t len, double v)
{
    int64_t lo = 0, hi = len;  // first index with e[idx] > v
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (e[mid] <= v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ void density_body(const double *people, const int64_t *kdev,
                             double xa, double ya, double g, int64_t nx, int64_t ny,
                             double *xe, double *ye, uint32_t *count,
                             double *grid_x, double *grid_y, double *density,
                             double *flat_x, double *flat_y, double *pos_scratch,
                             double *stats, int64_t *hot)
{
    const int64_t K = *kdev;
    const int tid = threadIdx.x;
    // np.arange: e[0] = a, e[1] = a + g, e[i] = a + i * (e[1] - e[0])
    const double dx = dsub(dadd(xa, g), xa), dy = dsub(dadd(ya, g), ya);
    for (int64_t i = tid; i <= nx; i += kT) xe[i] = i == 0 ? xa : (i == 1 ? dadd(xa, g) : dadd(xa, dmul((double)i, dx)));
    for (int64_t i = tid; i <= ny; i += kT) ye[i] = i == 0 ? ya : (i == 1 ? dadd(ya, g) : dadd(ya, dmul((double)i, dy)));
    for (int64_t i = tid; i < nx * ny; i += kT) count[i] = 0;
    __threadfence_block();
    __syncthreads();
    for (int64_t k = tid; k < K; k += kT) {
        const double px = people[2 * k], py = people[2 * k + 1];
        int64_t bx = searchsorted_right(xe, nx + 1, px), by = searchsorted_right(ye, ny + 1, py);
        if (px == xe[nx]) --bx;
        if (py == ye[ny]) --by;
        if (bx >= 1 && bx <= nx && by >= 1 && by <= ny) atomicAdd(&count[(bx - 1) * ny + (by - 1)], 1u);
    }
    __threadfence_block();
    __syncthreads();
    const double g2 = dmul(g, g);
    for (int64_t i = tid; i < nx; i += kT) grid_x[i] = ddiv(dadd(xe[i], xe[i + 1]), 2.0);
    for (int64_t i = tid; i < ny; i += kT) grid_y[i] = ddiv(dadd(ye[i], ye[i + 1]), 2.0);
    for (int64_t i = tid; i < nx * ny; i += kT) {
        density[i] = ddiv((double)count[i], g2);
        flat_x[i] = ddiv(dadd(xe[i / ny], xe[i / ny + 1]), 2.0);
        flat_y[i] = ddiv(dadd(ye[i % ny], ye[i % ny + 1]), 2.0);
    }
    __threadfence_block();
    __syncthreads();
    if (tid == 0) {
        // max, occupied cells in flat order, numpy mean, threshold, stable top-5
        double mx = -INFINITY;
        int64_t np_ = 0;
        for (int64_t i = 0; i < nx * ny; ++i) {
            const double d = density[i];
            mx = d > mx ? d : mx;
            if (d > 0.0) pos_scratch[np_++] = d;
        }
        const double avg = np_ > 0 ? ddiv(np_sum(pos_scratch, np_), (double)np_) : 0.0;
        const double a15 = dmul(avg, 1.5);
        const double thr = 0.5 >= a15 ? 0.5 : a15;
        int64_t nh = 0;
        double last = INFINITY;
        int64_t last_i = -1;
        for (; nh < 5; ++nh) {
            // next hotspot: highest density below (last, last_i) in (desc density, asc index) order
            int64_t best = -1;
            double bd = -INFINITY;
            for (int64_t i = 0; i < nx * ny; ++i) {
                const double d = density[i];
                if (!(d >= thr)) continue;
                const bool after = d < last || (d == last && i > last_i);
                if (!after) continue;
                if (best < 0 || d > bd) {
                    best = i;
                    bd = d;
                }
            }
            if (best < 0) break;
            hot[nh] = best;
            last = bd;
            last_i = best;
        }
        stats[0] = mx;
        stats[1] = avg;
        stats[2] = thr;
        stats[3] = (double)nh;
        stats[4] = (double)np_;
        stats[5] = (double)K;
    }
}

__global__ __launch_bounds__(kT) void density_kernel(const double *people, const int64_t *kdev,
                                                     double xa, double ya, double g, int64_t nx, int64_t ny,
                                                     double *xe, double *ye, uint32_t *count,
                                                     double *grid_x, double *grid_y, double *density,
                                                     double *flat_x, double *flat_y, double *pos_scratch,
                                                     double *stats, int64_t *hot)
{
    density_body(people, kdev, xa, ya, g, nx, ny, xe, ye, count, grid_x, grid_y, density, flat_x, flat_y,
                 pos_scratch, stats, hot);
}

// one workgroup per frame; job row f (8 doubles): xa, ya, g, nx, ny, out offset, scratch
// offset (doubles), unused.  out at its offset: grid_x | grid_y | density | flat_x | flat_y |
// stats(8) | hot(5 int64); scratch: xe (nx+1) | ye (ny+1) | pos (nx*ny) | count (nx*ny u32).
// Frames with no people (k == 0) are skipped (the caller returns the reference's empty dict).
__global__ __launch_bounds__(kT) void density_batch_kernel(const double *people_in, const int64_t *offs,
                                                           const int64_t *kdev, const double *jobs, double *out,
                                                           double *scratch)
{
    const int f = blockIdx.y;
    const double *J = jobs + 8 * (int64_t)f;
    if (kdev[f] <= 0) return;
    const int64_t nx = (int64_t)J[3], ny = (int64_t)J[4], m = nx * ny;
    double *o = out + (int64_t)J[5];
    double *sc = scratch + (int64_t)J[6];
    double *xe = sc, *ye = xe + nx + 1, *pos = ye + ny + 1;
    uint32_t *count = reinterpret_cast<uint32_t *>(pos + m);
    double *gx = o, *gy = gx + nx, *dens = gy + ny, *fx = dens + m, *fy = fx + m, *st = fy + m;
    density_body(people_in + 2 * offs[f], kdev + f, J[0], J[1], J[2], nx, ny, xe, ye, count, gx, gy, dens, fx, fy,
                 pos, st, reinterpret_cast<int64_t *>(st + 8));
}

}  // namespace

namespace lidar {
namespace tier_r {

int people_of_frames(lidar_handle *h, const double *xyz, const int64_t *labels, int64_t max_n, const int64_t *kdev,
                     double *people, const double *scalars, hipStream_t s, FrameMap fm, int frames)
{
    lidar::Span sp(h, "people", s);
    const unsigned pb = (unsigned)std::max(1, std::min(256, 2048 / std::max(1, frames)));
    hipLaunchKernelGGL(people_kernel, dim3(pb, frames), dim3(kT), 0, s, xyz, labels, max_n, kdev, people, scalars, fm);
    LAUNCH_CHECK();
    return LIDAR_OK;
}

}  // namespace tier_r
}  // namespace lidar

// ====================================================================== C-ABI
LIDAR_EXPORT int lidar_people_f64(lidar_handle *h, const double *xyz, const int64_t *labels, int64_t n,
                                  double *people, int64_t *k_host, void *stream)
{
    REQUIRE(h && xyz && labels && people && k_host, "lidar_people_f64: null pointer");
    REQUIRE(n >= 0, "lidar_people_f64: n < 0");
    *k_host = 0;
    if (n == 0) return LIDAR_OK;
    ON_DEVICE(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    int64_t *kd = static_cast<int64_t *>(lidar::workspace(h, 256));
    if (!kd) return LIDAR_ENOMEM;
    HIP_TRY(hipMemsetAsync(kd, 0, sizeof(int64_t), s));
    const unsigned gp = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 1024));
    hipLaunchKernelGGL(max_label_kernel, dim3(gp), dim3(256), 0, s, labels, n, kd, nullptr, FrameMap{});
    hipLaunchKernelGGL(people_kernel, dim3(256), dim3(kT), 0, s, xyz, labels, n, kd, people, nullptr, FrameMap{});
    LAUNCH_CHECK();
    int64_t *hk = static_cast<int64_t *>(h->host_pinned);
    HIP_TRY(hipMemcpyAsync(hk, kd, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *k_host = *hk;
    return LIDAR_OK;
}

LIDAR_EXPORT int lidar_grid_dims(double xmin, double xmax, double ymin, double ymax, double grid,
                                 int64_t *nx, int64_t *ny)
{
    REQUIRE(nx && ny && grid > 0.0, "lidar_grid_dims: bad arguments");
    // data_processing.py:305-313: margin 2g, np.arange(min - 2g, max + 2g + g, g)
    const double m = grid * 2.0;
    const double x0 = xmin - m, x1 = (xmax + m) + grid;
    const double y0 = ymin - m, y1 = (ymax + m) + grid;
    const double lx = std::ceil((x1 - x0) / grid), ly = std::ceil((y1 - y0) / grid);
    // numpy's errors (np.arange, then histogram2d's (nx, ny) float64 array): a length it cannot
    // compute or hold (not finite, >= 2^63 elements, or >= 2^63 bytes) is a ValueError ("Maximum
    // allowed size exceeded" / "array is too big") -> LIDAR_EINVAL; a representable grid of more
    // than 2^40 cells (8 TiB of float64) a MemoryError -> LIDAR_ENOMEM
    const double kBig = 1152921504606846976.0;  // 2^60 float64 elements = 2^63 bytes
    if (!(std::isfinite(lx) && std::isfinite(ly) && lx < kBig && ly < kBig && (lx - 1) * (ly - 1) < kBig)) {
        lidar::set_error("lidar_grid_dims: Maximum allowed size exceeded");
        return LIDAR_EINVAL;
    }
    REQUIRE(lx >= 2 && ly >= 2, "lidar_grid_dims: degenerate grid");
    if ((lx - 1) * (ly - 1) > 1099511627776.0) {
        lidar::set_error("lidar_grid_dims: the grid has more than 2^40 cells");
        return LIDAR_ENOMEM;
    }
    *nx = (int64_t)lx - 1;
    *ny = (int64_t)ly - 1;
    return LIDAR_OK;
}

// people (k, 2) -> grid_x (nx), grid_y (ny), density (nx*ny), flat_x, flat_y (nx*ny),
// stats [max, avg, thr, n_hot, n_occupied, k], hot (5) int64.  `out` layout (doubles):
// grid_x | grid_y | density | flat_x | flat_y | stats(8) | hot(5, int64)
LIDAR_EXPORT int lidar_density_grid_f64(lidar_handle *h, const double *people, int64_t k, double xmin,
                                        double xmax, double ymin, double ymax, double grid, int64_t nx,
                                        int64_t ny, double *grid_x, double *grid_y, double *density,
                                        void *stream)
{
    REQUIRE(h && people && grid_x && grid_y && density, "lidar_density_grid_f64: null pointer");
    REQUIRE(nx >= 1 && ny >= 1 && k >= 0, "lidar_density_grid_f64: bad sizes");
    ON_DEVICE(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    lidar::Carver cv;
    const uint64_t o_xe = cv.take<double>(nx + 1), o_ye = cv.take<double>(ny + 1);
    const uint64_t o_cnt = cv.take<uint32_t>(nx * ny), o_pos = cv.take<double>(nx * ny);
    const uint64_t o_k = cv.take<int64_t>(1);
    char *base = static_cast<char *>(lidar::workspace(h, cv.off));
    if (!base) return LIDAR_ENOMEM;
    int64_t *kd = reinterpret_cast<int64_t *>(base + o_k);
    int64_t *hk = static_cast<int64_t *>(h->host_pinned);
    *hk = k;
    HIP_TRY(hipMemcpyAsync(kd, hk, sizeof(int64_t), hipMemcpyHostToDevice, s));
    const double m = grid * 2.0;
    // density points at: density (nx*ny) | flat_x | flat_y | stats (8) | hot (5)
    double *flat_x = density + nx * ny, *flat_y = flat_x + nx * ny, *stats = flat_y + nx * ny;
    int64_t *hot = reinterpret_cast<int64_t *>(stats + 8);
    hipLaunchKernelGGL(density_kernel, dim3(1), dim3(kT), 0, s, people, kd, xmin - m, ymin - m, grid, nx, ny,
                       reinterpret_cast<double *>(base + o_xe), reinterpret_cast<double *>(base + o_ye),
                       reinterpret_cast<uint32_t *>(base + o_cnt), grid_x, grid_y, density, flat_x, flat_y,
                       reinterpret_cast<double *>(base + o_pos), stats, hot);
    LAUNCH_CHECK();
    HIP_TRY(hipStreamSynchronize(s));  // hk is reused by the next call
    return LIDAR_OK;
}

// people of every frame of a preprocess batch (CSR rows, device offsets, scalars of the
// batch): people rows of frame f start at row offsets[f]; kdev (device int64[frames])
// receives K per frame.  Asynchronous.
LIDAR_EXPORT int lidar_people_batch_f64(lidar_handle *h, const double *compact_xyz, const int64_t *labels,
                                        const int64_t *offsets, int32_t frames, int64_t max_n,
                                        const double *scalars, double *people, int64_t *kdev, void *stream)
{
    REQUIRE(h && compact_xyz && labels && offsets && scalars && people && kdev, "lidar_people_batch_f64: null pointer");
    REQUIRE(frames >= 1 && frames <= 65535 && max_n >= 1, "lidar_people_batch_f64: bad sizes");
    ON_DEVICE(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    FrameMap fm;
    fm.offs = offsets;
    HIP_TRY(hipMemsetAsync(kdev, 0, sizeof(int64_t) * frames, s));
    lidar::Span sp(h, "people", s);
    hipLaunchKernelGGL(max_label_kernel, dim3(point_blocks(max_n, frames), frames), dim3(256), 0, s, labels, max_n,
                       kdev, scalars, fm);
    const unsigned pb = (unsigned)std::max(1, std::min(256, 2048 / std::max(1, (int)frames)));
    hipLaunchKernelGGL(people_kernel, dim3(pb, frames), dim3(kT), 0, s, compact_xyz, labels, max_n, kdev, people,
                       scalars, fm);
    LAUNCH_CHECK();
    return LIDAR_OK;
}

// density grids of every frame (see density_batch_kernel for the job / output layout);
// scratch_doubles = the sum over frames of nx*ny + ceil(nx*ny/2) + nx + ny + 2.  Asynchronous.
LIDAR_EXPORT int lidar_density_batch_f64(lidar_handle *h, const double *people, const int64_t *offsets,
                                         const int64_t *kdev, int32_t frames, const double *jobs, double *out,
                                         int64_t scratch_doubles, void *stream)
{
    REQUIRE(h && people && offsets && kdev && jobs && out, "lidar_density_batch_f64: null pointer");
    REQUIRE(frames >= 1 && frames <= 65535 && scratch_doubles >= 0, "lidar_density_batch_f64: bad sizes");
    ON_DEVICE(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    double *scratch = static_cast<double *>(lidar::workspace(h, (uint64_t)std::max<int64_t>(1, scratch_doubles) * 8));
    if (!scratch) return LIDAR_ENOMEM;
    lidar::Span sp(h, "density_grid", s);
    hipLaunchKernelGGL(density_batch_kernel, dim3(1, frames), dim3(kT), 0, s, people, offsets, kdev, jobs, out,
                       scratch);
    LAUNCH_CHECK();
    return LIDAR_OK;
}

// np.histogram2d(a, b, bins=(bx, by), range=...) binning (the reference's heatmaps,
// utils/visualization.py:125-137, app_simplified.py:205-209): the edges are numpy's own
// (np.linspace, passed in); a value lands in bin searchsorted(edges, v, 'right') - 1, a value
// equal to the last edge in the last bin, anything outside (or NaN) nowhere.  counts is
// bx * by float64 (row-major, a-bins x b-bins), zeroed here.
__global__ void hist2d_kernel(const double *a, const double *b, int64_t n, const double *xe, int64_t bx,
                              const double *ye, int64_t by, unsigned long long *cnt)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double va = a[i], vb = b[i];
        int64_t ia = searchsorted_right(xe, bx + 1, va), ib = searchsorted_right(ye, by + 1, vb);
        if (va == xe[bx]) --ia;
        if (vb == ye[by]) --ib;
        if (ia >= 1 && ia <= bx && ib >= 1 && ib <= by) atomicAdd(&cnt[(ia - 1) * by + (ib - 1)], 1ull);
    }
}
__global__ void hist2d_finish_kernel(const unsigned long long *cnt, int64_t m, double *out)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = (double)cnt[i];
}

LIDAR_EXPORT int lidar_histogram2d_f64(lidar_handle *h, const double *a, const double *b, int64_t n,
                                       const double *xedges, int64_t bx, const double *yedges, int64_t by,
                                       double *counts, void *stream)
{
    REQUIRE(h && xedges && yedges && counts && (n == 0 || (a && b)), "lidar_histogram2d_f64: null pointer");
    REQUIRE(n >= 0 && bx >= 1 && by >= 1, "lidar_histogram2d_f64: bad sizes");
    ON_DEVICE(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t m = bx * by;
    auto *cnt = static_cast<unsigned long long *>(lidar::workspace(h, (uint64_t)m * 8));
    if (!cnt) return LIDAR_ENOMEM;
    HIP_TRY(hipMemsetAsync(cnt, 0, (size_t)m * 8, s));
    if (n > 0)
        hipLaunchKernelGGL(hist2d_kernel, dim3(point_blocks(n, 1)), dim3(256), 0, s, a, b, n, xedges, bx, yedges, by,
                           cnt);
    hipLaunchKernelGGL(hist2d_finish_kernel, dim3(point_blocks(m, 1)), dim3(256), 0, s, cnt, m, counts);
    LAUNCH_CHECK();
    return LIDAR_OK;
}

// the variant's grid density (app_simplified.py:262-282, app_with_db.py:266-286): cell (i, j)
// of the edges xg (nxg), yg (nyg) has centre ((xg[i] + xg[i+1]) / 2, (yg[j] + yg[j+1]) / 2);
// out[j * (nxg - 1) + i] = #{people p : (cx - px)^2 + (cy - py)^2 <= r*r} / divisor — the
// count of KDTree(people).query_radius([centre], r) (sklearn's rdist test, no FMA).
__global__ void cell_radius_density_kernel(const double *__restrict__ people, int64_t k,
                                           const double *__restrict__ xg, int64_t nx,
                                           const double *__restrict__ yg, int64_t ny, double r2, double divisor,
                                           double *__restrict__ out)
{
    extern __shared__ double pp[];  // people tile (x, y)
    const int64_t m = nx * ny;
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < m; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = base + threadIdx.x;
        double cx = 0.0, cy = 0.0;
        if (c < m) {
            const int64_t i = c % nx, j = c / nx;
            cx = ddiv(dadd(xg[i], xg[i + 1]), 2.0);
            cy = ddiv(dadd(yg[j], yg[j + 1]), 2.0);
        }
        int64_t cnt = 0;
        for (int64_t t0 = 0; t0 < k; t0 += blockDim.x) {
            const int64_t tn = k - t0 < (int64_t)blockDim.x ? k - t0 : (int64_t)blockDim.x;
            __syncthreads();
            if (threadIdx.x < tn) {
                pp[2 * threadIdx.x] = people[2 * (t0 + threadIdx.x)];
                pp[2 * threadIdx.x + 1] = people[2 * (t0 + threadIdx.x) + 1];
            }
            __syncthreads();
            for (int64_t u = 0; u < tn; ++u) {
                const double dx = dsub(cx, pp[2 * u]), dy = dsub(cy, pp[2 * u + 1]);
                cnt += dadd(dmul(dx, dx), dmul(dy, dy)) <= r2;
            }
        }
        if (c < m) out[c] = ddiv((double)cnt, divisor);  // row j = c / nx, column i = c % nx
    }
}

LIDAR_EXPORT int lidar_cell_radius_density_f64(lidar_handle *h, const double *people, int64_t k, const double *xg,
                                               int64_t nxg, const double *yg, int64_t nyg, double r, double divisor,
                                               double *out, void *stream)
{
    REQUIRE(h && xg && yg && out && (k == 0 || people), "lidar_cell_radius_density_f64: null pointer");
    REQUIRE(k >= 0 && nxg >= 2 && nyg >= 2, "lidar_cell_radius_density_f64: bad sizes");
    REQUIRE(r >= 0.0 && divisor != 0.0, "lidar_cell_radius_density_f64: bad r / divisor");
    ON_DEVICE(h->device);
    const int64_t nx = nxg - 1, ny = nyg - 1, m = nx * ny;
    const int64_t blocks = std::min<int64_t>((m + 255) / 256, 65535);
    hipLaunchKernelGGL(cell_radius_density_kernel, dim3((unsigned)blocks), dim3(256), 2 * 256 * sizeof(double),
                       static_cast<hipStream_t>(stream), people, k, xg, nx, yg, ny, r * r, divisor, out);
    LAUNCH_CHECK();
    return LIDAR_OK;
}

// ------------------------------------------------------------------ venue grid
// calculate_grid_density's binning (utils/data_processing.py:312-319) over a FIXED venue grid:
// edges np.arange(x0, ..., g) (e[0] = a, e[1] = a + g, e[i] = a + i * ((a + g) - a), numpy's
// DOUBLE_fill), searchsorted right with the last edge closed, points outside dropped.  Counts
// add into int32 cells, so the frames of a rank and then the ranks (one RCCL all-reduce) sum.
// arange_edge / arange_bin: tier_r.hpp (shared with track.hip's flow cells)
using lidar::tier_r::arange_bin;
__global__ void venue_counts_kernel(const double *__restrict__ people, int64_t k, double x0, double y0, double g,
                                    int64_t nx, int64_t ny, int32_t *__restrict__ counts)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < k; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t bx = arange_bin(x0, g, nx, people[2 * i]), by = arange_bin(y0, g, ny, people[2 * i + 1]);
        if (bx >= 1 && bx <= nx && by >= 1 && by <= ny) atomicAdd(&counts[(bx - 1) * ny + (by - 1)], 1);
    }
}

LIDAR_EXPORT int lidar_venue_counts_f64(lidar_handle *h, const double *people, int64_t k, double x0, double y0,
                                        double grid, int64_t nx, int64_t ny, int32_t *counts, void *stream)
{
    REQUIRE(h && counts && (k == 0 || people), "lidar_venue_counts_f64: null pointer");
    REQUIRE(k >= 0 && nx >= 1 && ny >= 1 && grid > 0.0, "lidar_venue_counts_f64: bad sizes");
    if (k == 0) return LIDAR_OK;
    ON_DEVICE(h->device);
    const unsigned blocks = (unsigned)std::min<int64_t>((k + 255) / 256, 4096);
    hipLaunchKernelGGL(venue_counts_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), people, k,
                       x0, y0, grid, nx, ny, counts);
    LAUNCH_CHECK();
    return LIDAR_OK;
}
