// track_events.hip — gate counts and zone occupancy from tracked people (DESIGN.md §3 "Gate and zone events",
// §4.12): what the links people_tracking leaves on the device (prev, gap) say about lines and areas of the venue.
//
// Contract (include/lidar_amd.h repeats it).  All arithmetic fp64, one rounding per operation.
//   people (T, cap, 2), k (T,), K_t = min(max(k[t], 0), cap) as in track.hip; prev (T, cap) int32; gap (T, cap)
//   int32 or null (null: every link spans one frame, the batch form); only the frames t >= first are evaluated.
//   Links: a row (t, j), j < K_t, is linked iff, with i = prev[t][j] and g = gap ? gap[t][j] : 1,
//   i >= 0 and 1 <= g <= 8 and g <= t and i < K_(t-g); then P = people[t-g][i], Q = people[t][j].  Every other
//   row is unlinked: no content of prev / gap makes the kernel read outside people.
//   Gates (G, 4) rows (ax, ay, bx, by).  side(a, b, p) = ((b.x - a.x) * (p.y - a.y)) - ((b.y - a.y) * (p.x - a.x));
//   sP = side(A, B, P), sQ = side(A, B, Q), sA = side(P, Q, A), sB = side(P, Q, B); the link crosses the gate iff
//   all four are finite and (sP >= 0) != (sQ >= 0) and (sA >= 0) != (sB >= 0); forward iff sQ >= 0 (from the right
//   of A -> B to its left or onto it), backward otherwise.  P == Q, A == B and a non-finite gate never cross.
//   Zones (Z, 4) rows (x0, x1, y0, y1).  inside(z, p) = x0 <= p.x < x1 and y0 <= p.y < y1 (a NaN: false).
//   gate_counts (T - first, G, 2) int32: the forward and backward crossings of the frame's linked rows (a crossing
//   belongs to the frame of Q).  zone_counts (T - first, Z, 3) int32: [0] the rows j < K_t with inside(Q), linked
//   or not; [1] the linked rows with inside(Q) and not inside(P); [2] the linked rows with inside(P) and not
//   inside(Q).  gate_fwd, gate_bwd, zone_in (T - first, cap) int64: bit g / z set for the gates the row crossed in
//   that direction / the zones that hold it; rows at or past K_t get 0.  Every element is written.
//   All results are integers: integer atomics leave them the same under every schedule.
//
// Kernels: events_kernel, one thread per row, the grid (row tile, frame) so that a workgroup belongs to one frame.
// The tables are staged once per workgroup in LDS (4 KiB at most) and read as broadcasts; a row's three masks live
// in registers and are stored once; per gate and zone a ballot and a popcount per wave go into the workgroup's LDS
// counters, and the workgroup adds its non-zero counters to the frame's.  A frame with one row tile (cap <= 256)
// stores its counters instead: no other workgroup adds to them, so that call needs no zero_counts_kernel before it.
#include <cmath>

#include "track_links.hpp"

namespace {

using namespace lidar::tier_r;
using namespace lidar::track;

constexpr int kB = 256;  // threads of events_kernel: one row each
static_assert(4 * kMaxTab <= kB && 3 * kMaxTab <= kB, "a table is staged, and the counters are flushed, in one round");

__device__ __forceinline__ double side(double ax, double ay, double bx, double by, double px, double py)
{
    return dsub(dmul(dsub(bx, ax), dsub(py, ay)), dmul(dsub(by, ay), dsub(px, ax)));
}

__device__ __forceinline__ bool finite4(double a, double b, double c, double d)
{
    // |v| < inf is false for an infinity and for a NaN
    return fabs(a) < INFINITY && fabs(b) < INFINITY && fabs(c) < INFINITY && fabs(d) < INFINITY;
}

__global__ __launch_bounds__(kB) void zero_counts_kernel(int32_t *__restrict__ a, int64_t na, int32_t *__restrict__ b,
                                                         int64_t nb)
{
    for (int64_t e = (int64_t)blockIdx.x * kB + threadIdx.x; e < na + nb; e += (int64_t)gridDim.x * kB) {
        if (e < na) a[e] = 0;
        else b[e - na] = 0;
    }
}

// blockIdx.y = t - first; blockIdx.x and gridDim.x stride over the frame's row tiles, every thread of a workgroup
// making the same number of rounds (the ballots and barriers are uniform).  gridDim.x == 1: the workgroup is the
// only one of its frame and stores its counters, zeros included; otherwise it adds the non-zero ones to counters
// zero_counts_kernel cleared.
__global__ __launch_bounds__(kB) void events_kernel(const double *__restrict__ people, const int64_t *__restrict__ k,
                                                    const int32_t *__restrict__ prev, const int32_t *__restrict__ gap,
                                                    int64_t cap, int64_t first, const double *__restrict__ gates, int G,
                                                    const double *__restrict__ zones, int Z,
                                                    int32_t *__restrict__ gate_counts, int32_t *__restrict__ zone_counts,
                                                    int64_t *__restrict__ gate_fwd, int64_t *__restrict__ gate_bwd,
                                                    int64_t *__restrict__ zone_in)
{
    __shared__ __attribute__((aligned(16))) double sg[4 * kMaxTab];
    __shared__ __attribute__((aligned(16))) double sz[4 * kMaxTab];
    __shared__ int32_t cg[2 * kMaxTab];
    __shared__ int32_t cz[3 * kMaxTab];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t f = blockIdx.y, t = first + f;
    if (tid < 4 * G) sg[tid] = gates[tid];
    if (tid < 4 * Z) sz[tid] = zones[tid];
    if (tid < 2 * G) cg[tid] = 0;
    if (tid < 3 * Z) cz[tid] = 0;
    __syncthreads();
    const int64_t K = clamp_k(k, t, cap);
    const double qnan = __builtin_nan("");
    for (int64_t j0 = (int64_t)blockIdx.x * kB; j0 < cap; j0 += (int64_t)gridDim.x * kB) {
        const int64_t j = j0 + tid, e = t * cap + j;
        const bool live = j < K;
        // a row at or past K_t keeps NaN for Q, an unlinked row NaN for P: neither is inside a zone, and a side
        // with a NaN in it is not finite
        double qx = qnan, qy = qnan, px = qnan, py = qnan;
        bool linked = false;
        if (live) {
            qx = people[2 * e];
            qy = people[2 * e + 1];
            int64_t g;
            const int64_t a = source_of(k, prev, gap, cap, t, e, g);  // inside people, or -1
            if (a >= 0) {
                linked = true;
                px = people[2 * a];
                py = people[2 * a + 1];
            }
        }
        uint64_t mf = 0, mb = 0, mz = 0;
        if (__ballot(linked)) {  // the wave has a link
            for (int g = 0; g < G; ++g) {
                const double ax = sg[4 * g], ay = sg[4 * g + 1], bx = sg[4 * g + 2], by = sg[4 * g + 3];
                const double sP = side(ax, ay, bx, by, px, py), sQ = side(ax, ay, bx, by, qx, qy);
                const double sA = side(px, py, qx, qy, ax, ay), sB = side(px, py, qx, qy, bx, by);
                const bool cross = finite4(sP, sQ, sA, sB) && (sP >= 0.0) != (sQ >= 0.0) && (sA >= 0.0) != (sB >= 0.0);
                const bool fw = cross && sQ >= 0.0, bw = cross && !(sQ >= 0.0);
                mf |= (uint64_t)fw << g;
                mb |= (uint64_t)bw << g;
                const uint64_t bf = __ballot(fw), bb = __ballot(bw);
                if (lane == 0) {
                    if (bf) atomicAdd(&cg[2 * g], __popcll(bf));
                    if (bb) atomicAdd(&cg[2 * g + 1], __popcll(bb));
                }
            }
        }
        if (__ballot(live)) {
            for (int z = 0; z < Z; ++z) {
                const double x0 = sz[4 * z], x1 = sz[4 * z + 1], y0 = sz[4 * z + 2], y1 = sz[4 * z + 3];
                const bool inq = inside(x0, x1, y0, y1, qx, qy), inp = inside(x0, x1, y0, y1, px, py);
                const bool in = linked && inq && !inp, out = linked && inp && !inq;
                mz |= (uint64_t)inq << z;
                const uint64_t bo = __ballot(inq), bi = __ballot(in), be = __ballot(out);
                if (lane == 0) {
                    if (bo) atomicAdd(&cz[3 * z], __popcll(bo));
                    if (bi) atomicAdd(&cz[3 * z + 1], __popcll(bi));
                    if (be) atomicAdd(&cz[3 * z + 2], __popcll(be));
                }
            }
        }
        if (j < cap) {
            const int64_t o = f * cap + j;
            if (G) {
                gate_fwd[o] = (int64_t)mf;
                gate_bwd[o] = (int64_t)mb;
            }
            if (Z) zone_in[o] = (int64_t)mz;
        }
    }
    __syncthreads();
    const bool only = gridDim.x == 1;
    if (tid < 2 * G) {
        int32_t *dst = gate_counts + f * 2 * G + tid;
        if (only) *dst = cg[tid];
        else if (cg[tid]) atomicAdd(dst, cg[tid]);
    }
    if (tid < 3 * Z) {
        int32_t *dst = zone_counts + f * 3 * Z + tid;
        if (only) *dst = cz[tid];
        else if (cz[tid]) atomicAdd(dst, cz[tid]);
    }
}

}  // namespace

// ====================================================================== C-ABI
LIDAR_EXPORT int lidar_track_events_f64(lidar_handle *h, const double *people, const int64_t *k, const int32_t *prev,
                                        const int32_t *gap, int64_t frames, int64_t cap, int64_t first,
                                        const double *gates, int32_t ngates, const double *zones, int32_t nzones,
                                        int32_t *gate_counts, int32_t *zone_counts, int64_t *gate_fwd, int64_t *gate_bwd,
                                        int64_t *zone_in, void *stream)
{
    const std::string f("lidar_track_events_f64");
    if (int rc = check_frames(f, h && people && k && prev, frames, cap)) return rc;
    REQUIRE(first >= 0 && first <= frames, f + ": first must be in 0 .. frames");
    REQUIRE(ngates >= 0 && ngates <= kMaxTab && nzones >= 0 && nzones <= kMaxTab,
            f + ": ngates and nzones must be in 0 .. 64");
    REQUIRE(ngates + nzones >= 1, f + ": no gate and no zone");
    REQUIRE(ngates == 0 || (gates && gate_counts && gate_fwd && gate_bwd), f + ": null gate table or gate output");
    REQUIRE(nzones == 0 || (zones && zone_counts && zone_in), f + ": null zone table or zone output");
    if (frames == first) return LIDAR_OK;  // no frame to evaluate (frames == 0 among them): nothing is written
    ON_DEVICE(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t nf = frames - first;
    const unsigned tiles = (unsigned)std::min<int64_t>((cap + kB - 1) / kB, 4096);

    lidar::Span sp(h, "track_events", s);
    if (tiles > 1) {
        const int64_t na = nf * 2 * ngates, nb = nf * 3 * nzones;
        const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>((na + nb + kB - 1) / kB, 4096));
        hipLaunchKernelGGL(zero_counts_kernel, dim3(blocks), dim3(kB), 0, s, gate_counts, na, zone_counts, nb);
    }
    hipLaunchKernelGGL(events_kernel, dim3(tiles, (unsigned)nf), dim3(kB), 0, s, people, k, prev, gap, cap, first, gates,
                       (int)ngates, zones, (int)nzones, gate_counts, zone_counts, gate_fwd, gate_bwd, zone_in);
    LAUNCH_CHECK();
    return LIDAR_OK;
}
