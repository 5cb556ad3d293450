// track_history.hip — per-track history from the links of tracked people (DESIGN.md §3 "Track history", §4.13):
// how long a track has lived, how often it was seen, how far it walked, where it came from, and how long it has
// been in each zone, for every detection, with the completed stays per frame and zone.
//
// Contract (include/lidar_amd.h repeats it).  All arithmetic fp64, one rounding per operation.
//   people (T, cap, 2), k (T,), K_t, prev (T, cap) int32, gap (T, cap) int32 or null (every link spans one frame)
//   and the link guard are lidar_track_events_f64's: a row (t, j), j < K_t, is linked iff, with i = prev[t][j] and
//   g = gap ? gap[t][j] : 1, i >= 0 and 1 <= g <= 8 and g <= t and i < K_(t-g); its source is the row (s, i),
//   s = t - g, P = people[s][i], Q = people[t][j].  No content of prev / gap makes a kernel read or write outside
//   the arrays.  zones (Z, 4) rows (x0, x1, y0, y1), 0 <= Z <= 64; inside(z, p) = x0 <= p.x < x1 and
//   y0 <= p.y < y1.  carry = C: the leading frames whose history state is given, never written.
//   Heirs: among the rows of frames >= C linked to the same source, the lowest in (t, j) order continues the
//   source's history; every other row of a frame >= C (unlinked, or linked and not the heir) starts one.
//   Per row of a frame >= C (every element written):     starts            continues (s, i) over g      j >= K_t
//     age (T, cap) int32                                 0                 age[s][i] + g                -1
//     hits (T, cap) int32                                1                 hits[s][i] + 1               0
//     path (T, cap) fp64                                 0.0               path[s][i] + sqrt((dx*dx) + (dy*dy))  0.0
//     origin (T, cap, 2) fp64                            Q                 origin[s][i]                 (0, 0)
//     stay (T, cap, Z) int32 (Z > 0)                     in(z, Q) ? 0 : -1 in(z, Q) ? (stay[s][i][z] >= 0 ?
//                                                                          stay[s][i][z] + g : 0) : -1  -1
//   dx = Q.x - P.x, dy = Q.y - P.y, the square root correctly rounded.
//   dwell (T - C, Z, 3) int64 (Z > 0), every element written: a continuing row of frame t with stay[s][i][z] >= 0
//   and not inside(z, Q) adds 1 to dwell[t - C][z][0], stay[s][i][z] to [1], and raises [2] to it.  Integers:
//   integer atomics leave them the same under every schedule.
//
// Kernels, three launches, no workgroup waiting for another:
//   init_kernel    (track_chain.hpp, shared with track_routes.hip) next[row] = kNone over the rows a claim can name,
//                  dwell = 0.
//   claim_kernel   (track_chain.hpp) a thread per row of the frames >= C; a linked row takes atomicMin(next[source],
//                  its own index): the minimum is the heir rule.
//   walk_kernel (Z = 0), walk_zones_kernel (Z > 0): a walker per row of the frames >= C.  A row at or past K_t gets
//                  the defaults.  A live row that is the heir of a row of a frame >= C leaves: the walker that comes
//                  through its source writes it.  Every other live row is a walk start (the start of a history, or
//                  the heir of a carried row, whose state is the anchor): the walker writes it and follows next[]
//                  until kNone.  Every live row is a walk start or the next[] of exactly one row, so it is written
//                  once, by one walker.  The state a step continues from (P, age, hits, path, origin) stays in
//                  registers; a step's dependent loads are next[cur], then Q and gap of that row side by side (the
//                  frame moves by gap: no division by cap).  Without zones the walker is a thread.  With zones it is
//                  a wave, lane z owning zone z: the zone's box and its stay counter are the lane's registers, a
//                  step stores the row's Z counters in one coalesced instruction and nothing is read back; a wave
//                  whose row is no walk start leaves after three loads.  (A thread per chain that loops over the
//                  zones and reads the counters back from the row it wrote the step before pays a memory round trip
//                  per zone and step: 3 times slower at 8 zones, 10 to 20 times at 64)
#include <cmath>

#include "track_chain.hpp"

namespace {

using namespace lidar::tier_r;
using namespace lidar::track;

constexpr int kWaves = kB / 64;
static_assert(kMaxTab <= 64, "a zone per lane");

// The history state a walker carries from one row to the next.
struct Hist {
    double px, py;  // the row's position: P of the next step
    double path, ox, oy;
    int32_t age, hits;
};

// The state of the carried row a: the anchor of its heir's walk.
__device__ __forceinline__ Hist anchor(const double *__restrict__ people, const int32_t *age, const int32_t *hits,
                                       const double *path, const double *origin, int64_t a)
{
    Hist h;
    h.px = people[2 * a];
    h.py = people[2 * a + 1];
    h.path = path[a];
    h.ox = origin[2 * a];
    h.oy = origin[2 * a + 1];
    h.age = age[a];
    h.hits = hits[a];
    return h;
}

// h, the state of the row Q continues over g frames (cont) or nothing it depends on (a start), becomes Q's own.
__device__ __forceinline__ void advance(Hist &h, bool cont, int64_t g, double qx, double qy)
{
    if (cont) {
        const double dx = dsub(qx, h.px), dy = dsub(qy, h.py);
        h.age += (int32_t)g;
        h.hits += 1;
        h.path = dadd(h.path, __dsqrt_rn(dadd(dmul(dx, dx), dmul(dy, dy))));
    } else {
        h.age = 0;
        h.hits = 1;
        h.path = 0.0;
        h.ox = qx;
        h.oy = qy;
    }
    h.px = qx;
    h.py = qy;
}

__device__ __forceinline__ void store_row(const Hist &h, int64_t e, int32_t *age, int32_t *hits, double *path,
                                          double *origin)
{
    age[e] = h.age;
    hits[e] = h.hits;
    path[e] = h.path;
    origin[2 * e] = h.ox;
    origin[2 * e + 1] = h.oy;
}

__device__ __forceinline__ void store_dead(int64_t e, int32_t *age, int32_t *hits, double *path, double *origin)
{
    age[e] = -1;
    hits[e] = 0;
    path[e] = 0.0;
    origin[2 * e] = 0.0;
    origin[2 * e + 1] = 0.0;
}

// Without zones: a thread per row.  blockIdx.y = t - carry; blockIdx.x and gridDim.x stride over the frame's row
// tiles.  age, hits, path and origin are read in the carry frames and written in the frames >= carry: no
// __restrict__.
__global__ __launch_bounds__(kB) void walk_kernel(const double *__restrict__ people, const int64_t *__restrict__ k,
                                                  const int32_t *__restrict__ prev, const int32_t *__restrict__ gap,
                                                  int64_t cap, int64_t carry, const int32_t *__restrict__ next,
                                                  int32_t *age, int32_t *hits, double *path, double *origin)
{
    const int64_t t0 = carry + blockIdx.y, first = carry * cap, K = clamp_k(k, t0, cap);
    for (int64_t j = (int64_t)blockIdx.x * kB + threadIdx.x; j < cap; j += (int64_t)gridDim.x * kB) {
        int64_t e = t0 * cap + j;
        if (j >= K) {
            store_dead(e, age, hits, path, origin);
            continue;
        }
        int64_t g;
        const int64_t a = source_of(k, prev, gap, cap, t0, e, g);
        bool cont = a >= 0 && next[a] == (int32_t)e;  // the heir of its source
        if (cont && a >= first) continue;             // the walker that comes through a writes this row
        Hist h;
        if (cont) h = anchor(people, age, hits, path, origin, a);  // the heir of a carried row
        double qx = people[2 * e], qy = people[2 * e + 1];
        for (;;) {
            advance(h, cont, g, qx, qy);
            store_row(h, e, age, hits, path, origin);
            const int32_t nx = next[e];
            if (nx == kNone) break;
            // nx passed claim_kernel's guard with e as its source: a live row of a later frame, inside the arrays
            e = nx;
            g = gap ? gap[e] : 1;
            qx = people[2 * e];
            qy = people[2 * e + 1];
            cont = true;
        }
    }
}

// With zones: a wave per row, lane z owning zone z: its box and its stay counter are the lane's registers, a step
// stores the row's Z counters in one coalesced instruction, and lane 0 stores age, hits, path and origin, which every
// lane computes from the same (broadcast) loads.  blockIdx.y = t - carry; the workgroup's waves stride over the
// frame's rows.  Everything but `in`, the stay counter and the dwell atomics is uniform across the wave.
__global__ __launch_bounds__(kB) void walk_zones_kernel(
    const double *__restrict__ people, const int64_t *__restrict__ k, const int32_t *__restrict__ prev,
    const int32_t *__restrict__ gap, int64_t cap, int64_t carry, const double *__restrict__ zones, int Z,
    const int32_t *__restrict__ next, int32_t *age, int32_t *hits, double *path, double *origin, int32_t *stay,
    int64_t *dwell)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool mine = lane < Z;
    const double qnan = __builtin_nan("");  // a lane without a zone holds nothing
    const double x0 = mine ? zones[4 * lane] : qnan, x1 = mine ? zones[4 * lane + 1] : qnan;
    const double y0 = mine ? zones[4 * lane + 2] : qnan, y1 = mine ? zones[4 * lane + 3] : qnan;
    const int64_t t0 = carry + blockIdx.y, first = carry * cap, K = clamp_k(k, t0, cap);
    for (int64_t j = (int64_t)blockIdx.x * kWaves + wave; j < cap; j += (int64_t)gridDim.x * kWaves) {
        int64_t e = t0 * cap + j;
        if (j >= K) {
            if (lane == 0) store_dead(e, age, hits, path, origin);
            if (mine) stay[e * Z + lane] = -1;
            continue;
        }
        int64_t g;
        const int64_t a = source_of(k, prev, gap, cap, t0, e, g);
        bool cont = a >= 0 && next[a] == (int32_t)e;  // the heir of its source
        if (cont && a >= first) continue;             // the walker that comes through a writes this row
        Hist h;
        int32_t st = -1;  // the lane's zone: frames since the present stay began
        if (cont) {       // the heir of a carried row
            h = anchor(people, age, hits, path, origin, a);
            if (mine) st = stay[a * Z + lane];
        }
        int64_t f = blockIdx.y;
        double qx = people[2 * e], qy = people[2 * e + 1];
        for (;;) {
            advance(h, cont, g, qx, qy);
            if (lane == 0) store_row(h, e, age, hits, path, origin);
            const bool in = inside(x0, x1, y0, y1, qx, qy);  // false in a lane without a zone
            const int32_t was = cont ? st : -1;
            st = in ? (was >= 0 ? was + (int32_t)g : 0) : -1;
            if (mine) stay[e * Z + lane] = st;
            // the stay has ended (only a lane with a zone ever holds was >= 0): its length is not negative, so the
            // unsigned forms hold
            if (was >= 0 && !in) {
                unsigned long long *d = reinterpret_cast<unsigned long long *>(dwell + (f * Z + lane) * 3);
                atomicAdd(d, 1ull);
                atomicAdd(d + 1, (unsigned long long)was);
                atomicMax(d + 2, (unsigned long long)was);
            }
            const int32_t nx = next[e];
            if (nx == kNone) break;
            // nx passed claim_kernel's guard with e as its source: a live row of frame f + g, inside the arrays
            e = nx;
            g = gap ? gap[e] : 1;
            qx = people[2 * e];
            qy = people[2 * e + 1];
            f += g;
            cont = true;
        }
    }
}

}  // namespace

// ====================================================================== C-ABI
LIDAR_EXPORT int lidar_track_history_f64(lidar_handle *h, const double *people, const int64_t *k, const int32_t *prev,
                                         const int32_t *gap, int64_t frames, int64_t cap, int64_t carry,
                                         const double *zones, int32_t nzones, int32_t *age, int32_t *hits, double *path,
                                         double *origin, int32_t *stay, int64_t *dwell, void *stream)
{
    const std::string f("lidar_track_history_f64");
    if (int rc = check_frames(f, h && people && k && prev && age && hits && path && origin, frames, cap)) return rc;
    REQUIRE(carry >= 0 && carry <= frames, f + ": carry must be in 0 .. frames");
    REQUIRE(nzones >= 0 && nzones <= kMaxTab, f + ": nzones must be in 0 .. 64");
    REQUIRE(nzones == 0 || (zones && stay && dwell), f + ": null zone table or zone output");
    if (frames == carry) return LIDAR_OK;  // no frame to compute (frames == 0 among them): nothing is written
    ON_DEVICE(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t nf = frames - carry;
    // next[] is indexed by the row; a claim names a row at most kMaxGap frames back: the rows from lo on are used
    const int64_t lo = std::max<int64_t>(0, carry - kMaxGap) * cap, nn = frames * cap - lo;
    int32_t *next = static_cast<int32_t *>(lidar::workspace(h, (uint64_t)(frames * cap) * sizeof(int32_t)));
    if (!next) return LIDAR_ENOMEM;
    const int64_t nd = nf * nzones * 3;
    const unsigned tiles = row_tiles(cap), blocks = init_blocks(nn + nd);

    lidar::Span sp(h, "track_history", s);
    hipLaunchKernelGGL(init_kernel, dim3(blocks), dim3(kB), 0, s, next + lo, nn, dwell, nd);
    hipLaunchKernelGGL(claim_kernel, dim3(tiles, (unsigned)nf), dim3(kB), 0, s, k, prev, gap, cap, carry, next);
    if (nzones) {
        const unsigned rows = (unsigned)std::min<int64_t>((cap + kWaves - 1) / kWaves, 65535);
        hipLaunchKernelGGL(walk_zones_kernel, dim3(rows, (unsigned)nf), dim3(kB), 0, s, people, k, prev, gap, cap,
                           carry, zones, (int)nzones, next, age, hits, path, origin, stay, dwell);
    } else {
        hipLaunchKernelGGL(walk_kernel, dim3(tiles, (unsigned)nf), dim3(kB), 0, s, people, k, prev, gap, cap, carry,
                           next, age, hits, path, origin);
    }
    LAUNCH_CHECK();
    return LIDAR_OK;
}
