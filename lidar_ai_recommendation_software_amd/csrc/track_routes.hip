// track_routes.hip — zone-to-zone trips of tracked people from their links (DESIGN.md §3 "Routes", §4.16): per
// detection the first and the last zone its track was seen in, how long ago, how many legs it has made and the leg
// it completes, and per pair of zones the trips, their summed and their longest travel time.
//
// Contract (include/lidar_amd.h repeats it).  Integers only.
//   people (T, cap, 2), k (T,), K_t, prev (T, cap) int32, gap (T, cap) int32 or null (every link spans one frame),
//   the link guard (track_links.hpp: source_of) and the heirs are lidar_track_history_f64's: a row (t, j), j < K_t,
//   is linked iff, with i = prev[t][j] and g = gap ? gap[t][j] : 1, i >= 0 and 1 <= g <= 8 and g <= t and
//   i < K_(t-g); its source is the row (s, i), s = t - g.  No content of prev / gap makes a kernel read or write
//   outside the arrays.  zones (Z, 4) rows (x0, x1, y0, y1), 1 <= Z <= 64; inside(z, p) = x0 <= p.x < x1 and
//   y0 <= p.y < y1; zone_of(p) = the lowest z with inside(z, p), -1 without one (a NaN position is in no zone).
//   carry = C: the leading frames whose route state is given, never written.
//   Heirs: among the rows of frames >= C linked to the same source, the lowest in (t, j) order continues the
//   source's route; every other row of a frame >= C (unlinked, or linked and not the heir) starts one.
//   Per row of a frame >= C (every element written), all (T, cap) int32; c = zone_of(Q), Q the row's own position,
//   g the link's frame distance, (F, L, A, N) the source's first_zone, last_zone, away, legs, and for a continuing
//   row with c >= 0: leg = L >= 0 and (L != c or A > 0).
//                    starts            continues, c < 0        continues, c >= 0     j >= K_t
//     first_zone     c                 F                       F >= 0 ? F : c        -1
//     last_zone      c                 L                       c                     -1
//     away           c >= 0 ? 0 : -1   L >= 0 ? A + g : -1     0                     -1
//     legs           0                 N                       N + leg               0
//     leg_from       -1                -1                      leg ? L : -1          -1
//     leg_frames     0                 0                       leg ? A + g : 0       0
//   trips (Z, Z, 3) int64: a row with a leg adds 1 to trips[L][c][0] and A + g to [1] and raises [2] to A + g.
//   accumulate = 0: from zero, every element written; 1: from what the array holds.  Integer atomics: the same
//   numbers under every schedule.  (A carried last_zone outside -1 .. Z - 1 is no zone of this table: such a leg
//   is written per row as the table says and adds no trip, so nothing is written outside trips.)
//
// Kernels, three launches, no workgroup waiting for another:
//   init_kernel, claim_kernel   track_chain.hpp, shared with track_history.hip: next[row] = kNone over the rows a
//                  claim can name and trips = 0 unless accumulating; then the heirs by atomicMin.
//   walk_kernel    a thread per row of the frames >= C, track_history.hip's walk_kernel in form: the grid is (row
//                  tile of 256, frame - C).  A row at or past K_t gets the defaults.  A live row that is the heir of
//                  a row of a frame >= C leaves: the walker that comes through its source writes it.  Every other
//                  live row is a walk start (the start of a route, or the heir of a carried row, whose state is the
//                  anchor): its thread writes it and follows next[] until kNone, (F, L, A, N) in registers.  The
//                  zone table is staged once per workgroup into LDS, 64 rows of 32 B; the loop over z reads it at an
//                  address every lane shares (a broadcast), descends from Z - 1 to 0 and keeps a hit with a select:
//                  the last hit kept is the lowest, and no lane leaves the loop before the others.  A step's
//                  dependent loads are next[cur], then Q and gap of that row; its stores six int32, and three 64-bit
//                  integer atomics when it is a leg.  History's wave per row exists because it stores Z counters per
//                  row and step; a route stores six words whatever Z is, so 64 chains per wave hide the chain of
//                  dependent loads that one chain per wave would not.
#include "track_chain.hpp"

namespace {

using namespace lidar::tier_r;
using namespace lidar::track;

// The route state a walker carries from one row to the next.
struct Route {
    int32_t first, last, away, legs;
};

// zone_of(q): the zones descend, so the hit that stays is the lowest; Z is uniform, every lane makes Z iterations.
__device__ __forceinline__ int32_t zone_of(const double (*box)[4], int Z, double qx, double qy)
{
    int32_t c = -1;
    for (int z = Z - 1; z >= 0; --z) c = inside(box[z][0], box[z][1], box[z][2], box[z][3], qx, qy) ? z : c;
    return c;
}

// blockIdx.y = t - carry; blockIdx.x and gridDim.x stride over the frame's row tiles.  The four state arrays are read
// in the carry frames and written in the frames >= carry: no __restrict__.
__global__ __launch_bounds__(kB) void walk_kernel(const double *__restrict__ people, const int64_t *__restrict__ k,
                                                  const int32_t *__restrict__ prev, const int32_t *__restrict__ gap,
                                                  int64_t cap, int64_t carry, const double *__restrict__ zones, int Z,
                                                  const int32_t *__restrict__ next, int32_t *first_zone,
                                                  int32_t *last_zone, int32_t *away, int32_t *legs,
                                                  int32_t *__restrict__ leg_from, int32_t *__restrict__ leg_frames,
                                                  int64_t *__restrict__ trips)
{
    __shared__ __attribute__((aligned(32))) double box[kMaxTab][4];
    for (int i = threadIdx.x; i < 4 * Z; i += kB) box[i >> 2][i & 3] = zones[i];
    __syncthreads();
    const int64_t t0 = carry + blockIdx.y, first = carry * cap, K = clamp_k(k, t0, cap);
    for (int64_t j = (int64_t)blockIdx.x * kB + threadIdx.x; j < cap; j += (int64_t)gridDim.x * kB) {
        int64_t e = t0 * cap + j;
        if (j >= K) {
            first_zone[e] = -1;
            last_zone[e] = -1;
            away[e] = -1;
            legs[e] = 0;
            leg_from[e] = -1;
            leg_frames[e] = 0;
            continue;
        }
        int64_t g;
        const int64_t a = source_of(k, prev, gap, cap, t0, e, g);
        bool cont = a >= 0 && next[a] == (int32_t)e;  // the heir of its source
        if (cont && a >= first) continue;             // the walker that comes through a writes this row
        Route r{-1, -1, -1, 0};
        if (cont) r = Route{first_zone[a], last_zone[a], away[a], legs[a]};  // the heir of a carried row
        double qx = people[2 * e], qy = people[2 * e + 1];
        for (;;) {
            const int32_t c = zone_of(box, Z, qx, qy);
            int32_t from = -1, took = 0;
            if (!cont) {
                r = Route{c, c, c >= 0 ? 0 : -1, 0};
            } else if (c < 0) {
                r.away = r.last >= 0 ? r.away + (int32_t)g : -1;
            } else {
                if (r.last >= 0 && (r.last != c || r.away > 0)) {  // a leg: from another zone, or back after being out
                    from = r.last;
                    took = r.away + (int32_t)g;
                    r.legs += 1;
                    // a travel time is not negative, so the unsigned forms hold
                    if (from < Z) {
                        unsigned long long *d = reinterpret_cast<unsigned long long *>(trips + ((int64_t)from * Z + c) * 3);
                        atomicAdd(d, 1ull);
                        atomicAdd(d + 1, (unsigned long long)took);
                        atomicMax(d + 2, (unsigned long long)took);
                    }
                }
                r.first = r.first >= 0 ? r.first : c;
                r.last = c;
                r.away = 0;
            }
            first_zone[e] = r.first;
            last_zone[e] = r.last;
            away[e] = r.away;
            legs[e] = r.legs;
            leg_from[e] = from;
            leg_frames[e] = took;
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

}  // namespace

// ====================================================================== C-ABI
LIDAR_EXPORT int lidar_track_routes_f64(lidar_handle *h, const double *people, const int64_t *k, const int32_t *prev,
                                        const int32_t *gap, int64_t frames, int64_t cap, int64_t carry,
                                        const double *zones, int32_t nzones, int32_t *first_zone, int32_t *last_zone,
                                        int32_t *away, int32_t *legs, int32_t *leg_from, int32_t *leg_frames,
                                        int64_t *trips, int32_t accumulate, void *stream)
{
    const std::string f("lidar_track_routes_f64");
    if (int rc = check_frames(f, h && people && k && prev && zones && first_zone && last_zone && away && legs &&
                                     leg_from && leg_frames && trips, frames, cap))
        return rc;
    REQUIRE(carry >= 0 && carry <= frames, f + ": carry must be in 0 .. frames");
    REQUIRE(nzones >= 1 && nzones <= kMaxTab, f + ": nzones must be in 1 .. 64");
    REQUIRE(accumulate == 0 || accumulate == 1, f + ": accumulate must be 0 or 1");
    const int64_t nz = accumulate ? 0 : (int64_t)nzones * nzones * 3;
    if (frames == carry && !nz) return LIDAR_OK;  // no frame to compute, and the trips go on: nothing is written
    ON_DEVICE(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    lidar::Span sp(h, "track_routes", s);
    if (frames == carry) {  // no frame to compute: the trips count from zero all the same
        hipLaunchKernelGGL(init_kernel, dim3(init_blocks(nz)), dim3(kB), 0, s, (int32_t *)nullptr, (int64_t)0, trips, nz);
        LAUNCH_CHECK();
        return LIDAR_OK;
    }
    const int64_t nf = frames - carry;
    // next[] is indexed by the row; a claim names a row at most kMaxGap frames back: the rows from lo on are used
    const int64_t lo = std::max<int64_t>(0, carry - kMaxGap) * cap, nn = frames * cap - lo;
    int32_t *next = static_cast<int32_t *>(lidar::workspace(h, (uint64_t)(frames * cap) * sizeof(int32_t)));
    if (!next) return LIDAR_ENOMEM;
    const unsigned tiles = row_tiles(cap);

    hipLaunchKernelGGL(init_kernel, dim3(init_blocks(nn + nz)), dim3(kB), 0, s, next + lo, nn, trips, nz);
    hipLaunchKernelGGL(claim_kernel, dim3(tiles, (unsigned)nf), dim3(kB), 0, s, k, prev, gap, cap, carry, next);
    hipLaunchKernelGGL(walk_kernel, dim3(tiles, (unsigned)nf), dim3(kB), 0, s, people, k, prev, gap, cap, carry, zones,
                       (int)nzones, next, first_zone, last_zone, away, legs, leg_from, leg_frames, trips);
    LAUNCH_CHECK();
    return LIDAR_OK;
}
