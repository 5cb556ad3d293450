// track.hip — measured crowd flow: people tracked across consecutive frames, and their velocities
// accumulated into the cells of the venue grid (DESIGN.md §3 "People tracking", §4.9).
//
// Contract (include/lidar_amd.h repeats it).  All arithmetic fp64, one rounding per operation.
//   people (T, cap, 2), k (T,): class_people's outputs for T consecutive frames; K_t = min(max(k[t], 0), cap);
//   rows at or past K_t are never read for meaning.
//   Association, per consecutive pair (t-1, t) independently, A = the K_(t-1) rows of frame t-1, B = the
//   K_t rows of frame t: d(i, j) = (dx*dx) + (dy*dy), dx = B[j].x - A[i].x, dy = B[j].y - A[i].y; (i, j) is
//   a candidate iff d <= gate*gate (inclusive; a NaN or infinite coordinate is never a candidate);
//   fwd[i] = the candidate j with the smallest (d, j), bwd[j] = the candidate i with the smallest (d, i),
//   -1 without one; j is matched to i iff bwd[j] == i and fwd[i] == j (mutual nearest neighbour: free of
//   any order, so exact under every parallel schedule).
//   prev[t][j] = i for a matched row, -1 otherwise (unmatched, frame 0, rows at or past K_t);
//   velocity[t][j] = ((B[j].x - A[i].x) / dt, (B[j].y - A[i].y) / dt) for a matched row, (0, 0) otherwise;
//   track_id: a row j < K_t with prev == -1 is a new detection, its id the number of new detections before
//   it in (t, j) ascending order; a matched row takes track_id[t-1][prev[t][j]]; rows at or past K_t -1;
//   ntracks = the number of new detections.
//   Flow cells over the venue grid (x0, y0, g, nx, ny; tier_r.hpp's arange_bin): every matched detection
//   (t >= 1, j < K_t, prev >= 0) is binned by its own position; count = the detections per cell, vsum = the
//   sum of their velocities added SEQUENTIALLY in (t, j) ascending order from 0.0 (no floating atomics:
//   their order is undefined).
//
// Kernels: nearest_kernel (both directions of every pair, three_nn_kernel's form), link_kernel (mutual
// test, prev, velocity, new-detection flags), an exclusive scan of the flags (partial sums, one workgroup
// over the partials, final: no workgroup waits for another), id_kernel (a matched row walks its prev chain
// to the root), cell_kernel and flow_accumulate_kernel (one thread per cell, the detections streamed
// through LDS in (t, j) order and handed to the cell's thread one after the other).
//
// The stream form (lidar_track_stream_f64, lidar_flow_cells_acc_f64; DESIGN.md §3 "Continuous people
// tracking", §4.10) repeats the association for frame distances 1 .. max_gap + 1 over the rows still open and
// takes the state of its first `carry` frames as given: its kernels follow id_kernel below.
#include <cmath>

#include "tier_r.hpp"

namespace {

using namespace lidar::tier_r;

constexpr int kB = 256;                // threads of nearest_kernel and the per-detection kernels
constexpr int kTile = 2048;            // rows of the other frame staged in LDS (16 B each: 32 KiB)
constexpr int kScanPer = 4 * kT;       // flags per workgroup of the scan
constexpr int kRec = 1024;             // detections per LDS tile of flow_accumulate_kernel

__device__ __forceinline__ int64_t clamp_k(const int64_t *k, int64_t t, int64_t cap)
{
    const int64_t v = k[t];
    return v < 0 ? 0 : (v < cap ? v : cap);
}

// blockIdx.y = the pair (t-1, t), blockIdx.z = the direction: 0 fwd (queries A = frame t-1, candidates
// B = frame t, best -> fwd), 1 bwd (queries B, candidates A, best -> bwd).  A thread owns one query row;
// the candidates pass through LDS in ascending tiles, every lane reading the same address (a broadcast).
// A tile's tail up to a multiple of four is NaN: a NaN distance never passes <= gate^2.  The running
// best is replaced under strict < while the candidate index ascends: the lowest index wins a tie.  Both
// directions compute candidate minus query, so a pair's dx in one is the negation of the other's and
// the squares, hence d, have the same bits.
__global__ __launch_bounds__(kB) void nearest_kernel(const double *__restrict__ people, const int64_t *__restrict__ k,
                                                     int64_t cap, double g2, int32_t *__restrict__ fwd,
                                                     int32_t *__restrict__ bwd)
{
    __shared__ double2 s[kTile];
    const int64_t t = (int64_t)blockIdx.y + 1;
    const bool back = blockIdx.z != 0;
    const int64_t fq = back ? t : t - 1, fc = back ? t - 1 : t;
    const int64_t Kq = clamp_k(k, fq, cap), Kc = clamp_k(k, fc, cap);
    int32_t *out = (back ? bwd : fwd) + (int64_t)blockIdx.y * cap;
    const int64_t q = (int64_t)blockIdx.x * kB + threadIdx.x;
    if ((int64_t)blockIdx.x * kB >= Kq) {  // the whole block is past the query frame's rows
        if (q < cap) out[q] = -1;
        return;
    }
    const double qnan = __builtin_nan("");
    double qx = qnan, qy = qnan;  // a thread past K_q keeps NaN: no candidate
    if (q < Kq) {
        qx = people[(fq * cap + q) * 2];
        qy = people[(fq * cap + q) * 2 + 1];
    }
    const double *cand = people + fc * cap * 2;
    double best = INFINITY;
    int32_t bj = -1;
    for (int64_t c0 = 0; c0 < Kc; c0 += kTile) {  // ascending: the tie rule holds across tiles
        const int cnt = (int)(Kc - c0 < kTile ? Kc - c0 : kTile);
        const int cnt4 = (cnt + 3) & ~3;
        __syncthreads();  // the previous tile has been read by every wave
        for (int i = threadIdx.x; i < cnt4; i += kB) {
            double2 v = make_double2(qnan, qnan);
            if (i < cnt) v = make_double2(cand[(c0 + i) * 2], cand[(c0 + i) * 2 + 1]);
            s[i] = v;
        }
        __syncthreads();
        const int32_t jbase = (int32_t)c0;
        for (int i = 0; i < cnt4; i += 4) {
            const double2 v4[4] = {s[i], s[i + 1], s[i + 2], s[i + 3]};  // four reads in flight before the first use
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const double dx = dsub(v4[u].x, qx), dy = dsub(v4[u].y, qy);
                const double d = dadd(dmul(dx, dx), dmul(dy, dy));
                if (d <= g2 && d < best) {
                    best = d;
                    bj = jbase + i + u;
                }
            }
        }
    }
    if (q < cap) out[q] = q < Kq ? bj : -1;
}

// One thread per (t, j): the mutual test, prev, velocity and the new-detection flag (the scan's input).
__global__ __launch_bounds__(kB) void link_kernel(const double *__restrict__ people, const int64_t *__restrict__ k,
                                                  int64_t frames, int64_t cap, double dt,
                                                  const int32_t *__restrict__ fwd, const int32_t *__restrict__ bwd,
                                                  int32_t *__restrict__ prev, double *__restrict__ velocity,
                                                  uint32_t *__restrict__ flag)
{
    const int64_t n = frames * cap;
    for (int64_t e = (int64_t)blockIdx.x * kB + threadIdx.x; e < n; e += (int64_t)gridDim.x * kB) {
        const int64_t t = e / cap, j = e % cap;
        const bool live = j < clamp_k(k, t, cap);
        int32_t p = -1;
        double vx = 0.0, vy = 0.0;
        if (live && t >= 1) {
            const int32_t i = bwd[(t - 1) * cap + j];
            // bwd only holds rows below K_(t-1), whose fwd entries nearest_kernel wrote
            if (i >= 0 && fwd[(t - 1) * cap + i] == (int32_t)j) {
                p = i;
                const double *a = people + ((t - 1) * cap + i) * 2, *b = people + e * 2;
                vx = ddiv(dsub(b[0], a[0]), dt);
                vy = ddiv(dsub(b[1], a[1]), dt);
            }
        }
        prev[e] = p;
        velocity[2 * e] = vx;
        velocity[2 * e + 1] = vy;
        flag[e] = live && p < 0 ? 1u : 0u;
    }
}

// --- exclusive scan of n flags: rank[i] = the sum of flag[0 .. i), rank[n] = the total.  Three launches
// (per-workgroup sums, one workgroup over the sums, the final pass), as dbscan.hip's run_scan; the middle
// one loops, so n is not bounded by kScanPer^2.
__global__ __launch_bounds__(kT) void scan_partial_kernel(const uint32_t *__restrict__ flag, int64_t n,
                                                          uint32_t *__restrict__ partial)
{
    const int64_t b0 = (int64_t)blockIdx.x * kScanPer;
    uint32_t v = 0;
    for (int u = 0; u < 4; ++u) {
        const int64_t i = b0 + threadIdx.x * 4 + u;
        v += i < n ? flag[i] : 0;
    }
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    __shared__ uint32_t ws[kW];
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
        for (int w = 0; w < kW; ++w) tot += ws[w];
        partial[blockIdx.x] = tot;
    }
}
// kScanPer entries from b0 on (4 per thread): out[i] = base + the sum of in[b0 .. i) for i < nout, entries
// from nin on counting 0; returns base + the sum of the thread's own and all earlier entries.  in == out
// is fine: a thread reads its four before it writes them.
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
__global__ __launch_bounds__(kT) void scan_top_kernel(uint32_t *partial, int64_t nblk)
{
    __shared__ uint32_t ws[kW];
    __shared__ uint32_t carry;
    uint32_t base = 0;
    for (int64_t b0 = 0; b0 < nblk; b0 += kScanPer) {
        const uint32_t e = scan_block(partial, nblk, partial, nblk, b0, base, ws);
        if (threadIdx.x == kT - 1) carry = e;
        __syncthreads();  // carry is written; ws is free for the next round
        base = carry;
        __syncthreads();  // carry is read before the next round writes it
    }
}
__global__ __launch_bounds__(kT) void scan_final_kernel(const uint32_t *__restrict__ flag, int64_t n,
                                                        const uint32_t *__restrict__ partial,
                                                        uint32_t *__restrict__ rank)
{
    __shared__ uint32_t ws[kW];
    scan_block(flag, n, rank, n + 1, (int64_t)blockIdx.x * kScanPer, partial[blockIdx.x], ws);
}

// A new detection's id is its rank among the new detections; a matched row walks its prev chain back to
// the root (at most t steps) and takes the root's.
__global__ __launch_bounds__(kB) void id_kernel(const int64_t *__restrict__ k, int64_t frames, int64_t cap,
                                                const int32_t *__restrict__ prev, const uint32_t *__restrict__ rank,
                                                int32_t *__restrict__ track_id, int64_t *__restrict__ ntracks)
{
    const int64_t n = frames * cap;
    for (int64_t e = (int64_t)blockIdx.x * kB + threadIdx.x; e < n; e += (int64_t)gridDim.x * kB) {
        int64_t t = e / cap, j = e % cap;
        int32_t id = -1;
        if (j < clamp_k(k, t, cap)) {
            int32_t p = prev[e];
            while (p >= 0 && t > 0) {  // prev >= 0 only in frames >= 1, and it names a row below K_(t-1)
                --t;
                j = p;
                p = prev[t * cap + j];
            }
            id = (int32_t)rank[t * cap + j];
        }
        track_id[e] = id;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *ntracks = (int64_t)rank[n];
}

// ====================================================================== the stream form
// lidar_track_stream_f64 (DESIGN.md §3 "Continuous people tracking", §4.10): passes g = 1 .. max_gap + 1 in
// ascending order, one launch pair each; pass g associates frame u - g with frame u for every start frame
// u >= max(carry, g), over the rows still open: an end (a row of frame u - g) is open while succ == 0, a
// start (a row of frame u) while prev == -1.  Within a pass a frame is the end frame of one pair and the
// start frame of one pair at most, a pair reads succ of its end frame and prev of its start frame and
// link_open_kernel writes only those two, in a launch of its own after the pass's nearest launch: the pairs
// of a pass are independent under any schedule.

// The frames >= carry start empty; the id base is copied out of *ntracks, which id_stream_kernel overwrites.
__global__ __launch_bounds__(kB) void init_stream_kernel(int64_t first, int64_t n, int32_t *__restrict__ prev,
                                                         int32_t *__restrict__ gap, uint8_t *__restrict__ succ,
                                                         double *__restrict__ velocity,
                                                         const int64_t *__restrict__ ntracks, int64_t *__restrict__ base)
{
    for (int64_t e = first + (int64_t)blockIdx.x * kB + threadIdx.x; e < n; e += (int64_t)gridDim.x * kB) {
        prev[e] = -1;
        gap[e] = 0;
        succ[e] = 0;
        velocity[2 * e] = 0.0;
        velocity[2 * e + 1] = 0.0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *base = *ntracks;
}

constexpr int kRounds = kTile / kB;  // staging rounds of a tile: row r * kB + thread
constexpr int kWaves = kB / 64;

// nearest_kernel over the open rows of the pair (u - g, u), u = u0 + blockIdx.y; fwd and bwd are indexed by
// the START frame u: fwd[u * cap + i] for the end row i, bwd[u * cap + j] for the start row j; a closed row,
// like a row at or past K, gets -1.  A closed query keeps NaN.  A workgroup without an open query writes -1
// and leaves at its first barrier.
//   Compact == false (pass 1, where nearly every row is open): a closed candidate is staged as NaN, which
//   never passes <= g2; the inner loop is nearest_kernel's.
//   Compact == true (passes g >= 2, where a few percent of the rows are open): the tile's open candidates
//   are packed to the front of the LDS tile in ascending row order, the row index beside (x, y): a ballot
//   per staging round, the lane's prefix from the ballot, the (round, wave) offsets through LDS.  The inner
//   loop runs over the open rows alone, in ascending row index, so the tie rule holds.
// Both directions compute candidate minus query (nearest_kernel's comment).
template <bool Compact>
__global__ __launch_bounds__(kB) void nearest_open_kernel(const double *__restrict__ people, const int64_t *__restrict__ k,
                                                          int64_t cap, int64_t u0, int64_t g, double g2,
                                                          const int32_t *__restrict__ prev, const uint8_t *__restrict__ succ,
                                                          int32_t *__restrict__ fwd, int32_t *__restrict__ bwd)
{
    __shared__ double2 s[kTile];
    __shared__ int32_t sj[Compact ? kTile : 1];
    __shared__ uint32_t wc[Compact ? kRounds * kWaves : 1];
    const int64_t u = u0 + (int64_t)blockIdx.y, t = u - g;
    const bool back = blockIdx.z != 0;
    const int64_t fq = back ? u : t, fc = back ? t : u;
    const int64_t Kq = clamp_k(k, fq, cap), Kc = clamp_k(k, fc, cap);
    int32_t *out = (back ? bwd : fwd) + u * cap;
    const int64_t q = (int64_t)blockIdx.x * kB + threadIdx.x;
    bool qopen = false;
    if (q < Kq) qopen = back ? prev[fq * cap + q] < 0 : succ[fq * cap + q] == 0;
    if (!__syncthreads_or(qopen)) {
        if (q < cap) out[q] = -1;
        return;
    }
    const double qnan = __builtin_nan("");
    double qx = qnan, qy = qnan;
    if (qopen) {
        qx = people[(fq * cap + q) * 2];
        qy = people[(fq * cap + q) * 2 + 1];
    }
    const double *cand = people + fc * cap * 2;
    const int32_t *cprev = prev + fc * cap;
    const uint8_t *csucc = succ + fc * cap;
    double best = INFINITY;
    int32_t bj = -1;
    for (int64_t c0 = 0; c0 < Kc; c0 += kTile) {  // ascending: the tie rule holds across tiles
        const int cnt = (int)(Kc - c0 < kTile ? Kc - c0 : kTile);
        int cnt4;
        if constexpr (Compact) {
            const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
            double2 v[kRounds];
            uint64_t m[kRounds];
#pragma unroll
            for (int r = 0; r < kRounds; ++r) {  // every load of the tile in flight before the first barrier
                const int i = r * kB + threadIdx.x;
                bool o = false;
                if (i < cnt) o = back ? csucc[c0 + i] == 0 : cprev[c0 + i] < 0;
                v[r] = o ? make_double2(cand[(c0 + i) * 2], cand[(c0 + i) * 2 + 1]) : make_double2(qnan, qnan);
                m[r] = __ballot(o);
            }
            __syncthreads();  // the previous tile (s, sj, wc) has been read by every wave
            if (lane == 0) {
#pragma unroll
                for (int r = 0; r < kRounds; ++r) wc[r * kWaves + wave] = (uint32_t)__popcll(m[r]);
            }
            __syncthreads();
            uint32_t run = 0, off[kRounds];
#pragma unroll
            for (int r = 0; r < kRounds; ++r) {  // (round, wave) ascending = row index ascending
#pragma unroll
                for (int w = 0; w < kWaves; ++w) {
                    if (w == wave) off[r] = run;
                    run += wc[r * kWaves + w];
                }
            }
            const uint64_t below = (1ull << lane) - 1;
#pragma unroll
            for (int r = 0; r < kRounds; ++r) {
                if ((m[r] >> lane) & 1) {
                    const int pos = (int)off[r] + __popcll(m[r] & below);  // pos < run <= cnt
                    s[pos] = v[r];
                    sj[pos] = (int32_t)(c0 + r * kB + threadIdx.x);
                }
            }
            const int total = (int)run;
            cnt4 = (total + 3) & ~3;  // <= kTile, a multiple of four
            if ((int)threadIdx.x < cnt4 - total) s[total + threadIdx.x] = make_double2(qnan, qnan);
            __syncthreads();
        } else {
            cnt4 = (cnt + 3) & ~3;
            __syncthreads();  // the previous tile has been read by every wave
            for (int i = threadIdx.x; i < cnt4; i += kB) {
                double2 v = make_double2(qnan, qnan);
                if (i < cnt && (back ? csucc[c0 + i] == 0 : cprev[c0 + i] < 0))
                    v = make_double2(cand[(c0 + i) * 2], cand[(c0 + i) * 2 + 1]);
                s[i] = v;
            }
            __syncthreads();
        }
        const int32_t jbase = (int32_t)c0;
        for (int i = 0; i < cnt4; i += 4) {
            const double2 v4[4] = {s[i], s[i + 1], s[i + 2], s[i + 3]};
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const double dx = dsub(v4[w].x, qx), dy = dsub(v4[w].y, qy);
                const double d = dadd(dmul(dx, dx), dmul(dy, dy));
                if (d <= g2 && d < best) {
                    best = d;
                    bj = Compact ? sj[i + w] : jbase + i + w;
                }
            }
        }
    }
    if (q < cap) out[q] = qopen ? bj : -1;
}

// One thread per row (u, j) of the start frames u >= u0 of pass g: the mutual test over the open rows, then
// prev, gap and velocity of the start row and succ of the end row.  An end row is named by at most one
// start row (mutual), so no two threads write the same element; no thread reads what another writes.
__global__ __launch_bounds__(kB) void link_open_kernel(const double *__restrict__ people, const int64_t *__restrict__ k,
                                                       int64_t frames, int64_t cap, int64_t u0, int64_t g, double dtg,
                                                       const int32_t *__restrict__ fwd, const int32_t *__restrict__ bwd,
                                                       int32_t *__restrict__ prev, int32_t *__restrict__ gap,
                                                       uint8_t *__restrict__ succ, double *__restrict__ velocity)
{
    const int64_t n = frames * cap;
    for (int64_t e = u0 * cap + (int64_t)blockIdx.x * kB + threadIdx.x; e < n; e += (int64_t)gridDim.x * kB) {
        const int64_t u = e / cap, j = e % cap;
        if (j >= clamp_k(k, u, cap) || prev[e] >= 0) continue;
        const int32_t i = bwd[e];
        // bwd only holds open rows below K_(u-g), whose fwd entries nearest_open_kernel wrote
        if (i < 0 || fwd[u * cap + i] != (int32_t)j) continue;
        const int64_t a = (u - g) * cap + i;
        prev[e] = i;
        gap[e] = (int32_t)g;
        succ[a] = 1;
        velocity[2 * e] = ddiv(dsub(people[2 * e], people[2 * a]), dtg);
        velocity[2 * e + 1] = ddiv(dsub(people[2 * e + 1], people[2 * a + 1]), dtg);
    }
}

// The new-detection flags of the frames >= carry (first = carry * cap), after the last pass: the scan's input.
__global__ __launch_bounds__(kB) void flag_stream_kernel(const int64_t *__restrict__ k, int64_t first, int64_t n,
                                                         int64_t cap, const int32_t *__restrict__ prev,
                                                         uint32_t *__restrict__ flag)
{
    for (int64_t e = first + (int64_t)blockIdx.x * kB + threadIdx.x; e < n; e += (int64_t)gridDim.x * kB)
        flag[e - first] = e % cap < clamp_k(k, e / cap, cap) && prev[e] < 0 ? 1u : 0u;
}

// id_kernel over (t - gap, prev) chains: the walk ends at a root of a frame >= carry (its id: the base plus its
// rank among the new detections) or at a row of a carry frame, whose track_id is given.  prev and gap of the
// carry frames are never read: every step leaves a frame this call linked, where gap >= 1 and t - gap >= 0.
__global__ __launch_bounds__(kB) void id_stream_kernel(const int64_t *__restrict__ k, int64_t frames, int64_t cap,
                                                       int64_t carry, const int32_t *__restrict__ prev,
                                                       const int32_t *__restrict__ gap, const uint32_t *__restrict__ rank,
                                                       const int64_t *__restrict__ base, int32_t *track_id,
                                                       int64_t *__restrict__ ntracks)
{
    const int64_t n = frames * cap, first = carry * cap;
    const int64_t b = *base;
    for (int64_t e = first + (int64_t)blockIdx.x * kB + threadIdx.x; e < n; e += (int64_t)gridDim.x * kB) {
        int64_t t = e / cap, j = e % cap;
        int32_t id = -1;
        if (j < clamp_k(k, t, cap)) {
            int32_t p;
            while (t >= carry && (p = prev[t * cap + j]) >= 0) {
                t -= gap[t * cap + j];
                j = p;
            }
            // a carry frame's id is read, this launch writes only frames >= carry: no element is both
            id = t >= carry ? (int32_t)(b + (int64_t)rank[t * cap + j - first]) : track_id[t * cap + j];
        }
        track_id[e] = id;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *ntracks = b + (int64_t)rank[n - first];
}

// The cell of every detection of the frames >= first: (bx - 1) * ny + (by - 1) for a matched one inside the
// grid, -1 otherwise.
__global__ __launch_bounds__(kB) void cell_kernel(const double *__restrict__ people, const int64_t *__restrict__ k,
                                                  const int32_t *__restrict__ prev, int64_t frames, int64_t cap,
                                                  int64_t first, double x0, double y0, double g, int64_t nx, int64_t ny,
                                                  int32_t *__restrict__ cell)
{
    const int64_t n = frames * cap;
    for (int64_t e = (int64_t)blockIdx.x * kB + threadIdx.x; e < n; e += (int64_t)gridDim.x * kB) {
        const int64_t t = e / cap, j = e % cap;
        int32_t c = -1;
        if (t >= first && j < clamp_k(k, t, cap) && prev[e] >= 0) {
            const int64_t bx = arange_bin(x0, g, nx, people[2 * e]), by = arange_bin(y0, g, ny, people[2 * e + 1]);
            if (bx >= 1 && bx <= nx && by >= 1 && by <= ny) c = (int32_t)((bx - 1) * ny + (by - 1));
        }
        cell[e] = c;
    }
}

__device__ __forceinline__ double readlane_d(double v, int src)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src),
                            __builtin_amdgcn_readlane(__double2loint(v), src));
}

// One thread per cell, a wave per 64 consecutive cells.  The detections' (cell, vx, vy) records pass through
// LDS in tiles of kRec in (t, j) order.  A wave reads a tile 64 records at a time, one per lane; the records
// that fall into its 64 cells (a ballot) are handed, in ascending record order, to the lane that owns the
// cell, which adds the velocity: every cell's sum has the order of the specification whatever the
// schedule, and a record outside the wave's cells costs one compare in one lane.  (The first form, every
// lane comparing every record with its own cell through broadcast reads, took 7.5 times as long at
// 32 x 4 096 people: DESIGN.md section 4.9.)  A tile in which no record falls into the workgroup's kB cells
// is skipped after staging.  velocity is read for every row of the tile, matched or not.
__global__ __launch_bounds__(kB) void flow_accumulate_kernel(const int32_t *__restrict__ cell,
                                                             const double *__restrict__ velocity, int64_t n,
                                                             int64_t ncell, int accumulate,
                                                             int32_t *__restrict__ count, double *__restrict__ vsum)
{
    __shared__ int32_t sc[kRec];
    __shared__ double2 sv[kRec];
    const int lane = threadIdx.x & 63;
    const int64_t c0 = (int64_t)blockIdx.x * kB, c = c0 + threadIdx.x;
    const int64_t w0 = c - lane;  // the wave's first cell
    double ax = 0.0, ay = 0.0;
    int32_t cnt = 0;
    if (accumulate && c < ncell) {  // the sequential sum goes on from what the earlier calls left
        cnt = count[c];
        ax = vsum[2 * c];
        ay = vsum[2 * c + 1];
    }
    for (int64_t r0 = 0; r0 < n; r0 += kRec) {
        const int tn = (int)(n - r0 < kRec ? n - r0 : kRec);
        int hit = 0;
        __syncthreads();  // the previous tile has been read by every wave
        int32_t v[kRec / kB];
        double2 w[kRec / kB];
#pragma unroll
        for (int u = 0; u < kRec / kB; ++u) {  // every load of the tile in flight at once: none depends on another
            const int i = u * kB + threadIdx.x;
            v[u] = i < tn ? cell[r0 + i] : -1;
            w[u] = i < tn ? make_double2(velocity[2 * (r0 + i)], velocity[2 * (r0 + i) + 1]) : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int u = 0; u < kRec / kB; ++u) {
            const int i = u * kB + threadIdx.x;
            sc[i] = v[u];
            sv[i] = w[u];
            hit |= v[u] >= c0 && v[u] < c0 + kB;
        }
        if (!__syncthreads_or(hit)) continue;
        for (int i = 0; i < kRec; i += 64) {
            const int32_t rc = sc[i + lane];
            const int64_t d = (int64_t)rc - w0;  // cell ids are below ncell (cell_kernel): d names a real cell
            const bool in = rc >= 0 && d >= 0 && d < 64;
            uint64_t m = __ballot(in);
            if (!m) continue;
            const double2 vel = in ? sv[i + lane] : make_double2(0.0, 0.0);
            while (m) {  // ascending lanes: ascending records
                const int src = __ffsll((unsigned long long)m) - 1;
                m &= m - 1;
                const int owner = __builtin_amdgcn_readlane((int)d, src);
                const double vx = readlane_d(vel.x, src), vy = readlane_d(vel.y, src);
                if (lane == owner) {
                    ax = dadd(ax, vx);
                    ay = dadd(ay, vy);
                    ++cnt;
                }
            }
        }
    }
    if (c < ncell) {
        count[c] = cnt;
        vsum[2 * c] = ax;
        vsum[2 * c + 1] = ay;
    }
}

inline bool pos_finite(double v) { return v > 0.0 && v < INFINITY; }

inline unsigned flat_blocks(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + kB - 1) / kB, 4096)); }

}  // namespace

// ====================================================================== C-ABI
LIDAR_EXPORT int lidar_track_people_f64(lidar_handle *h, const double *people, const int64_t *k, int64_t frames,
                                        int64_t cap, double dt, double gate, int32_t *prev, int32_t *track_id,
                                        double *velocity, int64_t *ntracks, void *stream)
{
    REQUIRE(h && people && k && prev && track_id && velocity && ntracks, "lidar_track_people_f64: null pointer");
    REQUIRE(frames >= 0 && frames <= 65535, "lidar_track_people_f64: frames out of range");
    REQUIRE(cap >= 1, "lidar_track_people_f64: cap must be >= 1");
    REQUIRE(cap < 0x80000000ll && frames * cap < 0x80000000ll, "lidar_track_people_f64: frames * cap must be below 2^31");
    REQUIRE(pos_finite(dt), "lidar_track_people_f64: dt must be positive and finite");
    REQUIRE(pos_finite(gate), "lidar_track_people_f64: gate must be positive and finite");
    if (frames == 0) return LIDAR_OK;
    ON_DEVICE(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t n = frames * cap, pairs = frames - 1;
    const int64_t nblk = (n + 1 + kScanPer - 1) / kScanPer;

    lidar::Carver cv;
    const uint64_t o_fwd = cv.take<int32_t>(std::max<int64_t>(1, pairs * cap));
    const uint64_t o_bwd = cv.take<int32_t>(std::max<int64_t>(1, pairs * cap));
    const uint64_t o_flag = cv.take<uint32_t>(n), o_rank = cv.take<uint32_t>(n + 1);
    const uint64_t o_part = cv.take<uint32_t>(nblk);
    char *base = static_cast<char *>(lidar::workspace(h, cv.off));
    if (!base) return LIDAR_ENOMEM;
    int32_t *fwd = reinterpret_cast<int32_t *>(base + o_fwd), *bwd = reinterpret_cast<int32_t *>(base + o_bwd);
    uint32_t *flag = reinterpret_cast<uint32_t *>(base + o_flag), *rank = reinterpret_cast<uint32_t *>(base + o_rank);
    uint32_t *partial = reinterpret_cast<uint32_t *>(base + o_part);

    lidar::Span sp(h, "track_people", s);
    if (pairs > 0)
        hipLaunchKernelGGL(nearest_kernel, dim3((unsigned)((cap + kB - 1) / kB), (unsigned)pairs, 2), dim3(kB), 0, s,
                           people, k, cap, gate * gate, fwd, bwd);
    hipLaunchKernelGGL(link_kernel, dim3(flat_blocks(n)), dim3(kB), 0, s, people, k, frames, cap, dt, fwd, bwd, prev,
                       velocity, flag);
    hipLaunchKernelGGL(scan_partial_kernel, dim3((unsigned)nblk), dim3(kT), 0, s, flag, n, partial);
    hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(kT), 0, s, partial, nblk);
    hipLaunchKernelGGL(scan_final_kernel, dim3((unsigned)nblk), dim3(kT), 0, s, flag, n, partial, rank);
    hipLaunchKernelGGL(id_kernel, dim3(flat_blocks(n)), dim3(kB), 0, s, k, frames, cap, prev, rank, track_id, ntracks);
    LAUNCH_CHECK();
    return LIDAR_OK;
}

LIDAR_EXPORT int lidar_track_stream_f64(lidar_handle *h, const double *people, const int64_t *k, int64_t frames,
                                        int64_t cap, int64_t carry, double dt, double gate, int32_t max_gap,
                                        int32_t *prev, int32_t *gap, uint8_t *succ, double *velocity,
                                        int32_t *track_id, int64_t *ntracks, void *stream)
{
    REQUIRE(h && people && k && prev && gap && succ && velocity && track_id && ntracks,
            "lidar_track_stream_f64: null pointer");
    REQUIRE(frames >= 0 && frames <= 65535, "lidar_track_stream_f64: frames out of range");
    REQUIRE(cap >= 1, "lidar_track_stream_f64: cap must be >= 1");
    REQUIRE(cap < 0x80000000ll && frames * cap < 0x80000000ll, "lidar_track_stream_f64: frames * cap must be below 2^31");
    REQUIRE(pos_finite(dt), "lidar_track_stream_f64: dt must be positive and finite");
    REQUIRE(pos_finite(gate), "lidar_track_stream_f64: gate must be positive and finite");
    REQUIRE(max_gap >= 0 && max_gap <= 7, "lidar_track_stream_f64: max_gap must be in 0 .. 7");
    REQUIRE(carry >= 0 && carry <= std::min<int64_t>(max_gap + 1, frames),
            "lidar_track_stream_f64: carry must be in 0 .. min(max_gap + 1, frames)");
    if (frames == carry) return LIDAR_OK;  // no frame to link (frames == 0 among them): nothing is written
    ON_DEVICE(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t n = frames * cap, first = carry * cap, nnew = n - first;
    const int64_t nblk = (nnew + 1 + kScanPer - 1) / kScanPer;

    lidar::Carver cv;
    const uint64_t o_fwd = cv.take<int32_t>(n), o_bwd = cv.take<int32_t>(n);  // indexed by the start frame
    const uint64_t o_flag = cv.take<uint32_t>(nnew), o_rank = cv.take<uint32_t>(nnew + 1);
    const uint64_t o_part = cv.take<uint32_t>(nblk), o_base = cv.take<int64_t>(1);
    char *base = static_cast<char *>(lidar::workspace(h, cv.off));
    if (!base) return LIDAR_ENOMEM;
    int32_t *fwd = reinterpret_cast<int32_t *>(base + o_fwd), *bwd = reinterpret_cast<int32_t *>(base + o_bwd);
    uint32_t *flag = reinterpret_cast<uint32_t *>(base + o_flag), *rank = reinterpret_cast<uint32_t *>(base + o_rank);
    uint32_t *partial = reinterpret_cast<uint32_t *>(base + o_part);
    int64_t *idbase = reinterpret_cast<int64_t *>(base + o_base);

    static const char *const kPass[8] = {"track_stream_pass1", "track_stream_pass2", "track_stream_pass3",
                                         "track_stream_pass4", "track_stream_pass5", "track_stream_pass6",
                                         "track_stream_pass7", "track_stream_pass8"};
    const dim3 rows((unsigned)((cap + kB - 1) / kB));
    {
        lidar::Span sp(h, "track_stream_init", s);
        hipLaunchKernelGGL(init_stream_kernel, dim3(flat_blocks(nnew)), dim3(kB), 0, s, first, n, prev, gap, succ,
                           velocity, ntracks, idbase);
    }
    for (int64_t g = 1; g <= max_gap + 1; ++g) {  // ascending: a pass sees what the passes before it linked
        const int64_t u0 = std::max(carry, g), pairs = frames - u0;
        if (pairs <= 0) break;
        const double gg = gate * (double)g, dtg = dt * (double)g;  // one fp64 product each
        const dim3 grid(rows.x, (unsigned)pairs, 2);
        lidar::Span sp(h, kPass[g - 1], s);
#ifdef LIDAR_TRACK_GAP_MASKED  // a measuring build: the masked form in every pass
        const bool compact = false;
#else
        const bool compact = g >= 2;
#endif
        if (compact)
            hipLaunchKernelGGL(nearest_open_kernel<true>, grid, dim3(kB), 0, s, people, k, cap, u0, g, gg * gg, prev, succ,
                               fwd, bwd);
        else
            hipLaunchKernelGGL(nearest_open_kernel<false>, grid, dim3(kB), 0, s, people, k, cap, u0, g, gg * gg, prev,
                               succ, fwd, bwd);
        hipLaunchKernelGGL(link_open_kernel, dim3(flat_blocks(pairs * cap)), dim3(kB), 0, s, people, k, frames, cap, u0, g,
                           dtg, fwd, bwd, prev, gap, succ, velocity);
    }
    {
        lidar::Span sp(h, "track_stream_ids", s);
        hipLaunchKernelGGL(flag_stream_kernel, dim3(flat_blocks(nnew)), dim3(kB), 0, s, k, first, n, cap, prev, flag);
        hipLaunchKernelGGL(scan_partial_kernel, dim3((unsigned)nblk), dim3(kT), 0, s, flag, nnew, partial);
        hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(kT), 0, s, partial, nblk);
        hipLaunchKernelGGL(scan_final_kernel, dim3((unsigned)nblk), dim3(kT), 0, s, flag, nnew, partial, rank);
        hipLaunchKernelGGL(id_stream_kernel, dim3(flat_blocks(nnew)), dim3(kB), 0, s, k, frames, cap, carry, prev, gap,
                           rank, idbase, track_id, ntracks);
    }
    LAUNCH_CHECK();
    return LIDAR_OK;
}

namespace {

int flow_cells(const char *fn, lidar_handle *h, const double *people, const int64_t *k, const int32_t *prev,
               const double *velocity, int64_t frames, int64_t cap, int64_t first, int accumulate, double x0, double y0,
               double grid, int64_t nx, int64_t ny, int32_t *count, double *vsum, void *stream)
{
    const std::string f(fn);
    REQUIRE(h && people && k && prev && velocity && count && vsum, f + ": null pointer");
    REQUIRE(frames >= 0 && frames <= 65535, f + ": frames out of range");
    REQUIRE(cap >= 1, f + ": cap must be >= 1");
    REQUIRE(cap < 0x80000000ll && frames * cap < 0x80000000ll, f + ": frames * cap must be below 2^31");
    REQUIRE(first >= 0 && first <= frames, f + ": first must be in 0 .. frames");
    REQUIRE(accumulate == 0 || accumulate == 1, f + ": accumulate must be 0 or 1");
    REQUIRE(pos_finite(grid), f + ": grid must be positive and finite");
    REQUIRE(nx >= 1 && ny >= 1, f + ": nx and ny must be >= 1");
    REQUIRE(nx < 0x80000000ll && ny < 0x80000000ll && nx * ny < 0x80000000ll, f + ": nx * ny must be below 2^31");
    REQUIRE(std::isfinite(x0) && std::isfinite(y0), f + ": x0 and y0 must be finite");
    if (frames == 0) return LIDAR_OK;
    ON_DEVICE(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t n = frames * cap, ncell = nx * ny;
    lidar::Carver cv;
    const uint64_t o_cell = cv.take<int32_t>(n);
    char *base = static_cast<char *>(lidar::workspace(h, cv.off));
    if (!base) return LIDAR_ENOMEM;
    int32_t *cell = reinterpret_cast<int32_t *>(base + o_cell);

    lidar::Span sp(h, "flow_cells", s);
    hipLaunchKernelGGL(cell_kernel, dim3(flat_blocks(n)), dim3(kB), 0, s, people, k, prev, frames, cap, first, x0, y0,
                       grid, nx, ny, cell);
    hipLaunchKernelGGL(flow_accumulate_kernel, dim3((unsigned)((ncell + kB - 1) / kB)), dim3(kB), 0, s, cell, velocity,
                       n, ncell, accumulate, count, vsum);
    LAUNCH_CHECK();
    return LIDAR_OK;
}

}  // namespace

LIDAR_EXPORT int lidar_flow_cells_f64(lidar_handle *h, const double *people, const int64_t *k, const int32_t *prev,
                                      const double *velocity, int64_t frames, int64_t cap, double x0, double y0,
                                      double grid, int64_t nx, int64_t ny, int32_t *count, double *vsum, void *stream)
{
    // first = 1: a frame-0 row has no predecessor in this call (0 frames: the range check of `first` has none to offer)
    return flow_cells("lidar_flow_cells_f64", h, people, k, prev, velocity, frames, cap, frames > 0 ? 1 : 0, 0, x0, y0,
                      grid, nx, ny, count, vsum, stream);
}

LIDAR_EXPORT int lidar_flow_cells_acc_f64(lidar_handle *h, const double *people, const int64_t *k, const int32_t *prev,
                                          const double *velocity, int64_t frames, int64_t cap, int64_t first,
                                          int32_t accumulate, double x0, double y0, double grid, int64_t nx, int64_t ny,
                                          int32_t *count, double *vsum, void *stream)
{
    return flow_cells("lidar_flow_cells_acc_f64", h, people, k, prev, velocity, frames, cap, first, accumulate, x0, y0,
                      grid, nx, ny, count, vsum, stream);
}
