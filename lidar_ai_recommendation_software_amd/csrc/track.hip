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
// The stream form (lidar_track_stream_f64, lidar_flow_cells_acc_f64; DESIGN.md §3 "Continuous people
// tracking", §4.10) repeats the association for frame distances 1 .. max_gap + 1 over the rows still open and
// takes the state of its first `carry` frames as given.  With max_gap = 0 and no carry it is the batch form
// bit for bit, and the two share every piece but the link kernel:
//
// Kernels: nearest_kernel<Rows> (both directions of every pair, three_nn_kernel's form; All: the batch form,
// Masked and Compact: the stream form's open rows), link_kernel (batch: mutual test, prev, velocity,
// new-detection flags in one launch) or init_stream_kernel, link_open_kernel per pass and flag_stream_kernel
// (stream), an exclusive scan of the flags (tier_r.hpp's device code in three launches: partial sums, one
// workgroup over the partials, final: no workgroup waits for another), id_kernel (a matched row walks its
// prev chain to a root or a carried row), cell_kernel and flow_accumulate_kernel (one thread per cell, the
// detections streamed through LDS in (t, j) order and handed to the cell's thread one after the other).
#include <cmath>

#include "track_links.hpp"

namespace {

using namespace lidar::tier_r;
using namespace lidar::track;

constexpr int kB = 256;                // threads of nearest_kernel and the per-detection kernels
constexpr int kTile = 2048;            // rows of the other frame staged in LDS (16 B each: 32 KiB)
constexpr int kRounds = kTile / kB;    // staging rounds of a tile in nearest_kernel<Compact>: row r * kB + thread
constexpr int kWaves = kB / 64;
constexpr int kRec = 1024;             // detections per LDS tile of flow_accumulate_kernel

// The rows nearest_kernel takes.  An end row (frame u - g) is open while succ == 0, a start row (frame u)
// while prev == -1.
enum class Rows {
    All,      // every row below K: the batch form.  prev and succ are never read (null)
    Masked,   // the open rows, a closed candidate staged as NaN (never passes <= g2): stream pass 1, where
              // nearly every row is open
    Compact,  // the open rows, a tile's open candidates packed to its front: stream passes g >= 2, where a
              // few percent of the rows are open
};

// The pair (u - g, u), u = u0 + blockIdx.y (the batch form: u0 = g = 1); blockIdx.z = the direction: 0 fwd
// (queries A = frame u - g, candidates B = frame u, best -> fwd), 1 bwd (queries B, candidates A, best ->
// bwd).  fwd and bwd are indexed by the START frame u: fwd[u * cap + i] for the end row i, bwd[u * cap + j]
// for the start row j; a closed row, like a row at or past K, gets -1.  A thread owns one query row (a
// closed one keeps NaN); the candidates pass through LDS in ascending tiles, every lane reading the same
// address (a broadcast).  A tile's tail up to a multiple of four is NaN: a NaN distance never passes
// <= gate^2.  The running best is replaced under strict < while the candidate index ascends: the lowest
// index wins a tie.  Both directions compute candidate minus query, so a pair's dx in one is the negation of
// the other's and the squares, hence d, have the same bits.
//   A workgroup without a query writes -1 and leaves: All on its block index alone (no block-wide OR, so no
//   LDS beside the tile), Masked and Compact at their first barrier.
//   Compact packs the open candidates in ascending row order, the row index beside (x, y): a ballot per
//   staging round, the lane's prefix from the ballot, the (round, wave) offsets through LDS.  The inner loop
//   runs over the open rows alone, in ascending row index, so the tie rule holds.
template <Rows R>
__global__ __launch_bounds__(kB) void nearest_kernel(const double *__restrict__ people, const int64_t *__restrict__ k,
                                                     int64_t cap, int64_t u0, int64_t g, double g2,
                                                     const int32_t *__restrict__ prev, const uint8_t *__restrict__ succ,
                                                     int32_t *__restrict__ fwd, int32_t *__restrict__ bwd)
{
    constexpr bool kCompact = R == Rows::Compact;
    __shared__ double2 s[kTile];
    __shared__ int32_t sj[kCompact ? kTile : 1];
    __shared__ uint32_t wc[kCompact ? kRounds * kWaves : 1];
    const int64_t u = u0 + (int64_t)blockIdx.y, t = u - g;
    const bool back = blockIdx.z != 0;
    const int64_t fq = back ? u : t, fc = back ? t : u;
    const int64_t Kq = clamp_k(k, fq, cap), Kc = clamp_k(k, fc, cap);
    int32_t *out = (back ? bwd : fwd) + u * cap;
    const int64_t q = (int64_t)blockIdx.x * kB + threadIdx.x;
    // bwd's queries and fwd's candidates are start rows; the other two are end rows
    const auto open = [&](int64_t row, bool start) {
        if constexpr (R == Rows::All) return true;
        else return start ? prev[row] < 0 : succ[row] == 0;
    };
    const bool qopen = q < Kq && open(fq * cap + q, back);
    bool none;
    if constexpr (R == Rows::All) none = (int64_t)blockIdx.x * kB >= Kq;  // the whole block is past the query frame's rows
    else none = !__syncthreads_or(qopen);
    if (none) {
        if (q < cap) out[q] = -1;
        return;
    }
    const double qnan = __builtin_nan("");
    double qx = qnan, qy = qnan;  // a thread without an open query keeps NaN: no candidate
    if (qopen) {
        qx = people[(fq * cap + q) * 2];
        qy = people[(fq * cap + q) * 2 + 1];
    }
    const double *cand = people + fc * cap * 2;
    double best = INFINITY;
    int32_t bj = -1;
    for (int64_t c0 = 0; c0 < Kc; c0 += kTile) {  // ascending: the tie rule holds across tiles
        const int cnt = (int)(Kc - c0 < kTile ? Kc - c0 : kTile);
        int cnt4;
        if constexpr (kCompact) {
            const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
            double2 v[kRounds];
            uint64_t m[kRounds];
#pragma unroll
            for (int r = 0; r < kRounds; ++r) {  // every load of the tile in flight before the first barrier
                const int i = r * kB + threadIdx.x;
                const bool o = i < cnt && open(fc * cap + c0 + i, !back);
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
                if (i < cnt && open(fc * cap + c0 + i, !back)) v = make_double2(cand[(c0 + i) * 2], cand[(c0 + i) * 2 + 1]);
                s[i] = v;
            }
            __syncthreads();
        }
        const int32_t jbase = (int32_t)c0;
        // The loop below runs with one wave per SIMD at K <= 1 024, and where its head falls in a 64-byte
        // instruction line shows: 3 % of the All kernel between offsets 4 and 24.  Anchoring
        // its preheader to a line keeps the head where it is whatever the code before it becomes.
        asm volatile(".p2align 6");
        for (int i = 0; i < cnt4; i += 4) {
            const double2 v4[4] = {s[i], s[i + 1], s[i + 2], s[i + 3]};  // four reads in flight before the first use
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const double dx = dsub(v4[w].x, qx), dy = dsub(v4[w].y, qy);
                const double d = dadd(dmul(dx, dx), dmul(dy, dy));
                if (d <= g2 && d < best) {
                    best = d;
                    bj = kCompact ? sj[i + w] : jbase + i + w;
                }
            }
        }
    }
    if (q < cap) out[q] = qopen ? bj : -1;
}

// The mutual test of the start row (u, j) over the pair (u - g, u): the end row i with bwd == i and fwd[i] == j,
// and the velocity over dtg into (vx, vy); -1 without one, (vx, vy) untouched.  bwd only holds (open) rows
// below K_(u-g), whose fwd entries nearest_kernel wrote.
__device__ __forceinline__ int32_t mutual(const double *__restrict__ people, const int32_t *__restrict__ fwd,
                                          const int32_t *__restrict__ bwd, int64_t cap, int64_t u, int64_t j, int64_t g,
                                          double dtg, double &vx, double &vy)
{
    const int64_t e = u * cap + j;
    const int32_t i = bwd[e];
    if (i < 0 || fwd[u * cap + i] != (int32_t)j) return -1;
    const int64_t a = (u - g) * cap + i;
    vx = ddiv(dsub(people[2 * e], people[2 * a]), dtg);
    vy = ddiv(dsub(people[2 * e + 1], people[2 * a + 1]), dtg);
    return i;
}

// The batch form, one thread per (t, j): the mutual test, prev, velocity and the new-detection flag (the
// scan's input).  Every row is written, so the batch form needs no init and no flag launch.
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
        if (live && t >= 1) p = mutual(people, fwd, bwd, cap, t, j, 1, dt, vx, vy);
        prev[e] = p;
        velocity[2 * e] = vx;
        velocity[2 * e + 1] = vy;
        flag[e] = live && p < 0 ? 1u : 0u;
    }
}

// --- exclusive scan of n flags: rank[i] = the sum of flag[0 .. i), rank[n] = the total.  Three launches over
// tier_r.hpp's scan_block_sum and scan_block; the middle one loops, so n is not bounded by kScanPer^2.
__global__ __launch_bounds__(kT) void scan_partial_kernel(const uint32_t *__restrict__ flag, int64_t n,
                                                          uint32_t *__restrict__ partial)
{
    __shared__ uint32_t ws[kW];
    scan_block_sum(flag, n, (int64_t)blockIdx.x * kScanPer, ws, &partial[blockIdx.x]);
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

// A row's walk along its (frame - gap, prev) chain, from the row j of the frame whose first row is `row` (t * cap:
// the frame is a carry frame iff row < first) to where it ends: at a row with prev < 0, or at a row of a carry
// frame.  Gaps == false: every step is one frame.  The walk is a chain of dependent loads with a wave or two per
// SIMD, so every instruction and every taken branch of a step counts: the frame moves by subtraction, the loop
// has one exit and no branch inside, and the launch-uniform choice of Gaps is made outside it.
template <bool Gaps>
__device__ __forceinline__ void walk(const int32_t *__restrict__ prev, const int32_t *__restrict__ gap, int64_t cap,
                                     int64_t first, int64_t &row, int64_t &j)
{
    int32_t p = prev[row + j];
    while (p >= 0) {
        row -= Gaps ? (int64_t)gap[row + j] * cap : cap;
        j = p;
        const int32_t q = prev[row + j];  // loaded, not used, in a carry frame: a select, no branch
        p = row >= first ? q : -1;
    }
}

// The ids of the frames >= carry (first = carry * cap; flag and rank start there).  gap == null: the batch form,
// every step of a walk is one frame.  A walk ends at a root of a frame >= carry, a new detection (its id: the
// base plus its rank among the new detections; base == null: 0), or at a row of a carry frame, whose track_id
// is given.  prev and gap of the carry frames are never used (walk() loads a carry row's prev and drops it):
// every step leaves a frame this call linked, where gap >= 1 and t - gap >= 0.
__global__ __launch_bounds__(kB) void id_kernel(const int64_t *__restrict__ k, int64_t frames, int64_t cap, int64_t carry,
                                                const int32_t *__restrict__ prev, const int32_t *__restrict__ gap,
                                                const uint32_t *__restrict__ rank, const int64_t *__restrict__ base,
                                                int32_t *track_id, int64_t *__restrict__ ntracks)
{
    const int64_t n = frames * cap, first = carry * cap;
    const int64_t b = base ? *base : 0;
    for (int64_t e = first + (int64_t)blockIdx.x * kB + threadIdx.x; e < n; e += (int64_t)gridDim.x * kB) {
        int64_t j = e % cap, row = e - j;
        int32_t id = -1;
        if (j < clamp_k(k, e / cap, cap)) {
            if (gap) walk<true>(prev, gap, cap, first, row, j);
            else walk<false>(prev, gap, cap, first, row, j);
            // a carry frame's id is read, this launch writes only frames >= carry: no element is both
            id = row >= first ? (int32_t)(b + (int64_t)rank[row + j - first]) : track_id[row + j];
        }
        track_id[e] = id;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *ntracks = b + (int64_t)rank[n - first];
}

// ====================================================================== the stream form's own kernels
// lidar_track_stream_f64 (DESIGN.md §3 "Continuous people tracking", §4.10): passes g = 1 .. max_gap + 1 in
// ascending order, one launch pair each; pass g associates frame u - g with frame u for every start frame
// u >= max(carry, g), over the rows still open.  Within a pass a frame is the end frame of one pair and the
// start frame of one pair at most, a pair reads succ of its end frame and prev of its start frame and
// link_open_kernel writes only those two, in a launch of its own after the pass's nearest launch: the pairs
// of a pass are independent under any schedule.

// The frames >= carry start empty; the id base is copied out of *ntracks, which id_kernel overwrites.
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
        double vx, vy;
        const int32_t i = mutual(people, fwd, bwd, cap, u, j, g, dtg, vx, vy);
        if (i < 0) continue;
        prev[e] = i;
        gap[e] = (int32_t)g;
        succ[(u - g) * cap + i] = 1;
        velocity[2 * e] = vx;
        velocity[2 * e + 1] = vy;
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

// ---------------------------------------------------------------------- the host path of both track entry points
// the argument checks the two share, under the entry point's name
int check_track(const char *fn, bool pointers, int64_t frames, int64_t cap, double dt, double gate)
{
    const std::string f(fn);
    if (int rc = check_frames(f, pointers, frames, cap)) return rc;
    REQUIRE(pos_finite(dt), f + ": dt must be positive and finite");
    REQUIRE(pos_finite(gate), f + ": gate must be positive and finite");
    return LIDAR_OK;
}

// A call's workspace: fwd and bwd over all frames (indexed by the start frame), the scan's buffers over the
// nnew rows of the frames >= carry, and the stream form's id base.
struct TrackWs {
    int32_t *fwd, *bwd;
    uint32_t *flag, *rank, *partial;
    int64_t *idbase;  // null without want_base
    int64_t nnew, nblk;
};
bool carve_track(lidar_handle *h, int64_t frames, int64_t cap, int64_t carry, bool want_base, TrackWs &w)
{
    const int64_t n = frames * cap;
    w.nnew = n - carry * cap;
    w.nblk = (w.nnew + 1 + kScanPer - 1) / kScanPer;
    lidar::Carver cv;
    const uint64_t o_fwd = cv.take<int32_t>(n), o_bwd = cv.take<int32_t>(n);
    const uint64_t o_flag = cv.take<uint32_t>(w.nnew), o_rank = cv.take<uint32_t>(w.nnew + 1);
    const uint64_t o_part = cv.take<uint32_t>(w.nblk), o_base = want_base ? cv.take<int64_t>(1) : 0;
    char *base = static_cast<char *>(lidar::workspace(h, cv.off));
    if (!base) return false;
    w.fwd = reinterpret_cast<int32_t *>(base + o_fwd), w.bwd = reinterpret_cast<int32_t *>(base + o_bwd);
    w.flag = reinterpret_cast<uint32_t *>(base + o_flag), w.rank = reinterpret_cast<uint32_t *>(base + o_rank);
    w.partial = reinterpret_cast<uint32_t *>(base + o_part);
    w.idbase = want_base ? reinterpret_cast<int64_t *>(base + o_base) : nullptr;
    return true;
}

// the flags of the frames >= carry -> their ranks (three launches) -> the ids
void launch_ids(const TrackWs &w, const int64_t *k, int64_t frames, int64_t cap, int64_t carry, const int32_t *prev,
                const int32_t *gap, int32_t *track_id, int64_t *ntracks, hipStream_t s)
{
    hipLaunchKernelGGL(scan_partial_kernel, dim3((unsigned)w.nblk), dim3(kT), 0, s, w.flag, w.nnew, w.partial);
    hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(kT), 0, s, w.partial, w.nblk);
    hipLaunchKernelGGL(scan_final_kernel, dim3((unsigned)w.nblk), dim3(kT), 0, s, w.flag, w.nnew, w.partial, w.rank);
    hipLaunchKernelGGL(id_kernel, dim3(flat_blocks(w.nnew)), dim3(kB), 0, s, k, frames, cap, carry, prev, gap, w.rank,
                       w.idbase, track_id, ntracks);
}

}  // namespace

// ====================================================================== C-ABI
LIDAR_EXPORT int lidar_track_people_f64(lidar_handle *h, const double *people, const int64_t *k, int64_t frames,
                                        int64_t cap, double dt, double gate, int32_t *prev, int32_t *track_id,
                                        double *velocity, int64_t *ntracks, void *stream)
{
    if (int rc = check_track("lidar_track_people_f64", h && people && k && prev && track_id && velocity && ntracks, frames,
                             cap, dt, gate))
        return rc;
    if (frames == 0) return LIDAR_OK;
    ON_DEVICE(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    TrackWs w;
    if (!carve_track(h, frames, cap, 0, false, w)) return LIDAR_ENOMEM;

    lidar::Span sp(h, "track_people", s);
    if (frames > 1)
        hipLaunchKernelGGL(nearest_kernel<Rows::All>, dim3((unsigned)((cap + kB - 1) / kB), (unsigned)(frames - 1), 2),
                           dim3(kB), 0, s, people, k, cap, 1, 1, gate * gate, nullptr, nullptr, w.fwd, w.bwd);
    hipLaunchKernelGGL(link_kernel, dim3(flat_blocks(frames * cap)), dim3(kB), 0, s, people, k, frames, cap, dt, w.fwd,
                       w.bwd, prev, velocity, w.flag);
    launch_ids(w, k, frames, cap, 0, prev, nullptr, track_id, ntracks, s);
    LAUNCH_CHECK();
    return LIDAR_OK;
}

LIDAR_EXPORT int lidar_track_stream_f64(lidar_handle *h, const double *people, const int64_t *k, int64_t frames,
                                        int64_t cap, int64_t carry, double dt, double gate, int32_t max_gap,
                                        int32_t *prev, int32_t *gap, uint8_t *succ, double *velocity,
                                        int32_t *track_id, int64_t *ntracks, void *stream)
{
    if (int rc = check_track("lidar_track_stream_f64",
                             h && people && k && prev && gap && succ && velocity && track_id && ntracks, frames, cap, dt,
                             gate))
        return rc;
    REQUIRE(max_gap >= 0 && max_gap + 1 <= kMaxGap, "lidar_track_stream_f64: max_gap must be in 0 .. 7");
    REQUIRE(carry >= 0 && carry <= std::min<int64_t>(max_gap + 1, frames),
            "lidar_track_stream_f64: carry must be in 0 .. min(max_gap + 1, frames)");
    if (frames == carry) return LIDAR_OK;  // no frame to link (frames == 0 among them): nothing is written
    ON_DEVICE(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t n = frames * cap, first = carry * cap;
    TrackWs w;
    if (!carve_track(h, frames, cap, carry, true, w)) return LIDAR_ENOMEM;

    static const char *const kPass[] = {"track_stream_pass1", "track_stream_pass2", "track_stream_pass3",
                                        "track_stream_pass4", "track_stream_pass5", "track_stream_pass6",
                                        "track_stream_pass7", "track_stream_pass8"};
    static_assert(sizeof(kPass) / sizeof(kPass[0]) == kMaxGap, "a span name per frame distance of a link");
    {
        lidar::Span sp(h, "track_stream_init", s);
        hipLaunchKernelGGL(init_stream_kernel, dim3(flat_blocks(w.nnew)), dim3(kB), 0, s, first, n, prev, gap, succ,
                           velocity, ntracks, w.idbase);
    }
    for (int64_t g = 1; g <= max_gap + 1; ++g) {  // ascending: a pass sees what the passes before it linked
        const int64_t u0 = std::max(carry, g), pairs = frames - u0;
        if (pairs <= 0) break;
        const double gg = gate * (double)g, dtg = dt * (double)g;  // one fp64 product each
        lidar::Span sp(h, kPass[g - 1], s);
#ifdef LIDAR_TRACK_GAP_MASKED  // a measuring build: the masked form in every pass
        const auto nearest = nearest_kernel<Rows::Masked>;
#else
        const auto nearest = g >= 2 ? nearest_kernel<Rows::Compact> : nearest_kernel<Rows::Masked>;
#endif
        hipLaunchKernelGGL(nearest, dim3((unsigned)((cap + kB - 1) / kB), (unsigned)pairs, 2), dim3(kB), 0, s, people, k,
                           cap, u0, g, gg * gg, prev, succ, w.fwd, w.bwd);
        hipLaunchKernelGGL(link_open_kernel, dim3(flat_blocks(pairs * cap)), dim3(kB), 0, s, people, k, frames, cap, u0, g,
                           dtg, w.fwd, w.bwd, prev, gap, succ, velocity);
    }
    {
        lidar::Span sp(h, "track_stream_ids", s);
        hipLaunchKernelGGL(flag_stream_kernel, dim3(flat_blocks(w.nnew)), dim3(kB), 0, s, k, first, n, cap, prev, w.flag);
        launch_ids(w, k, frames, cap, carry, prev, gap, track_id, ntracks, s);
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
    if (int rc = check_frames(f, h && people && k && prev && velocity && count && vsum, frames, cap)) return rc;
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
