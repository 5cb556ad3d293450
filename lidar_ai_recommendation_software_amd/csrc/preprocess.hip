// preprocess.hip — the reference density path's preprocess (Tier R) on gfx950, bit-exact with the CPU path.
//
// Replaces:
//   preprocess_kernel  utils/data_processing.py:143-195 — height colours, 3-sigma filter
//                      (numpy sequential axis-0 sums), 30th-percentile ground split
//                      (radix select + numpy's _lerp), ground plane (TSQR + Jacobi SVD with gelsd's
//                      rank rule; gelsd is not bit-reproducible, see plane_solve), StandardScaler
//                      (sklearn's corrected two-pass variance, near-constant mask), eps heuristic.
// Sequential sums are one lane each (numpy's axis-0 order is sequential: reproducing it
// bit for bit leaves no freedom); everything else is wave/workgroup parallel.
#include <cmath>

#include "tier_r.hpp"

namespace {

using namespace lidar::tier_r;

// deterministic block sum (row 2 + SLOT of s.d) — used only where the reference itself is not
// bit-reproducible (the gelsd plane fit).  Relies on block_reduce's fixed order (the xor butterfly
// from 32 down to 1 within a wave, then the waves' totals added in wave order): fp64 addition is not
// associative, so another order is another result
template <int SLOT>
__device__ __forceinline__ double block_sum(BlockScratch &s, double v)
{
    return block_reduce<2 + SLOT>(s, v, [](double a, double b) { return dadd(a, b); });
}
// exclusive scan of a 0/1 flag over the workgroup; returns the position, *total set
__device__ int block_flag_scan(BlockScratch &s, bool f, int *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t m = __ballot(f);
    const int inwave = __popcll(m & ((1ull << lane) - 1));
    __syncthreads();
    if (lane == 0) s.i[wave] = __popcll(m);
    __syncthreads();
    int base = 0, tot = 0;
    for (int w = 0; w < kW; ++w) {
        int c = s.i[w];
        base += w < wave ? c : 0;
        tot += c;
    }
    *total = tot;
    return base + inwave;
}

// ---- index-order fp64 chains with the rows streamed through LDS
// numpy's axis-0 reductions of a row-major (n, 3) array are sequential per column, so the
// result depends on every rounding in index order.  block_staged_rows streams the rows through LDS
// in chunks; two ways to run a chain on a staged chunk: seq_chain_rows, the dependent adds themselves
// (one lane per column), for sums of signed values (coordinates, deviations: their accumulator
// wanders across binades near zero), and sum_chain_rows below, a parallel emulation (one wave per
// column), for sums of squares.
// rows per staged chunk: 3 072 (147 KiB double-buffered; the kernel is one 1 024-thread workgroup per CU
// by its registers anyway): preprocess 2.70 ms per 32 frames vs 2.79 at 2 048 and 2.98 at 1 024
// (round-3 A/B): fewer chunk barriers, each waiting on the next chunk's staging
constexpr int kSeqRows = 3072;
// rows whose LDS reads are issued before their dependent adds (32 measured equal, 64 slower: the
// chain is bound by the dependent fp64 adds, not by the LDS reads)
constexpr int kSeqBatch = 16;
struct SeqStage {
    double v[2][kSeqRows * 3];
};

// rows [0, n) of x (row-major (n, 3)) through LDS in kSeqRows-row chunks, double buffered: the waves
// 0 .. WORKERS - 1 call work(chunk, rows) on chunk k (every thread of them; they never wait on global
// loads) while the waves from WORKERS up stage chunk k + 1.  One barrier per chunk; ends with a barrier.
template <int WORKERS, class Work>
__device__ __forceinline__ void block_staged_rows(const double *x, int64_t n, SeqStage &st, Work work)
{
    constexpr int kWorkT = 64 * WORKERS;  // the first staging thread
    const int tid = threadIdx.x;
    const int64_t nch = (n + kSeqRows - 1) / kSeqRows;
    auto rows_of = [&](int64_t k) { return n - k * kSeqRows < kSeqRows ? n - k * kSeqRows : kSeqRows; };
    auto stage = [&](int64_t k) {
        if (tid < kWorkT || k >= nch) return;
        const int64_t cnt = rows_of(k) * 3;
        double *d = st.v[k & 1];
        const double *src = x + 3 * k * kSeqRows;
        for (int64_t e = tid - kWorkT; e < cnt; e += kT - kWorkT) d[e] = src[e];
    };
    // every earlier memory access finished before the first chunk: the workspace pointers (FrameMap::ws goes
    // through an integer) are flat addresses to the compiler, a flat access counts on the LDS counter too, and
    // while one may be outstanding (the compaction's and the transform's stores) the compiler makes every LDS
    // wait of the chains a full one instead of counting a batch's 16 reads down: preprocess 2.64 vs 2.45 ms
    // per 32 frames
    __builtin_amdgcn_s_waitcnt(0);
    stage(0);
    __syncthreads();
    for (int64_t k = 0; k < nch; ++k) {
        stage(k + 1);
        if (tid < kWorkT) work(st.v[k & 1], (int)rows_of(k));
        __syncthreads();
    }
}

// one staged chunk's rows of an index-order chain a <- step(a, row) (one lane): b = the chunk's column
template <class Step>
__device__ __forceinline__ void seq_chain_rows(const double *b, int rows, Step step, double &a)
{
    // reads of a 16-row batch first, then its dependent adds (an explicit two-batch
    // software pipeline measured 2.4x slower: 7.6 vs 3.2 ms per 65k frame)
    int i = 0;
    for (; i + kSeqBatch <= rows; i += kSeqBatch) {
        double v[kSeqBatch];
#pragma unroll
        for (int u = 0; u < kSeqBatch; ++u) v[u] = b[3 * (i + u)];
#pragma unroll
        for (int u = 0; u < kSeqBatch; ++u) a = step(a, v[u]);
    }
    for (; i < rows; ++i) a = step(a, b[3 * i]);
}

// the index-order chains of the three columns, a <- step(a, x[i][c]) from a = +0.0, on lanes c = 0..2
// of wave 0 (waves 1..15 stage): thread c returns column c's result, the others 0
template <class Step>
__device__ __forceinline__ double block_seq_chain(const double *x, int64_t n, SeqStage &st, Step step)
{
    double a = 0.0;
    block_staged_rows<1>(x, n, st, [&](const double *chunk, int rows) {
        if (threadIdx.x < 3) seq_chain_rows(chunk + threadIdx.x, rows, step, a);
    });
    return a;
}

// ---- the same index-order chains, emulated in parallel, bit for bit
// A chain a <- fl(a + inc_i) (i = 0..n-1, a = +0.0 first) is reproduced without n dependent adds.
// While a stays in one binade [2^e, 2^(e+1)) (or its negative), with u = 2^(e-52), every partial
// result is a multiple of u, and fl(a + v) = a + u * rint(v / u) as long as the exact sum stays in
// that binade and v / u is not an exact tie (the tie goes to the even neighbour, which depends on a).
// So a wavefront takes 256 rows at a time (4 consecutive rows per lane): every row's increment is
// scaled to k = rint(inc * 2^(53-E)) (a = m 2^E, 0.5 <= |m| < 1: exact power-of-two scaling), a
// lane-local prefix plus a DPP scan of the lane totals (integers of at most 2^44 each, so every
// partial sum is exact in fp64) gives A_j = A + P_j, and the rows up to the first one whose A_j
// leaves (2^52, 2^53) in magnitude, or whose increment is a tie, huge (> 2^44 u), inf or NaN, are
// accepted at once: a = A_j * u.  The violating row is added with one
// dadd, exactly as the sequential chain does, and the scan restarts after it.  Near zero (a = 0,
// subnormal, non-finite) the rows go one dadd at a time; after a scan accepts fewer than
// kChainMinRun rows (an accumulator hovering near a binade edge, as a centred column's sum does),
// the next kChainSeqRun rows go one dadd at a time before the next scan.  Every accepted row has the
// value the dependent add would have produced, so the result is the sequential one bit for bit
// (tests/test_gpu_tier_r.py: the reference's goldens, byte-equal).
constexpr int kChainMinRun = 16, kChainSeqRun = 32, kChainRowsPerLane = 4;

// wave-uniform fp64 helpers (scalar registers: the chain's control flow stays scalar); readlane_d: tier_r.hpp
__device__ __forceinline__ double uniform_d(double v)
{
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)u);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(u >> 32));
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}
// DPP move of an fp64 value (both halves), 0 where the row / bank masks or the row bounds leave
// a lane without a source
template <int CTRL, int RM, bool BC>
__device__ __forceinline__ double dpp_d(double v)
{
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)u, CTRL, RM, 0xf, BC);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(u >> 32), CTRL, RM, 0xf, BC);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}
// inclusive wave scan of integer-valued doubles whose partial sums stay below 2^53 (exact):
// row_shr 1 / 2 / 4 / 8 within each 16-lane row, then row_bcast 15 (rows 1, 3) and 31 (rows 2, 3)
__device__ __forceinline__ double wave_scan_exact_d(double P)
{
    P = dadd(P, dpp_d<0x111, 0xf, true>(P));
    P = dadd(P, dpp_d<0x112, 0xf, true>(P));
    P = dadd(P, dpp_d<0x114, 0xf, true>(P));
    P = dadd(P, dpp_d<0x118, 0xf, true>(P));
    P = dadd(P, dpp_d<0x142, 0xa, false>(P));
    P = dadd(P, dpp_d<0x143, 0xc, false>(P));
    return P;
}

// one staged chunk's rows of the emulated chain a <- fl(a + inc(row)) (one wavefront; b = the chunk's
// column; a, from +0.0, and forced, from 0, carry over from chunk to chunk)
template <class Inc>
__device__ __forceinline__ void sum_chain_rows(const double *b, int rows, Inc inc, double &a, int &forced)
{
    constexpr double kTwo52 = 4503599627370496.0, kTwo53 = 9007199254740992.0, kTwo44 = 17592186044416.0;
    const int lane = threadIdx.x & 63;
    int i = 0;
    while (i < rows) {
        a = uniform_d(a);
        i = __builtin_amdgcn_readfirstlane(i);
        forced = __builtin_amdgcn_readfirstlane(forced);
        if (forced > 0 || !(fabs(a) >= 2.2250738585072014e-308) || !(fabs(a) < INFINITY)) {
            // one dadd per row (wave-uniform): near zero, non-finite, or a forced run
            const int run = forced > 0 ? (forced < rows - i ? forced : rows - i) : 1;
            int t = 0;
            for (; t + 8 <= run; t += 8) {
                double v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = inc(b[3 * (i + t + u)]);
#pragma unroll
                for (int u = 0; u < 8; ++u) a = dadd(a, v[u]);
            }
            for (; t < run; ++t) a = dadd(a, inc(b[3 * (i + t)]));
            i += run;
            forced = forced > run ? forced - run : 0;
            continue;
        }
        int e2;
        (void)frexp(a, &e2);  // a = m 2^e2, 0.5 <= |m| < 1
        const int sh = __builtin_amdgcn_readfirstlane(53 - e2);
        const double A = ldexp(a, sh);  // |A| in [2^52, 2^53), exact
        // lane l takes rows i + 4l .. i + 4l + 3: a window of 256 rows per scan
        double v[kChainRowsPerLane], L[kChainRowsPerLane], raw[kChainRowsPerLane];
        bool bad[kChainRowsPerLane], valid[kChainRowsPerLane];
        double run = 0.0;  // the lane's own prefix of its rounded increments
        // the window's LDS reads all issued first and unconditionally (rows past the end read row i, and
        // their values are dropped below): one wait, not one branch and wait per row
#pragma unroll
        for (int r = 0; r < kChainRowsPerLane; ++r) {
            const int j = i + kChainRowsPerLane * lane + r;
            valid[r] = j < rows;
            raw[r] = b[3 * (valid[r] ? j : i)];
        }
#pragma unroll
        for (int r = 0; r < kChainRowsPerLane; ++r) {
            v[r] = valid[r] ? inc(raw[r]) : 0.0;
            const double xs = ldexp(v[r], sh);
            double kq = rint(xs);
            bad[r] = valid[r] && (!(fabs(kq) <= kTwo44) || dsub(xs, floor(xs)) == 0.5);
            if (!valid[r] || bad[r]) kq = 0.0;
            run = dadd(run, kq);  // integers below 2^46: exact
            L[r] = run;
        }
        // exclusive prefix of the lane totals (<= 256 increments of <= 2^44: below 2^52, exact)
        const double E = dsub(wave_scan_exact_d(run), run);
        int first = kChainRowsPerLane;  // the lane's first violating row
#pragma unroll
        for (int r = kChainRowsPerLane - 1; r >= 0; --r) {
            const double Aj = dadd(A, dadd(E, L[r]));  // exact below 2^53; >= 2^53 stays
            const double sAj = a > 0.0 ? Aj : -Aj;
            if (valid[r] && (bad[r] || !(sAj > kTwo52 && sAj < kTwo53))) first = r;
        }
        const uint64_t vm = __ballot(first < kChainRowsPerLane);
        const int nv = rows - i < 64 * kChainRowsPerLane ? rows - i : 64 * kChainRowsPerLane;
        // the accumulator after the rows before window row t (t >= 1), and row t's increment
        // (the row choices read every candidate out of lane ln and select among the scalars: a select of
        // per-row registers with a runtime row made the compiler keep L[] and v[] in scratch memory)
        auto pick_at = [&](const double (&arr)[kChainRowsPerLane], int ln, int r) {
            double p = readlane_d(arr[0], ln);
#pragma unroll
            for (int u = 1; u < kChainRowsPerLane; ++u) {
                const double x = readlane_d(arr[u], ln);
                p = r == u ? x : p;
            }
            return p;
        };
        auto after = [&](int t) {
            const int ln = (t - 1) / kChainRowsPerLane, r = (t - 1) % kChainRowsPerLane;
            return ldexp(dadd(A, dadd(readlane_d(E, ln), pick_at(L, ln, r))), -sh);
        };
        if (vm == 0) {
            a = after(nv);
            i += nv;
        } else {
            const int ln = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)vm) - 1);
            const int rv = __builtin_amdgcn_readlane(first, ln);
            const int j0 = kChainRowsPerLane * ln + rv;
            if (j0 > 0) a = after(j0);
            a = dadd(a, pick_at(v, ln, rv));  // the violating row: the sequential add itself
            i += j0 + 1;
            if (j0 < kChainMinRun) forced = kChainSeqRun;
        }
    }
}

struct SqDev {  // the increment of every emulated chain here: the squared deviation from m
    double m;
    __device__ double operator()(double v) const
    {
        const double d = dsub(v, m);
        return dmul(d, d);
    }
};

// what the phases of preprocess_kernel hand to the whole workgroup through LDS: written by the few
// threads that computed it, read by all after a barrier
struct PreShared {
    double mean[3], std[3];      // col_moments
    uint64_t sel_prefix[2];      // select_z_threshold: the key digits chosen so far for the two order statistics,
    int64_t sel_rank[2];         // and each one's rank among the keys that share them
    double smean[3], sscale[3];  // scaler_fit
};

// sh.mean, sh.std = np.mean / np.std over axis 0 of the rows [0, n) of x: the mean by the index-order chain
// (lanes 0..2 of wave 0), then the population standard deviation from the emulated chain of squared
// deviations (waves 0..2, column = wave; waves 3..15 stage).  Ends with a barrier.
__device__ __forceinline__ void col_moments(const double *x, int64_t n, SeqStage &st, BlockScratch &s, PreShared &sh)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double sum = block_seq_chain(x, n, st, [](double a, double v) { return dadd(a, v); });
    if (tid < 3) sh.mean[tid] = ddiv(sum, (double)n);
    __syncthreads();
    const double mw = sh.mean[wave % 3];  // the mean of this wave's chain column
    double a = 0.0;
    int forced = 0;
    block_staged_rows<3>(x, n, st, [&](const double *chunk, int rows) {
        sum_chain_rows(chunk + wave, rows, SqDev{mw}, a, forced);
    });
    if (wave < 3 && lane == 0) s.chain[wave] = a;
    __syncthreads();
    if (tid < 3) sh.std[tid] = __dsqrt_rn(ddiv(s.chain[tid], (double)n));
    __syncthreads();
}

// ---- ground plane: numpy.linalg.lstsq(A, z, rcond=None), A = [x y 1] (data_processing.py:171-177)
// LAPACK gelsd returns the minimum-norm least-squares solution of A's SVD truncated at
// rcond = eps * max(M, 3): singular values s_i <= rcond * s_1 count as zero.  That decision is what
// makes a frame far from the origin (|x| ~ 1e12 with a unit spread) or at tiny magnitudes (1e-140)
// rank-deficient, and the truncated solution differs there from the plain least-squares plane.
// The device reproduces the decision and the solution: (1) a Givens QR of the centred rows
// w = [(x - mx) sx, (y - my) sx, 1, (z - mz) sz] (sx, sz powers of two: no overflow, exact
// unscaling), per thread over its rows, then merged as a fixed tree (TSQR); (2) since
// [x y 1] = [x - mx, y - my, 1] T with T = [[1,0,0],[0,1,0],[mx,my,1]], A = Q (R3 T) and Q^T z =
// R[:3,3] + mz R[:3,2], so A's singular values and the solution are those of the 3x3 system
// B = R3 T, c; (3) one-sided Jacobi SVD of B (high relative accuracy), the same rank rule, and
// x = sum over the kept i of v_i (u_i . c) / s_i.  The centring perturbs A far less than gelsd's own
// backward error, so the result agrees with gelsd to ~eps * s_1 / s_rank relative (both are
// backward-stable solvers of the same truncated problem); tests/test_gpu_tier_r.py states that
// tolerance.  Row 3 of R (the residual) is not needed and not formed.
__device__ __forceinline__ constexpr int plane_ro(int k) { return k == 0 ? 0 : k == 1 ? 4 : k == 2 ? 7 : 9; }
template <int K0>
__device__ __forceinline__ void plane_row(double (&r)[10], double (&w)[4])
{
#pragma unroll
    for (int k = K0; k < 3; ++k) {
        const double a = r[plane_ro(k)], b = w[k];
        const double h = __dsqrt_rn(dadd(dmul(a, a), dmul(b, b)));
        const bool skip = b == 0.0 || h == 0.0;  // h == 0: b's square underflowed (negligible)
        const double inv = skip ? 0.0 : ddiv(1.0, h);
        const double c = skip ? 1.0 : dmul(a, inv), s = skip ? 0.0 : dmul(b, inv);
        r[plane_ro(k)] = skip ? a : h;
#pragma unroll
        for (int j = k + 1; j < 4; ++j) {
            const double t = r[plane_ro(k) + j - k];
            r[plane_ro(k) + j - k] = dadd(dmul(c, t), dmul(s, w[j]));
            w[j] = dsub(dmul(c, w[j]), dmul(s, t));
        }
    }
}
__device__ __forceinline__ void plane_merge(double (&r)[10], const double (&p)[10])
{
    double w0[4] = {p[0], p[1], p[2], p[3]};
    plane_row<0>(r, w0);
    double w1[4] = {0.0, p[4], p[5], p[6]};
    plane_row<1>(r, w1);
    double w2[4] = {0.0, 0.0, p[7], p[8]};
    plane_row<2>(r, w2);
}
// the truncated minimum-norm solution from the merged R (one thread); returns the rank
__device__ int plane_solve(const double (&r)[10], double sx_inv_exp, double sz_inv_exp, double mx, double my,
                           double mz, double m_rows, double (&x)[3])
{
    auto R = [&](int i, int j) { return j < i ? 0.0 : r[plane_ro(i) + j - i]; };
    const int ex = (int)sx_inv_exp, ez = (int)sz_inv_exp;
    double B[3][3], c[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        B[i][0] = dadd(ldexp(R(i, 0), ex), dmul(R(i, 2), mx));
        B[i][1] = dadd(ldexp(R(i, 1), ex), dmul(R(i, 2), my));
        B[i][2] = R(i, 2);
        c[i] = dadd(ldexp(R(i, 3), ez), dmul(mz, R(i, 2)));
    }
    double bm = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) bm = fmax(bm, fabs(B[i][j]));
    int eb = 0;
    if (bm > 0.0 && bm < INFINITY) (void)frexp(bm, &eb);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        c[i] = ldexp(c[i], -eb);
#pragma unroll
        for (int j = 0; j < 3; ++j) B[i][j] = ldexp(B[i][j], -eb);
    }
    double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    constexpr double kEps = 2.220446049250313e-16;  // numpy.finfo(float64).eps
    for (int sweep = 0; sweep < 40; ++sweep) {
        bool rot = false;
#pragma unroll
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                al = dadd(al, dmul(B[i][p], B[i][p]));
                be = dadd(be, dmul(B[i][q], B[i][q]));
                ga = dadd(ga, dmul(B[i][p], B[i][q]));
            }
            if (ga == 0.0 || fabs(ga) <= dmul(kEps, dmul(__dsqrt_rn(al), __dsqrt_rn(be)))) continue;
            rot = true;
            const double zeta = ddiv(dsub(be, al), dmul(2.0, ga));
            const double t = fabs(zeta) > 1e150 ? ddiv(0.5, zeta)
                                                : ddiv(copysign(1.0, zeta),
                                                       dadd(fabs(zeta), __dsqrt_rn(dadd(1.0, dmul(zeta, zeta)))));
            const double cs = ddiv(1.0, __dsqrt_rn(dadd(1.0, dmul(t, t)))), sn = dmul(cs, t);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double bp = B[i][p], bq = B[i][q];
                B[i][p] = dsub(dmul(cs, bp), dmul(sn, bq));
                B[i][q] = dadd(dmul(sn, bp), dmul(cs, bq));
                const double vp = V[i][p], vq = V[i][q];
                V[i][p] = dsub(dmul(cs, vp), dmul(sn, vq));
                V[i][q] = dadd(dmul(sn, vp), dmul(cs, vq));
            }
        }
        if (!rot) break;
    }
    double s2[3], sv[3], smax = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        s2[k] = dadd(dadd(dmul(B[0][k], B[0][k]), dmul(B[1][k], B[1][k])), dmul(B[2][k], B[2][k]));
        sv[k] = __dsqrt_rn(s2[k]);
        smax = fmax(smax, sv[k]);
    }
    const double tol = dmul(dmul(kEps, fmax(m_rows, 3.0)), smax);  // numpy: rcond = eps * max(M, N)
    int rank = 0;
    x[0] = x[1] = x[2] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const bool keep = sv[k] > tol;
        rank += keep ? 1 : 0;
        const double coef = keep ? ddiv(dadd(dadd(dmul(B[0][k], c[0]), dmul(B[1][k], c[1])), dmul(B[2][k], c[2])), s2[k])
                                 : 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) x[i] = keep ? dadd(x[i], dmul(V[i][k], coef)) : x[i];
    }
    return rank;
}

__device__ __forceinline__ uint64_t ordkey(double v)
{
    uint64_t u = (uint64_t)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double unordkey(uint64_t k)
{
    uint64_t u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}

// ------------------------------------------------------------------ preprocess: the phases, in kernel order
// A: the z range over ALL points that the height colours normalise by (data_processing.py:143-147)
__device__ __forceinline__ void colour_range(BlockScratch &s, const double *xyz, int64_t n, double &zmin, double &denom)
{
    double lo = INFINITY, hi = -INFINITY;
    for (int64_t i = threadIdx.x; i < n; i += kT) {
        const double z = xyz[3 * i + 2];
        lo = fmin(lo, z);
        hi = fmax(hi, z);
    }
    zmin = block_min(s, lo);
    const double zmax = block_max(s, hi);
    denom = dadd(dsub(zmax, zmin), 1e-10);
}

// C: strict 3-sigma mask, order-preserving compaction of the inliers with their colours and normals
// (:155-161); returns the inlier count
__device__ __forceinline__ int64_t compact_inliers(BlockScratch &s, const double *xyz, int64_t n,
                                                   const double (&mean)[3], const double (&thr)[3], double zmin,
                                                   double denom, uint8_t *mask, double *comp, double *colors,
                                                   double *normals)
{
    int64_t nin = 0;
    for (int64_t b0 = 0; b0 < n; b0 += kT) {
        const int64_t i = b0 + threadIdx.x;
        bool f = false;
        double p[3] = {0, 0, 0};
        if (i < n) {
            f = true;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                p[c] = xyz[3 * i + c];
                f = f && (fabs(dsub(p[c], mean[c])) < thr[c]);
            }
            mask[i] = f ? 1 : 0;
        }
        int tot;
        const int pos = block_flag_scan(s, f, &tot);
        if (f) {
            const int64_t o = nin + pos;
#pragma unroll
            for (int c = 0; c < 3; ++c) comp[3 * o + c] = p[c];
            // colours of the inliers (:143-147, masked at :157), normals (:160-161)
            const double nh = ddiv(dsub(p[2], zmin), denom);
            colors[3 * o] = nh;
            colors[3 * o + 1] = dmul(0.5, dsub(1.0, nh));
            colors[3 * o + 2] = 0.5;
            normals[3 * o] = 0.0;
            normals[3 * o + 1] = 0.0;
            normals[3 * o + 2] = 1.0;
        }
        nin += tot;
    }
    return nin;
}

// D: z threshold = np.percentile(z, 30) 'linear' (:164) over the z column of the nin compacted points: a radix
// select of the two order statistics, then numpy's _lerp
__device__ __forceinline__ double select_z_threshold(BlockScratch &s, SeqStage &st, PreShared &sh, const double *comp,
                                                     int64_t nin)
{
    const int tid = threadIdx.x, wave = tid >> 6;
    const double q = ddiv(30.0, 100.0);
    const double v = dmul((double)(nin - 1), q);
    const double prev = floor(v);
    int64_t klo, khi;
    if (v >= (double)(nin - 1)) {
        klo = khi = nin - 1;
    } else {
        klo = (int64_t)prev;
        khi = klo + 1;
    }
    uint64_t pre[2] = {0, 0};
    int64_t kk[2] = {klo, khi};
    // per-wave histograms (16 waves x 2 targets x 256 bins) in the chain staging memory, idle
    // here: the early digits of a coordinate column share a few values, and one shared
    // histogram serialised every wave's atomics on them
    unsigned *wh = reinterpret_cast<unsigned *>(&st.v[0][0]);
    static_assert(sizeof(SeqStage) >= kW * 2 * 256 * sizeof(unsigned), "per-wave histograms");
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        for (int i = tid; i < kW * 2 * 256; i += kT) wh[i] = 0;
        __syncthreads();
        unsigned *mine = wh + wave * 2 * 256;
        for (int64_t i = tid; i < nin; i += kT) {
            const uint64_t key = ordkey(comp[3 * i + 2]);
            const uint64_t hk = pass == 0 ? 0 : key >> (shift + 8);
            const unsigned dig = (unsigned)(key >> shift) & 255u;
            if (hk == pre[0]) atomicAdd(&mine[dig], 1u);
            if (hk == pre[1]) atomicAdd(&mine[256 + dig], 1u);
        }
        __syncthreads();
        // thread r * 256 + d holds bin d of target r (waves 4r .. 4r + 3) and its running count: the
        // bins of one target sum to at most nin < 2^31, so the counts fit 32 bits.  Selected: the
        // first bin whose running count passes kk[r] (kk[r] is below the target's total: exactly one)
        const int r = (tid >> 8) & 1;
        unsigned h = 0;
        if (tid < 512)
            for (int w = 0; w < kW; ++w) h += wh[w * 512 + tid];
        const int64_t cum = block_excl_scan_u32(h, s.i, wave & ~3), kr = r ? kk[1] : kk[0];
        if (tid < 512 && cum <= kr && kr < cum + h) {
            sh.sel_prefix[r] = ((r ? pre[1] : pre[0]) << 8) | (uint64_t)(tid & 255);
            sh.sel_rank[r] = kr - cum;
        }
        __syncthreads();
        for (int r = 0; r < 2; ++r) {
            pre[r] = sh.sel_prefix[r];
            kk[r] = sh.sel_rank[r];
        }
        __syncthreads();
    }
    const double za = unordkey(pre[0]), zb = unordkey(pre[1]);
    const double t = dsub(v, prev);
    const double diff = dsub(zb, za);
    double zt = dadd(za, dmul(diff, t));
    if (t >= 0.5) zt = dsub(zb, dmul(diff, dsub(1.0, t)));
    return zt;
}

// E: ground count, dimensions and plane of the nin compacted points (:165-183), into the frame's scalars
__device__ __forceinline__ void ground_plane(BlockScratch &s, SeqStage &st, const double *comp, int64_t nin, double zt,
                                             double *S)
{
    const int tid = threadIdx.x;
    double cnt = 0, sx = 0, sy = 0, sz = 0, imin[3] = {INFINITY, INFINITY, INFINITY},
           imax[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = tid; i < nin; i += kT) {
        const double px = comp[3 * i], py = comp[3 * i + 1], pz = comp[3 * i + 2];
        imin[0] = fmin(imin[0], px);
        imin[1] = fmin(imin[1], py);
        imin[2] = fmin(imin[2], pz);
        imax[0] = fmax(imax[0], px);
        imax[1] = fmax(imax[1], py);
        imax[2] = fmax(imax[2], pz);
        if (pz <= zt) {
            cnt += 1.0;
            sx = dadd(sx, px);
            sy = dadd(sy, py);
            sz = dadd(sz, pz);
        }
    }
    double dmin[3], dmax[3];
    for (int c = 0; c < 3; ++c) {
        dmin[c] = block_min(s, imin[c]);
        dmax[c] = block_max(s, imax[c]);
    }
    const double ng = block_sum<0>(s, cnt);
    const int64_t nground = (int64_t)ng;
    double plane[4] = {0.0, 0.0, 1.0, -dmin[2]};
    double pkind = 1.0;
    if (nground > 10) {
        const double mx = block_sum<1>(s, sx) / ng, my = block_sum<2>(s, sy) / ng, mz = block_sum<3>(s, sz) / ng;
        // TSQR of the centred, power-of-two-scaled rows (see plane_solve): |w| < 1 per entry
        int exy = 0, ezz = 0;
        const double extxy = fmax(dmax[0] - dmin[0], dmax[1] - dmin[1]), extz = dmax[2] - dmin[2];
        if (extxy > 0.0 && extxy < INFINITY) (void)frexp(extxy, &exy);
        if (extz > 0.0 && extz < INFINITY) (void)frexp(extz, &ezz);
        double r[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int64_t i = tid; i < nin; i += kT) {
            const double pz = comp[3 * i + 2];
            if (pz <= zt) {
                double w[4] = {ldexp(dsub(comp[3 * i], mx), -exy), ldexp(dsub(comp[3 * i + 1], my), -exy), 1.0,
                               ldexp(dsub(pz, mz), -ezz)};
                plane_row<0>(r, w);
            }
        }
        for (int m = 1; m < 64; m <<= 1) {  // fixed butterfly: lane 0 ends with the wave's R
            double p[10];
#pragma unroll
            for (int k = 0; k < 10; ++k) p[k] = __shfl_xor(r[k], m, 64);
            plane_merge(r, p);
        }
        __syncthreads();  // st is free between the chains; its first 160 doubles hold the waves' R
        if ((tid & 63) == 0)
#pragma unroll
            for (int k = 0; k < 10; ++k) st.v[0][(tid >> 6) * 10 + k] = r[k];
        __syncthreads();
        if (tid < 64) {
#pragma unroll
            for (int k = 0; k < 10; ++k) r[k] = tid < kW ? st.v[0][tid * 10 + k] : 0.0;
            for (int m = 1; m < kW; m <<= 1) {
                double p[10];
#pragma unroll
                for (int k = 0; k < 10; ++k) p[k] = __shfl_xor(r[k], m, 64);
                plane_merge(r, p);
            }
            if (tid == 0) {
                double x[3];
                const int rank = plane_solve(r, (double)exy, (double)ezz, mx, my, mz, ng, x);
                plane[0] = x[0];
                plane[1] = x[1];
                plane[2] = -1.0;
                plane[3] = x[2];
                pkind = rank == 3 ? 0.0 : 2.0;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        S[S_ZT] = zt;
        S[S_NGROUND] = ng;
        for (int c = 0; c < 3; ++c) {
            S[S_DIMS + 2 * c] = dmin[c];
            S[S_DIMS + 2 * c + 1] = dmax[c];
        }
        for (int c = 0; c < 4; ++c) S[S_PLANE + c] = plane[c];
        S[S_PLANE_KIND] = pkind;
    }
}

// F: order-preserving compaction of the non-ground points (:186) into sc, their inlier indices into ng_pos;
// returns their count
__device__ __forceinline__ int64_t compact_non_ground(BlockScratch &s, const double *comp, int64_t nin, double zt,
                                                      double *sc, int32_t *ng_pos)
{
    int64_t nng = 0;
    for (int64_t b0 = 0; b0 < nin; b0 += kT) {
        const int64_t i = b0 + threadIdx.x;
        const bool f = i < nin && !(comp[3 * i + 2] <= zt);
        int tot;
        const int pos = block_flag_scan(s, f, &tot);
        if (f) {
            for (int c = 0; c < 3; ++c) sc[3 * (nng + pos) + c] = comp[3 * i + c];
            ng_pos[nng + pos] = (int32_t)i;
        }
        nng += tot;
    }
    return nng;
}

// G: sh.smean, sh.sscale = the StandardScaler fit (sklearn _incremental_mean_and_var, zero prior) (:190-191).
// Ends with a barrier.
__device__ __forceinline__ void scaler_fit(const double *sc, int64_t nng, SeqStage &st, BlockScratch &s, PreShared &sh)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double nn = (double)nng;
    const double sum = block_seq_chain(sc, nng, st, [](double a, double v) { return dadd(a, v); });
    if (tid < 3) sh.smean[tid] = ddiv(sum, nn);
    __syncthreads();
    // the second pass, both kinds of chain at once over the same staged rows (one pass instead of two, or
    // instead of a step carrying both): the sum of deviations stays sequential (lanes 0..2 of wave 0), the sum
    // of their squares is emulated beside it (waves 1..3, column = wave - 1); waves 4..15 stage
    const double T = tid < 3 ? sh.smean[tid] : 0.0;
    const int cw = (wave + 2) % 3;  // waves 1..3: column wave - 1
    const double Tw = sh.smean[cw];
    double corr = 0.0, a = 0.0;
    int forced = 0;
    block_staged_rows<4>(sc, nng, st, [&](const double *chunk, int rows) {
        if (wave > 0) sum_chain_rows(chunk + cw, rows, SqDev{Tw}, a, forced);
        else if (tid < 3) seq_chain_rows(chunk + tid, rows, [T](double cr, double v) { return dadd(cr, dsub(v, T)); }, corr);
    });
    if (wave >= 1 && wave <= 3 && lane == 0) s.chain[cw] = a;
    __syncthreads();
    if (tid < 3) {
        double un = s.chain[tid];
        un = dsub(un, ddiv(dmul(corr, corr), nn));
        const double var = ddiv(un, nn);
        const double e = 2.220446049250313e-16;
        const double ub = dadd(dmul(dmul(nn, e), var), dmul(dmul(dmul(nn, T), e), dmul(dmul(nn, T), e)));
        sh.sscale[tid] = var <= ub ? 1.0 : __dsqrt_rn(var);
    }
    __syncthreads();
}

// H: transform (X -= mean_; X /= scale_) in place; the bbox of the scaled cloud into the frame's scalars
__device__ __forceinline__ void scaler_transform(BlockScratch &s, const PreShared &sh, double *sc, int64_t nng, double *S)
{
    double smean[3], sscale[3], slo[3] = {INFINITY, INFINITY, INFINITY}, shi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int c = 0; c < 3; ++c) {
        smean[c] = sh.smean[c];
        sscale[c] = sh.sscale[c];
    }
    for (int64_t i = threadIdx.x; i < nng; i += kT)
        for (int c = 0; c < 3; ++c) {
            const double y = ddiv(dsub(sc[3 * i + c], smean[c]), sscale[c]);
            sc[3 * i + c] = y;
            slo[c] = fmin(slo[c], y);
            shi[c] = fmax(shi[c], y);
        }
    for (int c = 0; c < 3; ++c) {
        const double lo = block_min(s, slo[c]), hi = block_max(s, shi[c]);
        if (threadIdx.x == 0) {
            S[S_SLO + c] = lo;
            S[S_SHI + c] = hi;
        }
    }
}

// I: eps = max(0.2, min(0.5, mean(std(scaled, axis=0)) * 0.5)) (:194-195)
__device__ __forceinline__ double eps_heuristic(const double *sc, int64_t nng, SeqStage &st, BlockScratch &s,
                                                PreShared &sh)
{
    col_moments(sc, nng, st, s, sh);
    const double avg = dmul(ddiv(dadd(dadd(dadd(0.0, sh.std[0]), sh.std[1]), sh.std[2]), 3.0), 0.5);
    const double mn = avg < 0.5 ? avg : 0.5;
    return 0.2 >= mn ? 0.2 : mn;
}

// LIDAR_PRE_DIAG builds (tools/micro/pre_phases.py only): shader-clock stamps of the phases
// A..I into the frame's scalars 48..57 (cycles since the kernel start)
#ifdef LIDAR_PRE_DIAG
#define PRE_STAMP(k)                                                                   \
    do {                                                                               \
        __syncthreads();                                                               \
        if (threadIdx.x == 0) S[48 + (k)] = (double)(clock64() - pre_t0);              \
    } while (0)
#else
#define PRE_STAMP(k) ((void)0)
#endif
__global__ __launch_bounds__(kT) void preprocess_kernel(const double *__restrict__ xyz_in, int64_t n_in,
                                                        uint8_t *__restrict__ mask_in,
                                                        double *__restrict__ colors_in,
                                                        double *__restrict__ normals_in,
                                                        double *__restrict__ comp_in,
                                                        double *__restrict__ sc_in,
                                                        int32_t *__restrict__ ng_pos_in,
                                                        double *__restrict__ S_in, FrameMap fm,
                                                        double fixed_eps)
{
    __shared__ BlockScratch s;
    __shared__ SeqStage st;
    __shared__ PreShared sh;
    const int tid = threadIdx.x;
    const int64_t n = fm.n(n_in);
    const double *xyz = fm.rows(xyz_in, 3);
    uint8_t *mask = fm.rows(mask_in, 1);
    double *colors = fm.rows(colors_in, 3), *normals = fm.rows(normals_in, 3), *comp = fm.rows(comp_in, 3);
    double *sc = fm.ws(sc_in);
    int32_t *ng_pos = fm.ws(ng_pos_in);
    double *S = fm.scal(S_in);
#ifdef LIDAR_PRE_DIAG
    const long long pre_t0 = clock64();
#endif
    if (n == 0) {  // an empty frame of a batch: the reference raises ValueError (status 2)
        if (tid == 0) S[S_STATUS] = 2.0;
        return;
    }

    PRE_STAMP(0);  // A
    double zmin, denom;
    colour_range(s, xyz, n, zmin, denom);

    PRE_STAMP(1);  // B: mean / std with numpy's sequential axis-0 sums (:151-152)
    col_moments(xyz, n, st, s, sh);
    double mean[3], thr[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        mean[c] = sh.mean[c];
        thr[c] = dmul(3.0, sh.std[c]);
    }
    if (tid < 3) {
        S[S_MEAN + tid] = sh.mean[tid];
        S[S_STD + tid] = sh.std[tid];
    }

    PRE_STAMP(2);  // C
    const int64_t nin = compact_inliers(s, xyz, n, mean, thr, zmin, denom, mask, comp, colors, normals);
    if (tid == 0) {
        S[S_NIN] = (double)nin;
        S[S_STATUS] = nin == 0 ? 1.0 : 0.0;
        S[S_N] = (double)n;
    }
    if (nin == 0) return;  // reference: IndexError from np.percentile on an empty array
    __threadfence_block();
    __syncthreads();

    PRE_STAMP(3);  // D
    const double zt = select_z_threshold(s, st, sh, comp, nin);

    PRE_STAMP(4);  // E
    ground_plane(s, st, comp, nin, zt, S);

    PRE_STAMP(5);  // F
    const int64_t nng = compact_non_ground(s, comp, nin, zt, sc, ng_pos);
    if (tid == 0) S[S_NNG] = (double)nng;
    if (nng <= 10) return;  // reference: all non-ground labelled 0, no DBSCAN (:199-200)
    __threadfence_block();
    __syncthreads();
    if (fixed_eps > 0.0) {
        // app_simplified.py:104-108 / app_with_db.py:108-112 variant: DBSCAN(eps) on the
        // UNSCALED non-ground points — no StandardScaler, no eps heuristic; bbox of sc only
        block_bbox(s, sc, nng, S + S_SLO, S + S_SHI);
        if (tid == 0) {
            for (int c = 0; c < 3; ++c) {
                S[S_SMEAN + c] = 0.0;
                S[S_SSCALE + c] = 1.0;
            }
            S[S_EPS] = fixed_eps;
        }
        return;
    }

    PRE_STAMP(6);  // G
    scaler_fit(sc, nng, st, s, sh);
    if (tid < 3) {
        S[S_SMEAN + tid] = sh.smean[tid];
        S[S_SSCALE + tid] = sh.sscale[tid];
    }

    PRE_STAMP(7);  // H
    scaler_transform(s, sh, sc, nng, S);
    __threadfence_block();
    __syncthreads();

    PRE_STAMP(8);  // I
    const double eps = eps_heuristic(sc, nng, st, s, sh);
    if (tid == 0) S[S_EPS] = eps;
    PRE_STAMP(9);
}

// full labels over the inliers: ground -1, non-ground = DBSCAN label (or 0 when <= 10).  Two launches (a fill
// and a scatter in one would race across workgroups): first -1 everywhere,
__global__ void ground_fill_kernel(const double *S_in, int64_t *full_in, FrameMap fm)
{
    const double *S = fm.scal(S_in);
    int64_t *full = fm.rows(full_in, 1);
    if (S[S_STATUS] != 0.0) return;
    const int64_t nin = (int64_t)S[S_NIN];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nin; i += stride) full[i] = -1;
}
// then the non-ground points' labels at their inlier indices
__global__ void cluster_label_scatter_kernel(const double *S_in, const int64_t *ng_labels_in, const int32_t *ng_pos_in,
                                             int64_t *full_in, FrameMap fm)
{
    const double *S = fm.scal(S_in);
    const int64_t *ng_labels = fm.ws(ng_labels_in);
    const int32_t *ng_pos = fm.ws(ng_pos_in);
    int64_t *full = fm.rows(full_in, 1);
    if (S[S_STATUS] != 0.0) return;
    const int64_t nng = (int64_t)S[S_NNG];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nng; i += stride)
        full[ng_pos[i]] = nng > 10 ? ng_labels[i] : 0;
}

// preprocess + DBSCAN + label scatter for `frames` frames (CSR rows, offs on the device;
// offs == nullptr: one frame of n points)
int run_preprocess(lidar_handle *h, const double *xyz, int64_t n, const int64_t *offs, int frames, uint8_t *mask,
                   double *colors, double *normals, double *compact_xyz, int64_t *labels, double *scalars,
                   hipStream_t s, double fixed_eps)
{
    lidar::Carver cv;
    const uint64_t o_sc = cv.take<double>(3 * n);
    const uint64_t o_pos = cv.take<int32_t>(n);
    const uint64_t o_lab = cv.take<int64_t>(n);
    lidar::Carver at = cv;  // where the DBSCAN sub-buffers start
    carve_dbscan(cv, n, nullptr);
    const uint64_t wss = lidar::align_up(cv.off, 256);
    char *base = static_cast<char *>(lidar::workspace(h, wss * (uint64_t)frames));
    if (!base) return LIDAR_ENOMEM;
    double *sc = reinterpret_cast<double *>(base + o_sc);
    int32_t *ng_pos = reinterpret_cast<int32_t *>(base + o_pos);
    int64_t *ng_lab = reinterpret_cast<int64_t *>(base + o_lab);
    DbscanWs w = carve_dbscan(at, n, base);
    w.x = sc;  // DBSCAN clusters the (scaled) non-ground points
    FrameMap fm;
    fm.wss = (int64_t)wss;
    fm.offs = offs;
    HIP_TRY(hipMemsetAsync(scalars, 0, sizeof(double) * S_COUNT * frames, s));
    {
        lidar::Span sp(h, "preprocess", s);
        hipLaunchKernelGGL(preprocess_kernel, dim3(1, frames), dim3(kT), 0, s, xyz, n, mask, colors, normals,
                           compact_xyz, sc, ng_pos, scalars, fm, fixed_eps);
        dbscan_params_from_scalars(scalars, w, s, fm, frames);
    }
    int rc = run_dbscan(h, n, 5, w, ng_lab, s, fm, frames);
    if (rc) return rc;
    const unsigned gp = point_blocks(n, frames);
    lidar::Span sp(h, "label_scatter", s);
    hipLaunchKernelGGL(ground_fill_kernel, dim3(gp, frames), dim3(256), 0, s, scalars, labels, fm);
    hipLaunchKernelGGL(cluster_label_scatter_kernel, dim3(gp, frames), dim3(256), 0, s, scalars, ng_lab, ng_pos, labels,
                       fm);
    dbscan_nclust_to_scalars(w, scalars, s, fm, frames);
    LAUNCH_CHECK();
    return LIDAR_OK;
}

}  // namespace

// ====================================================================== C-ABI
// the three entry points' argument checks and call.  who: the entry point's name; nname: its name for the point
// count; offs_optional: offsets may be null (one frame of n points); eps: null for the scaled path
static int preprocess_entry(const std::string &who, const char *nname, bool offs_optional, lidar_handle *h,
                            const double *xyz, const int64_t *offsets, int32_t frames, int64_t n, const double *eps,
                            uint8_t *mask, double *colors, double *normals, double *compact_xyz, int64_t *labels,
                            double *scalars, void *stream)
{
    REQUIRE(h && xyz && (offsets || offs_optional) && mask && colors && normals && compact_xyz && labels && scalars,
            who + ": null pointer");
    REQUIRE(frames >= 1 && frames <= 65535 && (offsets || frames == 1),
            who + ": need 1 <= frames <= 65535" + (offs_optional ? " (offsets for frames > 1)" : ""));
    REQUIRE(n >= 1 && n < 0x7fffffff, who + ": need 1 <= " + nname + " < 2^31");
    REQUIRE(!eps || (*eps > 0.0 && *eps < INFINITY), who + ": eps must be finite and > 0");
    ON_DEVICE(h->device);
    return run_preprocess(h, xyz, n, offsets, frames, mask, colors, normals, compact_xyz, labels, scalars,
                          static_cast<hipStream_t>(stream), eps ? *eps : 0.0);
}

LIDAR_EXPORT int lidar_preprocess_f64(lidar_handle *h, const double *xyz, int64_t n, uint8_t *mask,
                                      double *colors, double *normals, double *compact_xyz,
                                      int64_t *labels, double *scalars, void *stream)
{
    return preprocess_entry("lidar_preprocess_f64", "n", true, h, xyz, nullptr, 1, n, nullptr, mask, colors, normals,
                            compact_xyz, labels, scalars, stream);
}

LIDAR_EXPORT int lidar_preprocess_batch_f64(lidar_handle *h, const double *xyz, const int64_t *offsets,
                                            int32_t frames, int64_t max_n, uint8_t *mask, double *colors,
                                            double *normals, double *compact_xyz, int64_t *labels,
                                            double *scalars, void *stream)
{
    return preprocess_entry("lidar_preprocess_batch_f64", "max_n", false, h, xyz, offsets, frames, max_n, nullptr, mask,
                            colors, normals, compact_xyz, labels, scalars, stream);
}

// the variant pipeline's preprocess (app_simplified.py:76-137, app_with_db.py:80-141):
// lidar_preprocess_batch_f64's phases with DBSCAN(eps, min_samples=5) on the unscaled
// non-ground points.  offsets == nullptr: one frame of max_n points.
LIDAR_EXPORT int lidar_preprocess_eps_batch_f64(lidar_handle *h, const double *xyz, const int64_t *offsets,
                                                int32_t frames, int64_t max_n, double eps, uint8_t *mask,
                                                double *colors, double *normals, double *compact_xyz,
                                                int64_t *labels, double *scalars, void *stream)
{
    return preprocess_entry("lidar_preprocess_eps_batch_f64", "max_n", true, h, xyz, offsets, frames, max_n, &eps, mask,
                            colors, normals, compact_xyz, labels, scalars, stream);
}
