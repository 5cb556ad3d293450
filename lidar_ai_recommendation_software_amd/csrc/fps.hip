// fps.hip — farthest-point sampling on gfx950, exact, bucket-pruned.
//
// Spec (oracle/lidar_oracle.c orc_fps): idx[0] = 0, dist = +inf,
// then npoint-1 times: dist = min(dist, d(., last)), last = argmax dist (lowest index
// on ties), d = (dx*dx + dy*dy) + dz*dz in fp32 with one rounding per operation.
//
// One workgroup of T = 1024 or 512 threads per frame (fps_bucket_kernel<T, BPL, DIAG, PPL>), in phases:
//   copy_prefix   the nested shortcut (below), instead of everything else
//   fps_prologue  frame bbox, counting sort of the points by a 16^3 Morton cell into a sorted copy in the
//                 workspace ((x, y, z, original index) float4s + a separate dist array), cut into buckets of
//                 64 x PPL consecutive sorted points (PPL = 1 up to 262 144 points) and padded to whole
//                 buckets with dist -1 sentinels
//   bucket_boxes, init_buckets
//                 every bucket gets a record (Bucket: bounding box, (max dist, index) key, the coordinates
//                 and the position of that point) in the registers of its owner lane, BPL records per lane
//   per step:     update_active (per owner slot), wave_argmax, publish, barrier, merge
//
// Step: a bucket can only change if some member gets closer to the new sample than
// its current dist.  lb = dist-from-bbox(q) computed with the SAME rounded operations
// as d is a lower bound of every member's d (fl() is monotone), so `lb >= bucket max`
// proves no member changes and the bucket is skipped — an exact pruning, not an
// approximation.  Active buckets are streamed (64 lanes x PPL points, coalesced float4 (x, y, z, index) +
// dist loads, the loads of up to 4 buckets of one owner slot in flight together; the sentinels keep the
// batch branch-free), updated, and re-reduced with DPP argmax reductions (max dist, lowest index on ties).
// A wave whose argmax bucket changed recomputes its DPP argmax; every wave then submits its merge key
// (pack_key: dist bits, index, wave) to ONE LDS 64-bit atomic max and its coordinates to a per-wave slot,
// so the frame argmax costs a single barrier per step.
//
// Nested FPS (SA2 samples SA1's centroids): FPS over the first m points of an FPS ordering
// is the identity 0..m-1 while the parent's winning distance stayed > 0 and finite — the parent
// run records the first step whose winning distance was 0, inf or NaN (`first_zero`), the child run
// takes it as `prefix_ok` and copies the prefix when m <= prefix_ok (DESIGN.md §3.1;
// tests/test_gpu_nonfinite.py::test_backbone_nonfinite_frame: a frame with an inf point).
#include <type_traits>
#ifdef LIDAR_DIAG
#include <algorithm>
#include <atomic>
#endif

#include "common.hpp"

namespace {

// default workgroup size: 16 waves (active-bucket updates and their reductions run in parallel
// across waves; the merge is an LDS atomic max).  lidar_fps_ex_f32 also offers 512 (8 waves,
// 2 buckets per lane: ~25 % longer steps, half the CU footprint beside other kernels)
constexpr int kDefaultThreads = 1024;
// one point per lane: 8 bucket slots per lane of a 512-thread workgroup (the register budget) hold
// 262 144 points; larger frames take buckets of 64 x PPL points (PPL 2 .. 16: up to 4 Mi points)
constexpr int64_t kMaxBucketPoints = 8 * 512 * 64;
constexpr int64_t kMaxFpsPoints = 16 * kMaxBucketPoints;
// the launch table (fps_kernel) offers at most 8 slots per lane at 512 threads and 4 at 1024
static_assert(kMaxBucketPoints / 64 <= 8 * 512 && kMaxBucketPoints / 64 <= 4 * 1024,
              "one-point-per-lane frames must fit the bucket slots of both workgroup sizes");
constexpr int kGrid = 16;  // Morton cells per axis for the bucket ordering
constexpr int kCells = kGrid * kGrid * kGrid;

__device__ __forceinline__ uint32_t spread3(uint32_t v)  // 4 bits -> every third bit
{
    v &= 0xf;
    v = (v | (v << 4)) & 0x0c3;
    v = (v | (v << 2)) & 0x249;
    return v;
}

struct FrameWs {
    float4 *p;  // sorted (x, y, z, original index bits): read-only after the prologue
    float *d;   // running min distance of each sorted point: the only per-step store, so an
                // update dirties 2 cache lines per bucket, not 8 (the L2 holds ~4 frames per XCD)
};

struct Query {  // the latest sample
    float x, y, z;
};

// one bucket, in the registers of its owner lane
struct Bucket {
    float lo[3], hi[3];  // bounding box of its points
    float d;             // key: the largest dist of a member ...
    uint32_t i;          // ... and the lowest original index that holds it
    float x[3];          // that member's coordinates
    int p;               // that member's position j * 64 + lane in the bucket; -1 until reduced
};

// the bucket that slot `slot` of lane `lane` of wave `wave` owns (NW waves per workgroup)
template <int NW>
__device__ __forceinline__ int owned_bucket(int wave, int slot, int lane)
{
    return wave + NW * (slot * 64 + lane);
}

// workspace position of sorted point j * 64 + lane of a bucket (lane l holds the bucket's points
// j * 64 + l: coalesced per j).  Unsigned: the loads take the SGPR base + 32-bit offset form
template <int PPL>
__device__ __forceinline__ uint32_t sorted_pos(int bucket, int j, int lane)
{
    return (uint32_t)(bucket * 64 * PPL + lane) + 64 * j;
}

// The merge key of a wave's candidate: dist bits << 32 | (2^27 - index) << 4 | wave.  A larger key is a
// larger distance (d >= 0 orders as unsigned), then a smaller index; a wave without a candidate (index
// 0xffffffff) carries index field 0, below every real one.
constexpr int kKeyWaveBits = 4;
constexpr int kKeyIndexBits = 32 - kKeyWaveBits;             // holds 2^27 - index: 1 .. 2^27
constexpr uint32_t kKeyIndexTop = 1u << (kKeyIndexBits - 1);  // indices stay below it
static_assert(kMaxFpsPoints <= kKeyIndexTop, "every point index must fit the merge key's index field");

struct MergeKey {
    uint32_t dist_bits, index;
    int wave;
};

__device__ __forceinline__ unsigned long long pack_key(float d, uint32_t index, int wave)
{
    const uint32_t fld = index < kKeyIndexTop ? kKeyIndexTop - index : 0u;
    return ((unsigned long long)__float_as_uint(d) << 32) | (fld << kKeyWaveBits) | (uint32_t)wave;
}

// of a wave-uniform key: the wave and the dist bits come back in scalar registers
__device__ __forceinline__ MergeKey unpack_key(unsigned long long key)
{
    MergeKey k;
    k.wave = __builtin_amdgcn_readfirstlane((int)(key & ((1u << kKeyWaveBits) - 1)));
    k.index = kKeyIndexTop - (((uint32_t)key) >> kKeyWaveBits);
    k.dist_bits = (uint32_t)__builtin_amdgcn_readfirstlane((int)(key >> 32));
    return k;
}

// distance from q to [lo, hi] along one axis: lo - q below, q - hi above, else 0 — as
// max3(lo - q, q - hi, 0) (one of the two differences is <= 0 whenever the other is > 0)
__device__ __forceinline__ float gap(float q, float lo, float hi)
{
    return fmaxf(fmaxf(__fsub_rn(lo, q), __fsub_rn(q, hi)), 0.0f);
}

// Update K active buckets of one owner slot (their loads issued together, their DPP
// reductions interleaved): new distances against q, bucket max + its lowest-index argmax
// point into the owner lane's record B (mask: the owner lanes of the slot's active buckets).
template <int K, int NW, int PPL>
__device__ __forceinline__ void update_batch(uint64_t &mask, const FrameWs &W, int wave, int slot, int lane,
                                             const Query &q, Bucket &B, int target, bool &hit)
{
    // branch-free: the workspace is padded to whole buckets with sentinel points
    // (dist -1: never the max, never updated since every real d >= 0)
    int bbs[K];
    uint32_t pos[K];
    float4 P[K][PPL];
    float D[K][PPL];
#pragma unroll
    for (int u = 0; u < K; ++u) {
        bbs[u] = __ffsll((unsigned long long)mask) - 1;
        mask &= mask - 1;
        pos[u] = sorted_pos<PPL>(owned_bucket<NW>(wave, slot, bbs[u]), 0, lane);
    }
#pragma unroll
    for (int u = 0; u < K; ++u)
#pragma unroll
        for (int j = 0; j < PPL; ++j) {
            P[u][j] = W.p[pos[u] + 64 * j];
            D[u][j] = W.d[pos[u] + 64 * j];
        }
    // distances in bit space (>= +0 or the -1 sentinel: signed int order = float order); per lane
    // the best of its PPL points (max dist, lowest index)
    int od[K], dm[K], lj[K];
    uint32_t I[K];
    // a bucket's key (max dist, lowest index) can only change if its argmax member got
    // closer: distances only decrease, so with that member untouched the max and its
    // lowest-index holder stand — the reduction is skipped (B.p = the member, -1 unknown)
    bool redo[K];
#pragma unroll
    for (int u = 0; u < K; ++u) {
        od[u] = -1;
        I[u] = 0xffffffffu;
        lj[u] = 0;
        uint64_t chm = 0;
        const int bpu = __builtin_amdgcn_readlane(B.p, bbs[u]);
#pragma unroll
        for (int j = 0; j < PPL; ++j) {
            // d >= +0 or NaN; the sign bit cleared, a NaN d (inf - inf) orders above every dist and never
            // replaces one, as in the oracle (a bare bit compare let a negative NaN in)
            const int db =
                __float_as_int(lidar::dist2f(P[u][j].x, P[u][j].y, P[u][j].z, q.x, q.y, q.z)) & 0x7fffffff;
            const int o = min(db, __float_as_int(D[u][j]));
            const bool lower = o != __float_as_int(D[u][j]);
            if (lower) W.d[pos[u] + 64 * j] = __int_as_float(o);  // only changed members dirty a line
            const uint64_t ch = __ballot(lower);
            if (PPL == 1 || (bpu >> 6) == j) chm = ch;
            const uint32_t ij = __float_as_uint(P[u][j].w);
            if (PPL == 1 || o > od[u] || (o == od[u] && ij < I[u])) {
                od[u] = o;
                I[u] = ij;
                lj[u] = j;
            }
        }
        redo[u] = bpu < 0 || ((chm >> (bpu & 63)) & 1ull);
    }
#pragma unroll
    for (int u = 0; u < K; ++u) {
        dm[u] = 0;
        if (redo[u]) dm[u] = lidar::wave_max_i32_dpp(od[u]);  // wave-uniform
    }
#pragma unroll
    for (int u = 0; u < K; ++u) {
        if (!redo[u]) continue;  // wave-uniform
        hit = hit || bbs[u] == target;
        const uint64_t c = __ballot(od[u] == dm[u]);
        int wl;
        if (__popcll(c) == 1) {
            wl = __ffsll((unsigned long long)c) - 1;
        } else {
            const uint32_t mi = lidar::wave_min_u32_dpp(od[u] == dm[u] ? I[u] : 0xffffffffu);
            wl = __ffsll((unsigned long long)__ballot(od[u] == dm[u] && I[u] == mi)) - 1;
        }
        float4 pb = P[u][0];
#pragma unroll
        for (int j = 1; j < PPL; ++j)
            if (lj[u] == j) pb = P[u][j];
        const uint32_t wi = (uint32_t)__builtin_amdgcn_readlane((int)I[u], wl);
        const float wx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pb.x), wl));
        const float wy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pb.y), wl));
        const float wz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pb.z), wl));
        const int wj = PPL == 1 ? 0 : __builtin_amdgcn_readlane(lj[u], wl);
        const bool me = lane == bbs[u];
        B.p = me ? wj * 64 + wl : B.p;
        B.d = me ? __int_as_float(dm[u]) : B.d;
        B.i = me ? wi : B.i;
        B.x[0] = me ? wx : B.x[0];
        B.x[1] = me ? wy : B.x[1];
        B.x[2] = me ? wz : B.x[2];
    }
}

__device__ __forceinline__ uint64_t stamp()
{
    uint64_t t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    return t;
}

// DIAG instantiations (the LIDAR_DIAG library only: lidar_diag_fps_phases, lidar_diag_fps_eager512_phases
// and the launches lidar_diag_fps_record catches) accumulate six words per wave, shader cycles between
// laps or plain counts: [0] bucket tests + active-bucket updates, [1] wave argmax, [2] LDS publish + barrier wait
// (tools/micro label the two "argmax+publish" and "barrier"), [3] merge, [4] active-bucket batches
// processed, [5] steps.  Without DIAG the clock is empty: the product reads no shader clock.
template <bool DIAG>
struct PhaseClock {
    __device__ __forceinline__ void start() {}
    __device__ __forceinline__ void lap(int) {}
    __device__ __forceinline__ void count(int) {}
    __device__ __forceinline__ void store(uint64_t *) const {}
};

template <>
struct PhaseClock<true> {
    uint64_t acc[6] = {0, 0, 0, 0, 0, 0};
    uint64_t t0 = 0;
    __device__ __forceinline__ void start()
    {
        __builtin_amdgcn_sched_barrier(0);
        t0 = stamp();
        __builtin_amdgcn_sched_barrier(0);
    }
    __device__ __forceinline__ void lap(int k)  // cycles since start() or the last lap into word k
    {
        __builtin_amdgcn_sched_barrier(0);
        const uint64_t t1 = stamp();
        acc[k] += t1 - t0;
        t0 = t1;
        __builtin_amdgcn_sched_barrier(0);
    }
    __device__ __forceinline__ void count(int k) { acc[k]++; }
    __device__ __forceinline__ void store(uint64_t *out) const
    {
        for (int k = 0; k < 6; ++k) out[k] = acc[k];
    }
};

__device__ __forceinline__ void write_sample(int32_t *out_idx, float *out_xyz, int64_t at, int32_t index,
                                             float x, float y, float z)
{
    out_idx[at] = index;
    if (out_xyz) {
        float *o = out_xyz + at * 3;
        o[0] = x;
        o[1] = y;
        o[2] = z;
    }
}

// nested FPS shortcut: FPS over the first m points of an FPS ordering returns 0..m-1
// as long as the parent's winning distance stayed > 0 and finite — exact.
template <int T>
__device__ __forceinline__ void copy_prefix(const float *__restrict__ p, int64_t b, int npoint, int32_t *out_idx,
                                            float *out_xyz, int32_t *first_zero, int32_t prefix_ok)
{
    const int tid = threadIdx.x;
    for (int i = tid; i < npoint; i += T)
        write_sample(out_idx, out_xyz, b * npoint + i, i, p[3 * i], p[3 * i + 1], p[3 * i + 2]);
    if (first_zero && tid == 0) first_zero[b] = prefix_ok;
}

// Prologue of one frame, run by the whole workgroup: frame bbox, counting sort of the points
// by 16^3 Morton cell into W (padded to whole buckets with dist -1 sentinels).  Ends with a
// barrier (hist is free afterwards).
template <int T>
__device__ __forceinline__ void fps_prologue(const float *__restrict__ p, int n, int npad, const FrameWs &W,
                                             uint32_t *hist, float (*red)[T / 64], uint32_t *wsum)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // ---- frame bounding box
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = tid; i < n; i += T) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            float v = p[3 * i + a];
            lo[a] = fminf(lo[a], v);
            hi[a] = fmaxf(hi[a], v);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        lo[a] = lidar::wave_min_f(lo[a]);
        hi[a] = lidar::wave_max_f(hi[a]);
    }
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            red[a][wave] = lo[a];
            red[3 + a][wave] = hi[a];
        }
    }
    for (int c = tid; c < kCells; c += T) hist[c] = 0;
    __syncthreads();
    float scale[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float l = red[a][0], h = red[3 + a][0];
        for (int w = 1; w < (T / 64); ++w) {
            l = fminf(l, red[a][w]);
            h = fmaxf(h, red[3 + a][w]);
        }
        lo[a] = l;
        scale[a] = h > l ? (float)kGrid / (h - l) : 0.0f;
    }

    // ---- counting sort by Morton cell (order inside a cell is irrelevant: exactness
    // never depends on the bucket layout, only the pruning rate does)
    auto cell_of = [&](int i) -> uint32_t {
        uint32_t c[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            int v = (int)((p[3 * i + a] - lo[a]) * scale[a]);
            c[a] = (uint32_t)min(max(v, 0), kGrid - 1);
        }
        return spread3(c[0]) | (spread3(c[1]) << 1) | (spread3(c[2]) << 2);
    };
    for (int i = tid; i < n; i += T) atomicAdd(&hist[cell_of(i)], 1u);
    __syncthreads();
    {  // exclusive scan of the cell counts, kCells / T consecutive cells per thread
        constexpr int per = kCells / T;
        uint32_t v[per], s = 0;
#pragma unroll
        for (int j = 0; j < per; ++j) {
            v[j] = hist[per * tid + j];
            s += v[j];
        }
        uint32_t incl = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            uint32_t t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint32_t e = incl - s;
        for (int w = 0; w < wave; ++w) e += wsum[w];
#pragma unroll
        for (int j = 0; j < per; ++j) {
            hist[per * tid + j] = e;
            e += v[j];
        }
    }
    __syncthreads();
    for (int i = tid; i < n; i += T) {
        uint32_t pos = atomicAdd(&hist[cell_of(i)], 1u);
        W.p[pos] = make_float4(p[3 * i], p[3 * i + 1], p[3 * i + 2], __uint_as_float((uint32_t)i));
        W.d[pos] = INFINITY;
    }
    for (int i = n + tid; i < npad; i += T) {
        W.p[i] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xffffffffu));
        W.d[i] = -1.0f;
    }
    __threadfence_block();
    __syncthreads();
}

// Bucket bounding boxes into the owner lanes' records: every wave reduces whole buckets into a table in
// the (free after the prologue) hist array, 512 buckets per pass (12 KiB), and the owner lanes pick theirs
// up — no LDS is held for it through the step loop (the kernel's LDS stays ~17 KiB beside other kernels).
// An empty slot keeps the box (inf, -inf).  Ends with a barrier.
constexpr int kBoxPass = 512;
static_assert(kCells >= kBoxPass * 6, "bbox pass table");
template <int T, int BPL, int PPL>
__device__ __forceinline__ void bucket_boxes(const FrameWs &W, int n, int nb, float *tab, Bucket (&bk)[BPL])
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int s = 0; s < BPL; ++s)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            bk[s].lo[a] = INFINITY;
            bk[s].hi[a] = -INFINITY;
        }
    for (int p0 = 0; p0 < nb; p0 += kBoxPass) {
        for (int bucket = p0 + wave; bucket < nb && bucket < p0 + kBoxPass; bucket += (T / 64)) {
            float v[3] = {INFINITY, INFINITY, INFINITY}, u[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
            for (int j = 0; j < PPL; ++j) {
                const int pos = (int)sorted_pos<PPL>(bucket, j, lane);
                if (pos < n) {
                    const float4 P = W.p[pos];
                    v[0] = fminf(v[0], P.x);
                    v[1] = fminf(v[1], P.y);
                    v[2] = fminf(v[2], P.z);
                    u[0] = fmaxf(u[0], P.x);
                    u[1] = fmaxf(u[1], P.y);
                    u[2] = fmaxf(u[2], P.z);
                }
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                v[a] = lidar::wave_min_f(v[a]);
                u[a] = lidar::wave_max_f(u[a]);
            }
            if (lane == 0) {
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    tab[(bucket - p0) * 6 + a] = v[a];
                    tab[(bucket - p0) * 6 + 3 + a] = u[a];
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < BPL; ++s) {
            const int bucket = owned_bucket<T / 64>(wave, s, lane);
            if (bucket >= p0 && bucket < p0 + kBoxPass && bucket < nb)
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    bk[s].lo[a] = tab[(bucket - p0) * 6 + a];
                    bk[s].hi[a] = tab[(bucket - p0) * 6 + 3 + a];
                }
        }
        __syncthreads();
    }
}

template <int T, int BPL>
__device__ __forceinline__ void init_buckets(int nb, Bucket (&bk)[BPL])
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int s = 0; s < BPL; ++s) {
        const bool have = owned_bucket<T / 64>(wave, s, lane) < nb;
#pragma unroll
        for (int a = 0; a < 3; ++a) bk[s].x[a] = 0.0f;
        bk[s].p = -1;
        // a bucket's key is a placeholder until its first update: NaN bits, above every lower bound in the
        // bit-space test of update_active, so step 1 updates every bucket — also one whose lower bound is inf
        // (all its points have an inf coordinate, or squared distances that overflow), which `lb < inf` left
        // with the placeholder (inf, index 0) as the frame's argmax.  Empty slot: never active, never the argmax
        bk[s].d = have ? __int_as_float(0x7fc00000) : 0.0f;
        bk[s].i = have ? 0u : 0xffffffffu;
    }
}

// a wave's argmax over its buckets, wave-uniform
struct WaveBest {
    float d = 0.0f;
    uint32_t i = 0xffffffffu;
    float x = 0.0f, y = 0.0f, z = 0.0f;
    // its bucket (slot `slot` of lane `lane`): updates only lower bucket keys (max dist, then lowest
    // index), so while that bucket is untouched the wave argmax stands
    int slot = 0, lane = 0;
};

// Test the buckets of owner slot `slot` against q and update the active ones.  target: the lane whose bucket
// in this slot is the wave's argmax (-1: none); dirty: that bucket's key changed.
template <int T, int PPL, bool DIAG>
__device__ __forceinline__ void update_active(const FrameWs &W, const Query &q, int slot, Bucket &B, int target,
                                              bool &dirty, PhaseClock<DIAG> &clk)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // up to 4 loads per lane in flight: K buckets of PPL points.  One instance per K, not one guarded
    // instance: that cost 72 VGPRs against 64 and measured slower
    constexpr int kMaxK = PPL == 1 ? 4 : PPL == 2 ? 2 : 1;
    const float gx = gap(q.x, B.lo[0], B.hi[0]);
    const float gy = gap(q.y, B.lo[1], B.hi[1]);
    const float gz = gap(q.z, B.lo[2], B.hi[2]);
    const float lb = __fadd_rn(__fadd_rn(__fmul_rn(gx, gx), __fmul_rn(gy, gy)), __fmul_rn(gz, gz));
    // lb and every real B.d are >= +0 and never NaN (gap() ends in fmaxf(., 0)): the signed order of
    // their bits is their float order
    uint64_t mask = __ballot(__float_as_int(lb) < __float_as_int(B.d));
    auto batch = [&](auto k) {
        update_batch<decltype(k)::value, T / 64, PPL>(mask, W, wave, slot, lane, q, B, target, dirty);
    };
    while (mask) {  // wave-uniform
        clk.count(4);
        const int cnt = __popcll(mask);
        if (kMaxK >= 4 && cnt >= 4) batch(std::integral_constant<int, 4>{});
        else if (kMaxK >= 3 && cnt == 3) batch(std::integral_constant<int, 3>{});  // one round trip, not 2 + 1
        else if (kMaxK >= 2 && cnt >= 2) batch(std::integral_constant<int, 2>{});
        else batch(std::integral_constant<int, 1>{});
    }
}

// lane best over its buckets -> wave argmax (DPP)
template <int BPL>
__device__ __forceinline__ void wave_argmax(const Bucket (&bk)[BPL], WaveBest &best)
{
    float d = bk[0].d;
    uint32_t i = bk[0].i;
    float cx = bk[0].x[0], cy = bk[0].x[1], cz = bk[0].x[2];
    int bs = 0;
#pragma unroll
    for (int s = 1; s < BPL; ++s) {
        // read before the test, not under it: the records stay in registers
        const float sd = bk[s].d, sx = bk[s].x[0], sy = bk[s].x[1], sz = bk[s].x[2];
        const uint32_t si = bk[s].i;
        if (sd > d || (sd == d && si < i)) {
            d = sd;
            i = si;
            cx = sx;
            cy = sy;
            cz = sz;
            bs = s;
        }
    }
    int wdb;
    const int wl = lidar::wave_argmax_lane_i32(__float_as_int(d), i, &wdb);
    best.d = __int_as_float(wdb);
    best.i = (uint32_t)__builtin_amdgcn_readlane((int)i, wl);
    best.x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cx), wl));
    best.y = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cy), wl));
    best.z = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cz), wl));
    best.lane = wl;
    best.slot = BPL > 1 ? __builtin_amdgcn_readlane(bs, wl) : 0;
}

// a wave submits its argmax: the key to the step's LDS atomic max, the coordinates to the wave's slot
__device__ __forceinline__ void publish(const WaveBest &best, unsigned long long *key, float *crd)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (lane == 0) {
        crd[0] = best.x;
        crd[1] = best.y;
        crd[2] = best.z;
        atomicMax(key, pack_key(best.d, best.i, wave));
    }
}

// The frame argmax after the barrier: the winner's key and every wave's candidate coordinates are read
// side by side (lane l < T / 64 reads wave l's slot: 256 B per wave instead of 1 KiB of LDS traffic); the
// winner's come back by readlane — one LDS round trip after the barrier instead of two dependent ones.
template <int T>
__device__ __forceinline__ MergeKey merge(const unsigned long long *key, const float (*crd)[4], Query &q)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long k = *key;
    float4 cand = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (lane < (T / 64)) cand = *reinterpret_cast<const float4 *>(crd[lane]);
    const MergeKey won = unpack_key(k);
    q.x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cand.x), won.wave));
    q.y = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cand.y), won.wave));
    q.z = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cand.z), won.wave));
    return won;
}

template <int T, int BPL, bool DIAG = false, int PPL = 1>
__global__ __launch_bounds__(T) void fps_bucket_kernel(
    const float *__restrict__ xyz, int n, int npoint, int32_t *__restrict__ out_idx, float *__restrict__ out_xyz,
    int32_t *__restrict__ first_zero, const int32_t *__restrict__ prefix_ok, float *__restrict__ ws,
    int64_t ws_stride, uint64_t *__restrict__ diag = nullptr)
{
    static_assert(T / 64 <= (1 << kKeyWaveBits), "every wave must fit the merge key's wave field");
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int wave = tid >> 6;
    const float *p = xyz + (int64_t)b * n * 3;
    if (prefix_ok != nullptr && prefix_ok[b] >= npoint) {
        copy_prefix<T>(p, b, npoint, out_idx, out_xyz, first_zero, prefix_ok[b]);
        return;
    }

    float *wsb = ws + (int64_t)b * ws_stride;
    const int npad = (n + 64 * PPL - 1) / (64 * PPL) * (64 * PPL);  // whole buckets; the tail holds sentinels
    FrameWs W{reinterpret_cast<float4 *>(wsb), wsb + 4 * (int64_t)npad};

    __shared__ uint32_t hist[kCells];
    __shared__ float red[6][(T / 64)];
    __shared__ uint32_t wsum[(T / 64)];
    // per-step merge: every wave submits its argmax as one 64-bit key to an LDS atomic max
    // (triple-buffered so a slot is cleared two barriers after its last read) and its
    // coordinates to a per-wave slot (double-buffered); one barrier per step
    __shared__ unsigned long long mkey[3];
    __shared__ __attribute__((aligned(16))) float mcrd[2][(T / 64)][4];

    fps_prologue<T>(p, n, npad, W, hist, red, wsum);
    const int nb = npad / (64 * PPL);
    Bucket bk[BPL];
    bucket_boxes<T, BPL, PPL>(W, n, nb, reinterpret_cast<float *>(hist), bk);
    init_buckets<T, BPL>(nb, bk);

    Query q{p[0], p[1], p[2]};  // sample 0 is index 0
    if (tid == 0) write_sample(out_idx, out_xyz, (int64_t)b * npoint, 0, q.x, q.y, q.z);
    int zero_at = npoint;  // first step whose winning distance is 0 or non-finite
    WaveBest best;
    if (tid < 3) mkey[tid] = 0ull;
    __syncthreads();
    int cur3 = 1, nxt3 = 2;
    PhaseClock<DIAG> clk;
    for (int it = 1; it < npoint; ++it) {
        bool wave_dirty = it == 1;  // the wave argmax is recomputed only when its bucket's key changed
        clk.start();
#pragma unroll
        for (int s = 0; s < BPL; ++s)
            update_active<T, PPL>(W, q, s, bk[s], s == best.slot ? best.lane : -1, wave_dirty, clk);
        clk.lap(0);
        if (wave_dirty) wave_argmax<BPL>(bk, best);
        clk.lap(1);
        publish(best, &mkey[cur3], mcrd[it & 1][wave]);
        if (tid == 0) mkey[nxt3] = 0ull;  // step it+1's slot, last read before the previous barrier
        __syncthreads();
        clk.lap(2);
        const MergeKey won = merge<T>(&mkey[cur3], mcrd[it & 1], q);
        if (tid == 0) write_sample(out_idx, out_xyz, (int64_t)b * npoint + it, (int32_t)won.index, q.x, q.y, q.z);
        // 0, or inf / NaN: a point with a non-finite coordinate, or one whose squared distances
        // overflow, keeps dist = inf for ever (no d is < inf once d is inf or NaN) and wins every
        // later step, so the ordering repeats it exactly as it does after a 0.  On the bits, in
        // scalar registers (the key is wave-uniform): bits - 1 wraps 0 above every finite value
        if (zero_at == npoint && won.dist_bits - 1u >= 0x7f7fffffu) zero_at = it;
        cur3 = nxt3;
        nxt3 = nxt3 == 2 ? 0 : nxt3 + 1;
        clk.lap(3);
        clk.count(5);
    }
    if (first_zero && tid == 0) first_zero[b] = zero_at;
    if (DIAG && (tid & 63) == 0) clk.store(diag + ((int64_t)b * (T / 64) + wave) * 6);
}

using FpsKernel = void (*)(const float *, int, int, int32_t *, float *, int32_t *, const int32_t *, float *, int64_t,
                           uint64_t *);

// The launch table: the instantiation for a workgroup of `threads` on frames of n points; stamped: its
// DIAG form, which only the LIDAR_DIAG library has, and only for these rows (else nullptr).
static FpsKernel fps_kernel(int threads, int64_t n, bool stamped)
{
    const int64_t nb = (n + 63) / 64;  // one bucket per lane and slot
    if (n > kMaxBucketPoints) {
        // large frames: 8 slots per lane at 512 threads, each bucket 64 x PPL points
        const int64_t ppl = (n + kMaxBucketPoints - 1) / kMaxBucketPoints;
        if (stamped || threads != 512) return nullptr;
        if (ppl <= 2) return fps_bucket_kernel<512, 8, false, 2>;
        if (ppl <= 4) return fps_bucket_kernel<512, 8, false, 4>;
        if (ppl <= 8) return fps_bucket_kernel<512, 8, false, 8>;
        return fps_bucket_kernel<512, 8, false, 16>;
    }
    if (stamped) {
#ifdef LIDAR_DIAG
        if (threads == 512 && nb <= 512) return fps_bucket_kernel<512, 1, true>;
        if (threads == 512 && nb <= 2 * 512) return fps_bucket_kernel<512, 2, true>;
        if (threads == 1024 && nb <= 1024) return fps_bucket_kernel<1024, 1, true>;
#endif
        return nullptr;
    }
    if (threads == 512) {
        if (nb <= 512) return fps_bucket_kernel<512, 1>;
        if (nb <= 2 * 512) return fps_bucket_kernel<512, 2>;
        if (nb <= 4 * 512) return fps_bucket_kernel<512, 4>;
        return fps_bucket_kernel<512, 8>;
    }
    if (nb <= 1024) return fps_bucket_kernel<1024, 1>;
    if (nb <= 2 * 1024) return fps_bucket_kernel<1024, 2>;
    return fps_bucket_kernel<1024, 4>;
}

}  // namespace

static int64_t fps_stride(int64_t n)  // floats per frame: (x, y, z, index) + dist over whole buckets
{
    const int64_t unit = n > kMaxBucketPoints ? 64 * 16 : 64;
    return lidar::align_up(5 * lidar::align_up(n, unit), 64);
}

// workspace bytes lidar_fps_f32 / lidar_fps_ex_f32 take from the handle for (batch, n)
LIDAR_EXPORT uint64_t lidar_fps_workspace_bytes(int64_t batch, int64_t n)
{
    return (uint64_t)(batch * fps_stride(n)) * 4;
}

// The one launch site: the handle's workspace for (batch, n) and the table's kernel for (threads, n);
// diag non-null: the stamped form, its phase words to diag.
static int run_fps(lidar_handle *h, int threads, const float *xyz, int64_t batch, int64_t n, int64_t npoint,
                   int32_t *idx, float *new_xyz, int32_t *first_zero, const int32_t *prefix_ok, uint64_t *diag,
                   void *stream)
{
    const FpsKernel kern = fps_kernel(threads, n, diag != nullptr);
    REQUIRE(kern, "run_fps: no kernel for this workgroup size and n");
    ON_DEVICE(h->device);
    const int64_t stride = fps_stride(n);
    float *ws = static_cast<float *>(lidar::workspace(h, (uint64_t)(batch * stride) * 4));
    if (!ws) return LIDAR_ENOMEM;
    hipLaunchKernelGGL(kern, dim3((unsigned)batch), dim3((unsigned)threads), 0, static_cast<hipStream_t>(stream), xyz,
                       (int)n, (int)npoint, idx, new_xyz, first_zero, prefix_ok, ws, stride, diag);
    LAUNCH_CHECK();
    return LIDAR_OK;
}

#ifdef LIDAR_DIAG
// diagnostic build only: phase stamps of the SA1 FPS launches a pipeline issues (lidar_diag_fps_record).
// Every 512-thread, one-point-per-lane launch without prefix_ok (SA1, not SA2's nested FPS) of n <= 65 536
// points takes the DIAG instantiation and appends its per-(frame, wave) phase totals (6 words, as
// lidar_diag_fps_eager512_phases) to the registered buffer while it has room.
static uint64_t *g_fps_rec = nullptr;
static int64_t g_fps_rec_cap = 0;
static std::atomic<int64_t> g_fps_rec_used{0};

// where such a launch records, or nullptr (not one of them, or the buffer is full)
static uint64_t *fps_record_slot(int threads, int64_t batch, int64_t n, const int32_t *prefix_ok)
{
    if (!g_fps_rec || threads != 512 || prefix_ok != nullptr || n > 65536) return nullptr;
    const int64_t need = batch * (512 / 64) * 6;
    const int64_t off = g_fps_rec_used.fetch_add(need);
    return off + need <= g_fps_rec_cap ? g_fps_rec + off : nullptr;
}
#endif

// threads: workgroup size per frame, 0 (the default, 1024), 1024 or 512 — same results
LIDAR_EXPORT int lidar_fps_ex_f32(lidar_handle *h, const float *xyz, int64_t batch, int64_t n, int64_t npoint,
                                  int32_t *idx, float *new_xyz, int32_t *first_zero, const int32_t *prefix_ok,
                                  int32_t threads, void *stream)
{
    REQUIRE(h && xyz && idx, "lidar_fps_ex_f32: null pointer");
    REQUIRE(batch >= 0 && n >= 1 && npoint >= 1, "lidar_fps_ex_f32: need n >= 1 and npoint >= 1");
    REQUIRE(n <= kMaxFpsPoints, "lidar_fps_ex_f32: n > 4194304 points per frame");
    if (threads == 0) threads = kDefaultThreads;
    REQUIRE(threads == 1024 || threads == 512, "lidar_fps_ex_f32: threads must be 0, 512 or 1024");
    if (n > kMaxBucketPoints) threads = 512;  // the large-frame kernels: 512 threads
    REQUIRE(batch <= 0x7fffffff, "lidar_fps_ex_f32: batch too large");
    if (batch == 0) return LIDAR_OK;
    REQUIRE(prefix_ok == nullptr || npoint <= n, "lidar_fps_ex_f32: prefix_ok needs npoint <= n");
    uint64_t *diag = nullptr;
#ifdef LIDAR_DIAG
    diag = fps_record_slot(threads, batch, n, prefix_ok);
#endif
    return run_fps(h, threads, xyz, batch, n, npoint, idx, new_xyz, first_zero, prefix_ok, diag, stream);
}

LIDAR_EXPORT int lidar_fps_f32(lidar_handle *h, const float *xyz, int64_t batch, int64_t n, int64_t npoint,
                               int32_t *idx, float *new_xyz, int32_t *first_zero, const int32_t *prefix_ok,
                               void *stream)
{
    return lidar_fps_ex_f32(h, xyz, batch, n, npoint, idx, new_xyz, first_zero, prefix_ok, 0, stream);
}

#ifdef LIDAR_DIAG
// diagnostic build only (`make diag`, not part of the product library or ABI)
// register (buf, cap_words) for the SA1 FPS launches' phase records (buf NULL: stop); returns 0
LIDAR_EXPORT int lidar_diag_fps_record(uint64_t *buf, int64_t cap_words)
{
    g_fps_rec = buf;
    g_fps_rec_cap = buf ? cap_words : 0;
    g_fps_rec_used = 0;
    return LIDAR_OK;
}
// words the registered buffer has received so far (launches past its capacity ran unstamped)
LIDAR_EXPORT int64_t lidar_diag_fps_recorded(void) { return std::min<int64_t>(g_fps_rec_used, g_fps_rec_cap); }

// per-wave phase totals of one FPS run of n <= 65 536 points: diag[(frame * (threads / 64) + wave) * 6 + k]
static int diag_fps_phases(const char *who, int threads, lidar_handle *h, const float *xyz, int64_t batch,
                           int64_t n, int64_t npoint, int32_t *idx, uint64_t *diag, void *stream)
{
    REQUIRE(h && xyz && idx && diag && n <= 65536 && n >= 1 && npoint >= 1, std::string(who) + ": bad args");
    return run_fps(h, threads, xyz, batch, n, npoint, idx, nullptr, nullptr, nullptr, diag, stream);
}

// at 512 threads (BPL 1 or 2 from n)
LIDAR_EXPORT int lidar_diag_fps_eager512_phases(lidar_handle *h, const float *xyz, int64_t batch, int64_t n,
                                                int64_t npoint, int32_t *idx, uint64_t *diag, void *stream)
{
    return diag_fps_phases("lidar_diag_fps_eager512_phases", 512, h, xyz, batch, n, npoint, idx, diag, stream);
}

// at the default 1024 threads (BPL 1)
LIDAR_EXPORT int lidar_diag_fps_phases(lidar_handle *h, const float *xyz, int64_t batch, int64_t n,
                                       int64_t npoint, int32_t *idx, uint64_t *diag, void *stream)
{
    return diag_fps_phases("lidar_diag_fps_phases", kDefaultThreads, h, xyz, batch, n, npoint, idx, diag, stream);
}
#endif
