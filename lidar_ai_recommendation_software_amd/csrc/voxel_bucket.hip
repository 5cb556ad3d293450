// voxel_bucket.hip — the bucket stage of the batched voxel downsampling: every bucket sorted, ranked against the
// buckets before it and emitted.  The design of both stages is told at the top of voxel_batch.hip.
#include "voxel_batch.hpp"

namespace {
using namespace lidar::vx;
// stable LSD radix sort of m pairs in global memory by one workgroup (a bucket above CAP), over the 8-bit digits whose
// bits vary across the bucket; returns the buffer holding the result
__device__ uint64_t *bucket_radix(uint64_t *a, uint64_t *b, int64_t m, uint32_t *cnt, uint32_t (*wc)[256],
                                  uint32_t *red, unsigned long long *vary)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) *vary = 0ull;
    __syncthreads();
    const uint64_t v0 = a[0];
    uint64_t x = 0;
    for (int64_t i = tid; i < m; i += UT) x |= a[i] ^ v0;
    for (int o = 32; o >= 1; o >>= 1) x |= (uint64_t)__shfl_xor((long long)x, o, 64);
    if (lane == 0) atomicOr(vary, (unsigned long long)x);
    __syncthreads();
    const uint64_t vb = *vary;
    for (int shift = 0; shift < 64; shift += 8) {
        if (((vb >> shift) & 0xffull) == 0) continue;  // uniform: this digit is constant
        if (tid < 256) cnt[tid] = 0;
        __syncthreads();
        for (int64_t i = tid; i < m; i += UT) atomicAdd(&cnt[(a[i] >> shift) & 255u], 1u);
        __syncthreads();
        uint32_t all;
        const uint32_t ex = block_excl_scan<UT>(tid < 256 ? cnt[tid] : 0u, red, &all);
        __syncthreads();
        if (tid < 256) cnt[tid] = ex;  // running offset per digit
        const uint64_t below = (1ull << lane) - 1;
        for (int64_t c0 = 0; c0 < m; c0 += UT) {
            const int64_t i = c0 + tid;
            const bool valid = i < m;
            const uint64_t v = valid ? a[i] : 0ull;
            const uint32_t dig = (uint32_t)(v >> shift) & 255u;
            uint64_t same = __ballot(valid);
            for (int bit = 0; bit < 8; ++bit) {
                const uint64_t bm = __ballot((dig >> bit) & 1u);
                same &= ((dig >> bit) & 1u) ? bm : ~bm;
            }
            for (int d = lane; d < 256; d += 64) wc[wave][d] = 0;
            __syncthreads();  // (also: cnt advanced by the previous chunk)
            if (valid && (same & below) == 0) wc[wave][dig] = (uint32_t)__popcll(same);
            __syncthreads();
            if (valid) {
                uint32_t o = cnt[dig] + (uint32_t)__popcll(same & below);
                for (int q = 0; q < wave; ++q) o += wc[q][dig];
                b[o] = v;
            }
            __syncthreads();
            if (tid < 256) {
                uint32_t s = 0;
                for (int q = 0; q < UT / 64; ++q) s += wc[q][tid];
                cnt[tid] += s;
            }
        }
        __syncthreads();
        uint64_t *tmp = a;
        a = b;
        b = tmp;
    }
    return a;
}

// the bucket's voxel offset: the sum of the earlier buckets' voxel counts, by a decoupled look-back over 64
// predecessors at a time (one wave; each lane one look-back word).  Publishes the bucket's own count first, its
// inclusive prefix last.  Waits only on lower part indices of the same frame, i.e. on workgroups dispatched before this
// one; every spin is bounded (hung: a bug, not a hang).  A look-back word is its own payload (status << 32 | count, one
// 8-byte sc1 store, read by sc1 loads that bypass the L1): relaxed agent-scope atomics, no fences (an acquire would
// invalidate the CU's L1 per poll and a release write back the XCD's L2 per store: MI355X_MICROARCH.md, ~1.7 us each).
__device__ __forceinline__ void look_back_publish(unsigned long long *fl, int64_t b, uint32_t nv)
{
    __hip_atomic_store(&fl[b], ((b == 0 ? 2ull : 1ull) << 32) | nv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long look_back_first(const unsigned long long *fl, int64_t b)
{
    const int64_t q = b - 1 - (threadIdx.x & 63);
    return q >= 0 ? __hip_atomic_load(&fl[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : (2ull << 32);
}
// Each path places publish and first where its own work hides them; first: this lane's word; spins: the polls
__device__ uint64_t look_back(unsigned long long *fl, int64_t b, uint32_t nv, unsigned long long first, bool &hung,
                              uint32_t &spins)
{
    const int lane = threadIdx.x & 63;
    uint64_t pre = 0;
    hung = false;
    int64_t top = b - 1;
    spins = 0;
    while (top >= 0) {
        const int64_t q = top - lane;
        const unsigned long long v = top == b - 1 && spins == 0 ? first
                                     : q >= 0 ? __hip_atomic_load(&fl[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                              : (2ull << 32);
        const uint32_t st = (uint32_t)(v >> 32);
        const uint64_t incl = __ballot(st == 2);
        const int k = incl ? __ffsll((unsigned long long)incl) - 1 : 63;
        const uint64_t upto = k == 63 ? ~0ull : ((2ull << k) - 1);
        if (__ballot(st == 0) & upto) {  // a predecessor before the first inclusive one has not published
            __builtin_amdgcn_s_sleep(2);
            if (++spins == (1u << 24)) {
                hung = true;
                break;
            }
            continue;
        }
        uint64_t s = lane <= k ? (v & 0xffffffffull) : 0ull;
        for (int o = 32; o >= 1; o >>= 1) s += (uint64_t)__shfl_xor((long long)s, o, 64);
        pre += s;
        if (incl) break;
        top -= 64;
    }
    if (lane == 0 && b > 0)
        __hip_atomic_store(&fl[b], (2ull << 32) | (pre + nv), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return pre;
}

#ifdef LIDAR_DIAG
__device__ int64_t g_vx_inject_bad = -1;  // the diagnostic library's failure injection (a bucket index)
#endif

// A bucket's outcome for nvox[f] (lane 0 of wave 0).  A failure — a look-back wait that timed out (hung: nvox -2) or a
// bucket table that is not a partition of [0, n) (bad: nvox -3), both bugs upstream, never expected — tags the frame's
// meta[4] with this call's epoch before it stores its code, and the frame's last bucket reads that tag after its own
// look-back has completed.  A failed bucket ends its wait before the predecessor it waited for publishes, and the last
// bucket's look-back needs that publication, so the tag is set before the last bucket reads it: a failure always wins
// over the frame's voxel count (the count alone, written by the last bucket, would look valid with ids and centroids at
// wrong offsets).
__device__ __forceinline__ void bucket_report(int32_t *nvox, uint32_t *m, int64_t f, int64_t b, int64_t nb,
                                              uint64_t total, bool hung, bool bad, uint32_t epoch)
{
    if (hung || bad) {
        const uint32_t code = bad ? 3u : 2u;
        __hip_atomic_store(&m[5], code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&m[4], epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        nvox[f] = -(int32_t)code;
    } else if (b == nb - 1) {
        nvox[f] = __hip_atomic_load(&m[4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == epoch
                      ? -(int32_t)__hip_atomic_load(&m[5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                      : (int32_t)total;
    }
}

// 34 KiB: four 512-thread workgroups per CU (at <= 64 VGPRs)
struct BucketLds {
    union {
        struct {
            uint32_t s[CAP];   // the counting sort's unordered runs: point indices (a run is one key)
            union {
                uint32_t cnt[KMAX];  // counting-sort counters, then per key its first sorted position | its
                                     // voxel's rank in the bucket << 16 (the radix path: its digit tables)
                struct {
                    uint32_t idx[CAP];     // the point indices in sorted order (written once cnt is dead;
                                           // the shifted sort: bit 31 marks a voxel's first point)
                    uint16_t vpos[CAP];    // the shifted sort: voxels up to each sorted position
                };
            };
        };
        uint64_t a[BITONIC_P];  // the bitonic path's pairs (over the above)
    };
    uint16_t vstart[CAP + 1];  // voxel v's first sorted position, then the voxels' end
    uint8_t rank[CAP];         // the dense sort: each pair's rank inside its key (load order)
    // the workgroup's few shared words
    unsigned long long prefix;           // the look-back's result
    alignas(16) uint32_t red[UT / 64];   // block_excl_scan's (read as two 16-byte words)
    unsigned long long vary;             // the radix sort's varying bits
    uint32_t rng[4];                     // the bucket's first pair and end, its key min and max
    uint32_t flag;                       // a run passed SEGMAX
};
static_assert(CAP < 65536, "packed first position | voxel rank");

// one bucket of one frame, as its phases see it
struct Bucket {
    const float *p;           // the frame's points
    const uint64_t *gp;       // the bucket's pairs, coarse-bin order
    unsigned long long *fl;   // the frame's look-back words
    int32_t *vf, *nf, *nvox;  // the frame's voxel ids and counts; the batch's voxel counts
    float *cf;                // the frame's centroids
    uint32_t *m;              // the frame's meta words
    int64_t n, f, b, nb, size;
    uint32_t okey, epoch;
    bool bad;
    BucketLds &L;
    uint32_t nvl = 0, spins = 0;  // its voxels (a point's rank nvl: outside every bin); the look-back's polls
};
using BucketClock = PhaseClock<8, kDiagPhases>;
constexpr int NP = CAP / UT;  // pairs per thread of the LDS sorts: pair i = tid + j UT is the thread's j-th
static_assert(CAP % UT == 0, "pairs per thread");
using Regs = uint32_t (&)[NP];  // a thread's pairs: one register each
using CRegs = const uint32_t (&)[NP];
template <class F>
__device__ __forceinline__ void for_pairs(int64_t size, F body)  // body(j, i) for the thread's pairs
{
#pragma unroll
    for (int j = 0; j < NP; ++j)
        if ((int)threadIdx.x + j * UT < size) body(j, (int)threadIdx.x + j * UT);
}

// phase 4: the bucket's voxel offset (wave 0's look-back from `first`; lane 0 reports).  Ends with a barrier.
__device__ __forceinline__ uint32_t bucket_offset(Bucket &c, unsigned long long first)
{
    const int tid = threadIdx.x;
    if (tid < 64) {
        bool hung;
        const uint64_t pre = look_back(c.fl, c.b, c.nvl, first, hung, c.spins);
        if (tid == 0) {
            c.L.prefix = pre;
            bucket_report(c.nvox, c.m, c.f, c.b, c.nb, pre + c.nvl, hung, c.bad, c.epoch);
        }
    }
    __syncthreads();
    return (uint32_t)c.L.prefix;
}

// voxel o of the frame: its centroid (the index-order sums over its count, one rounding each) and count
__device__ __forceinline__ void emit_voxel(const Bucket &c, int64_t o, float sx, float sy, float sz, int32_t count)
{
    const float d = (float)count;
    c.cf[3 * o] = __fdiv_rn(sx, d);
    c.cf[3 * o + 1] = __fdiv_rn(sy, d);
    c.cf[3 * o + 2] = __fdiv_rn(sz, d);
    c.nf[o] = count;
}

// phase 1: the pairs (kk: keys, id: point indices) and the range of the keys they hold in rng[2], rng[3] (not of their
// coarse bins: the first and last buckets' reach over the grid's empty margins).  Ends with a barrier.
__device__ __forceinline__ void load_pairs(Bucket &c, Regs kk, Regs id)
{
    const int tid = threadIdx.x;
    uint32_t kmin = 0xffffffffu, kmax = 0u;
    for (int j = 0; j < NP; ++j) {  // (every load in flight together: no guard around it)
        const uint64_t x = tid + j * UT < c.size ? c.gp[tid + j * UT] : 0ull;
        kk[j] = (uint32_t)(x >> 32);
        id[j] = (uint32_t)x;
    }
    for_pairs(c.size, [&](int j, int) {
        kmin = min(kmin, kk[j]);
        kmax = max(kmax, kk[j]);
    });
    kmin = lidar::wave_min_u32_dpp(kmin);
    kmax = ~lidar::wave_min_u32_dpp(~kmax);
    if ((tid & 63) == 0) {
        atomicMin(&c.L.rng[2], kmin);
        atomicMax(&c.L.rng[3], kmax);
    }
    __syncthreads();
}

// Local keys: (key - k0) >> sh, below KMAX.  sh = 0: one counter per key (the dense sort); sh > 0 (a sparse grid, the
// shifted sort): runs of a counter hold several keys, ordered by (key, index) as one 32-bit word (key's low sh bits <<
// ib | index) when that fits.
struct LocalKeys {
    uint64_t k0;
    int sh, ib;
    uint32_t nbin;  // counters in use (0: no counting sort)
    __device__ __forceinline__ uint32_t of(uint32_t key) const { return (key - (uint32_t)k0) >> sh; }
};
enum class Path { Dense, Shifted, Bitonic, Radix };
// phase 2, of a bucket within CAP: a counting sort when the words fit (sh == 0 || sh + ib <= 32) and no run of a local
// key passes SEGMAX (found by ranking every pair inside its local key: L.rank, counts left in L.cnt); else the bitonic
// network up to BITONIC_P pairs; else the radix sort.
__device__ __forceinline__ Path choose_path(Bucket &c, CRegs kk, LocalKeys &lk)
{
    const Path slow = c.size <= BITONIC_P ? Path::Bitonic : Path::Radix;
    BucketLds &L = c.L;
    static_assert(KMAX == 4096 && SEGMAX < 256, "12-bit local keys, 8-bit ranks");
    const uint64_t krange = c.size ? (uint64_t)c.L.rng[3] - c.L.rng[2] + 1 : 0;
    const int kb = krange > 1 ? 64 - __clzll((unsigned long long)(krange - 1)) : 0;
    lk.k0 = c.L.rng[2];
    lk.sh = max(0, kb - 12);
    lk.ib = 32 - __clz((uint32_t)max<int64_t>(c.n - 1, 1));
    const bool counting = lk.sh == 0 || lk.sh + lk.ib <= 32;
    lk.nbin = counting && krange ? (uint32_t)((krange - 1) >> lk.sh) + 1u : 0u;
    for (int64_t k = threadIdx.x; k < (int64_t)lk.nbin; k += UT) L.cnt[k] = 0;
    __syncthreads();
    if (!counting) return slow;
    for_pairs(c.size, [&](int j, int i) {
        const uint32_t r = atomicAdd(&L.cnt[lk.of(kk[j])], 1u);
        L.rank[i] = (uint8_t)r;
        if (r == SEGMAX) c.L.flag = 1;
    });
    __syncthreads();
    if (c.L.flag) return slow;  // (uniform)
    return lk.sh == 0 ? Path::Dense : Path::Shifted;
}

// phase 3, the two counting sorts: L.idx, L.vstart, sv (a pair's voxel rank; nvl: outside), c.nvl and lb0 are set
static_assert(CAP < 4096 && SEGMAX < 256, "packed run fields");
// counts -> starts: L.cnt[k] becomes the exclusive prefix of packed(k, count) over the counters (KMAX / UT consecutive
// ones per thread), seen(value, prefix) for what a path stores beside; returns the total
template <class Packed, class Seen>
__device__ __forceinline__ uint32_t scan_counts(Bucket &c, uint32_t nbin, Packed packed, Seen seen)
{
    constexpr int PT = KMAX / UT;
    const int tid = threadIdx.x;
    uint32_t cv[PT], sum = 0;
    for (int j = 0; j < PT; ++j) {
        const int64_t k = PT * tid + j;
        cv[j] = packed(k, k < (int64_t)nbin ? c.L.cnt[k] : 0u);
        sum += cv[j];
    }
    uint32_t all;
    uint32_t ex = block_excl_scan<UT>(sum, c.L.red, &all);
    for (int j = 0; j < PT; ++j) {
        const int64_t k = PT * tid + j;
        if (k < (int64_t)nbin) c.L.cnt[k] = ex;
        seen(cv[j], ex);
        ex += cv[j];
    }
    return all;
}

__device__ __forceinline__ void sort_dense(Bucket &c, const LocalKeys &lk, CRegs kk, CRegs id, Regs sv,
                                           unsigned long long &lb0, BucketClock &clk)
{
    BucketLds &L = c.L;
    const int tid = threadIdx.x;
    // one exclusive scan of (count | occupied << 16) over the keys gives every key its first sorted position and its
    // voxel's rank in the bucket (the outside key occupies no voxel), and the bucket's voxel count, published at once;
    // a voxel's first position goes to vstart (the outside key's run, the last: vstart[nvl])
    auto packed = [&](int64_t k, uint32_t x) {
        return x + (x != 0u && (uint32_t)(lk.k0 + k) != c.okey ? 0x10000u : 0u);
    };
    const uint32_t nvl = c.nvl = scan_counts(c, lk.nbin, packed, [&](uint32_t v, uint32_t ex) {
        if (v) L.vstart[ex >> 16] = (uint16_t)ex;
    }) >> 16;
    if (tid == 0) look_back_publish(c.fl, c.b, nvl);
    if (tid == 0 && c.L.rng[3] != c.okey) L.vstart[nvl] = (uint16_t)c.size;
    __syncthreads();
    clk.mark(3);
    // each key's run, unordered (sv: the point's voxel rank; the run: vstart[vp] .. vstart[vp + 1], or the bucket's end
    // for the outside key's run)
    for_pairs(c.size, [&](int j, int i) {
        const uint32_t e = L.cnt[lk.of(kk[j])];
        L.s[(e & 0xffffu) + L.rank[i]] = id[j];
        sv[j] = e >> 16;
    });
    __syncthreads();
    // (the earlier buckets publish their counts at the same point of their lives)
    if (tid < 64) lb0 = look_back_first(c.fl, c.b);
    // index order inside a run (< SEGMAX long): every element counts the smaller indices of its run; its index lands at
    // its sorted position
    for_pairs(c.size, [&](int j, int) {
        const uint32_t vp = sv[j], st = L.vstart[vp];
        const uint32_t en = vp == nvl ? (uint32_t)c.size : L.vstart[vp + 1];
        uint32_t r = 0;
        for (uint32_t x = st; x < en; ++x) r += L.s[x] < id[j] ? 1u : 0u;
        L.idx[st + r] = id[j];
    });
}

__device__ __forceinline__ void sort_shifted(Bucket &c, const LocalKeys &lk, Regs kk, CRegs id, Regs sv,
                                             unsigned long long &lb0, BucketClock &clk)
{
    BucketLds &L = c.L;
    const int tid = threadIdx.x, sh = lk.sh, ib = lk.ib;
    const int64_t size = c.size;
    // starts of the local keys' runs by an exclusive scan of the counts
    scan_counts(c, lk.nbin, [](int64_t, uint32_t x) { return x; }, [](uint32_t, uint32_t) {});
    __syncthreads();
    clk.mark(3);
    const uint32_t kmask = (1u << sh) - 1u;
    // each run, unordered (sv: its first position | its length << 12 | outside << 20; then a slot from the local key's
    // cursor for the point's word — (key's low sh bits, index) in order — which replaces its key in kk)
    for_pairs(size, [&](int j, int) {
        const uint32_t l = lk.of(kk[j]), st = L.cnt[l];
        const uint32_t en = l + 1 < lk.nbin ? L.cnt[l + 1] : (uint32_t)size;
        sv[j] = st | (en - st) << 12 | (kk[j] == c.okey ? 1u << 20 : 0u);
    });
    __syncthreads();
    for_pairs(size, [&](int j, int) {
        const uint32_t l = lk.of(kk[j]);
        kk[j] = ((kk[j] - (uint32_t)lk.k0) & kmask) << ib | id[j];
        L.s[atomicAdd(&L.cnt[l], 1u)] = kk[j];
    });
    __syncthreads();
    // (key, index) order inside a run: every element counts the smaller words of its run, and whether one of them holds
    // its key (else it is its voxel's first point; the outside key is no voxel)
    for_pairs(size, [&](int j, int) {
        const uint32_t st = sv[j] & 0xfffu, en = st + ((sv[j] >> 12) & 0xffu), wd = kk[j];
        const uint32_t hi = ib == 32 ? 0u : wd >> ib;
        uint32_t r = 0;
        bool dup = false;
        for (uint32_t x = st; x < en; ++x) {
            const uint32_t w2 = L.s[x];
            r += w2 < wd ? 1u : 0u;
            dup = dup || (w2 < wd && (ib == 32 ? 0u : w2 >> ib) == hi);
        }
        const bool out = (sv[j] >> 20) & 1u;
        L.idx[st + r] = id[j] | (!dup && !out ? 0x80000000u : 0u);
        sv[j] = (st + r) | (!dup ? 1u << 16 : 0u) | (out ? 1u << 17 : 0u);
    });
    __syncthreads();
    // voxel ranks: the voxels' first points up to each sorted position (NP consecutive positions per thread), the
    // bucket's count published at once
    uint32_t bits = 0, fc = 0;
    for (int k = 0; k < NP; ++k) {
        const int64_t o = NP * tid + k;
        const uint32_t fb = o < size ? L.idx[o] >> 31 : 0u;
        bits |= fb << k;
        fc += fb;
    }
    uint32_t nvl;
    uint32_t inc = block_excl_scan<UT>(fc, c.L.red, &nvl);
    for (int k = 0; k < NP; ++k) {
        const int64_t o = NP * tid + k;
        inc += (bits >> k) & 1u;
        if (o < size) L.vpos[o] = (uint16_t)inc;
    }
    c.nvl = nvl;
    if (tid == 0) look_back_publish(c.fl, c.b, nvl);
    __syncthreads();
    if (tid < 64) lb0 = look_back_first(c.fl, c.b);
    for_pairs(size, [&](int j, int) {
        const uint32_t o = sv[j] & 0xffffu;
        const bool first = (sv[j] >> 16) & 1u, out = (sv[j] >> 17) & 1u;
        const uint32_t vp = out ? nvl : (uint32_t)L.vpos[o] - 1u;
        if (first) L.vstart[vp] = (uint16_t)o;  // the outside key's first point ends the last voxel
        sv[j] = vp;
    });
    if (tid == 0 && c.L.rng[3] != c.okey) L.vstart[nvl] = (uint16_t)size;
}

// phase 5 after a counting sort: the points' voxel ids from registers (O: the bucket's voxel offset); then one thread
// per voxel: the sequential fp32 sums over its points in index order, their xyz gathered GB at a time (the frame's
// points are L2-resident since the keys launch), the centroid and count (consecutive threads: consecutive voxels)
__device__ __forceinline__ void emit_runs(const Bucket &c, uint32_t O, CRegs id, CRegs sv, BucketClock &clk)
{
    const BucketLds &L = c.L;
    const uint32_t nvl = c.nvl;
    for_pairs(c.size, [&](int j, int) { c.vf[id[j]] = sv[j] == nvl ? -1 : (int32_t)(O + sv[j]); });
    clk.mark(6);
    for (uint32_t vv = threadIdx.x; vv < nvl; vv += UT) {
        const int i0 = L.vstart[vv], i1 = L.vstart[vv + 1];
        float sx = 0.f, sy = 0.f, sz = 0.f;
        constexpr int GB = 8;  // one round trip for most voxels
        for (int e0 = i0; e0 < i1; e0 += GB) {
            float q[GB][3];
            for (int k = 0; k < GB; ++k) {
                const int64_t i = (e0 + k < i1 ? L.idx[e0 + k] : L.idx[i0]) & 0x7fffffffu;
                for (int a = 0; a < 3; ++a) q[k][a] = c.p[3 * i + a];
            }
            for (int k = 0; k < GB; ++k)
                if (e0 + k < i1) {
                    sx = __fadd_rn(sx, q[k][0]);
                    sy = __fadd_rn(sy, q[k][1]);
                    sz = __fadd_rn(sz, q[k][2]);
                }
        }
        emit_voxel(c, (int64_t)O + vv, sx, sy, sz, i1 - i0);
    }
}

// phase 3, a slow sort: bitonic network over the pairs in LDS (a key range past the counting sort, or a long run)
__device__ __forceinline__ const uint64_t *sort_bitonic(Bucket &c)
{
    BucketLds &L = c.L;
    const int tid = threadIdx.x;
    int64_t P = 1;
    while (P < c.size) P <<= 1;
    for (int64_t i = tid; i < P; i += UT) L.a[i] = i < c.size ? c.gp[i] : ~0ull;  // (reloaded; pads last)
    __syncthreads();
    for (int64_t k2 = 2; k2 <= P; k2 <<= 1)
        for (int64_t j = k2 >> 1; j > 0; j >>= 1) {
#pragma unroll 1
            for (int64_t i = tid; i < P; i += UT) {
                const int64_t l = i ^ j;
                if (l > i) {
                    const uint64_t x = L.a[i], y = L.a[l];
                    if ((x > y) == ((i & k2) == 0)) {
                        L.a[i] = y;
                        L.a[l] = x;
                    }
                }
            }
            __syncthreads();
        }
    return L.a;
}

// phases 4 and 5 after a slow sort (a thread: CH consecutive elements per chunk of CH UT)
__device__ __forceinline__ void emit_sorted(Bucket &c, const uint64_t *seq)
{
    constexpr int CH = 4;
    const int64_t size = c.size, t0 = CH * threadIdx.x;
    auto key_at = [&](int64_t i) { return (uint32_t)(seq[i] >> 32); };
    auto start_at = [&](int64_t i) { return key_at(i) != c.okey && (i == 0 || key_at(i) != key_at(i - 1)); };
    uint32_t all;
    for (int64_t c0 = t0; c0 - t0 < size; c0 += CH * UT) {
        uint32_t v = 0;
        for (int j = 0; j < CH; ++j) v += c0 + j < size && start_at(c0 + j) ? 1u : 0u;
        block_excl_scan<UT>(v, c.L.red, &all);
        c.nvl += all;
    }
    if (threadIdx.x == 0) look_back_publish(c.fl, c.b, c.nvl);
    const uint32_t O = bucket_offset(c, threadIdx.x < 64 ? look_back_first(c.fl, c.b) : 0ull);
    uint32_t carry = 0;
    for (int64_t c0 = t0; c0 - t0 < size; c0 += CH * UT) {
        bool st[CH];
        uint32_t v = 0;
        for (int j = 0; j < CH; ++j) {
            st[j] = c0 + j < size && start_at(c0 + j);
            v += st[j] ? 1u : 0u;
        }
        uint32_t r = O + carry + block_excl_scan<UT>(v, c.L.red, &all);  // voxels before this thread's elements
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            const int64_t i = c0 + j;
            if (i >= size) break;
            const uint32_t kk = key_at(i);
            r += st[j] ? 1u : 0u;
            c.vf[(uint32_t)seq[i]] = kk == c.okey ? -1 : (int32_t)(r - 1);
            if (st[j]) {  // this voxel's points in index order: the sequential fp32 sums
                float sx = 0.f, sy = 0.f, sz = 0.f;
                int64_t e = i;
                for (; e < size && key_at(e) == kk; ++e) {
                    const int64_t idx = (uint32_t)seq[e];
                    sx = __fadd_rn(sx, c.p[3 * idx]);
                    sy = __fadd_rn(sy, c.p[3 * idx + 1]);
                    sz = __fadd_rn(sz, c.p[3 * idx + 2]);
                }
                emit_voxel(c, r - 1, sx, sy, sz, (int32_t)(e - i));
            }
        }
        carry += all;
    }
}

// 1. load the pairs and find their key range; 2. choose a path; 3. sort; 4. look-back; 5. emit
__global__ __launch_bounds__(UT, 8) void vx_bucket_kernel(const float *__restrict__ xyz, int64_t n, Ws w,
                                                       int32_t *__restrict__ vid, float *__restrict__ cent,
                                                       int32_t *__restrict__ counts, int32_t *__restrict__ nvox,
                                                       int64_t batch, uint32_t epoch)
{
    const int64_t nb = n_buckets(n);
    int64_t f, b;
    if (!frame_part(batch, nb, f, b)) return;
    const int tid = threadIdx.x;
    BucketClock clk;
    clk.mark(0);
    // the bucket's pairs [bstart[b], bstart[b + 1]) (the bucket table), loaded beside the frame's meta words
    const uint32_t bs = tid < 2 ? w.bstart[(int64_t)f * (nb + 1) + b + tid] : 0u;
    uint32_t *m = w.meta + (int64_t)f * MW;
    if (!m[0] || m[3] == epoch) {
        if (b == 0 && tid == 0) nvox[f] = m[3] == epoch ? -2 : -1;
        return;  // every bucket of the frame returns: nothing waits on this frame's look-back words
    }
    __shared__ __attribute__((aligned(16))) BucketLds L;
    if (tid < 2) L.rng[tid] = bs;
    if (tid == 2) L.rng[2] = 0xffffffffu;  // [2], [3]: key min / max
    if (tid == 3) L.rng[3] = 0u;
    if (tid == 0) L.flag = 0;
    __syncthreads();
    clk.mark(1);
    // a bucket table that is not a partition of [0, n) is a bug upstream: the bucket sorts nothing (its count 0 still
    // goes out, so the frame's later buckets do not wait on it) and reports nvox -3
    bool bad = L.rng[0] > L.rng[1] || (int64_t)L.rng[1] > n;  // (uniform)
#ifdef LIDAR_DIAG
    bad = bad || b == g_vx_inject_bad;  // testing aid (lidar_debug_voxel_inject): this bucket's table is "bad"
#endif
    const int64_t p0 = bad ? 0 : L.rng[0], size = bad ? 0 : (int64_t)L.rng[1] - L.rng[0];
    const int64_t fn = (int64_t)f * n;
    Bucket c{xyz + fn * 3, w.pairs + fn + p0, reinterpret_cast<unsigned long long *>(w.flags + (int64_t)f * nb),
             vid + fn,     counts + fn,       nvox, cent + fn * 3, m, n, f, b, nb, size, m[1], epoch, bad, L};
    Path path = Path::Radix;  // (a bucket past CAP)
    if (size <= CAP) {
        uint32_t kk[NP], id[NP];  // the pairs' keys and point indices
        load_pairs(c, kk, id);
        LocalKeys lk;
        path = choose_path(c, kk, lk);
        clk.mark(2);
        if (path == Path::Dense || path == Path::Shifted) {  // (uniform)
            uint32_t sv[NP];  // the pairs' voxel ranks in the bucket
            unsigned long long lb0 = 0;
            if (path == Path::Dense) sort_dense(c, lk, kk, id, sv, lb0, clk);
            else sort_shifted(c, lk, kk, id, sv, lb0, clk);
            clk.mark(4);
            const uint32_t O = bucket_offset(c, lb0);  // (the earlier buckets have published: one pass)
            clk.mark(5);
            emit_runs(c, O, id, sv, clk);
        }
    }
    if (path == Path::Bitonic || path == Path::Radix) {  // (uniform)
        __syncthreads();  // the counting attempt's cnt reads are done: a and the digit tables overlay it
        const uint64_t *seq = path == Path::Bitonic
                                  ? sort_bitonic(c)
                                  : bucket_radix(const_cast<uint64_t *>(c.gp), w.scratch + fn + p0, size, L.cnt,
                                                 reinterpret_cast<uint32_t(*)[256]>(L.cnt + 256), L.red, &L.vary);
        __syncthreads();
        emit_sorted(c, seq);
    }
    clk.mark(7);
    clk.flush(c.nf + n - 16 * (b + 1), c.spins);  // 16 words per bucket into the scratch tail of the counts
}

}  // namespace

void lidar::vx::launch_buckets(const float *xyz, int64_t batch, int64_t n, const Ws &w, int32_t *voxel_id,
                               float *centroids, int32_t *counts, int32_t *nvox, uint32_t epoch, hipStream_t s)
{
    hipLaunchKernelGGL(vx_bucket_kernel, dim3(frame_grid(batch, n_buckets(n))), dim3(UT), 0, s, xyz, n, w, voxel_id,
                       centroids, counts, nvox, batch, epoch);
}

#ifdef LIDAR_DIAG
// testing aid (the diagnostic library only): the bucket launches that follow treat bucket `bucket` of every frame as
// having an inconsistent bucket table (-1: none), so the sticky failure report can be tested
LIDAR_EXPORT int lidar_debug_voxel_inject(int64_t bucket)
{
    const hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(g_vx_inject_bad), &bucket, sizeof(bucket));
    return e == hipSuccess ? LIDAR_OK : lidar::fail(LIDAR_EHIP, "lidar_debug_voxel_inject: hipMemcpyToSymbol");
}
#endif
