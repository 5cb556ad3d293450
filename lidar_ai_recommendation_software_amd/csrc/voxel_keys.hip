// voxel_keys.hip — the keys stage of the batched voxel downsampling: extents, keys, coarse-bin scatter. The design of
// both stages is told at the top of voxel_batch.hip.
#include "voxel_batch.hpp"
#include "voxel_grid.hpp"

namespace {
using namespace lidar::vx;
// An in-launch hand-off's wait: pass() loads a batch of self-tagged granules (all in flight together) and says whether
// every tag is this call's epoch; polled until it does, at most 2^22 times (false: the hung tag, nvox -2)
template <class Pass>
__device__ __forceinline__ bool poll_tags(Pass pass)
{
    for (uint32_t spins = 0; !pass();) {
        if (++spins == (1u << 22)) return false;
        __builtin_amdgcn_s_sleep(2);
    }
    return true;
}

// tile t of frame f: sums the frame's tile histograms (polling their granules until every tag is this call's), the
// exclusive scan over the coarse bins plus the counts of the tiles before it, the bucket table (tile 0), then its (key,
// index) pairs to their coarse bins.  kv: the tile's keys (thread tid: points t TILE + j KT + tid); off: NBIN words of
// LDS; red: KT / 64 words; clk: stamps 6 .. 8 of the keys launch's measuring build.
using KeysClock = PhaseClock<10, kDiagKeys>;
template <class Clock>
__device__ __forceinline__ void scatter_tile(const uint32_t (&kv)[PPT], int64_t f, int64_t t, int64_t n, int ntiles,
                                             int hs, uint32_t epoch, const Ws &w, uint32_t *off, uint32_t *red,
                                             Clock &clk)
{
    const int tid = threadIdx.x;
    // coarse bins BPT tid .. BPT tid + BPT - 1: frame totals and the counts of the tiles before this one
    uint32_t tot[BPT], pre[BPT], sum = 0;
    for (int j = 0; j < BPT; ++j) tot[j] = pre[j] = 0;
    const unsigned long long *hg = w.hgran + (int64_t)f * ntiles * (NBIN / 2) + (BPT / 2) * tid;
    bool hung = false;
    // four tiles' granules per pass, every load in flight together (one round trip per pass, not per tile)
    constexpr int UCH = 4;
    for (int u0 = 0; u0 < ntiles; u0 += UCH) {
        unsigned long long g2[UCH][BPT / 2];
        const bool came = poll_tags([&] {  // (a tile that never publishes is a bug, reported as nvox -2)
            bool ready = true;
            for (int uu = 0; uu < UCH; ++uu)
                for (int e = 0; e < BPT / 2; ++e) {
                    g2[uu][e] = u0 + uu < ntiles ? __hip_atomic_load(&hg[(int64_t)(u0 + uu) * (NBIN / 2) + e],
                                                                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                                 : ((unsigned long long)epoch << 32);
                }
            for (int uu = 0; uu < UCH; ++uu)
                for (int e = 0; e < BPT / 2; ++e) ready = ready && (uint32_t)(g2[uu][e] >> 32) == epoch;
            return ready;
        });
        hung = hung || !came;
        for (int uu = 0; uu < UCH; ++uu)
            for (int j = 0; j < BPT; ++j) {
                const uint32_t c = (uint32_t)(g2[uu][j >> 1] >> (16 * (j & 1))) & 0xffffu;  // 0 past ntiles
                tot[j] += c;
                pre[j] += u0 + uu < t ? c : 0u;
            }
    }
    if (hung) w.meta[f * MW + 3] = epoch;
    clk.mark(6);
    for (int j = 0; j < BPT; ++j) sum += tot[j];
    uint32_t all;
    uint32_t ex = block_excl_scan<KT>(sum, red, &all);
    uint32_t bsv[BPT];  // the frame-level start of each of this thread's bins
    for (int j = 0; j < BPT; ++j) {
        bsv[j] = ex;
        off[BPT * tid + j] = ex + pre[j];
        ex += tot[j];
    }
    __syncthreads();
    clk.mark(7);
    if (t == 0) {
        // the bucket table: bucket b = the bins whose start s has bk(s) = min(s nb / n, nb - 1) = b, so its first pair
        // is the start of the first bin with bk >= b; buckets past the last bin's bk start at n (empty), and bstart[nb]
        // = n.  The previous bin's start: off[] still holds the frame-level starts in this workgroup (t = 0: no earlier
        // tiles), read before the barrier below lets the scatter's atomics move them.
        const int64_t nb = n_buckets(n);
        const float inv = (float)nb / (float)n;
        auto bk = [&](uint32_t st) { return min<int64_t>((int64_t)((float)st * inv), nb - 1); };
        uint32_t *bst = w.bstart + (int64_t)f * (nb + 1);
        int64_t prev = tid == 0 ? -1 : bk(off[BPT * tid - 1]);
        for (int j = 0; j < BPT; ++j) {
            const int64_t cur = bk(bsv[j]);
            for (int64_t q = prev + 1; q <= cur; ++q) bst[q] = bsv[j];
            prev = cur;
        }
        if (tid == KT - 1)
            for (int64_t q = prev + 1; q <= nb; ++q) bst[q] = (uint32_t)n;
        __syncthreads();  // (uniform: t is the workgroup's)
    }
    clk.mark(8);
    uint64_t *pr = w.pairs + (int64_t)f * n;
    for (int j = 0; j < PPT; ++j) {
        const int64_t i = (int64_t)t * TILE + j * KT + tid;
        if (i < n) {
            const uint32_t pos = atomicAdd(&off[kv[j] >> hs], 1u);
            if (pos < (uint64_t)n) pr[pos] = ((uint64_t)kv[j] << 32) | (uint32_t)i;  // (hung: counts unknown)
        }
    }
}

constexpr int ETAB = lidar_vox::kTabEdges;  // edges per axis of the keys launch's LDS tables
using namespace lidar_vox;  // bin_of_c, bin_tab_c, bin_tab_search, ru_float

// tile t of a frame's n points p (thread tid: points t TILE + j KT + tid; 0 past the frame)
__device__ __forceinline__ void load_tile(const float *p, int64_t n, int64_t t, float (&q)[PPT][3])
{
    for (int j = 0; j < PPT; ++j) {
        const int64_t i = (int64_t)t * TILE + j * KT + threadIdx.x;
        for (int a = 0; a < 3; ++a) q[j][a] = i < n ? p[3 * i + a] : 0.f;
    }
}

// the tile's extent (min / max of ord() over its points in q) as six {epoch, value} granules gr[t * 6 ..]
template <typename Q>
__device__ __forceinline__ void publish_extent(const Q &q, int64_t n, int64_t t, unsigned long long *gr,
                                               uint32_t epoch, uint32_t (*red6)[6])
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t lo3[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi3[3] = {0u, 0u, 0u};
    for (int j = 0; j < PPT; ++j)
        if ((int64_t)t * TILE + j * KT + tid < n)
            for (int a = 0; a < 3; ++a) {
                lo3[a] = min(lo3[a], ord(q[j][a]));
                hi3[a] = max(hi3[a], ord(q[j][a]));
            }
    for (int a = 0; a < 3; ++a) {
        lo3[a] = lidar::wave_min_u32_dpp(lo3[a]);
        hi3[a] = ~lidar::wave_min_u32_dpp(~hi3[a]);
    }
    if (lane == 0)
        for (int a = 0; a < 3; ++a) {
            red6[wave][a] = lo3[a];
            red6[wave][3 + a] = hi3[a];
        }
    __syncthreads();
    if (tid < 6) {
        uint32_t v = red6[0][tid];
        for (int q2 = 1; q2 < KT / 64; ++q2) v = tid < 3 ? min(v, red6[q2][tid]) : max(v, red6[q2][tid]);
        __hip_atomic_store(&gr[t * 6 + tid], ((unsigned long long)epoch << 32) | v, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the extents of frames with more tiles than an XCD holds workgroups (the keys launch's poll then finds every granule
// already written): one launch more and the points read twice
__global__ __launch_bounds__(KT) void vx_extent_kernel(const float *__restrict__ xyz, int64_t n, Ws w, int ntiles,
                                                       int64_t batch, uint32_t epoch)
{
    int64_t f, t;
    if (!frame_part(batch, ntiles, f, t)) return;
    __shared__ uint32_t red6[KT / 64][6];
    const float *p = xyz + (int64_t)f * n * 3;
    float q[PPT][3];
    load_tile(p, n, t, q);
    publish_extent(q, n, t, w.gran + (int64_t)f * ntiles * 6, epoch, red6);
}

// the keys kv of the tile's points q on grid g (okey: a point outside every bin): in float against the LDS tables etab
// when the grid allows, else in float64
template <class Clock>
__device__ __forceinline__ void tile_keys(const lidar_vox::Grid &g, uint32_t okey, const float (&q)[PPT][3],
                                          float (*etab)[ETAB + 2], uint32_t (&kv)[PPT], Clock &clk)
{
    const int tid = threadIdx.x;
    // the float thresholds of every axis' edges in LDS when each axis has <= ETAB edges and the grid's span is a float
    // range (uniform); else every point runs lidar_vox::key in float64
    bool tab = true;
    int L[3];
    float s0[3], inv[3], lastf[3];
    for (int a = 0; a < 3; ++a) {
        const lidar_vox::FAxis fa = lidar_vox::faxis(g.ax[a], ETAB);
        tab = tab && fa.ok;
        L[a] = fa.L;
        s0[a] = fa.s0;
        inv[a] = fa.inv;
        lastf[a] = fa.lastf;
    }
    clk.mark(2);
    if (tab) {
        for (int a = 0; a < 3; ++a)
            for (int i = tid; i < L[a] + 2; i += KT)
                etab[a][i] = i == 0 ? -INFINITY : i > L[a] ? INFINITY : ru_float(lidar_vox::edge(g.ax[a], i - 1));
        __syncthreads();
    }
    clk.mark(3);
    const uint32_t ny = (uint32_t)g.ax[1].nb, nz = (uint32_t)g.ax[2].nb;
    if (tab) {
        // the table lookups of half the tile's points in flight together (branch-free), the rare guess off by more than
        // a bin fixed afterwards
        constexpr int H = PPT / 2;
        for (int h0 = 0; h0 < PPT; h0 += H) {
            int c[H][3];
            bool miss = false;
            for (int j = 0; j < H; ++j)
                for (int a = 0; a < 3; ++a) {
                    c[j][a] = bin_tab_c(etab[a] + 1, L[a], q[h0 + j][a], s0[a], inv[a]);
                    miss = miss || c[j][a] < 0;
                }
            if (miss)
                for (int j = 0; j < H; ++j)
                    for (int a = 0; a < 3; ++a)
                        if (c[j][a] < 0) c[j][a] = bin_tab_search(etab[a] + 1, L[a], q[h0 + j][a]);
            for (int j = 0; j < H; ++j) {
                const uint32_t bx = bin_of_c(c[j][0], q[h0 + j][0], lastf[0], L[0]);
                const uint32_t by = bin_of_c(c[j][1], q[h0 + j][1], lastf[1], L[1]);
                const uint32_t bz = bin_of_c(c[j][2], q[h0 + j][2], lastf[2], L[2]);
                // (bx ny + by) nz + bz < nx ny nz < 2^32: exact in 32 bits
                const bool out = bx == lidar_vox::kOutside || by == lidar_vox::kOutside || bz == lidar_vox::kOutside;
                kv[h0 + j] = out ? okey : (bx * ny + by) * nz + bz;
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            const uint32_t kk = lidar_vox::key(g, q[j][0], q[j][1], q[j][2]);
            kv[j] = kk == lidar_vox::kOutside ? okey : kk;  // sorts after every voxel's key
        }
    }
}

// tile t of frame f (xyz (batch, n, 3), ntiles tiles per frame, nb buckets): its extent published, the frame's polled,
// the grid at `voxel`, the tile's keys, its coarse-bin histogram published; then FUSED: scatter_tile from registers,
// else the keys to w.key for vx_scatter_kernel.  Tile 0 also writes the frame's meta and clears its look-back words.
template <bool FUSED>
__global__ __launch_bounds__(KT) void vx_keys_kernel(const float *__restrict__ xyz, int64_t n, double voxel, Ws w,
                                                     int ntiles, int64_t batch, uint32_t epoch,
                                                     int64_t nb VX_KEYS_DIAG(float *diag_cent))
{
    int64_t f, t;
    if (!frame_part(batch, ntiles, f, t)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    KeysClock clk;
    clk.mark(0);
    __shared__ uint32_t ext[6];
    __shared__ uint32_t red6[KT / 64][6];
    __shared__ uint32_t hist[NBIN];
    __shared__ float etab[3][ETAB + 2];  // -inf, the thresholds, +inf
    const float *p = xyz + (int64_t)f * n * 3;
    float q[PPT][3];  // the tile's points, loaded once: its extent, then its keys
    load_tile(p, n, t, q);
    for (int j = 0; j < BPT; ++j) hist[tid + j * KT] = 0;
    if (t == 0)  // the bucket launch's look-back words start at "nothing published"
        for (int64_t b = tid; b < nb; b += KT) w.flags[(int64_t)f * nb + b] = 0ull;
    {
        // the tile's extent (monotone bits: min / max of ord()), then the frame's from every tile's granules: {epoch,
        // value} in one 8-byte agent-scope store each, polled until every tag is this call's (self-contained: no fence;
        // MI355X_MICROARCH.md R2).  A tile waits only on tiles of its frame, which frame_part dispatches together, at
        // most kFuseTiles of them (an XCD holds 32 workgroups of this launch; larger frames run vx_extent_kernel
        // first); the spin is bounded (a frame whose tiles never all arrive sets the hung tag meta[3]: nvox -2).
        unsigned long long *gr = w.gran + (int64_t)f * ntiles * 6;
        publish_extent(q, n, t, gr, epoch, red6);
        clk.mark(1);
        if (wave == 0) {
            uint32_t m[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u};
            bool ok = true;
            for (int64_t c0 = 0; c0 < (int64_t)ntiles * 6; c0 += 60) {  // 10 tiles per pass, lane l: word l % 6
                const int64_t c = c0 + lane;
                const bool mine = lane < 60 && c < (int64_t)ntiles * 6;
                unsigned long long v = 0;
                ok = poll_tags([&] {
                    v = mine ? __hip_atomic_load(&gr[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
                    return __ballot(mine && (uint32_t)(v >> 32) != epoch) == 0;
                }) && ok;
                const int k = lane % 6;
                const uint32_t x = (uint32_t)v;
                for (int kk = 0; kk < 6; ++kk) {  // fold word kk over the lanes that hold it
                    uint32_t y = mine && k == kk ? x : (kk < 3 ? 0xffffffffu : 0u);
                    y = kk < 3 ? lidar::wave_min_u32_dpp(y) : ~lidar::wave_min_u32_dpp(~y);
                    m[kk] = kk < 3 ? min(m[kk], y) : max(m[kk], y);
                }
            }
            for (int kk = 0; kk < 6; ++kk)  // hung: NaN extent, the grid fails
                if (lane == kk) ext[kk] = ok ? m[kk] : ord(__builtin_nanf(""));
            if (!ok && lane == 0) w.meta[f * MW + 3] = epoch;  // reported as nvox -2
        }
    }
    __syncthreads();
    const double lo[3] = {unord(ext[0]), unord(ext[1]), unord(ext[2])};
    const double hi[3] = {unord(ext[3]), unord(ext[4]), unord(ext[5])};
    const lidar_vox::Grid g = lidar_vox::make_grid(lo, hi, voxel);
    uint32_t *m = w.meta + (int64_t)f * MW;
    const uint32_t okey = g.ok ? (uint32_t)g.keys : 0u;  // nx ny nz >= 1: one past the last voxel
    const int bits = g.ok ? 32 - __clz((int)okey) : 0;
    const int hs = max(0, bits - HB);
    if (t == 0 && tid == 0) {
        m[0] = g.ok ? 1u : 0u;
        m[1] = okey;
        m[2] = (uint32_t)hs;  // (m[3]: the hung tag, this call's epoch only when set by this call)
    }
    if (!g.ok) return;  // whole workgroup (uniform)
    uint32_t kv[PPT];
    tile_keys(g, okey, q, etab, kv, clk);
    for (int j = 0; j < PPT; ++j) {
        const int64_t i = (int64_t)t * TILE + j * KT + tid;
        if (i < n) atomicAdd(&hist[kv[j] >> hs], 1u);
        else kv[j] = 0u;
    }
    __syncthreads();
    clk.mark(4);
    // the tile's histogram as self-tagged granules (bins 2g, 2g + 1 in granule g; thread tid publishes the granules of
    // its own scatter bins BPT tid .. BPT tid + 3)
    unsigned long long *hg = w.hgran + ((int64_t)f * ntiles + t) * (NBIN / 2);
    for (int e = 0; e < BPT / 2; ++e) {
        const int gi = (BPT / 2) * tid + e;
        const unsigned long long v = ((unsigned long long)epoch << 32) | (hist[2 * gi + 1] << 16) | hist[2 * gi];
        __hip_atomic_store(&hg[gi], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if constexpr (!FUSED) {  // the scatter launch follows
        uint32_t *k = w.key + (int64_t)f * n;
        for (int j = 0; j < PPT; ++j) {
            const int64_t i = (int64_t)t * TILE + j * KT + tid;
            if (i < n) k[i] = kv[j];
        }
    } else {
        // every tile of the frame is resident (<= kFuseTiles, one XCD): scatter straight from registers
        __syncthreads();  // hist[] becomes the scatter's offsets
        clk.mark(5);
        scatter_tile(kv, f, t, n, ntiles, hs, epoch, w, hist, &red6[0][0], clk);
    }
    clk.mark(9);
#ifdef VX_DIAG_KEYS  // 12 words per tile into the tail rows of the frame's centroids
    clk.flush(reinterpret_cast<uint64_t *>(diag_cent + (f + 1) * n * 3) - 12 * (t + 1));
#endif
}

// the scatter of frames above kFuseTiles tiles (the keys launch wrote the keys)
__global__ __launch_bounds__(KT) void vx_scatter_kernel(int64_t n, Ws w, int ntiles, int64_t batch, uint32_t epoch)
{
    int64_t f, t;
    if (!frame_part(batch, ntiles, f, t)) return;
    const int tid = threadIdx.x;
    const uint32_t *m = w.meta + (int64_t)f * MW;
    if (!m[0]) return;
    const int hs = (int)m[2];
    __shared__ uint32_t off[NBIN];
    __shared__ uint32_t red[KT / 64];
    const uint32_t *k = w.key + (int64_t)f * n;
    uint32_t kv[PPT];
    for (int j = 0; j < PPT; ++j) {
        const int64_t i = (int64_t)t * TILE + j * KT + tid;
        kv[j] = i < n ? k[i] : 0u;
    }
    PhaseClock<10, false> none;
    scatter_tile(kv, f, t, n, ntiles, hs, epoch, w, off, red, none);
}

}  // namespace

// Frames of up to kFuseTiles tiles: keys and scatter in one launch (a frame's tiles all resident); larger ones: the
// extent launch, the keys launch that writes the keys, the scatter launch.
void lidar::vx::launch_keys(const float *xyz, int64_t batch, int64_t n, double voxel, const Ws &w, uint32_t epoch,
                            hipStream_t s VX_KEYS_DIAG(float *diag_cent))
{
    const int ntiles = n_tiles(n);
    const int64_t nb = n_buckets(n);
    const dim3 grid(frame_grid(batch, ntiles)), block(KT);
    const bool fused = ntiles <= kFuseTiles;
    if (!fused) hipLaunchKernelGGL(vx_extent_kernel, grid, block, 0, s, xyz, n, w, ntiles, batch, epoch);
    const auto keys = fused ? vx_keys_kernel<true> : vx_keys_kernel<false>;
    hipLaunchKernelGGL(keys, grid, block, 0, s, xyz, n, voxel, w, ntiles, batch, epoch, nb VX_KEYS_DIAG(diag_cent));
    if (!fused) hipLaunchKernelGGL(vx_scatter_kernel, grid, block, 0, s, n, w, ntiles, batch, epoch);
}
