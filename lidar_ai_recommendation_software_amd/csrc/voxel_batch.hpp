// voxel_batch.hpp — what the two stages of the batched voxel downsampling share (voxel_keys.hip, voxel_bucket.hip) and
// their host launchers.  The design is told once, at the top of voxel_batch.hip.
#pragma once
#include "common.hpp"

namespace lidar {
namespace vx {
constexpr int KT = 1024;           // keys / scatter threads
constexpr int TILE = 8192;         // points per keys / scatter workgroup (one round of the chip at B = 32)
constexpr int PPT = TILE / KT;     // points per keys / scatter thread
constexpr int kFuseTiles = 16;     // frames of up to this many tiles take their extent inside the keys launch
constexpr int HB = 12;             // coarse-bin bits of the key range
constexpr int NBIN = 1 << HB;      // coarse bins per frame
constexpr int BPT = NBIN / KT;     // coarse bins per scatter thread (its scan)
constexpr int UT = 512;            // bucket threads
constexpr int CAP = 2560;          // pairs a bucket sorts in LDS
constexpr int BITONIC_P = 2048;    // the LDS bitonic fallback's array (a power of two; larger buckets
                                   // sort in global memory: at P = 4 096 the LDS network is the slower)
constexpr int KMAX = 4096;         // local key range of the LDS counting sort
constexpr int SEGMAX = 128;        // longest equal-key run the counting sort orders by index itself
constexpr int BUCKET = 2048;       // target points per bucket (32 x 65 536 points: 1 024 buckets, one round of
                                   // four workgroups per CU)
constexpr int MW = 8;              // meta words per frame: [0] grid ok, [1] outside key, [2] hs, [3] hung tag
                                   // (keys / scatter), [4] the bucket launch's failure tag, [5] its nvox code
static_assert(NBIN % KT == 0 && NBIN % UT == 0, "bins per thread");

__device__ __forceinline__ uint32_t ord(float f)  // monotone float -> u32
{
    const uint32_t u = __float_as_uint(f);
    return u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u);
}
__device__ __forceinline__ float unord(uint32_t u) { return __uint_as_float(u ^ (((u >> 31) - 1u) | 0x80000000u)); }

struct Ws {  // per-batch workspace, every array frame-major
    unsigned long long *gran;  // [F][T][6] the tiles' extents: epoch << 32 | monotone bits (self-tagged granules)
    uint32_t *meta;    // [F][MW] ([3]: the call's epoch when a hand-off timed out)
    uint32_t *key;     // [F][n]
    unsigned long long *hgran;  // [F][T][NBIN / 2] tile histograms: epoch << 32 | count(2g + 1) << 16 | count(2g)
    uint32_t *bstart;  // [F][NB + 1] the buckets' first pairs (bstart[NB] = n)
    uint64_t *pairs;   // [F][n] (key << 32 | index), coarse-bin order
    uint64_t *scratch; // [F][n] the global sort's other buffer
    uint64_t *flags;   // [F][NB] look-back words: status << 32 | count
};

__host__ __device__ __forceinline__ int64_t n_buckets(int64_t n) { return (n + BUCKET - 1) / BUCKET; }
__host__ __forceinline__ int n_tiles(int64_t n) { return (int)((n + TILE - 1) / TILE); }
// (frame, part) of a 1-D grid of `parts` workgroups per frame.  XCD-affine (batch >= 8): workgroup L runs on XCD L % 8,
// which takes frames L % 8, L % 8 + 8, ... and their parts in order, so a frame's scattered writes and gathers stay in
// one L2 and its part p - 1 is dispatched before part p (the bucket look-back waits only on that); fewer frames: plain
// frame-major order.  false: padding.
__device__ __forceinline__ bool frame_part(int64_t batch, int64_t parts, int64_t &f, int64_t &p)
{
    const int64_t L = blockIdx.x;
    if (batch >= 8) {
        const int64_t x = L & 7, j = L >> 3;
        f = x + 8 * (j / parts);
        p = j % parts;
    } else {
        f = L / parts;
        p = L % parts;
    }
    return f < batch;
}
__host__ __forceinline__ unsigned frame_grid(int64_t batch, int64_t parts)
{
    return (unsigned)(batch >= 8 ? 8 * ((batch + 7) / 8) * parts : batch * parts);
}

// block-wide exclusive scan of one value per thread (T threads); returns the exclusive prefix and the total through
// *tot.  Uses red[T / 64], read after the function's last barrier: a caller that writes red[] again puts a barrier of
// its own first (as this function's start does).
template <int T>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *red, uint32_t *tot)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t inc = (uint32_t)wave_incl_scan_i32((int)v);
    __syncthreads();  // red[] free (a previous scan's readers are done)
    if (lane == 63) red[wave] = inc;
    __syncthreads();
    uint32_t pre = 0, all = 0;
#pragma unroll
    for (int w = 0; w < T / 64; ++w) {
        pre += w < wave ? red[w] : 0u;
        all += red[w];
    }
    *tot = all;
    return pre + inc - v;
}

// The phase stamps of the measuring builds (-DVX_DIAG_KEYS: tools/micro/voxel_keys_phases.py; -DVX_DIAG_PHASES:
// voxel_phases.py): mark(k) takes the shader and 100 MHz clocks as stamp k, flush() writes thread 0's stamps for the
// tool.  ON = false, every other build: an empty type.  VX_KEYS_DIAG: the keys launch's extra argument, that build's.
#ifdef VX_DIAG_KEYS
constexpr bool kDiagKeys = true;
#define VX_KEYS_DIAG(...) , __VA_ARGS__
#else
constexpr bool kDiagKeys = false;
#define VX_KEYS_DIAG(...)
#endif
#ifdef VX_DIAG_PHASES
constexpr bool kDiagPhases = true;
#else
constexpr bool kDiagPhases = false;
#endif
template <int N, bool ON>
struct PhaseClock {
    __device__ __forceinline__ void mark(int) {}
    template <class... A> __device__ __forceinline__ void flush(A...) const {}
};
template <int N>
struct PhaseClock<N, true> {
    uint64_t clk[N] = {}, real[N] = {};
    __device__ __forceinline__ void mark(int k)
    {
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(clk[k])::"memory");
        asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(real[k])::"memory");
    }
    __device__ __forceinline__ void flush(uint64_t *d) const  // N stamps, the first and last realtime words
    {
        if (threadIdx.x != 0) return;
        for (int k = 0; k < N; ++k) d[k] = clk[k];
        d[N] = real[0], d[N + 1] = real[N - 1];
    }
    // the N - 1 intervals in cycles, one word of the caller's, the N realtime words mod 2^31
    __device__ __forceinline__ void flush(int32_t *d, uint32_t extra) const
    {
        for (int k = 0; k < N && threadIdx.x == 0; ++k) {
            d[k] = k + 1 < N ? (int32_t)(clk[k + 1] - clk[k]) : (int32_t)extra;
            d[N + k] = (int32_t)(real[k] & 0x7fffffff);
        }
    }
};

// the two stages' launches on stream s (voxel_keys.hip, voxel_bucket.hip; diag_cent: the centroids output)
void launch_keys(const float *xyz, int64_t batch, int64_t n, double voxel, const Ws &w, uint32_t epoch,
                 hipStream_t s VX_KEYS_DIAG(float *diag_cent));
void launch_buckets(const float *xyz, int64_t batch, int64_t n, const Ws &w, int32_t *voxel_id, float *centroids,
                    int32_t *counts, int32_t *nvox, uint32_t epoch, hipStream_t s);
}  // namespace vx
}  // namespace lidar
