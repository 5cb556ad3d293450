// track_chain.hpp — what track_history.hip and track_routes.hip share beside track_links.hpp (which holds no kernels):
// the two launches that turn the links into chains.  next[row] is the heir of the row, the lowest row in (t, j) order
// of the frames >= carry that is linked to it, or kNone; a walk follows next[] from a chain's start.  The kernels sit
// in an unnamed namespace: each file that includes this header gets its own.
#pragma once
#include "track_links.hpp"

namespace {

constexpr int kB = 256;                // threads per workgroup
constexpr int32_t kNone = 0x7fffffff;  // above every row index: frames * cap < 2^31

// next[e] = kNone for e < nn, zero[e] = 0 for e < nz (the integer totals the walk adds to), in one launch.
__global__ __launch_bounds__(kB) void init_kernel(int32_t *__restrict__ next, int64_t nn, int64_t *__restrict__ zero,
                                                  int64_t nz)
{
    for (int64_t e = (int64_t)blockIdx.x * kB + threadIdx.x; e < nn + nz; e += (int64_t)gridDim.x * kB) {
        if (e < nn) next[e] = kNone;
        else zero[e - nn] = 0;
    }
}

// A thread per row of the frames >= carry; a linked row takes atomicMin(next[source], its own index): the minimum is
// the heir rule.  blockIdx.y = t - carry; blockIdx.x and gridDim.x stride over the frame's row tiles.
__global__ __launch_bounds__(kB) void claim_kernel(const int64_t *__restrict__ k, const int32_t *__restrict__ prev,
                                                   const int32_t *__restrict__ gap, int64_t cap, int64_t carry,
                                                   int32_t *__restrict__ next)
{
    using namespace lidar::track;
    const int64_t t = carry + blockIdx.y, K = clamp_k(k, t, cap);
    for (int64_t j = (int64_t)blockIdx.x * kB + threadIdx.x; j < K; j += (int64_t)gridDim.x * kB) {
        const int64_t e = t * cap + j;
        int64_t g;
        const int64_t a = source_of(k, prev, gap, cap, t, e, g);
        if (a >= 0) atomicMin(&next[a], (int32_t)e);
    }
}

// The grid of init_kernel over n elements.
inline unsigned init_blocks(int64_t n)
{
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + kB - 1) / kB, 4096));
}

// The row tiles of a frame: the x extent of claim_kernel's grid, and of a walk with a thread per row.
inline unsigned row_tiles(int64_t cap)
{
    return (unsigned)std::min<int64_t>((cap + kB - 1) / kB, 4096);
}

}  // namespace
