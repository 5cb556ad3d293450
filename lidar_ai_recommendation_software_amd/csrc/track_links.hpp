// track_links.hpp — what track.hip, track_events.hip, track_history.hip and track_routes.hip share: a frame's live row
// count, what a valid link (prev, gap) is, the zone predicate and the range checks of a (frames, cap) call.  No kernels
// here (the two that turn links into chains are in track_chain.hpp).
#pragma once
#include "tier_r.hpp"

namespace lidar {
namespace track {

constexpr int kMaxGap = 8;   // the largest frame distance of a link: lidar_track_stream_f64 takes max_gap <= 7 and
                             // links over 1 .. max_gap + 1 frames (a pass, and a profile span name, per distance)
constexpr int kMaxTab = 64;  // gates, and zones, at most: a bit of an int64 mask each, and a zone per lane of a wave

// K_t = min(max(k[t], 0), cap): the live rows of frame t
__device__ __forceinline__ int64_t clamp_k(const int64_t *k, int64_t t, int64_t cap)
{
    const int64_t v = k[t];
    return v < 0 ? 0 : (v < cap ? v : cap);
}

// The link guard: the source row index of the live row e = (t, j), -1 for an unlinked one; g: the link's frame
// distance.  Linked iff i = prev[e] >= 0 and 1 <= g <= kMaxGap and g <= t and i < K_(t-g): then 0 <= t - g and
// i < cap, so the source is inside the arrays whatever prev and gap hold.
__device__ __forceinline__ int64_t source_of(const int64_t *__restrict__ k, const int32_t *__restrict__ prev,
                                             const int32_t *__restrict__ gap, int64_t cap, int64_t t, int64_t e,
                                             int64_t &g)
{
    const int64_t i = prev[e];
    g = gap ? gap[e] : 1;
    if (i >= 0 && g >= 1 && g <= kMaxGap && g <= t && i < clamp_k(k, t - g, cap)) return (t - g) * cap + i;
    return -1;
}

// inside(z, p), half open: x0 <= p.x < x1 and y0 <= p.y < y1.  Every comparison with a NaN is false: a NaN position
// is inside no zone, and NaN bounds (a lane without a zone) hold no position.
__device__ __forceinline__ bool inside(double x0, double x1, double y0, double y1, double px, double py)
{
    return x0 <= px && px < x1 && y0 <= py && py < y1;
}

// The checks every (frames, cap) entry point starts with, under its own name; its own checks follow.
inline int check_frames(const std::string &f, bool pointers, int64_t frames, int64_t cap)
{
    REQUIRE(pointers, f + ": null pointer");
    REQUIRE(frames >= 0 && frames <= 65535, f + ": frames out of range");
    REQUIRE(cap >= 1, f + ": cap must be >= 1");
    REQUIRE(cap < 0x80000000ll && frames * cap < 0x80000000ll, f + ": frames * cap must be below 2^31");
    return LIDAR_OK;
}

}  // namespace track
}  // namespace lidar
