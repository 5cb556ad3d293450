// sa_shapes.hpp — the fused SetAbstraction shapes, listed once, and the host code the fused
// entry points share (sa_mlp16.hip, sa_mlp_x3.hip): argument checks, launch geometry, packer pieces.
// Host code only: no kernel reads anything from here.
#pragma once
#include <string>

#include "common.hpp"

// The shapes the fused kernels are built for: X(C1, C2, C3, NS, XYZ, LEAN).
//   XYZ   a level without features (layer 1 on the xyz offsets inside the kernel); else a feature
//         level (layer 1 per point / per centre, layer1_per_point)
//   LEAN  the fp32-contract x3 path runs sa_x3_lean_kernel (the wide feature levels: SA2, MSG's
//         128-sample branch)
// lidar_sa_group_mlp16_f32 and lidar_sa_group_mlp_x3_f32 take every entry, lidar_sa_group_mlp_x1_f32
// the xyz entries as mode 0 and the feature entries as mode 2, lidar_sa_group_mlp_bq_f32 the xyz
// entries.  The library cannot be asked for this list without an ABI change, so pointnet2.py's
// MLP16_SHAPES repeats it as (XYZ, C1, C2, C3, NS): an entry added here is added there.
#define LIDAR_SA_SHAPES(X)             \
    X(64, 64, 128, 32, true, false)    \
    X(32, 32, 64, 16, true, false)     \
    X(128, 128, 256, 64, false, true)  \
    X(128, 128, 256, 128, false, true) \
    X(64, 64, 128, 32, false, false)   \
    X(64, 96, 128, 128, true, false)

namespace lidar_sa {

// the checks every fused entry point makes on its arguments, reported under its own name `fn`
inline int check_args(const char *fn, bool pointers, bool sizes, bool p_stride, int64_t out_offset, int32_t c3,
                      int64_t out_stride)
{
    REQUIRE(pointers, std::string(fn) + ": null pointer");
    REQUIRE(sizes, std::string(fn) + ": bad sizes");
    REQUIRE(p_stride, std::string(fn) + ": bad p_stride");
    REQUIRE(out_offset >= 0 && out_offset + c3 <= out_stride, std::string(fn) + ": output columns exceed out_stride");
    return LIDAR_OK;
}

// one wave per centre, `wpg` waves per workgroup
inline int launch_geometry(const char *fn, int64_t batch, int64_t m, int wpg, int64_t &total, int64_t &blocks)
{
    total = batch * m;
    blocks = (total + wpg - 1) / wpg;
    REQUIRE(blocks <= 0x7fffffff, std::string(fn) + ": too many centres");
    return LIDAR_OK;
}

inline int check_pack_widths(const char *fn, int32_t c1, int32_t c2, int32_t c3)
{
    REQUIRE(c1 % 32 == 0 && c2 % 32 == 0 && c3 % 32 == 0 && c1 > 0 && c2 > 0 && c3 > 0,
            std::string(fn) + ": widths must be positive multiples of 32");
    return LIDAR_OK;
}

// layer 1 of an xyz level as the 16x16x4 MFMA's A operand: lane l of tile t holds
// round(W1[l >> 4][16 t + (l & 15)]), lane group 3 zero
template <class Round>
inline float *write_w1_lanes(float *o, const float *w1, int c1, Round round)
{
    for (int t = 0; t < c1 / 16; ++t)
        for (int l = 0; l < 64; ++l) {
            const int qq = l >> 4;
            *o++ = qq < 3 ? round(w1[(int64_t)qq * c1 + 16 * t + (l & 15)]) : 0.0f;
        }
    return o;
}
inline float *write_w1_lanes(float *o, const float *w1, int c1)
{
    return write_w1_lanes(o, w1, c1, [](float v) { return v; });
}

// b1 b2 b3
inline float *write_biases(float *o, const float *b1, int c1, const float *b2, int c2, const float *b3, int c3)
{
    for (int i = 0; i < c1; ++i) *o++ = b1[i];
    for (int i = 0; i < c2; ++i) *o++ = b2[i];
    for (int i = 0; i < c3; ++i) *o++ = b3[i];
    return o;
}

// a (cin, cout) layer in the 16x16x32 fragment order: chunk c = output tiles (2c, 2c+1); 16-bit
// element j of lane l, half h, tile t, k-step s is conv(W[in(s, l >> 4, j)][16(2c+t) + (l & 15)], h),
// in(s, g, j) = 32 s + 16 (j >> 2) + 4 g + (j & 3)
template <int HALVES, class Conv>
inline uint16_t *write_fragments(uint16_t *u, const float *w, int cin, int cout, Conv conv)
{
    for (int c = 0; c < cout / 32; ++c)
        for (int s = 0; s < cin / 32; ++s)
            for (int t = 0; t < 2; ++t)
                for (int h = 0; h < HALVES; ++h)
                    for (int l = 0; l < 64; ++l)
                        for (int j = 0; j < 8; ++j) {
                            const int in = 32 * s + 16 * (j >> 2) + 4 * (l >> 4) + (j & 3);
                            *u++ = conv(w[(int64_t)in * cout + 16 * (2 * c + t) + (l & 15)], h);
                        }
    return u;
}

}  // namespace lidar_sa
