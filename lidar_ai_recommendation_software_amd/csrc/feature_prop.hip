// feature_prop.hip — the PointNet++ decoder's operators (feature propagation):
//
//   three_nn           per fine ("unknown") point the three nearest coarse ("known") points of its
//                      frame in lexicographic (distance, index) order, exact fp32 distances, and the
//                      inverse-distance weights of pointnet2's PointnetFPModule
//   three_interpolate  out row = [w0 f[i0] + w1 f[i1] + w2 f[i2] | skip row | 0-pad], written straight
//                      as the padded A operand of the dense GEMMs (rows past batch*n zeroed, the
//                      convention of lidar_sa_group_rows_f32)
//   row_argmax         the per-point class of the head's logits (np.argmax: lowest index on ties, a
//                      NaN counts as the maximum)
//
// Every float operation rounds once (-ffp-contract=off; the products and sums below are written with
// the _rn intrinsics), so the three operators are reproducible bit for bit in numpy float32.
#include "common.hpp"

namespace {

constexpr int NT = 256;      // threads per block (four waves)
constexpr int NN_CH = 2048;  // known points staged in LDS per chunk (float4 each: 32 KiB)
typedef float f32x2 __attribute__((ext_vector_type(2)));

// One thread owns U unknown points (coordinates and the nine best-slot values in VGPRs); the block
// walks the frame's known points in ascending chunks of NN_CH staged in LDS as float4.  Every lane
// of a wave reads the same LDS address (a broadcast read, no bank conflict) and each read
// feeds all U unknowns: the distance (8 operations per pair, two unknowns per packed VALU
// instruction) and one compare against the third-best slot; the three-way insertion sits behind
// one guard over the thread's U compares (a wave skips it when no lane improves any unknown).
// A chunk's tail up to a multiple of four is filled with NaN coordinates: a NaN distance never
// wins, so the unrolled loop needs no remainder.  Measured against the same loop with one guard
// per unknown, with unpacked distances, and with the known points read through wave-uniform
// scalar loads instead of LDS: this form won.
template <int U>
__global__ __launch_bounds__(NT) void three_nn_kernel(const float *__restrict__ unknown,
                                                      const float *__restrict__ known, int64_t n, int64_t m,
                                                      int64_t blocks_per_frame, float *__restrict__ dist2,
                                                      int32_t *__restrict__ idx, float *__restrict__ weight)
{
    __shared__ float4 s[NN_CH];
    const int t = threadIdx.x;
    const int64_t frame = (int64_t)blockIdx.x / blocks_per_frame;
    const int64_t p0 = ((int64_t)blockIdx.x % blocks_per_frame) * (NT * U) + t;
    const float *kf = known + frame * m * 3;

    float ux[U], uy[U], uz[U], b0[U], b1[U], b2[U];
    int32_t i0[U], i1[U], i2[U];
    const float inf = __builtin_inff();
#pragma unroll
    for (int u = 0; u < U; ++u) {
        int64_t p = p0 + (int64_t)u * NT;
        p = p < n ? p : n - 1;  // the tail threads repeat the frame's last point and store nothing
        const float *q = unknown + (frame * n + p) * 3;
        ux[u] = q[0], uy[u] = q[1], uz[u] = q[2];
        b0[u] = b1[u] = b2[u] = inf;
        i0[u] = i1[u] = i2[u] = 0;
    }

    for (int64_t c0 = 0; c0 < m; c0 += NN_CH) {  // ascending: the tie rule holds across chunks
        const int cnt = (int)(m - c0 < NN_CH ? m - c0 : NN_CH);
        const int cnt4 = (cnt + 3) & ~3;
        const float qnan = __builtin_nanf("");
        __syncthreads();  // the previous chunk has been read by every wave
        for (int i = t; i < cnt4; i += NT) {
            float4 v = make_float4(qnan, qnan, qnan, 0.f);
            if (i < cnt) {
                const float *q = kf + (c0 + i) * 3;
                v = make_float4(q[0], q[1], q[2], 0.f);
            }
            s[i] = v;
        }
        __syncthreads();
        const int32_t jbase = (int32_t)c0;
        for (int i = 0; i < cnt4; i += 4) {
            const float4 v4[4] = {s[i], s[i + 1], s[i + 2], s[i + 3]};  // four reads in flight before the first use
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float4 v = v4[k];
                const int32_t j = jbase + i + k;
                // lidar::dist2f for two unknowns at a time (v_pk_add_f32 / v_pk_mul_f32: the same
                // roundings, two lanes of work per VALU issue)
                float dd[U];
#pragma unroll
                for (int u = 0; u < U; u += 2) {
                    const f32x2 dx = f32x2{ux[u], ux[u + 1]} - v.x, dy = f32x2{uy[u], uy[u + 1]} - v.y,
                                dz = f32x2{uz[u], uz[u + 1]} - v.z;
                    const f32x2 d2 = (dx * dx + dy * dy) + dz * dz;
                    dd[u] = d2.x, dd[u + 1] = d2.y;
                }
                // one guard for the thread's U unknowns: most candidates lose to every third-best slot, and
                // the wave then branches once per known point instead of U times
                bool any = false;
#pragma unroll
                for (int u = 0; u < U; ++u) any |= dd[u] < b2[u];
                if (!any) continue;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const float d = dd[u];
                    if (d < b2[u]) {
                        if (d < b1[u]) {
                            b2[u] = b1[u], i2[u] = i1[u];
                            if (d < b0[u]) {
                                b1[u] = b0[u], i1[u] = i0[u];
                                b0[u] = d, i0[u] = j;
                            } else {
                                b1[u] = d, i1[u] = j;
                            }
                        } else {
                            b2[u] = d, i2[u] = j;
                        }
                    }
                }
            }
        }
    }

#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t p = p0 + (int64_t)u * NT;
        if (p >= n) continue;
        const int64_t o = (frame * n + p) * 3;
        dist2[o] = b0[u], dist2[o + 1] = b1[u], dist2[o + 2] = b2[u];
        idx[o] = i0[u], idx[o + 1] = i1[u], idx[o + 2] = i2[u];
        if (weight) {
            // an unfilled slot holds +inf: 1 / (inf + 1e-8) = 0 exactly; all three unfilled: 0 / 0 = NaN
            // sqrtf and / are the correctly rounded sequences under the build's flags (scaled v_sqrt with
            // its fix-up, v_div_scale / v_div_fmas / v_div_fixup): numpy float32 reproduces them bit for bit
            const float r0 = 1.0f / __fadd_rn(sqrtf(b0[u]), 1e-8f);
            const float r1 = 1.0f / __fadd_rn(sqrtf(b1[u]), 1e-8f);
            const float r2 = 1.0f / __fadd_rn(sqrtf(b2[u]), 1e-8f);
            const float sum = __fadd_rn(__fadd_rn(r0, r1), r2);
            weight[o] = r0 / sum, weight[o + 1] = r1 / sum, weight[o + 2] = r2 / sum;
        }
    }
}

__device__ __forceinline__ float mix3(float w0, float w1, float w2, float a, float b, float c)
{
    return __fadd_rn(__fadd_rn(__fmul_rn(w0, a), __fmul_rn(w1, b)), __fmul_rn(w2, c));
}

// One thread per (output row, 4-column chunk): a row's chunks are adjacent lanes (coalesced float4
// stores; the three gathered rows and the skip row are read 16 B per lane when vk / vs say their
// strides and bases allow it).  Bound by HBM: per row 3 c2 + c1 floats read, ldo written.
__global__ __launch_bounds__(NT) void three_interpolate_kernel(const float *__restrict__ kf, int64_t ldk, int c2,
                                                               const int32_t *__restrict__ idx,
                                                               const float *__restrict__ weight,
                                                               const float *__restrict__ skip, int64_t lds, int c1,
                                                               int64_t n, int64_t m, int64_t live, int64_t rows,
                                                               float *__restrict__ out, int64_t ldo, int vk, int vs)
{
    const int64_t cpr = ldo / 4;
    const int64_t t = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (t >= rows * cpr) return;
    const int64_t r = t / cpr;
    const int c0 = (int)(t % cpr) * 4;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (r < live) {
        if (c0 < c2) {
            const int64_t f = (r / n) * m;
            const float w0 = weight[r * 3], w1 = weight[r * 3 + 1], w2 = weight[r * 3 + 2];
            const float *a = kf + (f + idx[r * 3]) * ldk, *b = kf + (f + idx[r * 3 + 1]) * ldk,
                        *c = kf + (f + idx[r * 3 + 2]) * ldk;
            if (vk && c0 + 4 <= c2) {
                const float4 x = *reinterpret_cast<const float4 *>(a + c0);
                const float4 y = *reinterpret_cast<const float4 *>(b + c0);
                const float4 z = *reinterpret_cast<const float4 *>(c + c0);
                v[0] = mix3(w0, w1, w2, x.x, y.x, z.x), v[1] = mix3(w0, w1, w2, x.y, y.y, z.y);
                v[2] = mix3(w0, w1, w2, x.z, y.z, z.z), v[3] = mix3(w0, w1, w2, x.w, y.w, z.w);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (c0 + j < c2) v[j] = mix3(w0, w1, w2, a[c0 + j], b[c0 + j], c[c0 + j]);
            }
        }
        if (c0 + 4 > c2 && c0 < c2 + c1) {
            const float *sr = skip + r * lds - c2;  // column c of the output is skip column c - c2
            if (vs && c0 >= c2 && c0 + 4 <= c2 + c1) {
                const float4 x = *reinterpret_cast<const float4 *>(sr + c0);
                v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (c0 + j >= c2 && c0 + j < c2 + c1) v[j] = sr[c0 + j];
            }
        }
    }
    *reinterpret_cast<float4 *>(out + r * ldo + c0) = make_float4(v[0], v[1], v[2], v[3]);
}

// one thread per row; np.argmax: the first maximum, and a NaN (the first one) counts as the maximum
__global__ __launch_bounds__(NT) void row_argmax_kernel(const float *__restrict__ x, int64_t rows, int64_t ldx, int c,
                                                        int32_t *__restrict__ out)
{
    const int64_t r = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (r >= rows) return;
    const float *p = x + r * ldx;
    float best = p[0];
    int32_t bi = 0;
    for (int j = 1; j < c && best == best; ++j) {
        const float v = p[j];
        if (v > best || v != v) best = v, bi = j;
    }
    out[r] = bi;
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

LIDAR_EXPORT int lidar_three_nn_f32(lidar_handle *h, const float *unknown, const float *known, int64_t batch,
                                    int64_t n, int64_t m, float *dist2, int32_t *idx, float *weight, void *stream)
{
    REQUIRE(h, "lidar_three_nn_f32: null handle");
    REQUIRE(unknown && known && dist2 && idx, "lidar_three_nn_f32: null pointer");
    REQUIRE(batch >= 0 && n >= 1 && m >= 1 && m <= 0x7fffffff, "lidar_three_nn_f32: bad shape (n >= 1, 1 <= m < 2^31)");
    if (batch == 0) return LIDAR_OK;
    // four unknowns per thread once that still leaves two blocks per CU, else two (more, smaller blocks)
    const int u = batch * n >= (int64_t)1 << 19 ? 4 : 2;
    const int64_t bpf = (n + NT * u - 1) / (NT * u);
    REQUIRE(batch <= 0x7fffffff / bpf, "lidar_three_nn_f32: too many points");
    ON_DEVICE(h->device);
    lidar::Span span(h, "three_nn", static_cast<hipStream_t>(stream));
    const dim3 grid((unsigned)(batch * bpf));
    if (u == 4)
        hipLaunchKernelGGL(three_nn_kernel<4>, grid, dim3(NT), 0, static_cast<hipStream_t>(stream), unknown, known, n,
                           m, bpf, dist2, idx, weight);
    else
        hipLaunchKernelGGL(three_nn_kernel<2>, grid, dim3(NT), 0, static_cast<hipStream_t>(stream), unknown, known, n,
                           m, bpf, dist2, idx, weight);
    LAUNCH_CHECK();
    return LIDAR_OK;
}

LIDAR_EXPORT int lidar_three_interpolate_f32(lidar_handle *h, const float *known_feat, int64_t ldk, int32_t c2,
                                             const int32_t *idx, const float *weight, const float *skip, int64_t lds,
                                             int32_t c1, int64_t batch, int64_t n, int64_t m, float *out, int64_t rows,
                                             int64_t ldo, void *stream)
{
    REQUIRE(h, "lidar_three_interpolate_f32: null handle");
    REQUIRE(known_feat && idx && weight && out, "lidar_three_interpolate_f32: null pointer");
    REQUIRE(batch >= 0 && n >= 1 && m >= 1 && c2 >= 1 && ldk >= c2, "lidar_three_interpolate_f32: bad shape");
    REQUIRE(c1 >= 0 && (c1 == 0 || (skip && lds >= c1)), "lidar_three_interpolate_f32: bad skip operand");
    REQUIRE(ldo % 4 == 0 && ldo >= (int64_t)c1 + c2, "lidar_three_interpolate_f32: ldo must be a multiple of 4 >= c1 + c2");
    REQUIRE(rows >= batch * n, "lidar_three_interpolate_f32: rows < batch * n");
    if (rows == 0) return LIDAR_OK;
    const int64_t threads = rows * (ldo / 4);
    REQUIRE((threads + NT - 1) / NT <= 0x7fffffff, "lidar_three_interpolate_f32: too many rows");
    const int vk = ldk % 4 == 0 && aligned16(known_feat);
    const int vs = c1 > 0 && c2 % 4 == 0 && lds % 4 == 0 && aligned16(skip);
    ON_DEVICE(h->device);
    lidar::Span span(h, "three_interpolate", static_cast<hipStream_t>(stream));
    hipLaunchKernelGGL(three_interpolate_kernel, dim3((unsigned)((threads + NT - 1) / NT)), dim3(NT), 0,
                       static_cast<hipStream_t>(stream), known_feat, ldk, (int)c2, idx, weight, skip, lds, (int)c1, n, m,
                       batch * n, rows, out, ldo, vk, vs);
    LAUNCH_CHECK();
    return LIDAR_OK;
}

LIDAR_EXPORT int lidar_row_argmax_f32(lidar_handle *h, const float *x, int64_t rows, int64_t ldx, int32_t c,
                                      int32_t *out, void *stream)
{
    REQUIRE(h, "lidar_row_argmax_f32: null handle");
    REQUIRE(x && out, "lidar_row_argmax_f32: null pointer");
    REQUIRE(rows >= 0 && c >= 1 && ldx >= c, "lidar_row_argmax_f32: bad shape");
    if (rows == 0) return LIDAR_OK;
    REQUIRE((rows + NT - 1) / NT <= 0x7fffffff, "lidar_row_argmax_f32: too many rows");
    ON_DEVICE(h->device);
    hipLaunchKernelGGL(row_argmax_kernel, dim3((unsigned)((rows + NT - 1) / NT)), dim3(NT), 0,
                       static_cast<hipStream_t>(stream), x, rows, ldx, (int)c, out);
    LAUNCH_CHECK();
    return LIDAR_OK;
}
