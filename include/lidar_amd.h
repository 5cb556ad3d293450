/*
 * lidar_amd.h — C-ABI of the MI355X (gfx950) LiDAR hot-path library, liblidar_amd.so.
 *
 * This is the drop-in boundary.  The reference (FortuneMU2025/LIDAR_AI_Recommendation_Software)
 * is pure Python; its hot path is the operator set in utils/data_processing.py and
 * models/crowd_density_model.py.  Each entry point below names the reference
 * interface it replaces (file:line in /root/reference).  The Python host layer
 * (lidar_ai_recommendation_software_amd/) binds these with ctypes, mirroring the
 * reference's Python signatures; INTEGRATION.md shows the binding.
 *
 * Conventions
 *  - Plain pointers and sizes only.  Every array pointer is a DEVICE pointer
 *    (hipMalloc / torch CUDA tensor storage) unless the name ends in `_host`.
 *  - The caller owns every input/output buffer.  The library owns only the scratch
 *    workspace inside a handle (grown on demand; lidar_reserve() pre-sizes it so a
 *    later call can be captured into a hipGraph).
 *  - Calls are asynchronous on `stream` (a hipStream_t; NULL = legacy default stream).
 *  - Return 0 on success, a negative LIDAR_E* code on failure; nothing throws across
 *    the ABI.  lidar_last_error() returns a thread-local message for the last failure.
 *  - A handle is bound to one device.  Use one handle per (thread, stream): calls on
 *    one handle must not run concurrently (the scratch workspace is shared).
 *  - Frames are batched: `batch` frames of `n` points, (batch, n, 3) row-major, unless a
 *    CSR `offsets` array is given (Tier R, ragged frames).
 */
#ifndef LIDAR_AMD_H
#define LIDAR_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LIDAR_OK 0
#define LIDAR_EINVAL -1   /* bad argument (shape, size, null pointer) */
#define LIDAR_EHIP -2     /* a HIP runtime call failed */
#define LIDAR_ENOMEM -3   /* workspace allocation failed */
#define LIDAR_EDEVICE -4  /* device is not gfx950 */
#define LIDAR_EPARSE -5   /* a text token the C parser does not reproduce exactly (caller falls back) */

typedef struct lidar_handle lidar_handle;

/* ------------------------------------------------------------------ handle */
int lidar_create(int device, lidar_handle **out);
int lidar_destroy(lidar_handle *h);
/* grow the scratch workspace to at least `bytes` now (not inside graph capture).  Growth never
 * synchronises the device: the replaced block is retired (queued kernels may still read it) and
 * freed by lidar_destroy or lidar_trim. */
int lidar_reserve(lidar_handle *h, uint64_t bytes);
/* free the workspaces retired by growth (*freed = their bytes, may be NULL); the caller guarantees
 * that the work it queued with this handle before the growth has completed */
int lidar_trim(lidar_handle *h, uint64_t *freed);
const char *lidar_last_error(void);
int lidar_version(void); /* 5 (what changed per version) */

/* Per-phase timing of a handle's launches (bench.py's in-window kernel durations): with
 * lidar_profile(h, 1) every kernel phase issued on h is bracketed by two HIP events on its
 * stream; lidar_profile_read waits for them and returns, in launch order, the phase names
 * ('\n'-separated into names, NUL terminated) and durations in ms; lidar_profile(h, 0) stops.
 * The Tier R entry points (preprocess, DBSCAN, people, density grid) record phases. */
int lidar_profile(lidar_handle *h, int32_t enable);
int lidar_profile_read(lidar_handle *h, char *names, int64_t names_cap, float *ms, int64_t cap, int64_t *count);

/* ============================================================ Tier N (SA stack)
 * North_star operators.  The reference has no PointNet++ code; these
 * are exposed beside utils/data_processing.py:231 (downsample_point_cloud) and drive
 * CrowdDensityModel's optional PointNet++ backbone (models/crowd_density_model.py:14).
 */

/* workspace bytes the FPS entry points take from a handle for (batch, n) (for lidar_reserve) */
uint64_t lidar_fps_workspace_bytes(int64_t batch, int64_t n);

/* farthest-point sampling: idx (batch, npoint) int32; optionally new_xyz (batch, npoint, 3)
 * = xyz[idx] (pass NULL to skip).  Start index 0, fp32 no-FMA distances, lowest index on
 * ties.  Optional first_zero (batch) receives the first step whose winning distance was 0 or
 * not finite (npoint if none).  Optional prefix_ok (batch): when xyz are the first points of a parent
 * FPS ordering, pass the parent's first_zero — frames with npoint <= prefix_ok[b] get the
 * exact identity result without running (nested SA levels).  Replaces:
 * downsample_point_cloud's random subset (utils/data_processing.py:231-249) where a
 * spatially uniform subset is wanted. */
int lidar_fps_f32(lidar_handle *h, const float *xyz, int64_t batch, int64_t n, int64_t npoint,
                  int32_t *idx, float *new_xyz, int32_t *first_zero, const int32_t *prefix_ok,
                  void *stream);
/* the same with an explicit workgroup size per frame: threads 0 (default, 1024), 1024 or 512.
 * 512 takes ~25 % longer per step and half the CU footprint (throughput pipelines that run
 * other kernels beside FPS).  Identical results. */
int lidar_fps_ex_f32(lidar_handle *h, const float *xyz, int64_t batch, int64_t n, int64_t npoint,
                     int32_t *idx, float *new_xyz, int32_t *first_zero, const int32_t *prefix_ok,
                     int32_t threads, void *stream);

/* ball query: idx (batch, m, nsample) int32 — the first `nsample` point indices (ascending)
 * with d < radius^2, padded with the first hit, 0 when there is none.  Replaces the eps-ball
 * query the reference runs through sklearn (utils/data_processing.py:197,
 * models/crowd_flow_model.py:216,228 query_radius) with a bounded-nsample form. */
int lidar_ball_query_f32(lidar_handle *h, const float *xyz, const float *centres, int64_t batch,
                         int64_t n, int64_t m, float radius, int32_t nsample, int32_t *idx,
                         void *stream);

/* the same query with an explicit kernel: mode 0 = auto (grid for n >= 1024), 1 = the
 * index-order scan, 2 = the (index window, cell) grid.  Results are identical. */
int lidar_ball_query_mode_f32(lidar_handle *h, const float *xyz, const float *centres,
                              int64_t batch, int64_t n, int64_t m, float radius, int32_t nsample,
                              int32_t mode, int32_t *idx, void *stream);

/* the grid path in two steps, so the binning of a frame (it depends only on xyz) can run
 * ahead on another stream: lidar_ball_query_bin_f32 writes the grid of every frame into a
 * caller-owned device buffer of lidar_ball_query_grid_bytes(batch, n) bytes;
 * lidar_ball_query_binned_f32 answers queries from it.  A grid binned for radius r answers
 * any radius exactly (radii above r fall back to scanning whole windows); nsample only tunes
 * the window size. */
uint64_t lidar_ball_query_grid_bytes(int64_t batch, int64_t n);
int lidar_ball_query_bin_f32(lidar_handle *h, const float *xyz, int64_t batch, int64_t n, float radius,
                             int32_t nsample, void *grid, void *stream);
int lidar_ball_query_binned_f32(lidar_handle *h, const float *xyz, const void *grid, const float *centres,
                                int64_t batch, int64_t n, int64_t m, float radius, int32_t nsample,
                                int32_t *idx, void *stream);

/* dense layer on MFMA: y (rows, cout) = relu(x (rows, k) W (k, cout) + b), fp32.
 * If pool_rows > 0: y is (rows / pool_rows, cout) = max over each run of pool_rows rows
 * (group_all's max-pool, fused); y must then be zeroed by the caller first.
 * k a multiple of 16, cout a multiple of 128, rows a multiple of 128
 * (pool_rows a multiple of 128 when used).  ReLU and max-pool propagate NaN (INTEGRATION.md
 * "Non-finite input"; tests/test_gpu_nonfinite.py). */
int lidar_dense_relu_f32(lidar_handle *h, const float *x, int64_t rows, int32_t k,
                         const float *w, const float *bias, int32_t cout, int32_t pool_rows,
                         float *y, void *stream);

/* as lidar_dense_relu_f32 with the ReLU optional (relu_on = 0: y = x W + b); the fused
 * max-pool requires relu_on. */
int lidar_dense_f32(lidar_handle *h, const float *x, int64_t rows, int32_t k, const float *w,
                    const float *bias, int32_t cout, int32_t relu_on, int32_t pool_rows, float *y,
                    void *stream);

/* The dense GEMM of the fp32 contract ("h3" arithmetic, csrc/h3.hpp: operands scaled by powers of
 * two and split exactly into fp16 hi + lo, products ah*bh + ah*bl + al*bh accumulated in fp32 on
 * the fp16 matrix cores, unscaled once: <= ~3 2^-22 |a b| per product) runs on a weight image packed
 * once: lidar_dense_x3_packed_size(k, cout) bytes, filled on the device by lidar_dense_x3_pack_f32
 * from W (k, cout) fp32 (fp16 hi / lo MFMA B fragments of W 2^s, K padded to 32, s in the image's
 * tail).  lidar_dense_x1_pack_f32 fills the same size with the bf16 image of the bf16 spec (X1). */
int64_t lidar_dense_x3_packed_size(int32_t k, int32_t cout);
int lidar_dense_x3_pack_f32(lidar_handle *h, const float *w, int32_t k, int32_t cout, void *packed, void *stream);
int lidar_dense_x1_pack_f32(lidar_handle *h, const float *w, int32_t k, int32_t cout, void *packed, void *stream);

/* y = x W + b on that image (csrc/dense_x3s.hip): A = fp32 rows (rows, k) of row stride lda
 * (k % 4 == 0, lda % 4 == 0; elements k..lda-1 are never read and may hold anything, as may columns
 * cout..ldo-1 of out, which are never written), each wave scales and splits the fragments it reads.  mode 0: y [ReLU] as fp32 rows (rows, ldo); mode 2: ReLU and max over runs
 * of pool_rows rows into fp32 (rows/pool_rows, ldo), out zeroed by the caller.  rows % 128 == 0,
 * cout % 128 == 0; o_plane is unused (0).  Mode flag 4 (mode 0 only, lidar_dense_x1_pack_f32's
 * image): one bf16 product per MFMA, bf16(x) bf16(w) in fp32 — the bf16 spec. */
int lidar_dense_x3f_f32(lidar_handle *h, const float *a, int32_t lda, int64_t rows, int32_t k, const void *packed,
                        const float *bias, int32_t cout, int32_t mode, int32_t relu_on, int32_t pool_rows, void *out,
                        int64_t o_plane, int64_t ldo, void *stream);

/* group_all's h3 chain (csrc/dense_x3s.hip): the same GEMM with the activations split ONCE, by the
 * producing layer.  A: fp32 rows (a_exp NULL; k % 4 == 0, lda % 4 == 0, elements k..lda-1 never
 * read) or h3 planes (a_exp (rows,) int32: |x| < 2^e per row; the fp16 hi plane (rows, lda) at a, the
 * lo plane at a + rows*lda halves, hi + lo = x 2^(14 - e) up to 2^-22; lda = k rounded up to 32, zeros
 * past k) — what mode 1 writes.  mode 0: fp32 rows (rows, ldo) [+ ReLU]; 1: h3 planes of y [+ ReLU]
 * (hi at out, lo at out + rows*ldo halves, ldo == cout) and out_exp (rows,): an exponent bound shared
 * by every column tile, 2^e_in w_colsum + b_max (w_colsum >= max_c sum_k |W_kc|, b_max >= max |b|,
 * the caller's, rounded up); 2: ReLU and max over runs of pool_rows rows (fp32, out zeroed by the
 * caller).  rows % 128 == 0, cout % 128 == 0; packed: lidar_dense_x3_pack_f32's image.
 * Non-finite operands, both entry points and every mode: INTEGRATION.md "Non-finite input" (a row or
 * pool group an inf / NaN reaches is non-finite wherever fp32 would be, ReLU and max-pool included; the
 * other rows and groups are bit-identical; tests/test_gpu_nonfinite.py). */
int lidar_dense_h3p_f32(lidar_handle *h, const void *a, int32_t lda, int64_t rows, int32_t k, const int32_t *a_exp,
                        const void *packed, const float *bias, int32_t cout, int32_t mode, int32_t relu_on,
                        int32_t pool_rows, void *out, int32_t *out_exp, int64_t ldo, float w_colsum, float b_max,
                        void *stream);

/* SA branch in the bf16 spec (BASELINE configs[4]) on the fused 16-row kernel of
 * lidar_sa_group_mlp_x3_f32 with one bf16 product per MFMA: layer inputs and weights rounded to
 * bf16 (RNE), fp32 accumulation, bias / ReLU / max-pool in fp32.  layer1_mode 0 (xyz level):
 * p = the level's points (batch, n, 3), q = centres (batch, m, 3).  layer1_mode 2 (feature
 * level): p (batch*n, p_stride) = bf16(f) bf16(W1_f) + b1 per point (lidar_dense_x3f_f32 with
 * mode flag 4), xyz = the level's points, centres = (batch, m, 3); a grouped row's layer 1 is
 * relu(p[k] + bf16(W1_xyz) . bf16(x_k - c)).  packed: lidar_mlp_packed_size_x1(c1, c2, c3)
 * bytes from lidar_mlp_pack_x1_f32 (host).  Shapes: those of lidar_sa_group_mlp_x3_f32. */
int64_t lidar_mlp_packed_size_x1(int32_t c1, int32_t c2, int32_t c3);
int lidar_mlp_pack_x1_f32(int32_t c1, int32_t c2, int32_t c3, const float *w1, const float *b1, const float *w2,
                          const float *b2, const float *w3, const float *b3, void *packed);
int lidar_sa_group_mlp_x1_f32(lidar_handle *h, int32_t layer1_mode, const float *p, int64_t p_stride, const float *q,
                              const float *xyz, const float *centres, const int32_t *idx, int64_t batch, int64_t n,
                              int64_t m, int32_t nsample, int32_t c1, int32_t c2, int32_t c3, const void *packed,
                              float *out, int64_t out_stride, int64_t out_offset, void *stream);

/* Grouped shared MLP (3 layers, BN folded, ReLU) + max-pool over nsample for one SA branch,
 * fused with the grouping gather, on the native fp32 matrix cores (v_mfma_f32_16x16x4_f32,
 * 16 grouped rows per wave; the strict-fp32 path):
 *   row (b, c, s) = [xyz[b, idx[b,c,s]] - centres[b,c], feats[b, idx[b,c,s]]]
 *   out[b, c, out_offset + j] = max_s relu(...relu(row W1 + b1)... W3 + b3)[j]
 * xyz_level != 0 (a level without features): p = xyz (batch*n, 3), q = centres (batch*m, 3),
 * layer 1 runs in-kernel.  xyz_level = 0: layer 1 was applied per point beforehand — p
 * (batch*n, p_stride) = [f, x] W1 + b1 for every point of the level, q (batch*m, p_stride) =
 * centre W1_xyz (lidar_dense_f32 / lidar_dense_x3f_f32, relu off); a grouped row's layer 1 is
 * relu(p[k] - q[c]).
 * packed: the lidar_mlp_pack16_f32 image of lidar_mlp_packed_size16 floats (w1 is read only
 * for an xyz level: its 3 xyz rows).  Same outputs up to fp32 re-association.
 * Non-finite points, centres or features (this kernel and the x3 / x1 / bq variants below): a centre
 * that one reaches is non-finite wherever the fp32 pipeline's relu / max_pool2d would be, every other
 * centre is bit-identical (INTEGRATION.md "Non-finite input"; tests/test_gpu_nonfinite.py). */
int64_t lidar_mlp_packed_size16(int32_t xyz_level, int32_t c1, int32_t c2, int32_t c3);
int lidar_mlp_pack16_f32(int32_t xyz_level, int32_t c1, int32_t c2, int32_t c3, const float *w1_host,
                         const float *b1_host, const float *w2_host, const float *b2_host,
                         const float *w3_host, const float *b3_host, float *packed_host);
int lidar_sa_group_mlp16_f32(lidar_handle *h, int32_t xyz_level, const float *p, int64_t p_stride,
                             const float *q, const int32_t *idx, int64_t batch, int64_t n,
                             int64_t m, int32_t nsample, int32_t c1, int32_t c2, int32_t c3,
                             const float *packed, float *out, int64_t out_stride,
                             int64_t out_offset, void *stream);

/* "x3" variants of the 16-row kernels: layers 2-3 in fp32 arithmetic carried by the bf16
 * matrix cores — every operand split exactly into bf16 hi + lo, products accumulated as
 * ah*bh + ah*bl + al*bh (v_mfma_f32_16x16x32_bf16, fp32 accumulation; error <= ~2^-15 per
 * product, within the fp32 path's 1e-4 contract).  Arguments as lidar_sa_group_mlp16_f32;
 * packed: lidar_mlp_pack_x3_f32's image of lidar_mlp_packed_size_x3 BYTES. */
int64_t lidar_mlp_packed_size_x3(int32_t xyz_level, int32_t c1, int32_t c2, int32_t c3);
int lidar_mlp_pack_x3_f32(int32_t xyz_level, int32_t c1, int32_t c2, int32_t c3, const float *w1_host,
                          const float *b1_host, const float *w2_host, const float *b2_host,
                          const float *w3_host, const float *b3_host, void *packed_host);
int lidar_sa_group_mlp_x3_f32(lidar_handle *h, int32_t xyz_level, const float *p, int64_t p_stride,
                              const float *q, const int32_t *idx, int64_t batch, int64_t n,
                              int64_t m, int32_t nsample, int32_t c1, int32_t c2, int32_t c3,
                              const void *packed, float *out, int64_t out_stride,
                              int64_t out_offset, void *stream);

/* An xyz level's SA branch with its ball queries answered inside the MLP kernel: grid =
 * lidar_ball_query_bin_f32(xyz, radius, nsample) for these frames; each wavefront queries its
 * centre from the grid into LDS, then groups, runs the MLP and max-pools.  Equal bit for bit to
 * lidar_ball_query_binned_f32 followed by lidar_sa_group_mlp_x3_f32 (x1 = 0; packed from
 * lidar_mlp_pack_x3_f32 with xyz_level = 1) or lidar_sa_group_mlp_x1_f32 mode 0 (x1 = 1; packed
 * from lidar_mlp_pack_x1_f32).  xyz (batch, n, 3), centres (batch, m, 3); out_idx (batch, m,
 * nsample) int32 or NULL receives the ball-query indices.  Shapes: (c1, c2, c3, nsample) in
 * {(64, 64, 128, 32), (32, 32, 64, 16), (64, 96, 128, 128)}.  Replaces, for these levels, the
 * pointnet2 `ball_query` + `group_points` + shared-MLP sequence behind the north_star's SA layer
 * (no reference counterpart: SURVEY §0). */
int lidar_sa_group_mlp_bq_f32(lidar_handle *h, int32_t x1, const float *xyz, const void *grid, const float *centres,
                              int64_t batch, int64_t n, int64_t m, float radius, int32_t nsample, int32_t c1,
                              int32_t c2, int32_t c3, const void *packed, float *out, int64_t out_stride,
                              int64_t out_offset, int32_t *out_idx, void *stream);

/* A set-abstraction branch of any shape (csrc/sa_generic.hip; the fused kernels above cover six):
 * grouped rows -> the dense GEMMs (lidar_dense_x3f_f32 / lidar_dense_f32, one per layer, ReLU)
 * -> the max over each group's nsample rows.  Replaces, for every other (c1, c2, c3, nsample),
 * pointnet2's QueryAndGroup(use_xyz) + shared MLP + max_pool2d of PointnetSAModuleMSG.forward.
 *
 * lidar_sa_group_rows_f32: rows_out[(b*m + j)*nsample + s] = [feat[b*n + idx] (cfeat columns,
 * row stride ldf; feat may be NULL when cfeat = 0), xyz[b*n + idx] - centres[b*m + j] (fp32),
 * zeros to ldr]; rows_out rows [batch*m*nsample, rows) are zeroed.  ldr % 4 == 0, ldr >= cfeat + 3.
 * lidar_group_max_f32: out[g*ldo + out_offset + c] = max_s in[(g*nsample + s)*ldi + c], c < C,
 * g < groups (a NaN propagates). */
int lidar_sa_group_rows_f32(lidar_handle *h, const float *feat, int64_t ldf, int32_t cfeat, const float *xyz,
                            const float *centres, const int32_t *idx, int64_t batch, int64_t n, int64_t m,
                            int32_t nsample, float *rows_out, int64_t rows, int64_t ldr, void *stream);
int lidar_group_max_f32(lidar_handle *h, const float *in, int64_t ldi, int64_t groups, int32_t nsample, int32_t c,
                        float *out, int64_t ldo, int64_t out_offset, void *stream);

/* PointNet++ feature propagation (csrc/feature_prop.hip; DESIGN.md §3 "Feature propagation"): the
 * decoder's operators, pointnet2's three_nn / three_interpolate of PointnetFPModule (no reference
 * counterpart: SURVEY §0).  All fp32, one rounding per operation, reproducible bit for bit in numpy.
 *
 * lidar_three_nn_f32: unknown (batch, n, 3), known (batch, m, 3), n >= 1, 1 <= m < 2^31.  Per unknown
 * point the three smallest d(j) = (dx*dx + dy*dy) + dz*dz over its frame's known points in
 * lexicographic (d, j) order (a sequential scan with strict <: lowest index on ties; a NaN or +inf
 * distance never wins): dist2 (batch, n, 3), idx (batch, n, 3) int32; unfilled slots (m < 3, non-finite
 * candidates) hold (+inf, 0).  weight (batch, n, 3) or NULL: w_i = r_i / ((r_0 + r_1) + r_2) with
 * r_i = 1 / (sqrt(d2_i) + 1e-8f) (correctly rounded sqrt and divisions; an unfilled slot gives 0, m = 1
 * gives exactly [1, 0, 0], three unfilled slots NaN).
 * lidar_three_interpolate_f32: out[b*n + i] = [(w0 f[i0] + w1 f[i1]) + w2 f[i2] (c2 columns, f =
 * known_feat rows (batch*m rows of stride ldk) of frame b), skip[b*n + i] (c1 columns, row stride lds;
 * NULL when c1 = 0), zeros to ldo]; out rows [batch*n, rows) are zeroed, so out is directly the A operand
 * of lidar_dense_x3f_f32 / lidar_dense_f32 (as lidar_sa_group_rows_f32).  ldo % 4 == 0, ldo >= c1 + c2,
 * rows >= batch*n; idx entries must lie in [0, m).
 * lidar_row_argmax_f32: out[r] = argmax over c < C of x[r*ldx + c] as int32: lowest index on ties, a NaN
 * counts as the maximum (np.argmax). */
int lidar_three_nn_f32(lidar_handle *h, const float *unknown, const float *known, int64_t batch, int64_t n,
                       int64_t m, float *dist2, int32_t *idx, float *weight, void *stream);
int lidar_three_interpolate_f32(lidar_handle *h, const float *known_feat, int64_t ldk, int32_t c2, const int32_t *idx,
                                const float *weight, const float *skip, int64_t lds, int32_t c1, int64_t batch,
                                int64_t n, int64_t m, float *out, int64_t rows, int64_t ldo, void *stream);
int lidar_row_argmax_f32(lidar_handle *h, const float *x, int64_t rows, int64_t ldx, int32_t c, int32_t *out,
                         void *stream);

/* y (batch*m, ldy) columns [col0, col0+3) = xyz rows; columns [col0+3, ldy) zeroed —
 * builds group_all's input [feats, xyz, 0-pad] next to features already in y. */
int lidar_concat_xyz_pad_f32(lidar_handle *h, const float *xyz, int64_t rows, float *y,
                             int64_t ldy, int64_t col0, void *stream);

/* voxel downsample.  The voxel of a point is calculate_grid_density's grid hash
 * (utils/data_processing.py:305-319) per axis: edges np.arange(lo - 2v, (hi + 2v) + v, v) over the
 * frame's extent, histogram2d's searchsorted-right binning with the last edge closed; key =
 * (bx*ny + by)*nz + bz.  Per-point voxel id (rank of its key, ascending; -1 outside every bin),
 * centroids (sequential fp32 sums in point order / count), counts; *nvox_host receives V
 * (synchronises `stream`).  centroids/counts must hold n entries.  LIDAR_EINVAL when the extent
 * is not finite or the grid has 2^32 keys or more. */
int lidar_voxel_downsample_f32(lidar_handle *h, const float *xyz, int64_t n, double voxel,
                               int32_t *voxel_id, float *centroids, int32_t *counts,
                               int64_t *nvox_host, void *stream);

/* Voxel downsampling of `batch` frames of n points over the whole chip (csrc/voxel_batch.hip):
 * xyz (batch, n, 3) fp32; voxel_id (batch, n) int32; centroids (batch, n, 3) and counts (batch, n),
 * the first nvox[f] rows of frame f valid; nvox (batch,) int32 on the device (-1: the frame's extent
 * is not finite or its grid has 2^32 keys or more; library bugs, never expected, and sticky — they win over
 * the count: -2 a bounded in-launch wait timed out, -3 an inconsistent bucket table).  No host
 * synchronisation; per frame equal to lidar_voxel_downsample_f32.  Workspace:
 * lidar_voxel_batch_workspace_bytes(batch, n), plus the handle's own voxel tag block (the in-launch
 * hand-offs' epoch-tagged granules, 8 KiB per 8 192-point tile; grown and zeroed on demand, written by
 * voxel calls only).  Calls on one handle must not run concurrently (as for the workspace). */
uint64_t lidar_voxel_batch_workspace_bytes(int64_t batch, int64_t n);
int lidar_voxel_downsample_batch_f32(lidar_handle *h, const float *xyz, int64_t batch, int64_t n, double voxel,
                                     int32_t *voxel_id, float *centroids, int32_t *counts, int32_t *nvox,
                                     void *stream);

/* ======================================================= Tier R (density path)
 * Bit-exact replacements for the reference's CPU path. */

/* eps-ball neighbour count over scaled points (self included, fp64,
 * ((dx*dx+dy*dy)+dz*dz) <= eps*eps) and DBSCAN labels (min_samples).  Replaces
 * sklearn DBSCAN(eps, min_samples).fit(x).labels_ at utils/data_processing.py:197. */
int lidar_dbscan_f64(lidar_handle *h, const double *x, int64_t n, double eps, int32_t min_samples,
                     int64_t *labels, int32_t *counts, void *stream);

/* KDTree(x).query_radius(x, r, count_only=True): counts[i] = #{j : ((dx*dx+dy*dy)+dz*dz)
 * <= r*r} in fp64, i itself included (utils/visualization.py:41-48, :165-168;
 * app_simplified.py:156-159).  x (n, 3) device; 2-D data with z = 0.  Synchronises. */
int lidar_radius_count_f64(lidar_handle *h, const double *x, int64_t n, double r, int64_t *counts,
                           void *stream);

/* np.histogram2d(a, b, bins=(bx, by), range=...) counts (float64, bx*by row-major) with
 * numpy's edges passed in (xedges bx+1, yedges by+1, device): searchsorted-right bins, the
 * last edge closed, outside / NaN dropped (utils/visualization.py:125-137). */
int lidar_histogram2d_f64(lidar_handle *h, const double *a, const double *b, int64_t n, const double *xedges,
                          int64_t bx, const double *yedges, int64_t by, double *counts, void *stream);

/* Host-only: the PCD / PLY ASCII data section of load_lidar_data (utils/data_processing.py
 * :43-104).  From 0-based line `first` (max_lines < 0: to the end; else that many lines),
 * every line with >= 3 whitespace-separated tokens yields float(tok0..2) into out (3 per
 * point, cap points); *n_out = points written.  LIDAR_EPARSE: some token needs Python's own
 * float() (the caller falls back to the reference's loop for the exact result / error). */
int lidar_parse_ascii_xyz(const char *buf, int64_t len, int64_t first, int64_t max_lines, double *out,
                          int64_t cap, int64_t *n_out);

/* The scalars block of a preprocessed frame: LIDAR_SCALARS doubles, the public slots below (the
 * others are the library's own).  The Python host layer restates them in density_abi.py. */
enum {
    LIDAR_S_N_IN = 0,           /* inliers of the 3-sigma filter */
    LIDAR_S_N_GROUND = 1,
    LIDAR_S_N_NONGROUND = 2,
    LIDAR_S_Z_THRESHOLD = 3,    /* the 30th-percentile ground split */
    LIDAR_S_EPS = 4,            /* DBSCAN's eps */
    LIDAR_S_DIMS = 5,           /* 5..10: x_min, x_max, y_min, y_max, z_min, z_max */
    LIDAR_S_PLANE = 11,         /* 11..14: ground plane a, b, c, d */
    LIDAR_S_STATUS = 15,        /* LIDAR_STATUS_* */
    LIDAR_S_MEAN = 16,          /* 16..18: 3-sigma mean */
    LIDAR_S_STD = 19,           /* 19..21: 3-sigma std */
    LIDAR_S_SCALER_MEAN = 22,   /* 22..24: StandardScaler mean */
    LIDAR_S_SCALER_SCALE = 25,  /* 25..27: StandardScaler scale */
    LIDAR_S_SCALED_BBOX = 28,   /* 28..33: lo (3), hi (3) of the scaled non-ground points */
    LIDAR_S_N_CLUSTERS = 39,    /* max label + 1 of the frame: DBSCAN's cluster count; 1 when DBSCAN is skipped (1..10
                                   non-ground points, all label 0); 0 without non-ground points or for a failed frame */
    LIDAR_S_PLANE_KIND = 40,    /* 0 lstsq, 1 min-z fallback, 2 rank-deficient ground */
    LIDAR_SCALARS = 64,
    LIDAR_STATUS_OK = 0,
    LIDAR_STATUS_NO_INLIER = 1, /* no point survives the 3-sigma filter -> the reference's IndexError */
    LIDAR_STATUS_EMPTY = 2      /* a batch frame without points -> the reference's ValueError */
};

/* Whole preprocess_lidar_data (utils/data_processing.py:127-229) on one frame already in
 * device memory (n >= 1 points, (n,3) f64).  Outputs (device, caller-allocated with n rows):
 *   mask (n) u8 inlier flag; colors, normals, compact_xyz (n,3) f64 of the inliers in input
 *   order (first LIDAR_S_N_IN rows valid); labels (n) int64 over the inliers (ground -1);
 *   scalars (LIDAR_SCALARS f64): the LIDAR_S_* slots above, LIDAR_S_STATUS being
 *   LIDAR_STATUS_OK or LIDAR_STATUS_NO_INLIER.  Asynchronous on `stream`. */
int lidar_preprocess_f64(lidar_handle *h, const double *xyz, int64_t n, uint8_t *mask,
                         double *colors, double *normals, double *compact_xyz, int64_t *labels,
                         double *scalars, void *stream);

/* lidar_preprocess_f64 over `frames` frames in one launch per phase (frames in
 * CSR layout).  xyz: the frames' rows concatenated; offsets: DEVICE int64[frames + 1] row
 * offsets (frame f = rows [offsets[f], offsets[f+1])); max_n >= every frame's size.  The
 * per-point outputs use the same row offsets (a frame's compact_xyz / labels rows start at
 * offsets[f] and run for its own n_in = scalars[f*LIDAR_SCALARS + LIDAR_S_N_IN]); scalars holds
 * LIDAR_SCALARS doubles per frame, LIDAR_S_STATUS being any of the three LIDAR_STATUS_* codes. */
int lidar_preprocess_batch_f64(lidar_handle *h, const double *xyz, const int64_t *offsets, int32_t frames,
                               int64_t max_n, uint8_t *mask, double *colors, double *normals,
                               double *compact_xyz, int64_t *labels, double *scalars, void *stream);

/* The Streamlit apps' variant preprocess_point_cloud (app_simplified.py:76-137,
 * app_with_db.py:80-141): lidar_preprocess_batch_f64's phases, then DBSCAN(eps,
 * min_samples=5) on the UNSCALED non-ground points (no StandardScaler / eps heuristic;
 * the reference passes eps = 0.3).  offsets == NULL: one frame of max_n points.  Same
 * outputs and status codes; the scaler slots (LIDAR_S_SCALER_MEAN / _SCALE) hold 0 / 1 and
 * LIDAR_S_SCALED_BBOX the unscaled bbox. */
int lidar_preprocess_eps_batch_f64(lidar_handle *h, const double *xyz, const int64_t *offsets,
                                   int32_t frames, int64_t max_n, double eps, uint8_t *mask,
                                   double *colors, double *normals, double *compact_xyz,
                                   int64_t *labels, double *scalars, void *stream);

/* The variant's analyze_crowd_density grid (app_simplified.py:262-282): for the edges xg
 * (nxg), yg (nyg) (np.arange, device), out (nyg-1, nxg-1) row-major [j][i] = #{people p :
 * (cx-px)^2 + (cy-py)^2 <= r*r} / divisor with centre ((xg[i]+xg[i+1])/2, (yg[j]+yg[j+1])/2)
 * — len(KDTree(people).query_radius([centre], r)[0]) / divisor.  people (k, 2) device. */
int lidar_cell_radius_density_f64(lidar_handle *h, const double *people, int64_t k, const double *xg,
                                  int64_t nxg, const double *yg, int64_t nyg, double r, double divisor,
                                  double *out, void *stream);

/* Optional global density over a FIXED venue grid (the reference derives its grid
 * per frame, models/crowd_density_model.py:49-54): counts (nx, ny) int32 += the histogram2d of
 * people (k, 2) over calculate_grid_density's edges (utils/data_processing.py:305-319:
 * np.arange(x0, ., grid) with x0 = x_min - 2 grid, searchsorted right, the last edge closed,
 * outside dropped).  Counts add, so the frames of a rank and then (one RCCL all-reduce, int32
 * sum) the ranks accumulate; counts / grid^2 is calculate_grid_density of all their people. */
int lidar_venue_counts_f64(lidar_handle *h, const double *people, int64_t k, double x0, double y0, double grid,
                           int64_t nx, int64_t ny, int32_t *counts, void *stream);

/* downsample_point_cloud's gather (utils/data_processing.py:247-249): dst[r] = src[idx[r]] for k
 * rows of row_bytes bytes each (any dtype: rows are moved as raw bytes); idx (k) int64 device,
 * the indices the host drew from the global legacy NumPy RNG (out-of-range indices skipped). */
int lidar_gather_rows(lidar_handle *h, const void *src, int64_t n_rows, int64_t row_bytes, const int64_t *idx,
                      int64_t k, void *dst, void *stream);

/* ---- models/crowd_flow_model.py, HOST code (host pointers): the
 * model's deciding arithmetic is glibc sin / cos / pow and sklearn's KD-tree traversal,
 * reproduced bit for bit on the host.
 * _generate_simulated_flow (crowd_flow_model.py:88-184) after its RNG draws: positions
 * (nx*ny, 2) = meshgrid(x_grid, y_grid) raveled, vectors (m, 2), magnitudes (m);
 * bottlenecks (nb, 2) = the (x, y) uniform draws. */
int lidar_flow_field_f64(const double *x_grid, int64_t nx, const double *y_grid, int64_t ny, double exit_x,
                         double exit_y, int32_t complexity, const double *bottlenecks, int32_t nb,
                         double speed_min, double speed_max, double *positions, double *vectors,
                         double *magnitudes);
/* _identify_bottlenecks (crowd_flow_model.py:186-279): nodes with magnitude <= slow, >=
 * min_close neighbours within r_close and >= min_far more within r_far (sklearn KDTree
 * query_radius order), severity > 1 -> (out_x, out_y, out_severity = min(10, round())) in
 * node order (out_raw: the unrounded severity, optional); *n_out = candidates. */
int lidar_flow_bottlenecks_f64(const double *positions, const double *vectors, const double *magnitudes,
                               int64_t m, double slow, double r_close, double r_far, int32_t min_close,
                               int32_t min_far, double *out_x, double *out_y, int64_t *out_severity,
                               double *out_raw, int64_t cap, int64_t *n_out);
/* sklearn KDTree(x, leaf_size).get_arrays()[1]: the build's index permutation (x (n, d)). */
int lidar_kdtree_order_f64(const double *x, int64_t n, int32_t d, int32_t leaf_size, int64_t *perm);

/* extract_people_positions for every frame of a preprocess batch: people rows of frame f
 * start at row offsets[f] (K_f rows); kdev (device int64[frames]) receives K_f.  Async. */
int lidar_people_batch_f64(lidar_handle *h, const double *compact_xyz, const int64_t *labels,
                           const int64_t *offsets, int32_t frames, int64_t max_n, const double *scalars,
                           double *people, int64_t *kdev, void *stream);

/* People from per-point class labels (csrc/class_people.hip): xyz (batch, n, 3) fp32,
 * labels (batch, n) int32 (a segmenter's output).  Per frame f, every frame independent and a batch equal
 * to its frames one at a time, bit for bit: S_f = the indices i, ascending, with labels[f, i] == cls and
 * three finite coordinates (a NaN or +-inf coordinate is never selected); nsel[f] = |S_f|.  The selected
 * points, widened to fp64 in index order, get the labels of lidar_dbscan_f64(eps, min_samples) (sklearn
 * DBSCAN).  instance (batch, n) int32: that label for a selected point, -1 for every other point (wrong
 * class, non-finite, noise).  people (batch, cap, 2) fp64: row c of frame f = the (x, y) centroid of cluster
 * c with lidar_people_f64's arithmetic (sequential index-order sums, one division); k[f] (int64) = the
 * number of clusters; when k[f] > cap only the first cap rows are written (k[f] keeps the true count), and
 * rows past min(k[f], cap) are not touched.  extent (batch, 4) fp64: x_min, x_max, y_min, y_max over ALL
 * finite points of the frame, of every class; a frame without a finite point gets +inf, -inf, +inf, -inf
 * and k = nsel = 0.  Asynchronous on `stream`: no host synchronisation, no host-staged parameter block;
 * all outputs are device arrays.  Workspace: the handle's, sized for nsel = n in every frame.
 * LIDAR_EINVAL: a null pointer, batch < 0 or > 65535, n < 1 or >= 2^31, eps not positive and finite,
 * min_samples < 1, cap < 1.  batch == 0 returns LIDAR_OK. */
int lidar_class_people_f32(lidar_handle *h, const float *xyz, const int32_t *labels, int64_t batch, int64_t n,
                           int32_t cls, double eps, int32_t min_samples, int64_t cap, int32_t *instance,
                           double *people, int64_t *k, int64_t *nsel, double *extent, void *stream);

/* Measured crowd flow (csrc/track.hip; DESIGN.md §3 "People tracking", §4.9): the people of T consecutive
 * frames associated across every consecutive pair of frames, and their velocities accumulated on the venue
 * grid.  All arithmetic fp64, one rounding per operation.  Both calls are asynchronous on `stream`: no host
 * synchronisation, no host-staged parameter block, every array a device array; scratch is the handle's
 * workspace.
 *
 * lidar_track_people_f64: people (frames, cap, 2) and k (frames) are lidar_class_people_f32's outputs;
 * K_t = min(max(k[t], 0), cap), rows at or past K_t are never read for meaning.  Per pair (t-1, t)
 * independently, A = the K_(t-1) rows of frame t-1, B = the K_t rows of frame t: d(i, j) = (dx*dx) + (dy*dy)
 * with dx = B[j].x - A[i].x, dy = B[j].y - A[i].y; (i, j) is a candidate iff d <= gate*gate (inclusive,
 * the fp64 product; a row with a NaN or infinite coordinate is never a candidate, in either role);
 * fwd[i] = the candidate j with the smallest (d, j) in lexicographic order, bwd[j] = the candidate i with
 * the smallest (d, i), -1 without a candidate; j is matched to i iff bwd[j] == i and fwd[i] == j (mutual
 * nearest neighbour).  prev (frames, cap) int32: i for a matched row, -1 otherwise (unmatched, every row
 * of frame 0, every row at or past K_t).  velocity (frames, cap, 2): ((B[j].x - A[i].x) / dt,
 * (B[j].y - A[i].y) / dt) for a matched row, (0, 0) for every other (prev == -1 means "no measurement",
 * not the zero).  track_id (frames, cap) int32: a row j < K_t with prev == -1 is a new detection, its id
 * the number of new detections before it in (t, j) ascending order; a matched row takes
 * track_id[t-1][prev[t][j]]; rows at or past K_t get -1.  ntracks (one int64): the number of new
 * detections.  Every element of every output is written.
 *
 * lidar_flow_cells_f64: the grid is lidar_venue_counts_f64's (x0 = x_min - 2 grid, y0 = y_min - 2 grid,
 * (nx, ny) = lidar_grid_dims; np.arange edges, searchsorted right, the last edge closed, outside dropped).
 * Every matched detection (t >= 1, j < K_t, prev[t][j] >= 0) is binned by its own position people[t][j]:
 * count (nx, ny) int32 = the matched detections per cell, vsum (nx, ny, 2) = the sum of their velocities
 * added sequentially in (t, j) ascending order starting from 0.0.  Both are overwritten; a cell without a
 * detection holds 0 and (0, 0).
 *
 * LIDAR_EINVAL: a null pointer, frames < 0 or > 65535, cap < 1, frames * cap >= 2^31, dt / gate / grid not
 * positive and finite, x0 / y0 not finite, nx or ny < 1, nx * ny >= 2^31.  frames == 0 returns LIDAR_OK
 * and writes nothing; frames == 1 is valid (no pairs: ids 0 .. K_0 - 1). */
int lidar_track_people_f64(lidar_handle *h, const double *people, const int64_t *k, int64_t frames, int64_t cap,
                           double dt, double gate, int32_t *prev, int32_t *track_id, double *velocity,
                           int64_t *ntracks, void *stream);
int lidar_flow_cells_f64(lidar_handle *h, const double *people, const int64_t *k, const int32_t *prev,
                         const double *velocity, int64_t frames, int64_t cap, double x0, double y0, double grid,
                         int64_t nx, int64_t ny, int32_t *count, double *vsum, void *stream);

/* Continuous people tracking (csrc/track.hip; DESIGN.md §3 "Continuous people tracking", §4.10): the
 * association of lidar_track_people_f64 carried across calls and stitched over missed frames.  Asynchronous
 * like its siblings: no host synchronisation, no host-staged parameter block, the id base read from device
 * memory, scratch from the handle's workspace.
 *
 * lidar_track_stream_f64: people, k, frames, cap, dt, gate as lidar_track_people_f64.  max_gap = M: the
 * number of consecutive frames a person may go undetected, 0 .. 7.  carry = C: the number of leading frames
 * whose association state is given, 0 .. min(M + 1, frames).  State per detection (t, j), j < K_t: prev
 * (frames, cap) int32, the predecessor's row or -1; gap (frames, cap) int32, the predecessor lives in frame
 * t - gap (0 iff prev == -1); succ (frames, cap) uint8, 1 iff a later detection has this one as its
 * predecessor; velocity (frames, cap, 2); track_id (frames, cap) int32.  The first C frames of all five are
 * inputs and stay as they are, except that succ may go from 0 to 1; every element of the other frames is
 * written (rows at or past K_t: prev -1, gap 0, succ 0, velocity (0, 0), track_id -1).
 * Passes g = 1 .. M + 1 in ascending order; pass g, for every start frame u with max(C, g) <= u < frames and
 * t = u - g, independently: A = the rows i < K_t of frame t with succ == 0, B = the rows j < K_u of frame u
 * with prev == -1, both as the passes before left them; (i, j) is a candidate iff d(i, j) <= (gate*g)*(gate*g)
 * (d as lidar_track_people_f64; gate*g, then its square, one fp64 product each); fwd, bwd and the mutual
 * test as there, over A and B alone, ties to the lowest row index.  A matched pair: prev[u][j] = i,
 * gap[u][j] = g, succ[t][i] = 1, velocity[u][j] = ((B.x - A.x) / (dt*g), (B.y - A.y) / (dt*g)), dt*g one fp64
 * product.  Ids, for (u, j) ascending, u >= C, j < K_u: a row with prev == -1 takes *ntracks (as it came in)
 * plus the number of such rows before it; a matched row takes track_id[u - gap][prev]; on return *ntracks
 * (one device int64) has grown by the number of new detections.  With M = 0 and C = 0 and *ntracks = 0 the
 * outputs are lidar_track_people_f64's bit for bit.  A sequence cut at any frame, the second call handed the
 * last min(M + 1, cut) frames of the first (people, k, the five arrays, *ntracks left in place) as its
 * carry, gives the frames from the cut on exactly what one call over the whole sequence gives.
 *
 * lidar_flow_cells_acc_f64: lidar_flow_cells_f64 over the detections of the frames t >= first only (a row
 * of frame 0 with prev >= 0 is legitimate once there is a carry: only prev >= 0 and the row's own velocity
 * are read); accumulate = 0 overwrites count and vsum, accumulate = 1 continues from them, every cell's
 * sequential sum starting from the stored value, so that the calls of a stream add up to the bits of one
 * call over the whole sequence.  lidar_flow_cells_f64 is first = 1, accumulate = 0.
 *
 * LIDAR_EINVAL: as lidar_track_people_f64 / lidar_flow_cells_f64, and max_gap outside 0 .. 7, carry outside
 * 0 .. min(max_gap + 1, frames), first outside 0 .. frames, accumulate not 0 or 1.  frames == 0 returns
 * LIDAR_OK and writes nothing; frames == carry is valid for lidar_track_stream_f64: nothing to link,
 * nothing written, *ntracks unchanged. */
int lidar_track_stream_f64(lidar_handle *h, const double *people, const int64_t *k, int64_t frames, int64_t cap,
                           int64_t carry, double dt, double gate, int32_t max_gap, int32_t *prev, int32_t *gap,
                           uint8_t *succ, double *velocity, int32_t *track_id, int64_t *ntracks, void *stream);
int lidar_flow_cells_acc_f64(lidar_handle *h, const double *people, const int64_t *k, const int32_t *prev,
                             const double *velocity, int64_t frames, int64_t cap, int64_t first,
                             int32_t accumulate, double x0, double y0, double grid, int64_t nx, int64_t ny,
                             int32_t *count, double *vsum, void *stream);

/* Gate counts and zone occupancy from tracked people (csrc/track_events.hip; DESIGN.md §3 "Gate and zone
 * events", §4.12): what the links of lidar_track_people_f64 / lidar_track_stream_f64 say about lines and
 * areas of the venue.  Asynchronous like its siblings: every pointer a device pointer, no host
 * synchronisation, nothing read back, no scratch.  All arithmetic fp64, one rounding per operation.
 *
 * lidar_track_events_f64: people, k, frames, cap and K_t as lidar_track_people_f64; prev (frames, cap) int32;
 * gap (frames, cap) int32 or null (null: every link spans one frame, lidar_track_people_f64's prev).  Only
 * the frames t >= first are evaluated (with a carry in front: first = carry, as lidar_flow_cells_acc_f64).
 * A row (t, j), j < K_t, is linked iff, with i = prev[t][j] and g = gap ? gap[t][j] : 1: i >= 0 and
 * 1 <= g <= 8 and g <= t and i < K_(t-g); then P = people[t-g][i] and Q = people[t][j].  Every other row is
 * unlinked: no content of prev / gap makes the call read outside people.
 * gates (ngates, 4), rows (ax, ay, bx, by).  side(a, b, p) = ((b.x - a.x) * (p.y - a.y)) - ((b.y - a.y) *
 * (p.x - a.x)); sP = side(A, B, P), sQ = side(A, B, Q), sA = side(P, Q, A), sB = side(P, Q, B).  The link
 * crosses the gate iff all four are finite and (sP >= 0) != (sQ >= 0) and (sA >= 0) != (sB >= 0); the
 * crossing is forward iff sQ >= 0 (from the right of A -> B to its left or onto it), backward otherwise.  A
 * detection exactly on the line counts as left, so a track that steps onto the line and then on counts once;
 * P == Q, A == B and a gate with a non-finite coordinate never cross: the tables need no validation here.
 * zones (nzones, 4), rows (x0, x1, y0, y1).  inside(z, p) = x0 <= p.x && p.x < x1 && y0 <= p.y && p.y < y1
 * (a NaN: false).
 * Outputs, indexed by t - first, every element written.  gate_counts (frames - first, ngates, 2) int32: the
 * forward and the backward crossings of the frame's linked rows (a crossing belongs to the frame of Q).
 * zone_counts (frames - first, nzones, 3) int32: [0] occupancy, the rows j < K_t with inside(Q), linked or
 * not; [1] entries, the linked rows with inside(Q) && !inside(P); [2] exits, the linked rows with inside(P)
 * && !inside(Q) (a new detection inside a zone is occupancy, not an entry).  gate_fwd, gate_bwd, zone_in
 * (frames - first, cap) int64: bit g / z set for the gates the row crossed forward / backward and the zones
 * that hold it (with track_id: the unique tracks per gate); rows at or past K_t get 0.  All results are
 * integers, the same under every schedule.
 *
 * LIDAR_EINVAL: a null handle, people, k or prev; frames < 0 or > 65535, cap < 1, frames * cap >= 2^31;
 * first outside 0 .. frames; ngates or nzones outside 0 .. 64, or both 0; with ngates > 0 a null gates,
 * gate_counts, gate_fwd or gate_bwd, with nzones > 0 a null zones, zone_counts or zone_in (the pointers of a
 * kind whose count is 0 are not used).  frames == first returns LIDAR_OK and writes nothing. */
int lidar_track_events_f64(lidar_handle *h, const double *people, const int64_t *k, const int32_t *prev,
                           const int32_t *gap, int64_t frames, int64_t cap, int64_t first, const double *gates,
                           int32_t ngates, const double *zones, int32_t nzones, int32_t *gate_counts,
                           int32_t *zone_counts, int64_t *gate_fwd, int64_t *gate_bwd, int64_t *zone_in,
                           void *stream);

/* Track history (csrc/track_history.hip; DESIGN.md §3 "Track history", §4.13): per detection, how long its
 * track has lived, how often it was seen, how far it walked, where it started and how long it has been in
 * each zone; per frame and zone, the stays that ended.  Asynchronous like its siblings: every pointer a device
 * pointer, no host synchronisation, nothing read back; scratch (4 bytes per row) from the handle's workspace.
 * All arithmetic fp64, one rounding per operation, the square root correctly rounded.
 *
 * lidar_track_history_f64: people, k, prev, gap (or null), frames, cap, K_t and the link guard exactly as
 * lidar_track_events_f64: a row (t, j), j < K_t, is linked iff, with i = prev[t][j] and g = gap ? gap[t][j] : 1:
 * i >= 0 and 1 <= g <= 8 and g <= t and i < K_(t-g); its source is the row (s, i), s = t - g, P = people[s][i],
 * Q = people[t][j].  No content of prev / gap makes the call read or write outside the arrays.
 * zones (nzones, 4) rows (x0, x1, y0, y1), 0 <= nzones <= 64, inside() as lidar_track_events_f64.
 * carry = C, 0 <= C <= frames: the leading frames whose history state is given; they are never written.
 * Heirs: among the rows of frames >= C that are linked to the same source, the lowest in (t, j) order is the
 * source's heir and continues its history; every other row of a frame >= C, unlinked or a linked non-heir,
 * starts a history.  (lidar_track_people_f64 and lidar_track_stream_f64 name a source at most once: on their
 * links every linked row is an heir.)
 * State, (frames, ...) arrays, every element of the frames >= C written:
 *   age (frames, cap) int32, frames since the history's first detection: 0 for a start, age[s][i] + g for a
 *     row that continues (s, i), -1 at or past K_t;
 *   hits (frames, cap) int32, detections so far: 1, hits[s][i] + 1, 0;
 *   path (frames, cap) fp64, metres walked: 0.0, path[s][i] + sqrt((dx*dx) + (dy*dy)) with dx = Q.x - P.x and
 *     dy = Q.y - P.y, 0.0 (a NaN coordinate makes it NaN from there on; a NaN's payload and sign are free);
 *   origin (frames, cap, 2) fp64, the first detection's position: Q, origin[s][i], (0, 0);
 *   stay (frames, cap, nzones) int32 (nzones > 0), frames since the present unbroken presence in zone z
 *     began: inside(z, Q) ? 0 : -1 for a start; inside(z, Q) ? (stay[s][i][z] >= 0 ? stay[s][i][z] + g : 0)
 *     : -1 for a row that continues; -1 at or past K_t.
 * dwell (frames - C, nzones, 3) int64 (nzones > 0), indexed by t - C, every element written: each continuing
 * row of frame t with stay[s][i][z] >= 0 and !inside(z, Q) (the track has left zone z) adds 1 to [0] and
 * stay[s][i][z] to [1] and raises [2] to stay[s][i][z].  A stay's length runs from its first to its last
 * detection inside (one detection: 0); a history that ends inside a zone is not a completed stay.  Integers:
 * the same under every schedule.  On the two tracking calls' links dwell[..][z][0] is zone_counts[..][z][2].
 *
 * LIDAR_EINVAL: a null handle, people, k, prev, age, hits, path or origin; frames < 0 or > 65535, cap < 1,
 * frames * cap >= 2^31; carry outside 0 .. frames; nzones outside 0 .. 64; with nzones > 0 a null zones, stay
 * or dwell (unused with nzones == 0).  frames == carry returns LIDAR_OK and writes nothing. */
int lidar_track_history_f64(lidar_handle *h, const double *people, const int64_t *k, const int32_t *prev,
                            const int32_t *gap, int64_t frames, int64_t cap, int64_t carry, const double *zones,
                            int32_t nzones, int32_t *age, int32_t *hits, double *path, double *origin,
                            int32_t *stay, int64_t *dwell, void *stream);

/* Routes (csrc/track_routes.hip; DESIGN.md §3 "Routes", §4.16): where tracked people go next.  Per detection the
 * first and the last zone its track was seen in, the frames since, the legs it has made and the leg it completes;
 * per ordered pair of zones the trips, their summed and their longest travel time in frames.  Asynchronous like its
 * siblings: every pointer a device pointer, no host synchronisation, nothing read back, nothing staged on the host;
 * scratch (4 bytes per row) from the handle's workspace.  Integers only.
 *
 * lidar_track_routes_f64: people, k, prev, gap (or null), frames, cap, K_t, the link guard, carry and the heirs
 * exactly as lidar_track_history_f64: a row (t, j), j < K_t, is linked iff, with i = prev[t][j] and
 * g = gap ? gap[t][j] : 1: i >= 0 and 1 <= g <= 8 and g <= t and i < K_(t-g); its source is the row (s, i), s = t - g.
 * No content of prev / gap makes the call read or write outside the arrays.  Among the rows of frames >= C = carry
 * that are linked to the same source, the lowest in (t, j) order continues the source's route; every other row of a
 * frame >= C starts one.  The frames < C hold the given state and are never written.
 * zones (nzones, 4) rows (x0, x1, y0, y1), 1 <= nzones <= 64, inside() as lidar_track_events_f64;
 * zone_of(p) = the lowest z with inside(z, p), -1 without one: zones may overlap and the lowest index wins; a NaN
 * position is in no zone.
 * Per row of a frame >= C, every element written, all (frames, cap) int32.  c = zone_of(Q), Q the row's own
 * position; g the frame distance of its link; (F, L, A, N) the source's first_zone, last_zone, away, legs; for a
 * continuing row with c >= 0, leg = L >= 0 and (L != c or A > 0):
 *                  starts            continues, c < 0        continues, c >= 0     j >= K_t
 *   first_zone     c                 F                       F >= 0 ? F : c        -1
 *   last_zone      c                 L                       c                     -1
 *   away           c >= 0 ? 0 : -1   L >= 0 ? A + g : -1     0                     -1
 *   legs           0                 N                       N + leg               0
 *   leg_from       -1                -1                      leg ? L : -1          -1
 *   leg_frames     0                 0                       leg ? A + g : 0       0
 * last_zone: the zone of the track's most recent detection inside any zone; away: the frames since it.  A leg is an
 * arrival in a zone from another one, or back into the same one after at least one detection outside every zone (a
 * return, on the diagonal); a link over g > 1 frames with both ends in one zone is one unbroken stay.  leg_frames
 * runs from the last detection in the zone left to the first in the zone reached.
 * trips (nzones, nzones, 3) int64, indexed [from][to]: a row with a leg adds 1 to trips[L][c][0] and A + g to
 * trips[L][c][1] and raises trips[L][c][2] to A + g.  accumulate = 0: trips counts from zero, every element written;
 * 1: it goes on from what the array holds (non-negative), so a stream's calls give one call's numbers.  Integer
 * atomics: the same under every schedule.  A carried last_zone >= nzones is no zone of this table: its leg is
 * written per row as above and adds no trip.
 *
 * LIDAR_EINVAL: a null handle, people, k, prev, zones or output; frames < 0 or > 65535, cap < 1, frames * cap >=
 * 2^31; carry outside 0 .. frames; nzones outside 1 .. 64; accumulate not 0 or 1.  frames == carry returns LIDAR_OK
 * and writes no row; with accumulate = 0 it still zeroes trips. */
int lidar_track_routes_f64(lidar_handle *h, const double *people, const int64_t *k, const int32_t *prev,
                           const int32_t *gap, int64_t frames, int64_t cap, int64_t carry, const double *zones,
                           int32_t nzones, int32_t *first_zone, int32_t *last_zone, int32_t *away, int32_t *legs,
                           int32_t *leg_from, int32_t *leg_frames, int64_t *trips, int32_t accumulate, void *stream);

/* Crowding (csrc/track_crowding.hip; DESIGN.md §3 "Crowding", §4.15): per tracked person the number of people
 * within a radius, the nearest one and the distance to it, the local density, and the variance of the velocities
 * around it with their product, the crowd pressure; per frame and per venue cell the counts above two limits and
 * the peaks.  Asynchronous like its siblings: every pointer a device pointer, no host synchronisation, nothing
 * read back, no host-staged parameter block, no scratch; no output depends on an earlier call.  All arithmetic
 * fp64, one rounding per operation, the square root and the divisions correctly rounded.
 *
 * lidar_track_crowding_f64: people, k, frames, cap and K_t as lidar_track_people_f64; prev (frames, cap) int32 and
 * velocity (frames, cap, 2) as lidar_track_people_f64 / lidar_track_stream_f64 leave them.  Only the frames
 * t >= first are evaluated (with a carry in front: first = carry, as lidar_track_events_f64), each on its own.
 * valid(j): j < K_t and both coordinates finite.  moving(j): valid(j) and prev[t][j] >= 0 and both velocity
 * components finite.  d(i, j) = (dx*dx) + (dy*dy), dx = P[i].x - P[j].x, dy = P[i].y - P[j].y.  near(i, j): i != j,
 * valid(i) and d <= R*R, R = radius (inclusive; R*R one product); d(i, j) and d(j, i) have the same bits, so near
 * is symmetric.
 * Per row, arrays (frames - first, cap) indexed by t - first, every element written; for a valid row j:
 *   neighbours int32 = #{i : near(i, j)};
 *   nearest int32 = the valid i != j with finite d and the smallest (d, i), lexicographic, over the whole frame
 *     (not only within R); -1 without one;
 *   spacing fp64 = sqrt(d(nearest, j)); +inf where nearest == -1;
 *   density fp64 = (double)(neighbours + 1) / ((pi * R) * R), pi = M_PI, the two products in that order;
 *   movers int32 = m = |M_j|, M_j = {i : moving(i) and (i == j or near(i, j))};
 *   variance fp64: sx, sy, sq = the sums of vx, vy and (vx*vx) + (vy*vy) over M_j, each added sequentially in
 *     ascending i from +0.0 (row j in its own place); m >= 2: mx = sx / m, my = sy / m,
 *     var = (sq / m) - ((mx*mx) + (my*my)), a non-NaN var that is not > 0.0 becomes +0.0; m < 2: +0.0;
 *   pressure fp64 = density * variance.
 * A row j < K_t that is not valid gets neighbours 0, nearest -1, spacing +inf, movers 0 and 0.0 for the three
 * other doubles and is counted nowhere below; a row at or past K_t the same with neighbours -1.  A NaN's payload
 * and sign are free.
 * crowded (frames - first, 2) int32: the valid rows with density >= density_limit, with pressure >=
 * pressure_limit.  peaks (frames - first, 3) fp64: the largest density and the largest pressure over the valid
 * rows (from +0.0, replaced under >: a NaN never wins), the smallest spacing (from +inf, replaced under <).
 * Cells, with nx > 0 (nx == 0: no cell output, the grid arguments and cell pointers unused): the grid
 * (x0, y0, grid, nx, ny) is lidar_flow_cells_f64's, a row outside it dropped.  cell_peak (nx, ny, 2) fp64: the
 * largest density and pressure, cell_crowded (nx, ny) int32: the number with density >= density_limit, of the
 * valid rows of the frames >= first, each binned by its own position.  accumulate = 0 starts from 0; 1 goes on
 * from the stored values (non-negative, not NaN: what a call leaves), so a stream's calls give the bits of one
 * call over the whole sequence.  Every result is the same under every schedule.
 *
 * LIDAR_EINVAL: a null handle, people, k, prev, velocity or per-row / per-frame output; frames < 0 or > 65535,
 * cap < 1, frames * cap >= 2^31; first outside 0 .. frames; radius not positive and finite; a limit that is NaN
 * or negative (+inf: never); accumulate not 0 or 1; nx < 0; with nx > 0 the grid conditions of
 * lidar_flow_cells_f64 or a null cell_peak / cell_crowded.  frames == first returns LIDAR_OK and writes nothing. */
int lidar_track_crowding_f64(lidar_handle *h, const double *people, const int64_t *k, const int32_t *prev,
                             const double *velocity, int64_t frames, int64_t cap, int64_t first, double radius,
                             double density_limit, double pressure_limit, double x0, double y0, double grid,
                             int64_t nx, int64_t ny, int32_t accumulate, int32_t *neighbours, int32_t *nearest,
                             double *spacing, double *density, int32_t *movers, double *variance, double *pressure,
                             int32_t *crowded, double *peaks, double *cell_peak, int32_t *cell_crowded,
                             void *stream);

/* the density grid + statistics + hotspots of every frame with K_f > 0.  jobs: device
 * double[8 * frames] rows (xa = x_min - 2g, ya = y_min - 2g, g, nx, ny (lidar_grid_dims),
 * output offset, scratch offset, 0); out at a frame's offset: grid_x (nx) | grid_y (ny) |
 * density (nx*ny) | flat_x | flat_y | stats (8) | hot (5 int64); scratch_doubles = sum over
 * frames of nx*ny + ceil(nx*ny/2) + nx + ny + 2.  Asynchronous. */
int lidar_density_batch_f64(lidar_handle *h, const double *people, const int64_t *offsets,
                            const int64_t *kdev, int32_t frames, const double *jobs, double *out,
                            int64_t scratch_doubles, void *stream);

/* people positions (extract_people_positions, utils/data_processing.py:251-280):
 * centroid (x, y) of every label >= 0, sequential index-order sums;
 * people (n,2) f64, *k_host receives K (synchronises). */
int lidar_people_f64(lidar_handle *h, const double *xyz, const int64_t *labels, int64_t n,
                     double *people, int64_t *k_host, void *stream);

/* grid density (calculate_grid_density, utils/data_processing.py:282-328, and the statistics
 * of CrowdDensityModel.analyze, models/crowd_density_model.py:56-82): np.arange edges
 * a + i*((a+g)-a), histogram2d binning (searchsorted right, last edge closed), /g^2.
 * lidar_grid_dims gives nx, ny (host arithmetic of np.arange's length).  Outputs: grid_x (nx),
 * grid_y (ny); `density` must hold 3*nx*ny + 13 doubles laid out as
 *   density (nx*ny) | flat_x (nx*ny) | flat_y (nx*ny) | stats (8) | hotspot index (5, int64)
 * stats = [max, avg of occupied cells (numpy pairwise mean), threshold, n_hotspots,
 * n_occupied, k].  Synchronises `stream`. */
int lidar_grid_dims(double xmin, double xmax, double ymin, double ymax, double grid,
                    int64_t *nx, int64_t *ny);
int lidar_density_grid_f64(lidar_handle *h, const double *people, int64_t k, double xmin,
                           double xmax, double ymin, double ymax, double grid, int64_t nx,
                           int64_t ny, double *grid_x, double *grid_y, double *density,
                           void *stream);

#ifdef __cplusplus
}
#endif
#endif
