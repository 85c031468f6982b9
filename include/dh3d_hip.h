/*
 * dh3d_hip.h -- C ABI of libdh3d_hip.so, the MI355X (gfx950) implementation of the DH3D
 * point-cloud feature-extraction hot path.
 *
 * Contract (every entry point):
 *   - plain device pointers + sizes, no framework types; `stream` is a hipStream_t passed as void*;
 *   - returns an int status (DH3D_OK = 0); never throws, never allocates or frees device memory,
 *     never synchronises the device; all work is enqueued on `stream` (graph-capturable);
 *   - the caller owns every buffer including scratch; gradient outputs of the reference's operators are zeroed by
 *     the library (hipMemsetAsync on `stream`), as the reference kernels do with cudaMemset.  The ACCUMULATORS of the
 *     training step's internal kernels (statistics partials and scatter targets of dh3d_bn_colstats / dh3d_bn_bwd_sums /
 *     dh3d_interp_bn_* / dh3d_netvlad_commuted_*, marked "zeroed by the CALLER" below) are not: a step takes all of them
 *     from one arena that it clears with ONE fill (each hipMemsetAsync is a ~4 us launch of its own; there were ~30);
 *   - float32 + int32 (the six flex operators of section A also for double: *_f64); re-entrant, no global mutable
 *     state.
 *
 * Section A are drop-ins for the reference's TF custom ops, in the reference's tensor layouts
 * (user_ops: channels-first [B,C,N]; tf_ops: channels-last [B,N,C]).  Section B are the fused
 * point-major ([B,N,C]) kernels the dh3d_amd model path is built from; they compute the same
 * functions (see each comment) with layouts chosen for gfx950.
 *
 * Reference citations are file:line in the upstream DH3D tree.
 */
#ifndef DH3D_HIP_H_
#define DH3D_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DH3D_OK 0
#define DH3D_ERR_INVALID_ARGUMENT 1 /* what TF reports as errors::InvalidArgument */
#define DH3D_ERR_UNSUPPORTED 2      /* shape outside what the kernels implement    */
#define DH3D_ERR_LAUNCH 3           /* hipGetLastError() != success after a launch  */

#define DH3D_ACT_NONE 0
#define DH3D_ACT_RELU 1
#define DH3D_ACT_SIGMOID 2

/* Library / build identification. */
int dh3d_version(void);                 /* 100*major + minor */
/* Bumped whenever the MEANING of an existing entry point changes under an unchanged signature (which a linker cannot
 * see).  History: 1 = rounds 1-2; 2 = the accumulators of dh3d_bn_colstats / dh3d_bn_bwd_sums / dh3d_interp_bn_colstats /
 * dh3d_interp_bn_bwd_sums / dh3d_interp_bn_bwd_apply are no longer zeroed by the library ("zeroed by the CALLER");
 * 3 (round 4) = dh3d_knn_grid takes the three outputs of dh3d_spatial_sort_cells (sorted, gbox, cells), serves any
 * N <= 16384 and hands clouds the sort flags as crowded (cells[4106]) to the pruned scan; 4 (round 5) = the cell table
 * describes a grid whose 12 code bits are dealt to the axes by extent (cells[4103..4105] = 2^(nb+2)/extent, cells[4107] =
 * the bit schedule; see dh3d_spatial_sort_cells) and dh3d_knn_grid reads that header.
 * A binding compares it with the DH3D_ABI_VERSION it was written against and refuses to run on a mismatch
 * (dh3d_amd/_lib.py does). */
#define DH3D_ABI_VERSION 4
int dh3d_abi_version(void);
const char *dh3d_arch(void);            /* "gfx950" */
/* First 16 hex digits of sha256 over (basename, content) of dh3d_amd/csrc/{*.hip, *.h, Makefile} and this header, sorted by
 * path as the Makefile's $(sort ...) orders them -- baked in at build time so that a binding (dh3d_amd/_lib.py
 * tree_source_hash, tests/test_abi.py) can tell a library built from THIS tree from a stale one that travelled with it. */
const char *dh3d_source_hash(void);
const char *dh3d_status_string(int st); /* static string */

/* Staging copy on the given stream by a KERNEL (not a copy engine): `src` / `dst` are device pointers or PINNED host
 * pointers (device-addressable: hipHostMalloc / torch pin_memory), 16-byte aligned.  For the serving loop around the hot
 * path (the reference feeds numpy arrays and saves numpy arrays: localdesc_extract.py:106-138, globaldesc_extract.py:84-100):
 * the batch goes host -> slot buffer and the descriptors slot buffer -> host on the SAME compute queue as the step, so no
 * engine-to-engine hand-over sits on the step's chain.  device_to_device != 0: both are device buffers (the launch is
 * sized for HBM instead of for the host link).  No reference counterpart (TF's feed_dict / fetches). */
int dh3d_stage_copy(const void *src, void *dst, size_t bytes, int device_to_device, void *stream);

/* ===================================================================================== *
 * A. Drop-in operators (reference layouts)
 * ===================================================================================== */

/* KnnBruteforce -- replaces KnnBruteforceFunctor<GPUDevice,float,int>
 * (user_ops/kernels/knn_bruteforce_kernel_gpu.cu.cc:163-228; op user_ops/ops/knn_bruteforce.cc:11-35).
 * positions [B,Dp,N] -> nn [B,N,K] int32, dist [B,N,K] (Euclidean, ascending; self at rank 0).
 * Bit-exact ids incl. the CUB tie order.  1 <= Dp <= 16 (Dp = 3: the fast kernels), 1 <= K <= 64.  N > 8192 (unsupported
 * upstream) is accepted with the ladder continued as (1024, ceil(N/1024)). */
int dh3d_knn_bruteforce(const float *positions, int B, int Dp, int N, int K, int32_t *nn,
                        float *dist, void *stream);

/* Same function on point-major coordinates xyz [B,N,3] (the layout the model holds clouds in,
 * core/model.py:146); saves the transpose of core/model.py:157. */
int dh3d_knn_bruteforce_xyz(const float *xyz, int B, int N, int K, int32_t *nn, float *dist,
                            void *stream);
/* The kernel dh3d_knn_bruteforce runs for (B, Dp, N, K) -- dh3d_knn_bruteforce_xyz: Dp = 3 -- from the same functions the
 * launchers use; host only, no GPU needed.  Returns family * 65536 + a * 256 + b, or -1 where the entry would refuse the
 * shape (K > 64, B > 65535, Dp > 16, a size <= 0):
 *   family 1 (Dp = 3, N <= 2048): a wave per query.  a = CPL, the candidates per lane (8: N <= 512, 16: N <= 1024, 32),
 *            b = Q, the queries per wave (2 while B * N <= 16384, else 4);
 *   family 2 (Dp = 3, N > 2048):  a lane per query.  a = 0, b = KMAX, the K-list width (4 / 8 / 16 / 32 / 64 >= K);
 *   family 3 (Dp != 3):           the any-Dp kernel.  a = 0, b = KMAX (8 / 16 / 64 >= K). */
int dh3d_knn_bruteforce_plan(int B, int Dp, int N, int K);

/* FlexConv -- replaces FlexConvFunctor<GPUDevice,float> (flex_conv_kernel_gpu.cu.cc:392-441;
 * op user_ops/ops/flex_conv.cc:25-83).  Argument order is the functor's:
 * features [B,Din,N], theta [Dp,Din,Dout], bias [Din,Dout], neighborhood [B,K,N] int32,
 * positions [B,Dp,N] -> output [B,Dout,N].  Centre point = point n (gpu.cu.cc:77-79). */
int dh3d_flex_conv_fwd(const float *features, const float *theta, const float *bias,
                       const int32_t *neighborhood, const float *positions, int B, int N, int K,
                       int Dp, int Din, int Dout, float *output, void *stream);

/* FlexConvGrad -- replaces FlexConvGrad<GPUDevice,float> (flex_conv_kernel_gpu.cu.cc:446-548).
 * Centre point = rank-0 neighbour (gpu.cu.cc:196-202,314).  Zeroes the three outputs first. */
int dh3d_flex_conv_bwd(const float *features, const float *theta, const float *bias,
                       const int32_t *neighborhood, const float *positions, const float *topdiff,
                       int B, int N, int K, int Dp, int Din, int Dout, float *grad_features,
                       float *grad_theta, float *grad_bias, void *stream);

/* FlexPool -- replaces FlexPoolFunctor<GPUDevice,float> (flex_pool_kernel_gpu.cu.cc:100-125).
 * features [B,D,N], neighborhood [B,K,N] -> output [B,D,N], argmax [B,D,N] (global point id). */
int dh3d_flex_pool_fwd(const float *features, const int32_t *neighborhood, int B, int N, int K,
                       int D, float *output, int32_t *argmax, void *stream);

/* FlexPoolGrad -- replaces FlexPoolGrad<GPUDevice,float> (flex_pool_kernel_gpu.cu.cc:131-157). */
int dh3d_flex_pool_bwd(const float *topdiff, const int32_t *argmax, int B, int N, int D,
                       float *grad_features, void *stream);

/* ConvPointset -- replaces ConvPointsetFunctor<GPUDevice,float>
 * (conv_pointset_kernel_gpu.cu.cc:354-402).  features [B,Din,N], theta [Din,Dout], bias [Dout],
 * neighborhood [B,K,N] -> output [B,Dout,N]; bias added once (the CPU functor's rule,
 * conv_pointset_kernel.cc:60). */
int dh3d_conv_pointset_fwd(const float *features, const float *theta, const float *bias,
                           const int32_t *neighborhood, int B, int N, int K, int Din, int Dout,
                           float *output, void *stream);

/* ConvPointsetGrad -- replaces ConvPointsetGrad<GPUDevice,float> (gpu.cu.cc:408-503). */
int dh3d_conv_pointset_bwd(const float *features, const float *theta,
                           const int32_t *neighborhood, const float *topdiff, int B, int N, int K,
                           int Din, int Dout, float *grad_features, float *grad_theta,
                           float *grad_bias, void *stream);

/* The same six operators for double (the reference registers float AND double kernels, flex_conv_op.cc:97-106 /
 * flex_pool_op.cc / conv_pointset_op.cc, and its gradient tests run in double, test_flex_convolution.py:93-115): the
 * reference formulation of csrc/flex_generic.hip instantiated for double, any shape. */
int dh3d_flex_conv_fwd_f64(const double *features, const double *theta, const double *bias, const int32_t *neighborhood,
                           const double *positions, int B, int N, int K, int Dp, int Din, int Dout, double *output,
                           void *stream);
int dh3d_flex_conv_bwd_f64(const double *features, const double *theta, const double *bias, const int32_t *neighborhood,
                           const double *positions, const double *topdiff, int B, int N, int K, int Dp, int Din, int Dout,
                           double *grad_features, double *grad_theta, double *grad_bias, void *stream);
int dh3d_flex_pool_fwd_f64(const double *features, const int32_t *neighborhood, int B, int N, int K, int D, double *output,
                           int32_t *argmax, void *stream);
int dh3d_flex_pool_bwd_f64(const double *topdiff, const int32_t *argmax, int B, int N, int D, double *grad_features,
                           void *stream);
int dh3d_conv_pointset_fwd_f64(const double *features, const double *theta, const double *bias,
                               const int32_t *neighborhood, int B, int N, int K, int Din, int Dout, double *output,
                               void *stream);
int dh3d_conv_pointset_bwd_f64(const double *features, const double *theta, const int32_t *neighborhood,
                               const double *topdiff, int B, int N, int K, int Din, int Dout, double *grad_features,
                               double *grad_theta, double *grad_bias, void *stream);

/* FlexDeconv -- replaces FlexDeconvFunctor / FlexDeconvGrad (op user_ops/ops/flex_deconv.cc; exposed as
 * user_ops.flex_convolution_transpose).  Argument order and layouts are FlexConv's: features [B,Din,N], theta
 * [Dp,Din,Dout], bias [Din,Dout], neighborhood [B,K,N] int32, positions [B,Dp,N] -> output [B,Dout,N].  Every source point
 * n spreads its centre s = nbr[b,0,n] to its targets m = nbr[b,k,n] (k = 0 included):
 *   out[b,:,m] += sum_din f[b,din,s] (bias[din,:] + sum_dp theta[dp,din,:] (p[b,dp,m] - p[b,dp,s])).
 * A point no list names gets 0.  The reference formulation (csrc/flex_deconv.hip), any shape, Dp <= 4; f32 / f64 atomics
 * into the outputs, which the library zeroes first.  The backward returns the gradients of all three parameters. */
int dh3d_flex_deconv_fwd(const float *features, const float *theta, const float *bias, const int32_t *neighborhood,
                         const float *positions, int B, int N, int K, int Dp, int Din, int Dout, float *output,
                         void *stream);
int dh3d_flex_deconv_bwd(const float *features, const float *theta, const float *bias, const int32_t *neighborhood,
                         const float *positions, const float *topdiff, int B, int N, int K, int Dp, int Din, int Dout,
                         float *grad_features, float *grad_theta, float *grad_bias, void *stream);
int dh3d_flex_deconv_fwd_f64(const double *features, const double *theta, const double *bias,
                             const int32_t *neighborhood, const double *positions, int B, int N, int K, int Dp, int Din,
                             int Dout, double *output, void *stream);
int dh3d_flex_deconv_bwd_f64(const double *features, const double *theta, const double *bias,
                             const int32_t *neighborhood, const double *positions, const double *topdiff, int B, int N,
                             int K, int Dp, int Din, int Dout, double *grad_features, double *grad_theta,
                             double *grad_bias, void *stream);

/* FarthestPointSample -- replaces farthestpointsamplingLauncher (tf_ops/sampling/tf_sampling.cpp:94,
 * tf_sampling_g.cu:105-170,203-205).  inp [B,N,3] -> out [B,m] int32, first pick 0, bit-exact tie
 * order.  `temp` is the reference's scratch (tf_sampling.cpp:115 allocates [32,N]): for N <= 16384 the
 * running min-distances live in registers and it may be NULL; above that it must hold B*N floats. */
int dh3d_farthest_point_sample(int B, int N, int m, const float *inp, float *temp, int32_t *out,
                               void *stream);

/* Same op with the rounding of d = (x2-x1)^2+(y2-y1)^2+(z2-z1)^2 (tf_sampling_g.cu:141) selectable:
 * contract = 1: fma(dz,dz,fma(dx,dx,dy*dy)) -- the LLVM/NVVM contraction, what the kernels above compute;
 * contract = 0: (dx*dx+dy*dy)+dz*dz -- an nvcc -fmad=false build.  Which one a given reference binary
 * used cannot be checked without nvcc (parity unpinned); an integrator who can check picks here.
 * Any N; temp [B*N] floats is REQUIRED (the running min-distances, as upstream). */
int dh3d_farthest_point_sample_mode(int B, int N, int m, const float *inp, float *temp, int32_t *out,
                                    int contract, void *stream);

/* GroupPoint / GroupPointGrad -- replace groupPointLauncher / groupPointGradLauncher
 * (tf_ops/grouping/tf_grouping.cpp:208-274, tf_grouping_g.cu:94-132).
 * points [b,n,c], idx [b,m,nsample] -> out [b,m,nsample,c]. */
int dh3d_group_point_fwd(int b, int n, int c, int m, int nsample, const float *points,
                         const int32_t *idx, float *out, void *stream);
int dh3d_group_point_bwd(int b, int n, int c, int m, int nsample, const float *grad_out,
                         const int32_t *idx, float *grad_points, void *stream);

/* QueryBallPoint / QueryBallPoint2 -- replace queryBallPointLauncher / queryBallPoint2Launcher
 * (tf_ops/grouping/tf_grouping.cpp:86-165, tf_grouping_g.cu:3-92,179-186; CPU twin test/query_ball_point.cpp:19-47).
 * xyz1 [b,n,3] (dataset), xyz2 [b,m,3] (queries) -> idx [b,m,nsample], pts_cnt [b,m].
 * ROW FORMAT: per query, over the dataset points in index order, d = max(sqrtf(dx*dx + dy*dy + dz*dz), 1e-20f) and a hit is
 * d < radius (strict); the row holds the min(hits, nsample) SMALLEST hit indices in ascending order, then the first of them
 * repeated; pts_cnt = min(hits, nsample).
 * EMPTY BALL: the row is nsample copies of the index of the point nearest to this query (same d, strict <, lowest index on
 * ties), pts_cnt = 0 -- the twin leaves such a row unwritten, the CUDA kernel writes a nearest point that queries
 * j >= 256 inherit from other queries.
 * ROUNDING: the twin's, ((dx*dx + dy*dy) + dz*dz) in f32 without fma contraction and an IEEE sqrtf.
 * dh3d_query_ball_point: one radius > 0.  dh3d_query_ball_point2: radii [b,m], one per query; a radius <= 0 or NaN has no
 * hits.  Both run the scan kernel (lane = query, the cloud staged through LDS in index order, a wave leaves when all its
 * balls are full): any n, m, nsample. */
int dh3d_query_ball_point(int b, int n, int m, float radius, int nsample, const float *xyz1, const float *xyz2,
                          int32_t *idx, int32_t *pts_cnt, void *stream);
int dh3d_query_ball_point2(int b, int n, int m, int nsample, const float *xyz1, const float *xyz2, const float *radii,
                           int32_t *idx, int32_t *pts_cnt, void *stream);
/* The same rows bit for bit by cell lists: sorted1 / gbox1 / cells1 are the three outputs of dh3d_spatial_sort_cells(xyz1),
 * n <= 16384.  radius_or_radii is DEVICE memory: one float (per_query = 0) or radii [b,m] (per_query = 1).  One wave per
 * query tests the records of the cells that the ball's axis-aligned box meets and marks the hits in a bit set over original
 * indices in LDS, whose nsample lowest bits are the row.  A box of more than 512 cells and a cloud the sort flagged as
 * crowded (cells[4106]) go over the 64-point groups whose box (gbox1) the ball meets; an empty ball scans the cloud for
 * its nearest point. */
int dh3d_query_ball_point_grid(int b, int n, int m, const float *radius_or_radii, int per_query, int nsample,
                               const float *sorted1, const float *gbox1, const int32_t *cells1, const float *xyz2,
                               int32_t *idx, int32_t *pts_cnt, void *stream);
/* Which of the two serves (n, m, nsample) in the operator: 0 the scan, 1 sort + cell lists, -1 a shape both refuse.  Host
 * only; looks at the shape alone, never at the batch or the data. */
int dh3d_query_ball_point_plan(int n, int m, int nsample);

/* SelectionSort (select_top_k) and KnnPoint -- replace selectionSortLauncher and the tile + reduce_sum + SelectionSort
 * composition of knn_point (tf_ops/grouping/tf_grouping.py:37-47,63-88, tf_grouping.cpp:50-58,175-206,
 * tf_grouping_g.cu:134-177).
 * dh3d_select_top_k: dist [b,m,n] -> outi [b,m,n] int32, out [b,m,n], 1 <= k <= n; out / outi must not overlap dist.
 * dh3d_knn_point: xyz1 [b,n,c] (dataset), xyz2 [b,m,c] (queries), c >= 1 -> val [b,m,k] (SQUARED distances, no root is
 * ever taken), idx [b,m,k] int32: the first k columns of dh3d_select_top_k on D[b,j,i] = sum_c (xyz1[b,i,c] - xyz2[b,j,c])^2,
 * which is never written to memory.
 * ROW FORMAT: a row is the reference's partial selection sort of that row, and the WHOLE row is the result: start from
 * out = dist, outi = 0 .. n-1; for s = 0 .. k-1 find the first position t >= s holding the smallest value (strict <) and
 * swap positions s and t of both arrays.  Entries from k on are the inputs where no swapped-out entry landed.
 * TIE ORDER: the swap walk's, reproduced exactly -- NOT lowest id first: a swapped-out entry re-enters at a higher
 * position and is then met later than entries of the same value with a higher id.  -0 and +0 are one value.  The kernels
 * scan a row once for the min(k, n-k) smallest (value, position) keys over the positions >= k and replay the walk on them
 * and the positions 0 .. k-1: nothing else ever moves (tests/test_knn_point_reference.py proves that on tie-heavy rows).
 * ROUNDING: every difference and every square is rounded to f32 on its own, without fma contraction, and the squares are
 * added left to right over c.  For c = 3 that is what the reference's reduce_sum of three elements does; for larger c the
 * order of its Eigen reduction cannot be read from the source: left to right is INFERRED there.
 * NaN and infinite inputs are outside the contract.  Both take the caller's stream, synchronise nothing and allocate
 * nothing.  dh3d_select_top_k serves every k <= n; dh3d_knn_point refuses k > 1024 (status 2). */
int dh3d_select_top_k(int b, int n, int m, int k, const float *dist, int32_t *outi, float *out, void *stream);
int dh3d_knn_point(int b, int n, int m, int c, int k, const float *xyz1, const float *xyz2, float *val, int32_t *idx,
                   void *stream);
/* Which kernel serves (n, m, c, k) in dh3d_knn_point: 1 the fused kernel (c = 3, k <= 64: the dataset streamed through
 * LDS past 16 queries per workgroup), 0 the generic one (any c, k <= 1024: a workgroup per query), -1 a shape it refuses.
 * Host only; looks at these four numbers alone, never at the batch or the data. */
int dh3d_knn_point_plan(int n, int m, int c, int k);

/* ThreeNN -- replaces threenn_cpu (tf_ops/interpolation/tf_interpolate.cpp:60-103).
 * xyz1 [b,n,3], xyz2 [b,m,3] -> dist [b,n,3] (SQUARED, ascending), idx [b,n,3]. */
int dh3d_three_nn(int b, int n, int m, const float *xyz1, const float *xyz2, float *dist,
                  int32_t *idx, void *stream);

/* ThreeInterpolate / Grad -- replace threeinterpolate_cpu / threeinterpolate_grad_cpu
 * (tf_interpolate.cpp:107-153).  points [b,m,c], idx/weight [b,n,3] -> out [b,n,c]. */
int dh3d_three_interpolate_fwd(int b, int m, int c, int n, const float *points,
                               const int32_t *idx, const float *weight, float *out, void *stream);
int dh3d_three_interpolate_bwd(int b, int n, int c, int m, const float *grad_out,
                               const int32_t *idx, const float *weight, float *grad_points,
                               void *stream);

/* ---- A'. The same operators on the fast kernels (reference layouts, caller-provided workspace) ----
 * FlexConv / FlexConvGrad / FlexPool with the signatures above + (workspace, workspace_bytes): the channels-first
 * tensors are transposed through LDS tiles into the workspace, the fused point-major MFMA kernels of section B run
 * (flex_conv: the bf16x6 pipeline for K = 8, Dout = 64, Din in {32, 64}; the exact-f32 MFMA kernel for the other
 * DH3D shapes; for ANY other Din, Dout that are multiples of four the same factorisation in two launches -- S =
 * [S0|Sx|Sy|Sz] materialised in the workspace, then S @ [bias; theta] on the GEMM kernels: 0.07 ms at 48 -> 96,
 * 8 x 8192, K = 8, against ~3 ms of the reference formulation), and the result is transposed back.  Same function as the section-A entry (forward centres on
 * point n, backward on the rank-0 neighbour); summation order differs (factorised form), within the reference's own
 * CPU-vs-GPU tolerance.  *_workspace_bytes returns 0 when the shape is not served -- use the section-A entry then.
 * The backward is  dWcat = S^T dOut,  dS = dOut Wcat^T  on the f32 MFMA pipe + an atomics scatter of dS over the
 * neighbour lists (the reference's feature gradient is atomics too, flex_conv_kernel_gpu.cu.cc:250-385). */
size_t dh3d_flex_conv_fwd_workspace_bytes(int B, int N, int K, int Dp, int Din, int Dout);
/* Which forward serves a shape in dh3d_flex_conv_fwd_ws: 3 the persistent bf16x6 kernel (Dp = 3, K = 8, Dout = 64, Din in
 * {32, 64}), 1 the fused f32-MFMA kernel (the seven DH3D (Din, Dout) pairs, any K), 2 flex_S + GEMM (any other Din, Dout
 * that are multiples of four), 0 not served: dh3d_flex_conv_fwd_workspace_bytes is 0 and the section-A entry runs (Dp != 3,
 * N = 1, other channel counts, extents beyond the kernels' 32-bit indices).  Host only; looks at the shape alone, never
 * at the data. */
int dh3d_flex_conv_fwd_plan(int B, int N, int K, int Dp, int Din, int Dout);
int dh3d_flex_conv_fwd_ws(const float *features, const float *theta, const float *bias,
                          const int32_t *neighborhood, const float *positions, int B, int N, int K, int Dp,
                          int Din, int Dout, float *output, void *workspace, size_t workspace_bytes, void *stream);
size_t dh3d_flex_conv_bwd_workspace_bytes(int B, int N, int K, int Dp, int Din, int Dout);
int dh3d_flex_conv_bwd_ws(const float *features, const float *theta, const float *bias,
                          const int32_t *neighborhood, const float *positions, const float *topdiff, int B, int N,
                          int K, int Dp, int Din, int Dout, float *grad_features, float *grad_theta,
                          float *grad_bias, void *workspace, size_t workspace_bytes, void *stream);
size_t dh3d_flex_pool_fwd_workspace_bytes(int B, int N, int K, int D);
int dh3d_flex_pool_fwd_ws(const float *features, const int32_t *neighborhood, int B, int N, int K, int D,
                          float *output, int32_t *argmax, void *workspace, size_t workspace_bytes, void *stream);

/* FlexDeconv / its gradient on the fast kernels, signatures of section A + (workspace, workspace_bytes).  Shapes:
 * Dp = 3, Din % 4 == 0, Dout % 4 == 0 (else, or when a buffer would overflow, *_workspace_bytes returns 0: use section A).
 * The factorised form of FlexConv read through INVERTED neighbour lists (a CSR per cloud, built in the workspace, every
 * list in ascending edge order n*K + k): forward out = S' @ [bias; theta] with S' = flex_conv's S summed over each
 * point's inverted list; backward Q = flex_conv's S of the upstream gradient centred on rank 0, summed over the rank-0
 * inverted lists, then two GEMMs.  No atomics but the weight gradients' split-K GEMM: the output and grad_features are
 * bitwise reproducible (for 4*Din resp. 4*Dout <= 256, where the GEMM's reduction is not split). */
size_t dh3d_flex_deconv_fwd_workspace_bytes(int B, int N, int K, int Dp, int Din, int Dout);
int dh3d_flex_deconv_fwd_ws(const float *features, const float *theta, const float *bias,
                            const int32_t *neighborhood, const float *positions, int B, int N, int K, int Dp,
                            int Din, int Dout, float *output, void *workspace, size_t workspace_bytes, void *stream);
size_t dh3d_flex_deconv_bwd_workspace_bytes(int B, int N, int K, int Dp, int Din, int Dout);
int dh3d_flex_deconv_bwd_ws(const float *features, const float *theta, const float *bias,
                            const int32_t *neighborhood, const float *positions, const float *topdiff, int B, int N,
                            int K, int Dp, int Din, int Dout, float *grad_features, float *grad_theta,
                            float *grad_bias, void *workspace, size_t workspace_bytes, void *stream);

/* ===================================================================================== *
 * B. Fused point-major kernels (model path)
 *    Activations are [B,N,C] (C contiguous).  Neighbourhoods are [B,N,K] (the kNN op's native
 *    output, knn_bruteforce_op.cc:44-49).  Every kernel can apply the per-channel epilogue
 *        y = act( scale[c] * (x + pre_bias[c]) + shift[c] )
 *    which folds feature_bias (core/layers.py:330-331), inference BatchNorm
 *    (core/tf_utils.py:60-63) and the activation; scale/shift/pre_bias may be NULL.
 * ===================================================================================== */

typedef struct dh3d_epilogue {
  const float *pre_bias; /* [C] or NULL */
  const float *scale;    /* [C] or NULL */
  const float *shift;    /* [C] or NULL */
  int act;               /* DH3D_ACT_* */
} dh3d_epilogue;

/* Packs a row-major weight W [Kd, Dout] (Kd%8==0, Dout%32==0) into the MFMA fragment order the
 * GEMM kernels stream: out[(nb*KB+kb)*256 + lane*4 + t] = W[kb*8 + 4*(lane>>5) + t][nb*32 + (lane&31)].
 * For flex_conv, W is the stacked [bias; theta_x; theta_y; theta_z] of shape [4*Din, Dout]. */
int dh3d_pack_weight(const float *W, int Kd, int Dout, float *packed, void *stream);
/* Stacks flex_conv parameters theta [3,Din,Dout], bias [Din,Dout] into packed [4*Din,Dout]. */
int dh3d_pack_flex_weight(const float *theta, const float *bias, int Din, int Dout, float *packed,
                          void *stream);

/* Spatial (Morton) ordering of each cloud -- a preprocessing step with no reference counterpart that
 * changes no result; it lets kNN and FPS skip work exactly (csrc/spatial.hip).
 * xyz [B,N,3] -> sorted [B,N,4] records (x, y, z, bits(original index)) in Morton order, and
 * gbox [B, ceil(N/64), 8] = (min xyz, 0, max xyz, 0) of every 64 consecutive records.  N <= 16384. */
int dh3d_spatial_sort(const float *xyz, int B, int N, float *sorted, float *gbox, void *stream);

/* KnnBruteforce on an ordered cloud: identical outputs to dh3d_knn_bruteforce_xyz (ids are ORIGINAL point
 * indices, rows are in original query order); candidate groups whose box is provably too far are skipped. */
int dh3d_knn_sorted(const float *sorted, const float *gbox, int B, int N, int K, int32_t *nn, float *dist,
                    void *stream);
/* The kernel dh3d_knn_sorted launches for (B, N, K), from the same function the launcher uses; host only, no GPU needed.
 * Returns S * 256 + KMAX, or -1 where dh3d_knn_sorted would refuse the shape (K > 64, B > 65535, a size <= 0).
 * G = B * ceil(N / 64) query groups decide S, the waves that share one group's scan: 8 (G <= 256), 4 (G <= 1280),
 * 2 (G <= 4096), 0 = the one-wave kernel (beyond, and for every K > 16).  KMAX is the K-list width of the kernel that is
 * actually instantiated: 4 / 8 / 16 at S = 4 and 2, 8 / 16 at S = 8 (K <= 4 runs the width-8 kernel there), 4 / 8 / 16 /
 * 32 / 64 at S = 0. */
int dh3d_knn_sorted_plan(int B, int N, int K);

/* dh3d_spatial_sort that also writes the CELL TABLE of a 4096-cell grid over each cloud's bounding box: cells
 * [B, DH3D_CELL_INTS] int32.  The sort key is an 18-bit code; its top 12 bits are the GRID code, and since ABI 4 those 12
 * bits are dealt to the axes BY EXTENT -- one at a time to the axis whose cells are the widest so far (at most 6 per axis;
 * cell widths within 25 % of each other: z first, then y, then x), so axis a gets nb[a] grid bits (a cube: 4 + 4 + 4 = the
 * plain z-y-x Morton code of ABI <= 3; a 60 x 60 x 8 slab: 5 + 5 + 2) and the grid is 2^nb[0] x 2^nb[1] x 2^nb[2] cells.
 *   [0..4095]     first sorted position of every cell, cells ordered by their 12-bit code (an empty cell's entry = the
 *                 next cell's); [4096] = N
 *   [4100..4102]  as floats: the grid origin (x, y, z) = the bounding box's minimum
 *   [4103..4105]  as floats: the quantisation scale per axis, 2^(nb[a] + 2) / extent[a] (a cell = 4 quantisation steps; the
 *                 two sub-cell bits per axis are the key's low 6 bits, z y x z y x)
 *   [4106]        1 when the cloud's points crowd into fewer than 0.6 x the cells a uniform cloud of N points would occupy
 *                 (street scenes, clusters: dh3d_knn_grid then serves this cloud with the pruned scan of
 *                 dh3d_knn_sorted), else 0
 *   [4107]        the bit SCHEDULE: 12 x 2 bits, field s (bits 2s, 2s+1) = the axis (0 x, 1 y, 2 z) that grid-code bit
 *                 11 - s belongs to -- field 0 is the code's MOST significant bit; within an axis the bits appear in the
 *                 code from that axis' most significant cell-coordinate bit downwards.  0x186186 = z y x z y x ... (cube).
 *   [4097..4099], [4108..4111]  no field: written as 0 (every int of the table is written by the call)
 * To decode cell code c into per-axis cell coordinates: walk s = 0..11, append bit (c >> (11 - s)) & 1 to the coordinate of
 * axis (sched >> 2s) & 3.  A table written by an ABI <= 3 sort (no schedule, scale 64 / extent) must not be handed to an
 * ABI 4 dh3d_knn_grid.  (The device-side definitions -- slots, header decode, cell map, cell code -- live in
 * csrc/cell_grid.h.) */
#define DH3D_CELL_INTS 4112
int dh3d_spatial_sort_cells(const float *xyz, int B, int N, float *sorted, float *gbox, int32_t *cells, void *stream);

/* KnnBruteforce on that grid (cell-list search: every query scans the cells its K-th distance reaches, candidates pooled
 * per query in LDS, 4 lanes per query; csrc/knn.hip knn_grid_kernel).  Same outputs as dh3d_knn_bruteforce_xyz bit for
 * bit -- ids in the reference's (distance, CUB rank) order, IEEE distances, original point order.  K <= 8, any
 * N <= 16384 (small sets search a coarser grid: 2^D consecutive cells of the same table).  sorted / gbox / cells are the
 * three outputs of dh3d_spatial_sort_cells: a query the two cell passes cannot serve (no K-th distance after 27
 * cells, a search ball wider than two cells in x: sparse corners, outliers) restarts over the 64-point groups whose box
 * (gbox) its search ball meets; a cloud the sort flagged as crowded (cells[4106]) is served by dh3d_knn_sorted's
 * kernels instead, from the same launch sequence (same results either way). */
int dh3d_knn_grid(const float *sorted, const float *gbox, const int32_t *cells, int B, int N, int K, int32_t *nn, float *dist,
                  void *stream);
/* The launch plan dh3d_knn_grid makes for (B, N, K), from the same function the launcher uses; host only, no GPU needed.
 * Returns sf + 16 * D, or -1 where dh3d_knn_grid would refuse the shape (K > 8, N > 16384, ...).  G = B * ceil(N / 64)
 * query groups decide sf, i.e. how a cloud flagged as crowded is served:
 *   4: G <= 1280, one launch: the pruned scan inside the cell-list kernel, four waves per query group;
 *   2: G <= 4096, one launch: the same with two query groups per 256-thread workgroup, two waves each;
 *   0: beyond, two launches: the cell lists for the uniform clouds, then dh3d_knn_sorted's kernel gated on cells[4106].
 * D (0..6): the grid bits dropped for small sets -- 2^D consecutive cells of the table are searched as one. */
int dh3d_knn_grid_plan(int B, int N, int K);


/* ThreeNN on ordered clouds: identical dist / idx to dh3d_three_nn (original indexing on both sides) from the
 * dh3d_spatial_sort outputs of the query cloud (sorted1 [b,n,4], gbox1) and of the candidate set (sorted2 [b,m,4],
 * gbox2).  With 128 <= m <= 1024 and both boxes given, the candidates' 64-sample groups are pruned by their boxes (a query
 * group stages all m records and scans about half of them: 22.2 us at 8 x 8192 vs 1024, 29.5 at 32 x 4096 vs 512, uniform
 * clouds, the kernel alone); otherwise -- the boxes may be NULL -- every candidate is visited, and the ordering makes the
 * 3-deep insertion rare (a wave's queries are a compact region and its scan starts at the matching place of the
 * candidates' order). */
int dh3d_three_nn_sorted(int b, int n, int m, const float *sorted1, const float *gbox1, const float *sorted2,
                         const float *gbox2, float *dist, int32_t *idx, void *stream);
/* The same with the candidates chosen through the candidate set's CELL TABLE cells2 [b, DH3D_CELL_INTS]: the table
 * dh3d_fps_sorted_ordered writes for the sampled set on the cloud's grid, or dh3d_spatial_sort_cells of the candidate set
 * itself (queries outside that grid reach its border cells).  A 64-query group stages and scans only the samples of the
 * cells it can reach: the coarse cells (2^3 table cells each, 2^4 below 768 samples) of its box +- 1, widened once to the
 * cells its queries' third distances span -- about 130 records instead of m: 16.3 / 27.0 us at the two shapes above
 * (15.2 / 22.7 on street-scene-like clouds, where the boxes take 25.1 / 26.0; profiles/three_nn_cells.txt).  Identical
 * dist / idx to dh3d_three_nn bit for bit.  Serves 128 <= m <= 1024, n <= 16384 with gbox1 given; outside that range, or
 * with cells2 == NULL, it is dh3d_three_nn_sorted.  No workspace, no allocation: capture-safe. */
int dh3d_three_nn_cells(int b, int n, int m, const float *sorted1, const float *gbox1, const float *sorted2,
                        const float *gbox2, const int32_t *cells2, float *dist, int32_t *idx, void *stream);

/* FarthestPointSample on an ordered cloud: identical outputs to dh3d_farthest_point_sample (original
 * indices); per round only the 64-point groups the new sample can affect are re-evaluated.  N <= 12288, and the
 * by-index coordinate table plus the picks must fit one CU's LDS: 1104 + 4m + 12N <= 162816 bytes (at N = 12288:
 * m <= 3564).  Shapes beyond: DH3D_ERR_UNSUPPORTED (dh3d_fps_sorted_cloud takes them). */
int dh3d_fps_sorted(const float *sorted, const float *gbox, int B, int N, int m, int32_t *out, void *stream);
/* the same + xyz_out [B,m,3] = the sampled coordinates (group_point of the cloud by `out`, core/tf_utils.py:92-95) */
int dh3d_fps_sorted_xyz(const float *sorted, const float *gbox, int B, int N, int m, int32_t *out, float *xyz_out,
                        void *stream);
/* the same + the SAMPLED SET IN MORTON ORDER out of the same launch (round 6): sorted_s [B,m,4] records (x, y, z, bits(pick
 * rank)), gbox_s [B, ceil(m/64), 8], and -- when `cells`, the cloud's table from dh3d_spatial_sort_cells, is given (else both
 * NULL) -- cells_s [B, DH3D_CELL_INTS]: the subset's cell table on the CLOUD's grid (same origin / scales / schedule header,
 * its own crowded verdict).  The picks are a subset of a sorted cloud, so a stable compaction of the picked positions is their
 * spatial order: these are valid inputs for dh3d_three_nn_sorted (candidate side) and dh3d_knn_grid / dh3d_knn_sorted on
 * the sampled set, without dh3d_spatial_sort_cells(xyz_out) on the chain behind the sampling.  N <= 8192, and the
 * ordering's tables go beside the coordinate table: + 4(N+1) + 2((N+1) & ~1) + 24 ceil(m/64) bytes (at N = 8192: m <= 3257;
 * at dilate 2, m = N/2: N <= 8009).  Shapes beyond: DH3D_ERR_UNSUPPORTED. */
int dh3d_fps_sorted_ordered(const float *sorted, const float *gbox, const int32_t *cells, int B, int N, int m, int32_t *out,
                            float *xyz_out, float *sorted_s, float *gbox_s, int32_t *cells_s, void *stream);
/* Same with the cloud itself (xyz [B,N,3], what dh3d_spatial_sort was given): clouds of up to 16384 points (above
 * 12288 the by-index coordinate table no longer fits the LDS and the kernel reads winners from xyz).  xyz_out may be NULL. */
int dh3d_fps_sorted_cloud(const float *sorted, const float *gbox, const float *xyz, int B, int N, int m, int32_t *out,
                          float *xyz_out, void *stream);
/* 1 if the dh3d_fps_sorted* entry point selected by (ordered, with_cloud) takes N points -> m picks, else 0 (it would
 * return DH3D_ERR_UNSUPPORTED).  ordered != 0: dh3d_fps_sorted_ordered (with_cloud ignored); with_cloud != 0:
 * dh3d_fps_sorted_cloud; else dh3d_fps_sorted / dh3d_fps_sorted_xyz.  The same LDS byte count the launcher checks;
 * host only, no GPU needed. */
int dh3d_fps_sorted_fits(int N, int m, int ordered, int with_cloud);

/* flex_conv forward (same function as dh3d_flex_conv_fwd, Dp = 3) in the factorised form
 *   out[n,:] = [S0 | Sx | Sy | Sz][n,:] @ [bias; theta_x; theta_y; theta_z],
 *   S0[n,i] = sum_k f[nk,i],  Sd[n,i] = sum_k (p[nk,d]-p[n,d]) f[nk,i]
 * as one kernel: K-neighbour gather-reduce into LDS, then an exact-f32 MFMA GEMM, then epilogue.
 * features [B,N,Din], xyz [B,N,3], nbr [B,N,K], wpacked from dh3d_pack_flex_weight.
 * Din in {32,64,128}, Dout % 32 == 0, Dout <= 256. */
int dh3d_flex_conv_pm_fwd(const float *features, const float *xyz, const int32_t *nbr,
                          const float *wpacked, int B, int N, int K, int Din, int Dout,
                          const dh3d_epilogue *ep, float *out, void *stream);

/* The same operator on 32-point tiles with the tile GEMM on the bf16 matrix pipe at f32 accuracy (six bf16 products per
 * f32 product, like dh3d_flex_conv_pm_x6_fwd; csrc/flex_tx6.hip): the sampled levels' layers, whose f32-MFMA GEMM phase
 * sits at the f32 pipe's floor for one tile per CU.  wpacked_x3 from dh3d_pack_flex_weight_x3.  wpost_packed (may be
 * NULL; then Dpost / out2 are ignored): one more linear layer on the finished output tile before it leaves the chip,
 * out2 [B,N,Dpost] = out @ Wpost (dh3d_pack_weight of [Dout, Dpost], no bias / activation) -- NetVLAD's cluster logits on
 * the sampled rows of the global step (core/backbones.py:213-216, commuted through the up-sampling); Din == 128,
 * Dout == 256, Dpost == 64.
 * (Din, Dout, K) in {(64,128,8), (128,128,8), (128,256,8), (128,128,12)}. */
int dh3d_flex_conv_pm_tile_x6_fwd(const float *features, const float *xyz, const int32_t *nbr, const void *wpacked_x3,
                                  int B, int N, int K, int Din, int Dout, const dh3d_epilogue *ep, float *out,
                                  const float *wpost_packed, int Dpost, float *out2, void *stream);
/* Same with group_point fused in: `features` is the [B, Nsrc, Din] map of the level above and point j of this level
 * (xyz / nbr / out are [B, N, ...]) is its row remap[b*N + j] (remap = the farthest-point-sampling picks).  Equal to
 * dh3d_flex_conv_pm_fwd(group_point(features, remap), ...) bit for bit. */
int dh3d_flex_conv_pm_gather_fwd(const float *features, const int32_t *remap, int Nsrc, const float *xyz,
                                 const int32_t *nbr, const float *wpacked, int B, int N, int K, int Din, int Dout,
                                 const dh3d_epilogue *ep, float *out, void *stream);

/* flex_conv of the full-resolution layers on the bf16 matrix pipe with f32 accuracy (three-way bf16 split of
 * both operands, six products; see csrc/flex_x6.hip).  Same operands and result as dh3d_flex_conv_pm_fwd up
 * to f32 summation order; K == 8, (Din, Dout) in {(32,64), (64,64)}.  The weight comes from
 * dh3d_pack_flex_weight_x3 ( [bias; theta_x; theta_y; theta_z] as three bf16 planes, 6*4*Din*Dout bytes ). */
int dh3d_pack_flex_weight_x3(const float *theta, const float *bias, int Din, int Dout, void *packed, void *stream);
int dh3d_flex_conv_pm_x6_fwd(const float *features, const float *xyz, const int32_t *nbr, const void *wpacked_x3,
                             int B, int N, int K, int Din, int Dout, const dh3d_epilogue *ep, float *out,
                             void *stream);

/* Same kernel with a placement hint: reserve_cus_per_xcd CUs of every XCD are known to be held by another stream's
 * kernel with a large LDS allocation (the model's farthest-point sampling: one CU per cloud for the whole step); the
 * persistent launch leaves that many workgroups per XCD out so that all of its workgroups are resident at once
 * instead of the last ones running as a second wave.  Speed only -- results are identical for any value in [0, 31]. */
int dh3d_flex_conv_pm_x6_fwd_r(const float *features, const float *xyz, const int32_t *nbr, const void *wpacked_x3,
                               int B, int N, int K, int Din, int Dout, const dh3d_epilogue *ep,
                               int reserve_cus_per_xcd, float *out, void *stream);

/* flex_pool forward, point-major: out[n,c] = max_k f[nbr[n,k],c], argmax may be NULL. C % 4 == 0. */
int dh3d_flex_pool_pm_fwd(const float *features, const int32_t *nbr, int B, int N, int K, int C,
                          float *out, int32_t *argmax, void *stream);

/* Flex_Avg forward (core/layers.py:342-436 = flex_conv with theta 0, bias eye), point-major:
 * out[n,c] = scale * sum_k f[nbr[n,k],c]  (backbones.py:80-82 passes scale = 1/knn).  C % 4 == 0. */
int dh3d_flex_avg_pm_fwd(const float *features, const int32_t *nbr, int B, int N, int K, int C,
                         float scale, float *out, void *stream);

/* conv_pointset forward on coordinates (Din = 3), point-major, + epilogue:
 * xyz [B,N,3], theta [3,Dout], bias [Dout] -> out [B,N,Dout].  Dout % 4 == 0, Dout <= 128. */
int dh3d_conv_pointset_pm_fwd(const float *xyz, const int32_t *nbr, const float *theta,
                              const float *bias, int B, int N, int K, int Dout,
                              const dh3d_epilogue *ep, float *out, void *stream);

/* S[n] = sum_k (xyz[nbr[n,k]] - xyz[nbr[n,0]]) as [B*N, 4] floats (x, y, z, 0): the one 3-vector conv_pointset on
 * coordinates is linear in (conv_pointset_kernel.cc:46-64, Din = 3) -- out = theta^T S + bias, grad_theta = S^T grad_out
 * (ConvPointsetGrad, conv_pointset_kernel_gpu.cu.cc:157-347, as one GEMM).  K == 8. */
int dh3d_pointset_sum_pm(const float *xyz, const int32_t *nbr, int B, int N, int K, float *S, void *stream);

/* conv_pointset on the coordinates (Din = 3) -> epilogue (bias once, BatchNorm, activation) -> flex_pool over the same
 * neighbourhoods, fused (core/backbones.py:107-110; conv_pointset_kernel.cc:46-64 + flex_pool_kernel.cc:41-57): the
 * [B,N,Dout] map between the two is never materialised.  out [B,N,Dout] = max_k act(bn(conv[nbr[n,k]])).  K == 8,
 * Dout in {32, 64, 128}; scratch: B*N*4 floats (one 3-vector per point, the sum of its neighbour offsets). */
int dh3d_conv_pointset_pool_pm_fwd(const float *xyz, const int32_t *nbr, const float *theta, const float *bias, int B,
                                   int N, int K, int Dout, const dh3d_epilogue *ep, float *scratch, float *out,
                                   void *stream);

/* Per-point linear layer (the 1x1 Conv2D of core/tf_utils.py:99-109):
 *   out[r,:] = epilogue( [x1[r,:] | x2[r,:]] @ W + b ) (+ residual[r,:] after the activation)
 * x1 [R,C1], x2 [R,C2] or NULL (fuses the concat of core/backbones.py:98-100), wpacked from
 * dh3d_pack_weight with Kd = C1+C2; b folded into ep->pre_bias.  C1,C2 % 8 == 0, Dout % 32 == 0. */
int dh3d_linear_pm_fwd(const float *x1, int C1, const float *x2, int C2, const float *wpacked,
                       int R, int Dout, const dh3d_epilogue *ep, const float *residual, float *out,
                       void *stream);

/* Squeeze-excite residual block (core/backbones.py:45-55), one kernel:
 *   g = sigmoid(relu(pool @ W1 + b1) @ W2 + b2);  out = relu(x + x*g)
 * x, pool [R,C]; W1 [C,C/4], W2 [C/4,C] row-major (unpacked).  C in {64,128}. */
int dh3d_se_res_pm_fwd(const float *x, const float *pool, const float *W1, const float *b1,
                       const float *W2, const float *b2, int R, int C, float *out, void *stream);
/* The same block on the matrix pipe: w1packed = dh3d_pack_weight of W1 zero-padded to [C,32] columns, b1pad = b1
 * zero-padded to 32, w2packed = dh3d_pack_weight of W2 zero-padded to [32,C] rows. */
int dh3d_se_res_pm_packed_fwd(const float *x, const float *pool, const float *w1packed, const float *b1pad,
                              const float *w2packed, const float *b2, int R, int C, float *out, void *stream);
/* the same block on flex_pool(x, nbr) (core/backbones.py:76-79) in one launch: the pooled rows are formed while staging,
 * the [B*N, C] pooled map is never written.  x [B*N, C], nbr [B, N, K] int32; C = 64 or 128. */
int dh3d_se_res_pool_pm_packed_fwd(const float *x, const int32_t *nbr, int B, int N, int K, const float *w1packed,
                                   const float *b1pad, const float *w2packed, const float *b2, int C, float *out,
                                   void *stream);
/* ... followed by a 1x1 conv C -> C (+ bias / BatchNorm / activation `ep`) on the block's output in the same launch:
 * out and out2 [B*N, C] are both stored.  C = Dout = 64 (stage 1 -> before_stage2_conv1d, core/backbones.py:115-117) or
 * C = Dout = 128 (stage 2's SE block -> the upper block of its commuted concat conv on the sampled rows). */
int dh3d_se_res_pool_conv_pm_fwd(const float *x, const int32_t *nbr, int B, int N, int K, const float *w1packed,
                                 const float *b1pad, const float *w2packed, const float *b2, int C, float *out,
                                 const float *wconv_packed, const dh3d_epilogue *ep, int Dout, float *out2, void *stream);

/* three_nn + inverse-distance weights + three_interpolate (core/backbones.py:90-96) fused:
 * weight = (1/max(d,1e-10)) / sum(1/max(d,1e-10)).  idx/dist from dh3d_three_nn.
 * points [b,m,c] -> out [b,n,c] (16-byte accesses when c % 4 == 0, one channel per thread otherwise, like
 * dh3d_three_interpolate_fwd). */
int dh3d_three_interpolate_idw_fwd(int b, int m, int c, int n, const float *points,
                                   const int32_t *idx, const float *dist, float *out, void *stream);

/* Row-wise L2 normalisation x / sqrt(max(sum x^2, eps)) (tf.nn.l2_normalize, core/model.py:177,205)
 * with optional prefix columns copied in front (the xyz of 'xyz_feat', core/model.py:181):
 * out[r,:] = [prefix[r,:P] | normalised x[r,:C]]. */
int dh3d_l2norm_concat_fwd(const float *x, int R, int C, float eps, const float *prefix, int P,
                           float *out, void *stream);

/* Point-wise attention / detector head (core/backbones.py:132-173): a chain of per-point linear
 * layers ending in a 1-channel logit + sigmoid, with the last wide hidden layer never written to
 * memory:  att[r] = sigmoid( relu(bn(h[r,:] @ W + b)) . w_fc + b_fc ),  h [R,C], W packed [C,H]. */
int dh3d_mlp_head_pm_fwd(const float *h, int R, int C, const float *wpacked, int H,
                         const dh3d_epilogue *ep, const float *w_fc, float b_fc, float *att,
                         void *stream);

/* dh3d_linear_pm_fwd on the bf16 matrix pipe at f32 accuracy (bf16x6, csrc/dense_x6.hip) for the wide 1x1 convs:
 * Dout in {128, 256}, C1 and C2 multiples of 32, weight from dh3d_pack_weight_x3.  Same result up to f32
 * summation order. */
int dh3d_linear_pm_x6_fwd(const float *x1, int C1, const float *x2, int C2, const void *wpacked_x3, int R, int Dout,
                          const dh3d_epilogue *ep, const float *residual, float *out, void *stream);
/* The same GEMM with its x1 half up-sampled on the fly: x1[b,j,:] = three_interpolate(points [B,m,C1], idx [B,n,3],
 * inverse-distance weights of dist [B,n,3]) (core/backbones.py:91-95 + tf_interpolate.cpp:107-127) -- the
 * interpolated [B,n,C1] tensor is never written.  Bit-identical to dh3d_three_interpolate_idw_fwd followed by
 * dh3d_linear_pm_x6_fwd. */
int dh3d_upsample_linear_pm_x6_fwd(const float *points, const int32_t *idx, const float *dist, int B, int n, int m,
                                   int C1, const float *x2, int C2, const void *wpacked_x3, int Dout,
                                   const dh3d_epilogue *ep, const float *residual, float *out, void *stream);
/* the same with the local path's last step fused into the store (core/model.py:177-181): out_cat [B*n, 3+128] =
 * [prefix [B*n,3] | l2_normalize(y, l2_eps)], Dout == 128; y itself is not written */
int dh3d_upsample_linear_l2cat_pm_x6_fwd(const float *points, const int32_t *idx, const float *dist, int B, int n,
                                         int m, int C1, const float *x2, int C2, const void *wpacked_x3, int Dout,
                                         const dh3d_epilogue *ep, const float *residual, const float *prefix,
                                         float l2_eps, float *out_cat, void *stream);
/* out = act(BN([upsample(points) | x2] W)) + act_sc(BN_sc(x3 W_sc)): the concat conv with the local backbone's shortcut
 * conv (core/backbones.py:123) in one kernel; wpacked_x3 = dh3d_pack_weight_x3 of [W; W_sc] ([C1+C2+C3, Dout]),
 * Dout == 128; prefix != NULL: out is [B*n, 3+128] = [prefix | l2_normalize(sum, l2_eps)] */
int dh3d_upsample_linear_shortcut_pm_x6_fwd(const float *points, const int32_t *idx, const float *dist, int B, int n,
                                            int m, int C1, const float *x2, int C2, const float *x3, int C3,
                                            const void *wpacked_x3, int Dout, const dh3d_epilogue *ep,
                                            const dh3d_epilogue *ep_shortcut, const float *prefix, float l2_eps,
                                            float *out, void *stream);

/* The same head with the GEMM on the bf16 matrix pipe at f32 accuracy ("bf16x6": every f32 operand is split
 * exactly into three bf16 chunks, six chunk products are accumulated in f32; error <= 2^-23 per product, see
 * csrc/dense_x6.hip).  wpacked_x3 from dh3d_pack_weight_x3 (3 * Kd * Dout * 2 bytes).  C % 16 == 0. */
int dh3d_pack_weight_x3(const float *W, int Kd, int Dout, void *packed, void *stream);
int dh3d_mlp_head_pm_x6_fwd(const float *h, int R, int C, const void *wpacked_x3, int H,
                            const dh3d_epilogue *ep, const float *w_fc, float b_fc, float *att, void *stream);

/* The same head on an up-sampled input with the wide conv commuted through the (linear, weights sum to 1) 3-NN
 * interpolation of core/backbones.py:91-95:  att = sigmoid(w_fc . act(BN(interp(H) + pre_bias)) + b_fc),  H = x_coarse W
 * computed on the m coarse rows, layout [Hd/256][B*m][256] (one dh3d_linear_pm_x6_fwd per 256-column weight slice);
 * idx / dist [B*n,3] from dh3d_three_nn.  8x fewer GEMM flops than running the head on the up-sampled rows. */
int dh3d_interp_head_fwd(const float *H, int Hd, const int32_t *idx, const float *dist, int B, int n, int m,
                         const dh3d_epilogue *ep, const float *w_fc, float b_fc, float *att, void *stream);
/* Same head with the fine points walked in the Morton order of `order` (the dh3d_spatial_sort records [B,n,4] of the
 * fine cloud; NULL = index order) and the distinct coarse rows of 128 consecutive points staged in LDS, one 256-channel
 * slice at a time: ~10x less L2 traffic.  m <= 1024.  Equal to dh3d_interp_head_fwd up to the summation order of the
 * row dot. */
int dh3d_interp_head_sorted_fwd(const float *H, int Hd, const int32_t *idx, const float *dist, const float *order, int B,
                                int n, int m, const dh3d_epilogue *ep, const float *w_fc, float b_fc, float *att,
                                void *stream);
/* the same with the fc bias in device memory (a trainable parameter); row_major != 0: H is [B*m][Hd] (one GEMM's
 * output) instead of the 256-column slices */
int dh3d_interp_head_sorted_fwd_dev(const float *H, int Hd, int row_major, const int32_t *idx, const float *dist,
                                    const float *order, int B, int n, int m, const dh3d_epilogue *ep, const float *w_fc,
                                    const float *b_fc_dev, float *att, void *stream);
/* The tail of a concat conv commuted through the up-sampling (C = 128):
 *   out[n] = act(BN(interp3(coarse_w)[n] + partial[n] + pre_bias)) + residual[n]     (or [prefix | l2_normalize(.)])
 * coarse_w [B,M,C] = coarse rows already multiplied by the conv's upper weight block, partial [B,N,C] = the lower block
 * applied to the full-resolution input (may be NULL), idx/dist [B,N,3] from three_nn (inverse-distance weights as
 * core/backbones.py:92-95), residual / prefix ([B,N,3]) may be NULL. */
int dh3d_interp_combine_fwd(const float *coarse_w, const int32_t *idx, const float *dist, const float *partial, int B,
                            int N, int M, int C, const dh3d_epilogue *ep, const float *residual, const float *prefix,
                            float l2_eps, float *out, void *stream);
/* The whole tail of the local-descriptor forward behind the sampled level in one launch (core/backbones.py:89-100,
 * 117-123; core/model.py:177-181) -- dh3d_interp_combine_fwd with its `partial` and `residual` operands computed on the
 * fly instead of read back from memory:
 *   out[n] = [ prefix[n] | l2_normalize( relu(BN_c(interp3(coarse_w)[n] + x2[n] W_lower + b_c)) + relu(BN_s(x1[n] W_s + b_s)) ) ]
 * x1, x2 [B,N,64]; wpacked_x3_* = dh3d_pack_weight_x3 of the [64,128] shortcut weight / of the concat conv's lower block
 * (f32-accurate bf16x6 products); ep_shortcut / ep_concat: bias + folded BatchNorm, activation ReLU; coarse_w [B,M,128];
 * idx / dist [B,N,3] from three_nn; prefix [B,N,3]; out [B,N,131].  N % 32 == 0.
 * prefix == NULL: out [B,N,128] = the sum before the normalisation (the global path's local features; l2_eps unused). */
int dh3d_local_tail_fused_fwd(const float *x1, const float *x2, const void *wpacked_x3_shortcut,
                              const void *wpacked_x3_lower, const dh3d_epilogue *ep_shortcut,
                              const dh3d_epilogue *ep_concat, const float *coarse_w, const int32_t *idx, const float *dist,
                              const float *prefix, float l2_eps, int B, int N, int M, float *out, void *stream);

/* a layer wider than 256 as `slices` column slices of 256 in one launch: out [slices][R][256] = x1 @ W[:, 256 j ..],
 * wpacked_x3 = the dh3d_pack_weight_x3 images of the slices back to back (the H operand of dh3d_interp_head_fwd) */
int dh3d_linear_slices_pm_x6_fwd(const float *x1, int C1, const void *wpacked_x3, int R, int slices, float *out,
                                 void *stream);

/* Attention-weighted NetVLAD aggregation (core/backbones.py:202-262), stage 1+2:
 *   xn = l2norm(x); a = softmax(bn(xn @ Wc)) * att;  vlad[b,d,c] = sum_n a[n,c] xn[n,d] - (sum_n a[n,c]) W2[d,c]
 *   then intra-normalise over d per cluster and L2-normalise the flattened [D*Cl] vector (d-major).
 * x [B,N,D], att [B,N], wc_packed = pack(Wc [D,Cl]), bn as (scale,shift) [Cl], W2 [D,Cl]
 * -> vlad [B, D*Cl].  D = 256, Cl = 64.  workspace: dh3d_netvlad_workspace_bytes(B,N,D,Cl). */
size_t dh3d_netvlad_workspace_bytes(int B, int N, int D, int Cl);
int dh3d_netvlad_aggregate_fwd(const float *x, const float *att, const float *wc_packed,
                               const float *bn_scale, const float *bn_shift, const float *W2, int B,
                               int N, int D, int Cl, void *workspace, size_t workspace_bytes,
                               float *vlad, void *stream);

/* NetVLAD projection + context gating (core/backbones.py:262-320):
 *   h = bn1(vlad @ Wh);  out = h * sigmoid(bn2(h @ Wg));  optional final L2 normalise (model.py:205).
 * vlad [B,Kd], Wh [Kd,O], Wg [O,O] row-major (NULL: no gating); bn as (scale,shift) [O]. O = 256, Kd % 8 == 0 (the
 * split-K projection takes k in blocks of eight; anything else is DH3D_ERR_UNSUPPORTED).  l2_eps == 0: no final normalise.
 * workspace: dh3d_netvlad_head_workspace_bytes(B,Kd,O). */
size_t dh3d_netvlad_head_workspace_bytes(int B, int Kd, int O);
int dh3d_netvlad_head_fwd(const float *vlad, const float *Wh, const float *bn1_scale,
                          const float *bn1_shift, const float *Wg, const float *bn2_scale,
                          const float *bn2_shift, int B, int Kd, int O, float l2_eps,
                          void *workspace, size_t workspace_bytes, float *out, void *stream);

/* ===================================================================================== *
 * C. Backward / training kernels (point-major)
 * ===================================================================================== */

/* flex_conv backward, factorised (csrc/flex_bwd.hip): features [B,N,Din], xyz [B,N,3], nbr [B,N,K], theta [3,Din,Dout],
 * bias [Din,Dout], grad_out [B,N,Dout] -> grad_features [B,N,Din] (may be NULL: weights only), grad_theta, grad_bias.
 * center_rank0: offsets relative to the rank-0 neighbour (the reference backward's rule) instead of the point itself.
 * Zeroes its outputs.  workspace: dh3d_flex_conv_pm_bwd_workspace_bytes.  Din % 4 == 0, Dout % 4 == 0. */
size_t dh3d_flex_conv_pm_bwd_workspace_bytes(int B, int N, int Din, int Dout);
int dh3d_flex_conv_pm_bwd(const float *features, const float *xyz, const int32_t *nbr, const float *theta,
                          const float *bias, const float *grad_out, int B, int N, int K, int Din, int Dout,
                          int center_rank0, void *workspace, size_t workspace_bytes, float *grad_features,
                          float *grad_theta, float *grad_bias, void *stream);

/* f32 GEMMs of the backward passes (csrc/gemm.hip), all row-major; f32-accurate: the exact-f32 matrix pipe for small
 * products, the bf16 pipe with a three-way split of BOTH operands (six products, ~2^-23 relative) from 2^26
 * multiply-adds when K % 4 == 0:
 *   tn: C[M,N] (+)= A[K,M]^T B[K,N]  (weight gradients: reduction over rows, split over workgroups + f32 atomics)
 *   nn: C[M,N] (+)= A[M,K]   B[K,N] (+ colbias[N], may be NULL; not with accumulate)  (linear layers of the
 *       training step, input gradients with W^T materialised)
 * accumulate = 0 overwrites C.  M, N (tn) / K, N (nn) multiples of 4. */
/* 1 when the product's reduction is split over workgroups (C is then zeroed by the call and the partials added with f32
 * atomics; with accumulate = 1 they are added onto the caller's C -- a caller holding zeroed memory saves the fill). */
int dh3d_gemm_is_split(int ta /* 1: tn form */, int M, int N, int K, int batch);
/* Which kernel of csrc/gemm.hip serves a shape at the four GEMM entry points, and how its reduction is cut: the decision
 * the launcher itself runs.  batch > 1: the batched forms; with_bias: nn with a colbias.  *chunks workgroups along the
 * reduction take *kchunk steps each (the last one the remainder), *kchunk a multiple of *stage, the reduction steps per LDS
 * stage (1 for the plain-FMA kernels, which take the whole reduction in one pass); any of the three may be NULL.  0, and
 * zeros, for a shape the entry points refuse.  chunks > 1 implies dh3d_gemm_is_split; a bias implies chunks == 1.
 * Host only; looks at the shape alone, never at the data. */
#define DH3D_GEMM_ROWS1 1      /* gemm_rows_kernel<RB>: nn, M <= 32, K <= 512; id = RB = ceil(M / 8), 1 .. 4 */
#define DH3D_GEMM_ROWS4 4
#define DH3D_GEMM_SHORTK 5     /* gemm_shortk_kernel: tn, K <= 32 */
#define DH3D_GEMM_F32_NARROW 6 /* gemm_f32_kernel, 128 x 64 tiles (N <= 64), stage 16 */
#define DH3D_GEMM_F32_WIDE 7   /* gemm_f32_kernel, 128 x 128 tiles, stage 16 */
#define DH3D_GEMM_X6_NARROW 8  /* gemm_x6_kernel, 128 x 64 tiles, stage 32: >= 2^26 multiply-adds, K % 32 == 0 */
#define DH3D_GEMM_X6_WIDE 9    /* gemm_x6_kernel, 128 x 128 tiles, stage 16 */
int dh3d_gemm_plan(int ta, int M, int N, int K, int batch, int with_bias, int *chunks, int *kchunk, int *stage);
int dh3d_gemm_tn_f32(const float *A, const float *B, int K, int M, int N, int accumulate, float *C, void *stream);
int dh3d_gemm_nn_f32(const float *A, const float *B, const float *colbias, int M, int K, int N, int accumulate,
                     float *C, void *stream);
/* [Bt,R,C] -> [Bt,C,R] of 32-bit elements; out[c] (+)= sum_r x[r,c]. */
int dh3d_transpose32(const void *in, int Bt, int R, int C, void *out, void *stream);
int dh3d_colsum_f32(const float *x, long long R, int C, int accumulate, float *out, void *stream);

/* Training-mode BatchNorm in two HBM-bound passes per direction and the attention head's element-wise passes
 * (csrc/train.hip; tensorpack BatchNorm / slim batch_norm with is_training -- core/tf_utils.py:60-63,
 * core/backbones.py:145-173,218-223,271-274).  x [R,C] row-major; mask (may be NULL): one byte per cloud of
 * rows_per_cloud rows, 0 = padding cloud, excluded.  Sums are f64 (f32 per thread, f64 atomics across workgroups).
 *   colstats       : sum[c] = sum_r x, sumsq[c] = sum_r x^2                         (zeroes its outputs)
 *   scale_shift_act: y = act(x*scale[c] + shift[c])   (relu = 0/1; y may alias x)
 *   row_logit_sigmoid: att[r] = sigmoid(sum_c relu(h*scale+shift)[r,c] w[c] + b)    (attention head, backbones.py:170-173)
 *   bn_colstats    : sum / sumsq [C] f64 += column sums of x over the live rows (zeroed by the CALLER)
 *   bn_bwd_sums    : (S1, S2, S3 zeroed by the CALLER) S1 = sum dz, S2 = sum dz*xhat with xhat = (x-mean)*rstd, dz = dy masked by
 *                    x*scale+shift > 0 -- the forward's own float32 expression, (scale, shift) folded from (mean, rstd, gamma, beta) exactly
 *                    as bn_finalize folds them, so forward, sums and apply agree on every gate bit for bit;
 *                    dy == NULL: dy[r,c] = rowscale[r]*colvec[c] (rank one) and S3[c] = sum_r rowscale[r]*y[r,c]
 *   bn_finalize    : (sum, sumsq, count) -> mean, rstd, scale = gamma*rstd, shift = beta - mean*scale; running buffers
 *                    <- momentum*old + (1-momentum)*batch statistic (untouched when count == 0)
 *   bn_bwd_finalize: (S1, S2, count) -> k2, k3 of bn_bwd_apply
 *   bn_bwd_apply   : dx = scale*dz - k2[c] - k3[c]*x  == gamma*rstd*(dz - S1/n - xhat*S2/n)   (dx may alias x) */
/* bn_bwd_finalize from per-cloud partial sums part [nk][P][C] f64 (nk = 2: S1, S2; 3: + S3): their sums over P give k2 / k3
 * and, as float32, grads [nk][C] (dbeta, dgamma, d w_fc).  dh3d_sigmoid_bwd: dlogit = datt*att*(1-att) (0 on rows of
 * masked clouds) and sum[0] += sum dlogit (sum zeroed by the CALLER). */
int dh3d_bn_finalize_parts(const double *part /* [2][P][C]: sum | sumsq per cloud */, int P, const double *count,
                           const float *gamma, const float *beta, float eps, float momentum, int unbiased, float *run_mean,
                           float *run_var, int C, float *mean, float *rstd, float *scale, float *shift, void *stream);
int dh3d_bn_bwd_finalize_parts(const double *part, int nk, int P, const double *count, const float *mean,
                               const float *rstd, const float *gamma, int C, float *k2, float *k3, float *grads,
                               void *stream);
int dh3d_sigmoid_bwd(const float *datt, const float *att, const unsigned char *mask, int rows_per_cloud, long long n,
                     float *dlogit, float *sum, void *stream);
int dh3d_bn_colstats(const float *x, long long R, int C, const unsigned char *mask, int rows_per_cloud, double *sum,
                     double *sumsq, void *stream);
int dh3d_scale_shift_act(const float *x, long long R, int C, const float *scale, const float *shift, int relu,
                         float *y, void *stream);
/* The same pass with `residual` [R,C] (or NULL) added AFTER the activation: y = act(x*scale+shift) + residual -- the
 * shortcut sum behind the last BatchNorm of the local backbone in training mode (core/backbones.py:123). */
int dh3d_scale_shift_act_res(const float *x, long long R, int C, const float *scale, const float *shift, int relu,
                             const float *residual, float *y, void *stream);

/* Element-wise / scatter passes of the LOCAL backbone's training step (stage 1-2: basic_config / detection_config,
 * core/model.py:212-246; dh3d_amd/training.py LocalTrainer), point-major rows:
 *   dh3d_flex_pool_pm_bwd : FlexPoolGrad (flex_pool_kernel_gpu.cu.cc:65-93) -- din[cloud(n) + argmax[n,c], c] += dout[n,c]
 *                           with f32 atomics (as the reference); din [B*N, C] zeroed by the CALLER;
 *   dh3d_se_gate_fwd/_bwd : y = relu(x + x * sigmoid(z)) and its gradients (se_res_bottleneck's tail, backbones.py:52-55);
 *   dh3d_relu_fwd/_bwd    : y = relu(x);  dx = y > 0 ? dy : 0.   Element counts are multiples of 4. */
/* pairwise_dist (core/tf_utils.py:125-136) of the local losses: out[b,i,j] = sum_d (A[b,i,d] - Bm[b,j,d])^2 with the
 * differences formed as upstream; A [B,n,D], Bm [B,m,D] -> out [B,n,m]. */
int dh3d_pairwise_sqdist(const float *A, const float *Bm, int B, int n, int m, int D, float *out, void *stream);
int dh3d_flex_pool_pm_bwd(const float *dout, const int32_t *argmax, int B, int N, int C, float *din, void *stream);
int dh3d_se_gate_fwd(const float *x, const float *z, long long n, float *y, void *stream);
int dh3d_se_gate_bwd(const float *x, const float *z, const float *dy, long long n, float *dx, float *dz, void *stream);
int dh3d_relu_fwd(const float *x, long long n, float *y, void *stream);
int dh3d_relu_bwd(const float *y, const float *dy, long long n, float *dx, void *stream);
int dh3d_row_logit_sigmoid(const float *h, long long R, int C, const float *scale, const float *shift, const float *w,
                           const float *b /* device scalar */, float *att, void *stream);
int dh3d_bn_bwd_sums(const float *x, const float *dy, const float *rowscale, const float *colvec, long long R, int C,
                     const float *mean, const float *rstd, const float *gamma, const float *beta, int relu,
                     const unsigned char *mask, int rows_per_cloud, double *S1, double *S2, double *S3, void *stream);
int dh3d_bn_bwd_apply(const float *x, const float *dy, const float *rowscale, const float *colvec, long long R, int C,
                      const float *scale, const float *shift, const float *k2, const float *k3, int relu,
                      const unsigned char *mask, int rows_per_cloud, float *dx, void *stream);
int dh3d_bn_finalize(const double *sum, const double *sumsq, const double *count /* device scalar */,
                     const float *gamma, const float *beta, float eps, float momentum,
                     int unbiased /* moving variance <- Bessel-corrected batch variance (fused_batch_norm) */,
                     float *run_mean, float *run_var, int C, float *mean, float *rstd, float *scale, float *shift,
                     void *stream);
int dh3d_bn_bwd_finalize(const double *S1, const double *S2, const double *count, const float *mean, const float *rstd,
                         const float *gamma, int C, float *k2, float *k3, void *stream);

/* NetVLAD soft assignment rows (core/backbones.py:214-238; Cl = 64, one wave per row):
 *   a[r,:] = softmax(s[r,:]*scale + shift) * att[r];   backward: da -> dz (gradient at the BatchNorm output), datt.
 * asum (may be NULL) [R / rows_per_cloud, 64]: the per-cloud column sums of a (backbones.py:241) from the same pass
 * (rows_per_cloud % 64 == 0).  l2norm_rows_bwd: backward of xn = x * rsqrt(max(sum x^2, eps)) (tf.nn.l2_normalize).
 * idw_weights: three_interpolate's inverse-distance weights from three_nn's distances (backbones.py:92-95).
 * context_gate: y = v * sigmoid(g) (backbones.py:271-277) and its backward. */
int dh3d_netvlad_assign_rows(const float *s, long long R, int Cl, const float *scale, const float *shift,
                             const float *att, float *a, float *asum, long long rows_per_cloud, void *stream);
int dh3d_netvlad_assign_rows_bwd(const float *s, long long R, int Cl, const float *scale, const float *shift,
                                 const float *att, const float *da, float *dz, float *datt, void *stream);
int dh3d_l2norm_rows_bwd(const float *x, const float *dxn, long long R, int C, float eps, float *dx, void *stream);
int dh3d_idw_weights(const float *dist, long long R, float *w, void *stream);
int dh3d_context_gate_fwd(const float *v, const float *g, long long n, float *y, void *stream);
int dh3d_context_gate_bwd(const float *v, const float *g, const float *dy, long long n, float *dv, float *dg,
                          void *stream);
/* Training-mode attention head with its convolution commuted through the up-sampling (csrc/interp_train.hip): the
 * pre-activation h = three_interpolate(G) of globalatt_block (core/backbones.py:89-100,156-173), G = coarse @ W + b as
 * 256-column slices [Hd/256][B*m][256] (row_major = 0) or as the GEMM's own [B*m][Hd] output (row_major = 1; dG likewise),
 * is never materialised.  idx / dist [B,n,3] = three_nn of the fine points, order =
 * dh3d_spatial_sort records [B,n,4] of the fine cloud (NULL: index order), mask [B] bytes (NULL: all clouds live).
 *   colstats : per-cloud partials part [2][B][Hd] f64 (zeroed by the CALLER) of sum / sumsq of h over the live rows; their
 *              sums over B -> dh3d_bn_finalize
 *   forward  : dh3d_interp_head_sorted_fwd with the folded batch statistics as its epilogue
 *   bwd_sums : per-cloud partials part [3][B][Hd] f64 (zeroed by the CALLER) of S1, S2, S3 of dh3d_bn_bwd_sums for dy = dlogit x w_fc (dlogit [B*n]
 *              by original point index); the gate is bwd_apply's h*scale+shift > 0 on the same folded coefficients
 *   bwd_apply: dG [Hd/256][B*m][256] = interp^T(scale dz - k2 - k3 h) (zeroed by the CALLER, f32 atomics), from which
 *              dW = coarse^T dG and dcoarse = dG W^T are GEMMs on B*m rows.  Hd <= 1024, m <= 1024. */
int dh3d_interp_bn_colstats(const float *G, int Hd, int row_major, const int32_t *idx, const float *dist,
                            const float *order, int B, int n, int m, const unsigned char *mask,
                            double *part /* [2][B][Hd] */, void *stream);
int dh3d_interp_bn_bwd_sums(const float *G, int Hd, int row_major, const int32_t *idx, const float *dist,
                            const float *order, int B, int n, int m, const unsigned char *mask, const float *dlogit, const float *w_fc,
                            const float *mean, const float *rstd, const float *gamma, const float *beta,
                            double *part /* [3][B][Hd] */, void *stream);
int dh3d_interp_bn_bwd_apply(const float *G, int Hd, int row_major, const int32_t *idx, const float *dist,
                             const float *order, int B, int n, int m, const unsigned char *mask, const float *dlogit, const float *w_fc,
                             const float *scale, const float *shift, const float *k2, const float *k3, float *dG,
                             void *stream);
/* three_interpolate's backward (threeinterpolate_grad_cpu, tf_interpolate.cpp:131-153) on the Morton order of the fine
 * cloud (order = dh3d_spatial_sort records [b,n,4], NULL: index order): the rows of a 128-point block are scattered onto
 * the <= 56 coarse rows it touches by an MFMA product in LDS, then added to grad_points [b,m,c] (zeroed by the call) with
 * one f32 atomic per (block, row, channel).  c == 256, m <= 1024; same result as dh3d_three_interpolate_bwd up to the
 * summation order. */
int dh3d_three_interpolate_bwd_sorted(int b, int n, int c, int m, const float *grad_out, const int32_t *idx,
                                      const float *weight, const float *order, float *grad_points, void *stream);
/* NetVLAD's assignment (core/backbones.py:202-256) in the training step with its rows commuted through
 * three_interpolate (core/backbones.py:89-100), csrc/netvlad_train.hip: c [B*m,256] are the sampled rows, cw = c Wc and
 * E = c dV^T GEMMs on them; s / p / dz [B*n,64], rinv / att / datt / t2 / q [B*n] live on the fine points (by original
 * point index); idx / dist = dh3d_three_nn of the fine points [B,n,3], order = dh3d_spatial_sort records of the fine
 * clouds [B,n,4] (NULL: index order), mask [B] bytes (NULL: every cloud).  m <= 1024.  A masked (padding) cloud takes no
 * part in any sum, and its rows of every per-point output (s, rinv, p, dz, datt, t2, q) are written as 0.
 *   fwd_stats : s = rinv * interp(cw), rinv = rsqrt(max(|interp(c)|^2, 1e-12)), part [2][B][64] f64 = per-cloud column
 *               sums / sums of squares of s (zeroed by the CALLER)
 *   fwd_assign: p = softmax(s*scale + shift), asum [B,64] = sum_n p*att, Ap [B*m,64] = interp^T(p*att*rinv) (both zeroed
 *               by the CALLER; V[b] = Ap[b]^T c[b])
 *   bwd_sums  : da = rinv*interp(E) + dasum; datt = sum_k da p (0 for masked clouds); dz = softmax backward of da*att;
 *               t2 = sum_k p att interp(E); part [2][B][64] f64 (zeroed by the CALLER) = per-cloud sums of dz and dz*(s - mean)*rstd
 *   bwd_apply : ds = k1*dz - k2 - k3*s (dh3d_bn_bwd_finalize); q = rinv^2 sum_k ds s + rinv^3 t2, 0 on rows the l2
 *               clamp held (rinv = rsqrt(1e-12): no gradient through it); dcw [B*m,64] = interp^T(rinv*ds) (zeroed by the CALLER)
 * dh3d_interp_scatter_scaled: dc [B*m,256] += interp^T(-q * interp(c)) (dc NOT zeroed: it holds Ap dV + dcw Wc^T). */
int dh3d_netvlad_commuted_fwd_stats(const float *c, const float *cw, const int32_t *idx, const float *dist,
                                    const float *order, int B, int n, int m, const unsigned char *mask, float *s,
                                    float *rinv, double *part, void *stream);
int dh3d_netvlad_commuted_fwd_assign(const float *s, const float *rinv, const float *att, const float *scale,
                                     const float *shift, const int32_t *idx, const float *dist, const float *order, int B,
                                     int n, int m, const unsigned char *mask, float *p, float *asum, float *Ap,
                                     void *stream);
int dh3d_netvlad_commuted_bwd_sums(const float *E, const float *p, const float *s, const float *att, const float *rinv,
                                   const float *dasum, const float *mean, const float *rstd, const int32_t *idx,
                                   const float *dist, const float *order, int B, int n, int m, const unsigned char *mask,
                                   float *dz, float *datt, float *t2, double *part, void *stream);
int dh3d_netvlad_commuted_bwd_apply(const float *dz, const float *s, const float *rinv, const float *t2, const float *k1,
                                    const float *k2, const float *k3, const int32_t *idx, const float *dist,
                                    const float *order, int B, int n, int m, const unsigned char *mask, float *q,
                                    float *dcw, void *stream);
int dh3d_interp_scatter_scaled(const float *c, const float *q, const int32_t *idx, const float *dist, const float *order,
                               int B, int n, int m, const unsigned char *mask, float *dc, void *stream);
/* NetVLAD between the VLAD contraction and the hidden projection (core/backbones.py:241-262) for the training step:
 * out[b, d*64 + c] = l2norm_all( intra_norm_d( V[b,c,d] - asum[b,c] * W2[d,c] ) ), one workgroup per cloud, and its
 * gradients (dW2 zeroed by the call, f32 atomics over the clouds).  D == 256, Cl == 64. */
int dh3d_vlad_normalize_fwd(const float *V, const float *asum, const float *W2, int B, int D, int Cl, float eps,
                            float *out, float *inv_c, float *inv_t, void *stream);
int dh3d_vlad_normalize_bwd(const float *V, const float *asum, const float *W2, const float *grad_out, int B, int D,
                            int Cl, float eps, float *dV, float *dasum, float *dW2, void *stream);
/* lazy quadruplet loss (core/losses.py:137-200) and its gradient in one launch: desc [B*(2+P+Ng), 256] role-ordered
 * (queries | positives | negatives | other negatives); loss[0] is zeroed by the call; grad has desc's shape. */
int dh3d_quadruplet_loss(const float *desc, int B, int P, int Ng, int D, float margin, float margin2, float *loss,
                         float *grad, void *stream);
/* training-mode BatchNorm (+ReLU) of a short tensor (R <= 64 rows, e.g. the [clouds, 256] activations behind NetVLAD) in
 * one launch per direction; stats [4,C] = mean, rstd, scale, shift of the forward; mask [R] bytes or NULL. */
int dh3d_bn_small_fwd(const float *x, int R, int C, const float *gamma, const float *beta, float eps, float momentum,
                      int unbiased, int relu, const unsigned char *mask, float *run_mean, float *run_var, float *stats,
                      float *y, void *stream);
int dh3d_bn_small_bwd(const float *x, const float *dy, int R, int C, const float *gamma, const float *stats, int relu,
                      const unsigned char *mask, float *dx, float *dgamma, float *dbeta, void *stream);
/* batched GEMMs: `batch` independent products on operands stored back to back; colbias [batch, N] (nn only). */
int dh3d_gemm_tn_f32_batched(const float *A, const float *B, int batch, int K, int M, int N, float *C, void *stream);
int dh3d_gemm_nn_f32_batched(const float *A, const float *B, const float *colbias, int batch, int M, int K, int N,
                             float *C, void *stream);

/* The global-descriptor tail with the up-sampling commuted through BOTH consumers of the up-sampled map (attention MLP
 * and NetVLAD; csrc/dense_x6.hip VladTail), two calls.  dh3d_global_walk_planned_fwd walks the fine points once (Morton
 * order of `order`, coarse rows staged in LDS) from H = the 256-column slices of coarse @ W_att
 * (dh3d_linear_slices_pm_x6_fwd), coarse [B,m,256] and cw = coarse @ cluster_weights [B,m,64], and produces att [B,n]
 * (may be NULL) and accum = [ apart B*m*64 | asum B*64 ] floats (zero_accum != 0: cleared by the call; 0: zeroed by the
 * CALLER, e.g. by a fill issued beside the sampling chain): apart = A' (softmax * attention scattered onto the coarse
 * rows, f32 atomics), asum its per-cluster sums.  dh3d_netvlad_tail_assign_fwd finishes: it forms V = apart^T coarse
 * inside its finalize kernel (a fixed summation order), subtracts asum*W2, intra-normalises, projects and gates.  Same
 * function as three_interpolate -> attention head -> dh3d_netvlad_fused_fwd, reassociated; m <= 1024; workspace:
 * dh3d_netvlad_tail_workspace_bytes. */
/* Round 6: the walk's slot tables built AHEAD of it.  Inside the walk the table of a 128-point block (bitmap of the coarse
 * rows its points touch -> prefix popcounts -> slots; three dependent global round trips + five barriers) was 17 of the
 * launch's ~95 us at 32 x 4096.  dh3d_walk_plan builds every block's table from the three_nn result (idx, dist [B,n,3], order =
 * dh3d_spatial_sort records of the fine cloud, may be NULL) into `plan` (dh3d_walk_plan_bytes(B, n) bytes, opaque:
 * per block the slot table and the slot-major lists of the references to every staged row, which the planned walk's
 * NetVLAD scatter follows instead of forming a selection matrix on the matrix pipe) -- launched behind dh3d_three_nn_*, off the critical chain -- and dh3d_global_walk_planned_fwd
 * reads it (plan == NULL: the table is built inside the walk).  Same results bit for bit either way, up to the order of
 * the f32 atomics.  m <= 1024. */
size_t dh3d_walk_plan_bytes(int B, int n);
int dh3d_walk_plan(const int32_t *idx, const float *dist, const float *order, int B, int n, int m, void *plan, void *stream);
size_t dh3d_netvlad_tail_workspace_bytes(int B, int D, int Cl, int O);
int dh3d_global_walk_planned_fwd(const float *H, int Hd, const float *coarse, const float *cw, const int32_t *idx,
                                 const float *dist, const float *order, const void *plan, int B, int n, int m,
                                 const dh3d_epilogue *ep, const float *w_fc, float b_fc, const float *cl_scale,
                                 const float *cl_shift, float *att, float *accum, int zero_accum, void *stream);
int dh3d_netvlad_tail_assign_fwd(const float *apart, const float *coarse, const float *asum, int m, const float *W2,
                                 const float *Wh, const float *bn1_scale, const float *bn1_shift, const float *Wg,
                                 const float *bn2_scale, const float *bn2_shift, int B, int D, int Cl, int O, float l2_eps,
                                 void *workspace, size_t workspace_bytes, float *out, void *stream);

/* NetVLAD aggregation + projection + gating in one call (what the model runs): dh3d_netvlad_aggregate_fwd followed by
 * dh3d_netvlad_head_fwd, without the separate whole-vector L2-normalisation kernel (its factor is applied to the
 * projected vector).  Wg may be NULL (no gating).  workspace: dh3d_netvlad_fused_workspace_bytes. */
size_t dh3d_netvlad_fused_workspace_bytes(int B, int N, int D, int Cl, int O);
int dh3d_netvlad_fused_fwd(const float *x, const float *att, const float *wc_packed, const float *bn_scale,
                           const float *bn_shift, const float *W2, const float *Wh, const float *bn1_scale,
                           const float *bn1_shift, const float *Wg, const float *bn2_scale, const float *bn2_shift, int B,
                           int N, int D, int Cl, int O, float l2_eps, void *workspace, size_t workspace_bytes, float *out,
                           void *stream);

/* Keypoint non-maximum suppression for a batch of clouds (localdesc_extract.py --perform_nms: core/utils.py:15-43
 * single_nms, run by the reference once per cloud on the host; csrc/keypoints.hip).  Same ids as dh3d_amd/utils.py
 * single_nms, cloud by cloud, bit for bit.  Per cloud b:
 *   a[i]  = score[(b*N + i) * score_stride] (invert != 0: 1 - that), muted to 0 when remove_noise and K > 7 and
 *           dist[i][7] > 2.0 (-0 reads as +0);
 *   thr   = f32(max a over the real points) * ratio;
 *   s[i][r] = a[nn[i][r]] when dist[i][r] <= radius and nn[i][r] is a real point, else 0;
 *   i is kept iff it is a real point, s[i][r] <= s[i][0] for every r >= 1 (first maximum wins) and a[i] > thr.
 * The kept points ordered by (a, i) descending and cut to M: count [B] = how many, inds [B, M] their ids, padded with -1.
 * nn / dist [B, N, K] from the project's kNN (dh3d_knn_bruteforce_xyz / dh3d_knn_sorted, K = min(knn, N)).
 * num_valid [B] (may be NULL: all N): points i >= num_valid[b] are never kept, take no part in the maximum and, as
 * neighbours, count as outside the ball.  score_stride in elements (132 reads column 131 of xyz_feat_att given a pointer to
 * its first row's column 131).  workspace: dh3d_keypoint_nms_workspace_bytes(B, N, M) bytes, caller-owned, no clearing
 * needed.  1 <= M <= 4096 and K <= 64 (else DH3D_ERR_UNSUPPORTED), any N. */
size_t dh3d_keypoint_nms_workspace_bytes(int B, int N, int M);
int dh3d_keypoint_nms(const float *score, long long score_stride, int invert, const int32_t *nn, const float *dist,
                      const int32_t *num_valid, int B, int N, int K, float radius, float ratio, int M, int remove_noise,
                      int32_t *count, int32_t *inds, void *workspace, size_t workspace_bytes, void *stream);
/* dst [B, M, C] <- src [B, N, C] rows: dst[b, j] = src[b, inds[b, j]] for j < count[b] (and 0 <= inds < N), zero rows
 * after that.  Any C (4-byte elements).  With the outputs of dh3d_keypoint_nms: only the keypoints' rows of a map. */
int dh3d_gather_rows(const float *src, int B, int N, int C, const int32_t *inds, const int32_t *count, int M, float *dst,
                     void *stream);

/* Descriptor matching of P cloud pairs (eval_align.m: pdist2(pos_desc, anc_desc, 'euclidean', 'smallest', 1), run there one
 * pair at a time; csrc/registration.hip).  Anchor descriptors: row (p, i) at anchor_desc + (p*Ma + i) * anchor_stride, D floats;
 * positive descriptors likewise with positive_stride (strides in elements: xyz_feat_att_nms + 3 with stride 132 is read in
 * place).  For every pair p and anchor i < a = clamp(anchor_count[p], 0, Ma):
 *   match [P, Ma] = argmin over j < b = clamp(positive_count[p], 0, Mb) of the Euclidean distance, ties to the lowest j;
 *   dist  [P, Ma] = that distance (float32: sqrt of the f32 sum over d ascending of (a_d - b_d)^2, no fma contraction).
 * Rows i >= a, and every row when b = 0, get match -1 and dist +inf.  A pair's result does not depend on the batch.
 * D <= 256 and a multiple of 4, Ma, Mb <= 4096 (else DH3D_ERR_UNSUPPORTED); NULL pointers, P / Ma / Mb / D <= 0 or a stride
 * below D: DH3D_ERR_INVALID_ARGUMENT.  No workspace. */
int dh3d_match_descriptors(const float *anchor_desc, long long anchor_stride, const int32_t *anchor_count,
                           const float *positive_desc, long long positive_stride, const int32_t *positive_count, int P, int Ma,
                           int Mb, int D, int32_t *match, float *dist, void *stream);
/* The two nearest positives of every anchor, the nearest anchor of every positive, and Lowe's ratio test and the mutual
 * (cross) check on them (csrc/match.hip).  Inputs, strides, counts and limits as dh3d_match_descriptors; a = clamp(anchor_count
 * [p], 0, Ma), b = clamp(positive_count[p], 0, Mb), and S(i, j) is that entry's f32 sum over d ascending of (a_d - b_d)^2, no
 * fma contraction (S = +inf or NaN is no neighbour).  For every pair p:
 *   nn1, nn2 [P, Ma]     the two smallest (S, j) over j < b in lexicographic order: ties go to the lowest id, duplicate
 *                        positives give nn2 the next id at the same S; -1 where there is none (i >= a, b = 0, b = 1 for nn2);
 *   dist1, dist2 [P, Ma] sqrtf of those sums, +inf where the id is -1.  nn1 / dist1 equal dh3d_match_descriptors' match /
 *                        dist bit for bit;
 *   rev, rev_dist [P, Mb] the smallest (S, i) over i < a of every positive j < b, else -1 / +inf (S is symmetric in f32).
 *                        Both may be NULL when mutual == 0: the reverse search is then not run;
 *   match [P, Ma]        nn1[i] if the row is kept, else -1.  Kept: nn1 >= 0; and ratio2 <= 0 or S1 < ratio2 * S2 (f32, one
 *                        rounded product, strict; S2 = +inf without a second neighbour: a lone candidate is kept, an exact
 *                        tie at ratio2 = 1 is not); and mutual == 0 or rev[nn1[i]] == i.  ratio2 is the SQUARE of Lowe's
 *                        ratio: the test is on the sums, nothing depends on sqrtf;
 *   num_kept [P]         how many rows of match are >= 0.
 * Every element of every output is written.  A pair's result depends neither on the batch nor on the run: the f32 MFMA only
 * screens which pairs the rule evaluates (a proved bound, csrc/match.hip), the ids and sums are the rule's, merged by integer
 * minima.  No workspace, no host sync, graph-capturable.  Errors as dh3d_match_descriptors; also DH3D_ERR_INVALID_ARGUMENT
 * for ratio2 > 1 or NaN, for only one of rev / rev_dist, and for mutual != 0 without them. */
int dh3d_match_descriptors2(const float *anchor_desc, long long anchor_stride, const int32_t *anchor_count,
                            const float *positive_desc, long long positive_stride, const int32_t *positive_count, int P, int Ma,
                            int Mb, int D, float ratio2, int mutual, int32_t *nn1, float *dist1, int32_t *nn2, float *dist2,
                            int32_t *rev, float *rev_dist, int32_t *match, int32_t *num_kept, void *stream);
/* RANSAC rigid registration of P cloud pairs (ransacfitRt.m over ransac.m and estimateRigidTransform.m with isdegenerate = 0,
 * batched; csrc/registration.hip).  One workgroup per pair; no workspace (the correspondences are staged in LDS).
 * Coordinates: anchor point i of pair p at anchor_xyz + (p*Ma + i) * anchor_stride (3 floats), positive point j at
 * positive_xyz + (p*Mb + j) * positive_stride (strides in elements, >= 3).  The correspondences are the anchors
 * i < clamp(anchor_count[p], 0, Ma) with 0 <= match[p, i] < Mb, in ascending i; n = their number (num_corr [P], may be NULL).
 * The model maps positive into anchor coordinates, anchor ~ R * positive + t; everything below is float64 on the exact
 * float64 values of the float32 inputs.
 *   fit of a point set: centroids (sums in set order / count), B = sum over the set of A^T A with
 *     A = [0, (Y - X)^T; X - Y, [Y + X]x] on the centred points (crossTimesMatrix sign convention), q = the unit eigenvector
 *     of B's smallest eigenvalue (cyclic Jacobi), R = quat2rot(q), t = x_centroid - R * y_centroid;
 *   inlier: sqrt(|x - (R y + t)|^2) < threshold;
 *   sample of trial k: splitmix64(z) = { z += 0x9E3779B97F4A7C15; z = (z ^ z>>30) * 0xBF58476D1CE4E5B9;
 *     z = (z ^ z>>27) * 0x94D049BB133111EB; return z ^ z>>31 } (uint64 wrap-around); h = splitmix64(splitmix64(seed) ^ k),
 *     u_j = splitmix64(h + j); i0 = u0 mod n; i1 = u1 mod (n-1), + 1 if i1 >= i0; i2 = u2 mod (n-2), then + 1 if i2 >= min(i0,
 *     i1), then + 1 if i2 >= max(i0, i1); the fit sums in the order i0, i1, i2.  The same sequence for every pair (ransac.m
 *     resets its stream on every call; it replaces randsample, whose stream cannot be reproduced);
 *   stop rule: c_k = the inlier count of trial k's model, best_k = max(c_0..c_k), N_k = max(log(1 - confidence) /
 *     log(clamp(1 - (best_k / n)^3, eps, 1 - eps)), 10) with eps = 2^-52; the loop stops after trial k*, the first k with
 *     N_k <= k + 1 or k + 1 > max_trials (at most max_trials + 1 trials); trials[p] = k* + 1; the winner is the LAST trial
 *     in 0..k* whose count equals best_k* (ransac.m accepts on >=);
 *   n < 3: no model, trials 0; n == 3: the fit of the three, all three inliers, trials 0.
 * Outputs: inliers [P, Ma] uint8 (1 at the anchor rows of the winner's inliers, the winner's mask, not recomputed after the
 * refit), num_inliers [P], trials [P], Rt [P, 3, 4] float64 = [R | t] of the fit over the winner's inliers (sums of each lane
 * in ascending order, then a fixed tree), valid [P] = n >= 3 and num_inliers >= 3; Rt is NaN where valid is 0.
 * threshold > 0, 0 < confidence < 1, max_trials >= 0, NULL pointers (num_corr excepted), P / Ma / Mb <= 0 or a stride below
 * 3: DH3D_ERR_INVALID_ARGUMENT; Ma or Mb > 4096: DH3D_ERR_UNSUPPORTED. */
int dh3d_ransac_rigid(const float *anchor_xyz, long long anchor_stride, const float *positive_xyz, long long positive_stride,
                      const int32_t *match, const int32_t *anchor_count, int P, int Ma, int Mb, double threshold,
                      double confidence, int max_trials, unsigned long long seed, double *Rt, int32_t *valid,
                      uint8_t *inliers, int32_t *num_inliers, int32_t *trials, int32_t *num_corr, void *stream);
/* Graduated non-convexity (GNC) rigid registration of P cloud pairs: the Geman-McClure objective of Fast Global
 * Registration (Zhou, Park & Koltun, ECCV 2016) solved by iteratively re-weighted closed-form fits (Yang, Antonante,
 * Tzoumas & Carlone, RA-L 2020, GNC-GM); csrc/registration.hip gnc_kernel.  A deterministic estimator beside
 * dh3d_ransac_rigid: no sampling, no seed, and a fit count that depends only on the cloud's extent and the threshold.  It is
 * a local method with a good record, not a guarantee.  One workgroup per pair, one launch, no workspace, no host sync, no
 * atomics: graph-capturable.  Inputs, strides, the correspondences (anchors i < clamp(anchor_count[p], 0, Ma) with
 * 0 <= match[p, i] < Mb, compacted in ascending i, n of them) and the model's direction (x ~ R y + t, x anchor, y positive)
 * are dh3d_ransac_rigid's.  Everything below is float64 on the exact float64 values of the float32 inputs.
 *   n < 3: no model (Rt NaN, valid 0, num_inliers 0, iterations 0, weights 0).
 *   xc = (sum x) / n, yc = (sum y) / n;  X = x - xc, Y = y - yc
 *   D2 = max over j of max(|X_j|^2, |Y_j|^2), taken as D2 = 0 then D2 = v where v > D2 (a NaN term is skipped);
 *   d2 = threshold * threshold;  mu = D2 > d2 ? D2 : d2
 *   w_j = 1;  at = 0;  k = 0
 *   loop:
 *       (R, t) = weighted_fit(w);  k += 1
 *       if mu == d2: at += 1
 *       if at > settle or k >= max_iterations: break
 *       r_j = X_j - ((R Y_j) + t);  w_j = (mu / (|r_j|^2 + mu))^2
 *       mu = mu / division;  mu = mu > d2 ? mu : d2
 *   Rt = [R | (xc - R yc) + t]
 *   weighted_fit: W = sum w, cx = (sum w X) / W, cy = (sum w Y) / W, B = sum over j of w_j * (A^T A of the pair
 *     (X_j - cx, Y_j - cy), dh3d_ransac_rigid's A), R = quat2rot(the unit eigenvector of B's smallest eigenvalue, cyclic
 *     Jacobi), t = cx - R cy.  Sums: each of the 256 lanes over its j = lane, lane + 256, ... in order, then a fixed tree.
 * So the schedule runs m + settle + 1 fits, m the number of divisions that bring D2 down to d2 (0 when D2 <= d2), unless
 * max_iterations ends it first; max_iterations = 1 is the plain least-squares fit.  The weights are never stored: w of fit
 * k + 1 is recomputed from the pose of fit k and that fit's mu.
 * Outputs, every element written: Rt [P, 3, 4] float64 (NaN where valid is 0); weights [P, Ma] float64 (the w the last fit
 * used, at the anchor rows of the correspondences, 0 at every other row); inliers [P, Ma] uint8 (1 where
 * sqrt(|x - (R y + t)|^2) < threshold under Rt, dh3d_ransac_rigid's inlier expression); num_inliers [P]; num_corr [P] = n;
 * iterations [P] = k; valid [P] = n >= 3 and every entry of the pose finite and num_inliers >= 3.
 * NULL pointers, P / Ma / Mb <= 0, a stride below 3, threshold <= 0, division <= 1, settle < 0, max_iterations outside
 * 1 .. 1024 (NaN scalars included): DH3D_ERR_INVALID_ARGUMENT, checked first; then Ma or Mb > 4096 or P > 65535:
 * DH3D_ERR_UNSUPPORTED. */
int dh3d_gnc_rigid(const float *anchor_xyz, long long anchor_stride, const float *positive_xyz, long long positive_stride,
                   const int32_t *match, const int32_t *anchor_count, int P, int Ma, int Mb, double threshold, double division,
                   int settle, int max_iterations, double *Rt, double *weights, int32_t *valid, uint8_t *inliers,
                   int32_t *num_inliers, int32_t *num_corr, int32_t *iterations, void *stream);

/* Dense point-to-point ICP refinement of P registered cloud pairs (csrc/icp.hip): from a pose of dh3d_ransac_rigid to the
 * least-squares pose over the clouds' nearest-neighbour pairs, with the dense overlap of the result.
 * INPUTS: anchor point i of pair p at anchor + (p*Na + i) * anchor_stride (3 floats), positive point j at positive +
 *   (p*Nb + j) * positive_stride (strides in elements, >= 3).  na = clamp(anchor_count[p], 0, Na), nb likewise; a NULL count
 *   means Na / Nb.  Rt0 [P, 3, 4] float64 = [R | t], dh3d_ransac_rigid's convention: anchor ~ R * positive + t.  valid0 [P]
 *   or NULL.  Everything below is float64 on the exact values of the float32 inputs, every operation rounded on its own.
 * ASSOCIATION A(R, t): for every positive j < nb, y'_r = ((R_r0 * y_0 + R_r1 * y_1) + R_r2 * y_2) + t_r; for every anchor
 *   i < na, d2(i, j) = (dx*dx + dy*dy) + dz*dz with dx = (double)x_i0 - y'_0 (dy, dz likewise); nn[j] = the i with the smallest
 *   d2 among those with d2 < max_dist * max_dist (strict; the product in double), ties to the lowest i; nn[j] = -1 when there is
 *   none or j >= nb.  The result does not depend on how the search is organised (scan or cell lists).
 * FIT F(nn): the pairs (anchor[nn[j]], positive[j]) with nn[j] >= 0 in ascending j, n of them.  n >= 3: estimateRigidTransform
 *   as dh3d_ransac_rigid's refit -- centroids, B over the centred pairs, the eigenvector of B's smallest eigenvalue (cyclic
 *   Jacobi), R = quat2rot(q), t = x_centroid - R * y_centroid; sums: lane j % 256 over its j in ascending order, then a fixed
 *   tree.  n < 3: the pose stays as it was.
 * LOOP: pose = Rt0; `iterations` times { nn = A(pose); pose = F(nn) }; then nn = A(pose) once more, which describes the
 *   returned pose.  No early exit: a pure function of the inputs.  iterations = 0 evaluates the given pose.
 * OUTPUTS: Rt [P, 3, 4] float64; nn [P, Nb] the last association; num_corr [P] = #{j : nn[j] >= 0}; fitness [P] float64 =
 *   num_corr / max(nb, 1); rmse [P] float64 = sqrt(sum of d2(nn[j], j) / num_corr) (the sum in the fit's order), NaN when
 *   num_corr = 0; valid [P].  A pair whose valid0 is 0 or whose Rt0 has a non-finite entry: Rt NaN, nn -1, num_corr 0,
 *   fitness 0, rmse NaN, valid 0; every other pair has valid 1.  Every element is written.  Rt may be Rt0.
 * INDEPENDENCE: a pair's result does not depend on the batch, on the path, on the workspace's content or on the run.  NaN and
 *   infinite coordinates are outside the contract.
 * path: 0 = the plan's choice, 1 = scan (any shape), 2 = cell lists over dh3d_spatial_sort_cells(anchor) (Na <= 16384).
 * dh3d_icp_plan (host only; the shape alone): 1 scan, 2 cell lists, -1 for a shape the call refuses.
 * dh3d_icp_refine_ws_bytes (host only): bytes of the caller-owned workspace (16-byte aligned, no clearing needed); 0 exactly
 *   where the plan is -1 or P is out of range.
 * SIDE EFFECTS: caller's stream, one launch after the other (no parallel branches), no host sync, no allocation, no
 *   floating-point atomics; graph-capturable.
 * STATUS: NULL pointers (the counts and valid0 excepted), P / Na / Nb <= 0, a stride below 3, max_dist not positive and
 *   finite, iterations < 0, a path other than 0 / 1 / 2, a NULL, misaligned or too small workspace:
 *   DH3D_ERR_INVALID_ARGUMENT.  Na or Nb > 131072, P > 65535, iterations > 256, path 2 with Na > 16384: DH3D_ERR_UNSUPPORTED. */
int dh3d_icp_plan(int Na, int Nb);
size_t dh3d_icp_refine_ws_bytes(int P, int Na, int Nb);
int dh3d_icp_refine(const float *anchor, long long anchor_stride, const int32_t *anchor_count, const float *positive,
                    long long positive_stride, const int32_t *positive_count, const double *Rt0, const int32_t *valid0, int P,
                    int Na, int Nb, double max_dist, int iterations, int path, double *Rt, int32_t *nn, int32_t *num_corr,
                    double *fitness, double *rmse, int32_t *valid, void *workspace, size_t workspace_bytes, void *stream);

/* Surface normals from given neighbour lists (csrc/normals.hip) -- external/findPointNormals.m of the reference's
 * evaluation: PCA of a point's k nearest neighbours, the eigenvector of the smallest eigenvalue flipped towards a view point.
 * INPUTS: point i of cloud p at xyz + (p*N + i) * xyz_stride (3 floats; the stride in elements, >= 3).  n = clamp(count[p], 0,
 *   N); a NULL count means N.  nbr [P, N, K] int32: the neighbour ids of every point, from the caller's exact kNN (the call
 *   searches nothing).  viewpoint: three doubles in HOST memory, read before the call returns.
 * RULE, float64 on the exact values of the float32 coordinates, every operation rounded on its own.  For every point i < n:
 *   the usable neighbours are the entries of nbr[p, i, :] with 0 <= id < n, in list order, m of them; duplicates count as
 *   given and i itself takes part only where the list holds it.  c = (sum of x) / m per axis; C_ab = (sum of (x_a - c_a) *
 *   (x_b - c_b)) / m for ab = 00 01 02 11 12 22; every sum starts from 0 and runs in list order.  Cyclic Jacobi on C (the
 *   rotations and the drop rule of dh3d_ransac_rigid's refit, on 3 x 3; csrc/rigid_fit.h) leaves the eigenvalues on the
 *   diagonal, in their places d_0 d_1 d_2, and the accumulated rotations V.  l_0 = the first smallest d_k, e = column k of V
 *   (unit up to the rotations' roundings; not normalised again).  sum = (d_0 + d_1) + d_2.
 *   s = ((v_0 - x_i0) * e_0 + (v_1 - x_i1) * e_1) + (v_2 - x_i2) * e_2; the normal is -e when s < 0, else e.
 * OUTPUTS: normals [P, N, 3] float32 (the float64 normal rounded once), curvature [P, N] float32 = l_0 / sum.  m < 3 or a sum
 *   that is not > 0 (coincident neighbours): normal (0, 0, 0), curvature 0.  Rows i >= n: normal 0, curvature 0.  Every
 *   element is written.  A point's result does not depend on the batch or on the run.  NaN and infinite coordinates are
 *   outside the contract.
 * SIDE EFFECTS: one launch on the caller's stream, no host sync, no allocation, no workspace, no atomics; graph-capturable
 *   (the viewpoint is captured by value).
 * STATUS: NULL pointers (count excepted), P / N / K <= 0, a stride below 3: DH3D_ERR_INVALID_ARGUMENT.  K > 64, N > 131072,
 *   P > 65535: DH3D_ERR_UNSUPPORTED. */
int dh3d_estimate_normals(const float *xyz, long long xyz_stride, const int32_t *count, const int32_t *nbr, int P, int N, int K,
                          const double *viewpoint, float *normals, float *curvature, void *stream);

/* Dense point-to-plane ICP refinement (csrc/icp.hip): dh3d_icp_refine with another fit.  The inputs, the ASSOCIATION A, the
 * LOOP (pose = Rt0; `iterations` times { nn = A(pose); pose = F_plane(nn, pose) }; then nn = A(pose) once more), the paths,
 * the plan, the limits and the independence guarantees are dh3d_icp_refine's, word for word.  In addition:
 * INPUTS: the normal of anchor point i of pair p at anchor_normals + (p*Na + i) * normals_stride (3 floats, stride in elements,
 *   >= 3), as dh3d_estimate_normals writes them; a zero normal takes its point out of the fit, not out of the association.
 * FIT F_plane(nn, pose = [R | t]), float64 on the exact float32 values, every operation rounded on its own.  The pairs are
 *   the j < nb in ascending order with i = nn[j] >= 0 and (n_0*n_0 + n_1*n_1) + n_2*n_2 > 0 for n = the normal of anchor i;
 *   n_pl of them.  n_pl < 6: the pose stays as it was.  m_j = y'_j of the association under the pose; c = (sum of m_j) / n_pl.
 *   Per pair q = m_j - c; a = (q_1*n_2 - q_2*n_1, q_2*n_0 - q_0*n_2, q_0*n_1 - q_1*n_0, n_0, n_1, n_2); d = (double)x_i - m_j
 *   per axis; r = (d_0*n_0 + d_1*n_1) + d_2*n_2.  H_uv = sum of a_u * a_v (u <= v, 21 sums), g_u = sum of a_u * r (6 sums).
 *   Every sum (n_pl's three for c included): lane j % 256 over its j in ascending order from 0, then a fixed tree.
 *   H s = g by Cholesky, row by row: for k = 0..5, for j = 0..k: v = H_jk, then v = v - L_kq * L_jq for q = 0..j-1; j < k:
 *   L_kj = v / L_jj; j = k: the pivot v, L_kk = sqrt(v).  A pivot that is not finite or is <= 1e-12 * max_u H_uu leaves the
 *   pose as it was.  z_k = (g_k - L_k0 z_0 - ... - L_k,k-1 z_k-1) / L_kk for k = 0..5 and s_k = (z_k - L_k+1,k s_k+1 - ... -
 *   L_5k s_5) / L_kk for k = 5..0, the subtractions one after the other in that order.  A non-finite s leaves the pose.
 *   w = s[0:3], tt = (w_0*w_0 + w_1*w_1) + w_2*w_2, th = sqrt(tt).  th == 0: dR = I.  Else A = sin(th) / th, hs = sin(th / 2),
 *   B = (2 * (hs * hs)) / (th * th), K = [[0, -w_2, w_1], [w_2, 0, -w_0], [-w_1, w_0, 0]], K2_uv = w_u * w_v (minus tt on the
 *   diagonal), dR_uv = (I_uv + A * K_uv) + B * K2_uv.  The new pose: R_uv = (dR_u0 * R_0v + dR_u1 * R_1v) + dR_u2 * R_2v;
 *   u = t - c; t_u = (((dR_u0 * u_0 + dR_u1 * u_1) + dR_u2 * u_2) + c_u) + s_3+u.
 * OUTPUTS: Rt, nn, num_corr, fitness, rmse (point-to-point, over all pairs of nn: the two methods compare) and valid as
 *   dh3d_icp_refine gives them; num_plane [P] int32 = n_pl of the last association; rmse_plane [P] float64 = sqrt(sum of
 *   r * r / num_plane) under the returned pose (the sum in the fit's order), NaN when num_plane = 0.  A pair that is not valid
 *   comes back as from dh3d_icp_refine, with num_plane 0 and rmse_plane NaN.  Every element is written.  Rt may be Rt0.
 * dh3d_icp_refine_plane_ws_bytes (host only): the workspace, as dh3d_icp_refine_ws_bytes; the plan is dh3d_icp_plan.
 * SIDE EFFECTS: caller's stream, one launch after the other (no parallel branches), no host sync, no allocation, no
 *   floating-point atomics; graph-capturable.
 * STATUS: dh3d_icp_refine's, with NULL anchor_normals / num_plane / rmse_plane or a normals_stride below 3 among the
 *   DH3D_ERR_INVALID_ARGUMENT cases. */
size_t dh3d_icp_refine_plane_ws_bytes(int P, int Na, int Nb);
int dh3d_icp_refine_plane(const float *anchor, long long anchor_stride, const int32_t *anchor_count, const float *anchor_normals,
                          long long normals_stride, const float *positive, long long positive_stride,
                          const int32_t *positive_count, const double *Rt0, const int32_t *valid0, int P, int Na, int Nb,
                          double max_dist, int iterations, int path, double *Rt, int32_t *nn, int32_t *num_corr, double *fitness,
                          double *rmse, int32_t *valid, int32_t *num_plane, double *rmse_plane, void *workspace,
                          size_t workspace_bytes, void *stream);

/* FPFH descriptors from given normals and neighbour lists (csrc/fpfh.hip) -- Fast Point Feature Histograms (Rusu, Blodow,
 * Beetz, ICRA 2009): per point three 11-bin histograms of the angular features of its point pairs (the SPFH), then the
 * 1 / d^2 weighted sum of its neighbours' SPFHs.  The reference tree holds no FPFH: the rule below is this project's own; it
 * follows the published definition and the usual conventions (3 x 11 bins, weights 1 / d^2, blocks scaled to 100), and DESIGN.md
 * lists every point where it had to choose (INFERRED).
 * INPUTS: point i of cloud p at xyz + (p*N + i) * xyz_stride and its normal at normals + (p*N + i) * normals_stride (3 floats
 *   each; the strides in elements, >= 3); normals are used as given, never normalised again.  n = clamp(count[p], 0, N); a
 *   NULL count means N.  nbr [P, N, K] int32, 1 <= K <= 64: the neighbour ids of every point, from the caller's exact kNN (the
 *   calls search nothing).  max_dist: <= 0 (or NaN) means no radius, else r2 = max_dist * max_dist.
 * ARITHMETIC: float64 on the exact values of the float32 inputs, every operation rounded on its own.
 *   dot(a, b) = (a_0*b_0 + a_1*b_1) + a_2*b_2; cross(a, b) = (a_1*b_2 - a_2*b_1, a_2*b_0 - a_0*b_2, a_0*b_1 - a_1*b_0);
 *   sqrt is IEEE; atan2 is the device library's.
 * PAIRS: for point i < n and k ascending, j = nbr[p, i, k]: d = x_j - x_i per axis, d2 = dot(d, d).  The pair is NEAR iff
 *   0 <= j < n, j != i, d2 > 0 and (no radius or d2 <= r2).  A repeated id counts as often as it occurs.  A near pair is USABLE
 *   iff dot(n_i, n_i) > 0, dot(n_j, n_j) > 0 and vn > 0 below.
 * STAGE 1, dh3d_spfh_counts.  Per usable pair: len = sqrt(d2), a1 = dot(n_i, d) / len, a2 = dot(n_j, d) / len.  If |a1| < |a2|
 *   then (n1, n2, d, f3) = (n_j, n_i, -d, -a2), else (n1, n2, d, f3) = (n_i, n_j, d, a1).  v = cross(d, n1), vn = sqrt(dot(v,
 *   v)), v = v / vn per axis, w = cross(n1, v); f2 = dot(v, n2), f1 = atan2(dot(w, n2), dot(n1, n2)).  Bin coordinates s1 =
 *   (f1 + pi) * (11 / (2 pi)), s2 = (f2 + 1) * 5.5, s3 = (f3 + 1) * 5.5 (pi the double nearest pi, 11 / (2 pi) = 11.0 /
 *   (2.0 * pi) rounded as written); bin = min(max(floor(s), 0), 10).
 *   OUTPUT counts [P, N, 36] uint8 (4-byte aligned): bytes 0-10 the f1 histogram, 11-21 f2, 22-32 f3, byte 33 m_i = the
 *   number of usable pairs, bytes 34-35 zero.  Rows i >= n are all zero.  Every byte is written.  counts is an ordinary
 *   output of the caller's, not scratch memory: dh3d_fpfh reads it.
 * STAGE 2, dh3d_fpfh.  Output row r < M of cloud p describes point i = ids[p, r] (ids [P, M] int32), or i = r when ids is NULL
 *   (then M must equal N); an i outside 0 .. n-1 gives a zero row.  SPFH(i)[c] = counts[i][c] * (100.0 / m_i) for c < 33, zero
 *   when m_i = 0.  acc[c] starts from 0 and runs over the NEAR pairs of i in list order (usable or not; the lists, count and
 *   max_dist must be stage 1's): acc[c] = acc[c] + (1.0 / d2) * SPFH(j)[c].  Per block t = 0, 1, 2 of 11 bins: S_t = the sum
 *   of acc[11 t .. 11 t + 10] in ascending order from 0; scale_t = S_t > 0 ? 100.0 / S_t : 0.
 *   OUTPUT fpfh [P, M, 36] float32: fpfh[c] = (float)(acc[c] * scale_t + SPFH(i)[c]) for c < 33; columns 33-35 are zero, so
 *   dh3d_match_descriptors (D a multiple of 4) reads the rows in place.  Up to rounding a block sums to 200 when m_i > 0 and a near neighbour has m_j > 0, to 100
 *   when only one of the two holds (a point without near pairs gets its own SPFH), else to 0.  Every element is written.
 * A point's result does not depend on the batch or on the run.  NaN and infinite inputs are outside the contract.
 * SIDE EFFECTS: one launch each on the caller's stream, no host sync, no allocation, no scratch buffer, no atomics on global
 *   memory; graph-capturable.
 * STATUS: NULL pointers (count and ids excepted), a counts pointer that is not 4-byte aligned, P / N / M <= 0, K < 1 or K > 64,
 *   a stride below 3, ids NULL with M != N: DH3D_ERR_INVALID_ARGUMENT.  N or M > 131072, P > 65535: DH3D_ERR_UNSUPPORTED. */
int dh3d_spfh_counts(const float *xyz, long long xyz_stride, const float *normals, long long normals_stride, const int32_t *count,
                     const int32_t *nbr, int P, int N, int K, double max_dist, uint8_t *counts, void *stream);
int dh3d_fpfh(const float *xyz, long long xyz_stride, const int32_t *count, const int32_t *nbr, const uint8_t *counts,
              const int32_t *ids, int P, int N, int K, int M, double max_dist, float *fpfh, void *stream);

/* Preparation of raw clouds (csrc/prepare.hip) -- get_fixednum_pcd(need_downsample = True, randsample = False)
 * (core/utils.py:87-110: open3d voxel_down_sample, remove_radius_outlier(nb_points, radius), crop to the points nearest the
 * centroid or pad), batched, for clouds of different sizes, with every size kept on the device.
 * raw [B, Nraw, 3], num_raw [B]: cloud b is raw[b, :n], n = clamp(num_raw[b], 0, Nraw); its rows must be finite.
 * STAGE 1, voxel grid (voxel_size > 0; voxel_size == 0 skips it: the stage-1 points are the raw ones).  lo = the per-axis
 *   minimum of the cloud; origin = double(lo) - voxel_size / 2 (INFERRED); cell = floor((double(p) - origin) / voxel_size)
 *   per axis, in double, by a true division.  Points of equal cell triples form one voxel; its point is
 *   float32((sum of double(p)) / count), the sum starting from 0 and running over the members in ascending index
 *   (INFERRED: point order); the voxels come out in the order of their lowest member index.  (open3d returns float64
 *   points in its hash map's order; nothing downstream depends on either.)
 * STAGE 2, radius outliers (radius > 0; radius == 0 skips it), on the stage-1 points: i is kept iff
 *   #{j : d2(i, j) < r2} > nb_points, j over all points of the cloud, i included (INFERRED: the strict <; INFERRED: more
 *   than nb_points with the point itself counted); d2 = (dx*dx + dy*dy) + dz*dz in double on the float32 coordinates, no
 *   contraction; r2 = radius * radius in double.  The kept points stay in order.
 * STAGE 3, fixed size, m = the number of survivors.  centroid [B, 3] float64 = their mean (a fixed summation tree: within
 *   m * 2^-52 * max|coordinate| of any other order; zeros when m = 0).  m <= targetnum: the survivors, then rows of 100000.0,
 *   num_valid = m.  m > targetnum: num_valid = targetnum and the rows are, in their stage-2 order, the targetnum points with
 *   the smallest (d2 to the centroid, index) (sortby_dis != 0, d2 as in stage 2 with the returned centroid), or the first
 *   targetnum points (sortby_dis == 0).  The reference then shuffles the kept points with an unseeded permutation; here they
 *   keep their order.  Padding by re-drawn points (randsample = True) is not on the device.
 * Outputs: points [B, targetnum, 3], num_valid [B], counts [B, 3] = (n, voxels, survivors), centroid [B, 3]; every element
 *   is written.  A result does not depend on the batch, on the workspace's content or on the run.
 * LIMITS: Nraw <= 131072, targetnum <= 2^20, B <= 65535 (else DH3D_ERR_UNSUPPORTED); B, Nraw, targetnum <= 0, NULL pointers,
 *   a negative or non-finite voxel_size / radius, nb_points < 0, a workspace smaller than dh3d_prepare_clouds_workspace() or
 *   not 16-byte aligned: DH3D_ERR_INVALID_ARGUMENT.  A cell index of 2^21 or more on an axis (stage 1, or the stage-2 cells
 *   of edge radius) is beyond the 63-bit keys.  It depends on the data, which the host never reads (no synchronisation), so
 *   it cannot be this call's status: that cloud comes back void -- num_valid 0, every row 100000.0, counts (n, -1, -1) -- and
 *   a caller that wants DH3D_ERR_UNSUPPORTED for it tests counts[b][1] < 0 where it next synchronises.
 * Caller's stream, no allocation, no synchronisation, graph-capturable; the workspace needs no clearing. */
size_t dh3d_prepare_clouds_workspace(int B, int Nraw, int targetnum); /* bytes; 0 for a shape the call refuses.  Host only. */
int dh3d_prepare_clouds(int B, int Nraw, int targetnum, const float *raw, const int32_t *num_raw, double voxel_size,
                        double radius, int nb_points, int sortby_dis, float *points, int32_t *num_valid, int32_t *counts,
                        double *centroid, void *workspace, size_t workspace_bytes, void *stream);

/* Place retrieval (csrc/retrieval.hip) -- evaluation_retrieval.py:37-40, cKDTree(database).query(queries, k): the exact
 * float64 top-k search of Q query descriptors in a map of R reference descriptors, without a [Q, R] matrix.
 * INPUTS: ref holds R rows of D floats, row j at ref + j * ref_stride; qry holds Q rows likewise with qry_stride (strides in
 *   elements, any value >= D: a column view such as rows[:, 3:131] of 132-column rows is read in place, as
 *   dh3d_match_descriptors does).  ref_count: a device pointer to one int32, or NULL.  The live map is rows 0 .. r-1 with
 *   r = clamp(*ref_count, 0, R); NULL means r = R.  Rows >= r are never read.  The host never learns r: a captured graph
 *   keeps serving a map that grows inside its capacity R.
 * DISTANCE: d2(q, j) = the sum over c ascending, starting from 0, of ((double)q_c - (double)r_jc)^2; every subtraction,
 *   product and addition is rounded to float64 on its own (no fma contraction).
 * ORDER: ascending by (d2, j): ties go to the lowest map id.
 * OUTPUTS: idx [Q, k] and dist2 [Q, k] hold the first min(k, r) entries of that order per query; the remaining entries are
 *   -1 and +inf.  Every element is written.
 * INDEPENDENCE: a query's row does not depend on Q, on the other queries, on the capacity R beyond r, on the number of
 *   slices S, on the workspace's content or on the run.
 * NaN and infinite inputs are outside the contract.
 * dh3d_retrieve_plan (host only; looks at the four numbers alone): the number S >= 1 of contiguous slices the map is cut into,
 *   each scanned by its own workgroups (slice s = rows [s * L, (s + 1) * L) with L = 256 * ceil(ceil(R / 256) / S); none is
 *   empty), or -1 for a shape the call refuses.  S = min(ceil(R / 256), max(1, 512 / ceil(Q / 16))), then lowered to
 *   ceil(ceil(R / 256) / (L / 256)): a few queries against a large map still fill the machine, many queries do not split.
 *   S > 1 adds one launch that merges the S partial lists of the workspace.
 * dh3d_retrieve_ws_bytes (host only): bytes of the caller-owned workspace (16-byte aligned, no clearing needed); 0
 *   exactly where the plan is -1.
 * SIDE EFFECTS: caller's stream, no host sync, no allocation, no atomics on global memory; graph-capturable, one launch
 *   after the other (no parallel branches).
 * STATUS: D % 4 != 0, D > 256 or k > 64: DH3D_ERR_UNSUPPORTED (plan -1, workspace 0).  NULL ref, qry, idx or dist2,
 *   Q / R / D / k <= 0, a stride below D, a NULL, misaligned or too small workspace: DH3D_ERR_INVALID_ARGUMENT. */
int dh3d_retrieve_plan(int Q, int R, int D, int k);
size_t dh3d_retrieve_ws_bytes(int Q, int R, int D, int k);
int dh3d_retrieve(const float *ref, long long ref_stride, const int32_t *ref_count, const float *qry, long long qry_stride,
                  int Q, int R, int D, int k, int32_t *idx, double *dist2, void *ws, size_t ws_bytes, void *stream);

/* Training batches (csrc/pairs.hip) -- what core/datasets.py builds on the host, one cloud at a time, between the prepared
 * clouds and the trainers: Local_train_dataset_selfpair.loadPair (:119-151) and Global_train_dataset_triplet.loadPC
 * (:184-191) over core/utils.py get_fixednum_pcd(randsample = True), core/augment.py and FarthestSampler.sample.
 * RANDOMNESS.  numpy's streams cannot be reproduced; every draw is a pure function of (seed, stream, b, j), with splitmix64
 *   as written out at dh3d_ransac_rigid and uint64 wrap-around everywhere:
 *     h(stream, b) = splitmix64(splitmix64(seed) ^ ((uint64(stream) << 32) | uint64(b)))
 *     u(stream, b, j) = splitmix64(h(stream, b) + j)
 *   b is the cloud's (for dh3d_pair_rotate / dh3d_sample_pair_nodes: the pair's) index in the call.  A uniform double in
 *   [0, 1) is U = (u >> 11) * 2^-53; in (0, 1] it is (u >> 11) * 2^-53 + 2^-53.  An integer in [0, n) is u mod n.  A standard
 *   normal for element e is z(stream, b, e) = sqrt(-2 ln U1) * cos(2 pi U2) in float64 (Box-Muller, cosine branch only) with
 *   U1 in (0, 1] from u(stream, b, 2e) and U2 in [0, 1) from u(stream, b, 2e + 1).  A random choice of m from n without
 *   replacement is the m indices i with the smallest keys (u(stream, b, i), i), emitted in ascending i (a stable compaction;
 *   splitmix64 is a bijection, so the u alone never tie).  The streams:
 *     1 resample keys   2 pad draws   3 Rotate1D angle   4 jitter   5 scale   6 RotateSmall angles   7 shift
 *     8 pair rotation   9 subset keys   10 first pick
 *   ("Training tuples" below takes 11 .. 15, "Weighted sampling" 16.)
 *   seed is a DEVICE pointer to one uint64, read by the kernels: a captured graph draws a fresh batch on every replay when
 *   the caller changes that scalar between replays.
 * Every entry point below: caller's stream, no allocation, no synchronisation, graph-capturable (launches one after the
 *   other, no parallel branches); every output element is written; cloud b's result depends on (seed, b) and its own rows,
 *   not on B, on the other clouds, on the workspace's content or on the run.  B, N, Nsrc, targetnum <= 0 or a NULL pointer:
 *   DH3D_ERR_INVALID_ARGUMENT; B > 65535: DH3D_ERR_UNSUPPORTED.  NaN and infinite coordinates are outside the contract.
 *
 * dh3d_resample_clouds -- get_fixednum_pcd(randsample = True, sortby_dis = False) after its outlier removal (which
 *   dh3d_prepare_clouds does; its sortby_dis crop followed by this call restates loadPC's sortby_dis = True draw).
 *   points [B, Nsrc, 3], num_valid [B]: cloud b is rows 0 .. n-1, n = clamp(num_valid[b], 0, Nsrc); rows >= n are never read.
 *   n >= targetnum: a random choice (stream 1) of targetnum from n.  0 < n < targetnum: the n rows, then row
 *   u(2, b, j) mod n for j = 0 .. targetnum-n-1.  n == 0: rows of 100000.0.  out [B, targetnum, 3], num_orig [B] =
 *   min(n, targetnum).  Nsrc <= 131072, targetnum <= 2^20 (else DH3D_ERR_UNSUPPORTED, workspace 0); a NULL, too small or not
 *   16-byte aligned workspace: DH3D_ERR_INVALID_ARGUMENT.  The workspace needs no clearing. */
size_t dh3d_resample_clouds_ws_bytes(int B, int Nsrc, int targetnum); /* bytes; 0 for a shape the call refuses.  Host only. */
int dh3d_resample_clouds(int B, int Nsrc, int targetnum, const float *points, const int32_t *num_valid,
                         const unsigned long long *seed, float *out, int32_t *num_orig, void *workspace, size_t workspace_bytes,
                         void *stream);
/* dh3d_augment_clouds -- core/augment.py.  aug_mask selects augmentations; they run in the fixed order of
 *   get_augmentations_from_list (upright axis z), as one float64 chain on the exact float64 values of the float32 input, each
 *   operation rounded to float64 on its own, the result rounded ONCE to float32 (the reference computes in float64 and casts
 *   at the feed).  row * M below is ((x M[0][c] + y M[1][c]) + z M[2][c]) for c = 0, 1, 2; a 3 x 3 product A B has elements
 *   (A[r][0] B[0][c] + A[r][1] B[1][c]) + A[r][2] B[2][c].
 *     Rotate1D     angle = (U * 2) * pi, U = U(3, b, 0); M = [[c, s, 0], [-s, c, 0], [0, 0, 1]]; row = row * M
 *     Jitter       coordinate c of point i: e = 3 i + c; v = clip(sigma * z(4, b, e), -clip, clip) + v
 *     Scale        s = scale_low + (scale_high - scale_low) * U(5, b, 0); v = v * s
 *     RotateSmall  a_e = clip(angle_sigma * z(6, b, e), -angle_clip, angle_clip), e = 0, 1, 2; Rx = [[1, 0, 0], [0, c0, -s0],
 *                  [0, s0, c0]], Ry = [[c1, 0, s1], [0, 1, 0], [-s1, 0, c1]], Rz = [[c2, -s2, 0], [s2, c2, 0], [0, 0, 1]];
 *                  M = Rz (Ry Rx); row = row * M
 *     Shift        t_c = -shift_range + (shift_range - -shift_range) * U(7, b, c); v_c = v_c + t_c
 *   The reference's defaults: sigma 0.05, clip 0.1, scale 0.8 .. 1.25, angle_sigma 0.06, angle_clip 0.18, shift_range 0.1.
 *   Outputs: out [B, N, 3]; the cloud's parameters in float64 -- rot1d [B, 3, 3], scale [B], rot_small [B, 3, 3], shift
 *   [B, 3] -- the identity, 1 and 0 for an augmentation that is off.  out may be points (in place).  A bit of aug_mask outside
 *   DH3D_AUG_ALL, a negative or non-finite parameter, clip <= 0, scale_low <= 0 or > scale_high: DH3D_ERR_INVALID_ARGUMENT. */
#define DH3D_AUG_ROTATE1D 1u
#define DH3D_AUG_JITTER 2u
#define DH3D_AUG_SCALE 4u
#define DH3D_AUG_ROTATESMALL 8u
#define DH3D_AUG_SHIFT 16u
#define DH3D_AUG_ALL 31u
int dh3d_augment_clouds(int B, int N, const float *points, unsigned aug_mask, double sigma, double clip, double scale_low,
                        double scale_high, double angle_sigma, double angle_clip, double shift_range,
                        const unsigned long long *seed, float *out, double *rot1d, double *scale, double *rot_small,
                        double *shift, void *stream);
/* dh3d_pair_rotate -- loadPair's rotation of the second cloud: angle = (2 U - 1) * rot_maxv, U = U(8, b, 0); Rot = [[c, s, 0],
 *   [-s, c, 0], [0, 0, 1]] in float64; pc2_trans [B, N, 3] = float32(row * Rot) on the float64 values of pc2's rows; R [B, 3, 3]
 *   = float32(Rot).  pc2_trans may be pc2.  rot_maxv negative or non-finite: DH3D_ERR_INVALID_ARGUMENT. */
int dh3d_pair_rotate(int B, int N, const float *pc2, double rot_maxv, const unsigned long long *seed, float *pc2_trans, float *R,
                     void *stream);
/* dh3d_sample_pair_nodes -- the second half of loadPair for B pairs pc1, pc2 [B, N, 3].
 *   subset = a random choice (stream 9) of N / 2 (rounded down) from N, in index order.  pick_0 = u(10, b, 0) mod (N / 2), a
 *   POSITION in subset.  FarthestSampler.sample: dmin = d2(subset[pick_0], .); for t = 1 .. sample_nodes-1: pick_t = the
 *   FIRST position holding the maximum of dmin; dmin = min(dmin, d2(subset[pick_t], .)).  d2 = (dx*dx + dy*dy) + dz*dz in
 *   float64 on the float32 coordinates, no contraction (the rule of dh3d_prepare_clouds' radius test).
 *   anc [B, sample_nodes] = the row in pc1 of subset[pick_t]; pos [B, sample_nodes] = the j with the smallest
 *   d2(pc1[anc], pc2[j]), the lowest j on ties.  N <= 16384 and 1 <= sample_nodes <= N / 2, else DH3D_ERR_UNSUPPORTED.
 *   (dh3d_farthest_point_sample* start at index 0 with a contracted float32 distance: another contract.)  No workspace. */
int dh3d_sample_pair_nodes(int B, int N, int sample_nodes, const float *pc1, const float *pc2, const unsigned long long *seed,
                           int32_t *anc, int32_t *pos, void *stream);

/* Training tuples (csrc/tuples.hip) -- which places form a quadruplet: Global_train_dataset_triplet.__iter__
 * (core/datasets.py:202-233), there Python set differences over the whole training set, here decided on the device from
 * the positions (and, for hard negatives, the descriptors) of a map of places; the ids feed "Training batches".
 * MAP.  pos holds M rows of two float64 (16-byte aligned).  count: a device pointer to one int32, or NULL.  The live map is
 *   places 0 .. n-1 with n = clamp(*count, 0, M); NULL means n = M.  Rows at or beyond n are never read (positions and
 *   descriptors alike).  The host never learns n.
 * DISTANCE.  Planar: d2(i, j) = (dx*dx) + (dy*dy) with dx = pos[j][0] - pos[i][0], dy = pos[j][1] - pos[i][1]; every
 *   operation is rounded to float64 on its own (no fma contraction).  rp2 = pos_radius * pos_radius and rn2 = neg_radius *
 *   neg_radius are rounded likewise, on the host side of the entry point.
 * SETS of a query place q -- the positives / nonnegtives convention of the tuple pickles the reference's loader reads; the
 *   query is its own non-negative:
 *     POS(q) = { j < n, j != q, d2(q, j) <= rp2 }          NEG(q) = { j < n, d2(q, j) > rn2 }
 *   The reference's radii: pos_radius = 10.0, neg_radius = 50.0.  A non-finite or non-positive radius, or neg_radius <
 *   pos_radius: DH3D_ERR_INVALID_ARGUMENT.
 * RANDOMNESS.  The scheme of "Training batches": u(stream, b, j) and U = (u >> 11) * 2^-53, with b = the query's slot in
 *   the call (dh3d_draw_queries: b = 0) and j = the place id.  The streams:
 *     11 positive keys   12 negative keys   13 pool membership   14 other-negative keys   15 query keys
 *   "The k smallest of a set by a stream" are the k members with the smallest keys (u(stream, b, j), j), emitted in
 *   ASCENDING KEY order: a uniform random k-subset in uniform random order.  (dh3d_resample_clouds emits its choice in index
 *   order: another rule.)  seed is a DEVICE pointer to one uint64, as there.
 * Every entry point below: caller's stream, no allocation, no synchronisation, graph-capturable (launches one after the
 *   other, no parallel branches); every output element is written; slot b's result depends on (seed, b, queries[b]) and the
 *   live map, not on Q, on the other slots, on the capacity M beyond n, on the workspace's content or on the run.
 * LIMITS.  M <= 2^20, Q <= 65535, 1 <= num_pos <= 64, 1 <= num_neg <= 64, 0 <= num_hard <= num_neg, D <= 256 and a multiple
 *   of 4; a shape beyond them: DH3D_ERR_UNSUPPORTED.  A NULL pointer (count, other_idx and desc excepted), M, Q, num_pos,
 *   num_neg or (with desc) D <= 0, num_hard < 0, a misaligned pos: DH3D_ERR_INVALID_ARGUMENT.  NaN and infinite values in
 *   the live map are outside the contract.
 *
 * dh3d_tuple_counts -- n_pos [M] = |POS(i)|, n_neg [M] = |NEG(i)| for i < n, 0 for i >= n.  O(n^2): once per map, or
 *   whenever the map grows. */
int dh3d_tuple_counts(const double *pos, const int32_t *count, int M, double pos_radius, double neg_radius, int32_t *n_pos,
                      int32_t *n_neg, void *stream);
/* dh3d_draw_queries -- the reference's shuffle plus its `continue` on too few positives: queries [Q] = the Q smallest by
 *   stream 15 of { i < n : n_pos[i] >= num_pos and n_neg[i] >= num_neg }.  Fewer than Q such places: the remaining entries
 *   are -1 and ok[0] = 0; otherwise ok[0] = 1.  The workspace (dh3d_draw_queries_ws_bytes: 0 for a shape the call refuses;
 *   16-byte aligned, no clearing needed; NULL, too small or misaligned: DH3D_ERR_INVALID_ARGUMENT) holds the chosen keys. */
size_t dh3d_draw_queries_ws_bytes(int M, int Q);
int dh3d_draw_queries(const int32_t *n_pos, const int32_t *n_neg, const int32_t *count, int M, int Q, int num_pos, int num_neg,
                      const unsigned long long *seed, int32_t *queries, int32_t *ok, void *workspace, size_t workspace_bytes,
                      void *stream);
/* dh3d_sample_tuples -- queries [Q] (device) -> pos_idx [Q, num_pos], neg_idx [Q, num_neg], other_idx [Q] (NULL: that stage
 *   is skipped), valid [Q].  Slot b with q = queries[b]:
 *   q < 0 or q >= n: everything is -1, valid = 0.
 *   POSITIVES  the num_pos smallest of POS(q) by stream 11; |POS(q)| < num_pos: the row is all -1.
 *   HARD NEGATIVES  only with num_hard > 0 and desc != NULL: desc holds M rows of D floats, row j at desc + j * desc_stride
 *     (elements; desc_stride >= D and a multiple of 4, desc 16-byte aligned, 0 <= pool_fraction <= 1, else
 *     DH3D_ERR_INVALID_ARGUMENT).  POOL = { j in NEG(q) : U(13, b, j) < pool_fraction } (1.0: all of NEG(q), 0.0: none).
 *     D2(q, j) = the sum over c ascending, starting from 0, of ((double)desc[q][c] - (double)desc[j][c])^2, every operation
 *     rounded on its own -- dh3d_retrieve's rule.  The hard negatives are the h' = min(num_hard, |POOL|) smallest of POOL
 *     by (bits of D2, j), ascending.  Without them h' = 0.
 *   RANDOM NEGATIVES  the num_neg - h' smallest of NEG(q) minus the hard ones, by stream 12.
 *   The negative row is [hard | random]; |NEG(q)| < num_neg: the row is all -1.
 *   OTHER NEGATIVE  -1 when the negative row is unfilled.  Otherwise, with BAR = { j < n : d2(q, j) <= rp2, or
 *     d2(g, j) <= rp2 for some g in the negative row }, other_idx[b] = the smallest of { j < n } \ BAR by stream 14, or -1
 *     if there is none.  DEVIATION from the reference: BAR holds the query and the chosen negatives themselves (their
 *     d2 = 0); the reference's set difference (datasets.py:224-232) subtracts only their neighbours and leaves them
 *     eligible, which can hand the loss the query as its own "other negative".
 *   valid [b] = 1 only if the positive row, the negative row and (when asked for) the other negative are all filled.
 *   No workspace. */
int dh3d_sample_tuples(const double *pos, const int32_t *count, int M, const int32_t *queries, int Q, int num_pos, int num_neg,
                       double pos_radius, double neg_radius, const float *desc, long long desc_stride, int D, int num_hard,
                       double pool_fraction, const unsigned long long *seed, int32_t *pos_idx, int32_t *neg_idx,
                       int32_t *other_idx, int32_t *valid, void *stream);

/* Weighted sampling (csrc/prob_sample.hip) -- ProbSample of tf_ops/sampling (tf_sampling.py:15-26, tf_sampling.cpp:65-92,
 * tf_sampling_g.cu:7-104) and its seeded form: m indices a row, WITH replacement, with probability proportional to a row of
 * n non-negative weights.  The op has no CPU twin upstream; the contract is the arithmetic of its two kernels.  All values
 * are float32 and every operation is rounded on its own (no fma contraction).
 * CUMULATIVE SUMS of a row w[0 .. n-1] (cumsumKernel, tf_sampling_g.cu:7-88).  Chunks of 8192 entries, the last may be
 *   shorter; the running sum R and its compensation C start at 0.  A chunk of L entries has G = ceil(L / 4) quads.
 *     full quad (a, b, c, d):  l0 = a, l1 = b + a, t = d + c, l2 = c + l1, l3 = t + l1, s[g] = l3
 *     partial last quad (1 .. 3 entries):  v = 0, then v += x in order; l_i = the running v, s[g] = the last v
 *     tree over s[0 .. G-1], in place:
 *       up-sweep    for u = 0, 1, .. while 2^(u+1) <= G, for k < floor(G / 2^(u+1)):  s[(2k+2) 2^u - 1] += s[(2k+1) 2^u - 1]
 *       down-sweep  from the last such u down to 0, for k < floor((G - 2^u) / 2^(u+1)):  s[(2k+3) 2^u - 1] += s[(2k+2) 2^u - 1]
 *     quads g >= 1:  l_i += s[g-1];   cum = l_i + R;   then t = s[G-1] + C, R' = R + t, C = t - (R' - R), R = R'
 *   The result is within 16 * 2^-24 relative of the exact sums, differs from a sequential float32 prefix sum in most entries
 *   and is NOT monotone: it can step down by an ulp between two quads.
 * SEARCH of one draw r_in (binarysearchKernel, :90-104).  P = the smallest power of two >= n, q = r_in * cum[n-1] (one
 *   multiply), r = n-1; for k = P, P/2, .. 1: if r >= k and cum[r-k] >= q then r -= k; the id is r.  The walk never assumes
 *   order, so on a non-monotone row it is not a lower bound of a sorted search; on a monotone row it is the first index with
 *   cum >= q, held to n-1.  A draw of 0 gives id 0 whatever its weight (the reference's behaviour).
 * Both entry points: caller's stream, no allocation, no synchronisation, graph-capturable (two launches, one after the other);
 *   every element of out is written; row b's result does not depend on the batch size, on the other rows or on temp's prior
 *   content.  b, n or m <= 0 or a NULL pointer (count excepted): DH3D_ERR_INVALID_ARGUMENT; b > 65535, n > 2^20 or m > 2^20:
 *   DH3D_ERR_UNSUPPORTED.  Negative, NaN and infinite weights are outside the contract.
 *
 * dh3d_prob_sample -- probsampleLauncher's arguments: inp_p [b, n] weights, inp_r [b, m] draws (the op feeds uniform values
 *   in [0, 1)), temp [b, n] the reference's scratch, which HOLDS THE CUMULATIVE SUMS on return, out [b, m].
 * dh3d_prob_sample_seeded -- the draws are made on the device by the scheme of "Training batches", stream 16:
 *     r_in(b, j) = (float)((u(16, b, j) >> 40) + 1) * 2^-24       exact in float32, in (0, 1]: q > 0
 *   count: NULL, or a device pointer [b]: row b is its entries 0 .. n_b-1 with n_b = clamp(count[b], 0, n) (NULL: n_b = n);
 *   entries at or beyond n_b are never read, and temp holds the sums of the first n_b entries, then zeros.  n_b == 0, or a total
 *   cum[n_b-1] that is not > 0: every id of the row is -1.  Otherwise no id has weight 0 as long as the sums before it are
 *   exact (q > 0 and the walk stops at the first cum >= q).  seed is a DEVICE pointer to one uint64, as there. */
int dh3d_prob_sample(int b, int n, int m, const float *inp_p, const float *inp_r, float *temp, int32_t *out, void *stream);
int dh3d_prob_sample_seeded(int b, int n, int m, const float *inp_p, const int32_t *count, const unsigned long long *seed,
                            float *temp, int32_t *out, void *stream);

/* Scan Context (csrc/scan_context.hip) -- Kim & Kim, "Scan Context: Egocentric Spatial Descriptor for Place Recognition
 * within 3D Point Cloud Map", IROS 2018: a rings x sectors polar height image per cloud, a rotation-invariant ring key to
 * short-list map places with (the exact top-k search of "Place retrieval" above takes it: Nr is a multiple of 4), and a
 * column-shifted cosine distance whose best shift is the yaw between two clouds.  The reference tree holds no Scan Context:
 * the rules below are this project's own statement of it, written so that the image is bit-defined.  No trained weights.
 *
 * THE IMAGE.  xyz holds P clouds of N rows, row i of cloud p at xyz + (p * N + i) * xyz_stride (stride in elements, >= 3: the
 *   first three columns of wider rows are read in place).  count: NULL, or [P] int32 -- cloud p is its rows 0 .. n_p-1 with
 *   n_p = clamp(count[p], 0, N) (NULL: N); rows at or beyond n_p are never read.  center: NULL (the origin), or [P, 2] float32
 *   (cx, cy).  z_offset: the sensor's height above the ground, added so that heights are positive.
 *   TABLES, made by the caller ONCE in float64 and read as they are -- no trigonometry and no division runs on the device, so
 *   the kernel and any restatement that reads the same tables see identical bits:
 *     sector_dir [Ns/2 - 1, 2] = (cos, sin)(2 pi k / Ns) for k = 1 .. Ns/2 - 1       ring_edge2 [Nr + 1] = (i * max_radius / Nr)^2
 *   PER POINT (x, y, z):  dx = x - cx, dy = y - cy, h = z + z_offset, each rounded once in float32;  X, Y = dx, dy as float64;
 *     r2 = X * X + Y * Y (two products, one addition).  The point COUNTS iff dx, dy and h are finite, r2 < ring_edge2[Nr] and
 *     h > 0 strictly (-0.0 does not count: the bit pattern of every counted height orders as an unsigned integer).
 *     RING    = the number of i in 1 .. Nr-1 with r2 >= ring_edge2[i].
 *     HALF    H = 0 if Y > 0, or if Y == 0 and X > 0; otherwise H = 1 and (X, Y) is negated.  (The origin is H = 1.)
 *     SECTOR  = H * Ns/2 + the number of k in 1 .. Ns/2-1 with c_k * Y - s_k * X >= 0: two products and a subtraction, each
 *               rounded on its own (no fma contraction).  The count is what is defined, not the search that finds it.
 *   OUTPUT desc [P, Nr, Ns] float32: a bin holds the maximum h of its counted points; an empty bin holds 0.  A maximum does
 *     not depend on order, so desc is bit-defined.  A point reflected through the centre lands exactly Ns/2 sectors on.
 *   OUTPUT ring_key [P, Nr] float32: the ring's mean, s = 0.0; for j ascending: s += (double)desc[p, r, j]; then
 *     ring_key[p, r] = (float)(s / (double)Ns).  It does not change when the columns are rolled, up to the sum's rounding.
 *   Every element of both outputs is written; a cloud's image does not depend on P or on the other clouds.
 *
 * THE DISTANCE.  qry [Q, Nr, Ns] and map [R, Nr, Ns] float32 images, contiguous.  map_count: NULL, or a device pointer to
 *   one int32: the live map is rows 0 .. r-1 with r = clamp(*map_count, 0, R) (NULL: R); the host never learns r.
 *   cand [Q, C] int32: the map ids to compare with each query (the id output of the top-k search, -1 past the map's end).
 *   All arithmetic is float64.  For an image D and a column j, w_j = the sum over the rings of D[i, j]^2; the column is EMPTY
 *   iff w_j == 0.  For a shift n in 0 .. Ns-1 take the j for which query column j and candidate column (j + n) % Ns are both
 *   non-empty, m_n of them:
 *     d_n = 1 - (1 / m_n) * sum over those j of dot(q_j, c_(j+n)) / sqrt(wq_j * wc_(j+n));      m_n == 0: d_n = 1.0 exactly
 *   dist = the minimum of d_n and shift = the smallest n that attains it.  If the map cloud is the query cloud turned by
 *   Rz(theta), shift = theta / (2 pi / Ns): place ~ Rz(2 pi shift / Ns) query.  The order of the sums inside a shift, and
 *   whether a column is divided by its norm before or after the dot product, are FREE: dist is defined to rounding (a few
 *   1e-16 per term, at most Ns unit-size terms), not to the bit; two images of zeros give exactly (1.0, 0).
 *   A candidate id below 0, or at or above r, gives dist = +inf and shift = -1, and nothing of the map is read for it.
 *   OUTPUTS dist [Q, C] float64, shift [Q, C] int32, and order [Q, C] int32: the slots 0 .. C-1 of query q sorted ascending
 *   by (the dist this call wrote, the id in cand, the slot) -- a permutation.  Every element is written.  A query's row does
 *   not depend on Q, on the other queries or on the run.
 *
 * BOTH: caller's stream, caller-owned outputs, no allocation, no synchronisation, no scratch memory of any kind;
 *   graph-capturable (the image: three launches, one after the other, the first clears desc; the distance: one launch).
 * STATUS, before anything is enqueued.  DH3D_ERR_INVALID_ARGUMENT: a NULL pointer (count, center and map_count excepted),
 *   xyz_stride < 3, P, N, Q, R or C <= 0, C > 64, Nr outside 4 .. 32 or not a multiple of 4, Ns outside 8 .. 128 or not a
 *   multiple of 4.  DH3D_ERR_UNSUPPORTED: N > 2^20, P > 65535, Q > 2^20, R > 2^24.
 * NaN and infinite image values are outside the distance's contract (in a cloud they are simply not counted). */
int dh3d_scan_context(const float *xyz, long long xyz_stride, const int32_t *count, const float *center,
                      const double *sector_dir, const double *ring_edge2, int P, int N, int Nr, int Ns, float z_offset,
                      float *desc, float *ring_key, void *stream);
int dh3d_scan_context_distance(const float *qry, const float *map, const int32_t *map_count, const int32_t *cand, int Q, int R,
                               int C, int Nr, int Ns, double *dist, int32_t *shift, int32_t *order, void *stream);

/* Dense generalized (plane-to-plane) ICP refinement (csrc/icp.hip) -- Generalized-ICP, Segal, Haehnel & Thrun, RSS 2009:
 * dh3d_icp_refine with a third fit, which models both surfaces.  The inputs, the ASSOCIATION A, the LOOP (pose = Rt0;
 * `iterations` times { nn = A(pose); pose = F_gicp(nn, pose) }; then nn = A(pose) once more), the paths, the plan, the limits,
 * the validity rule and the independence guarantees are dh3d_icp_refine's, word for word.  In addition:
 * INPUTS: the normal of anchor point i of pair p at anchor_normals + (p*Na + i) * normals_stride and the normal of positive
 *   point j at positive_normals + (p*Nb + j) * positive_normals_stride (3 floats each, strides in elements, >= 3), as
 *   dh3d_estimate_normals writes them.  Their sign and their length do not matter.  A zero normal makes its point isotropic
 *   and does NOT take it out of the fit.  epsilon, 0 < epsilon <= 1: the covariance along a normal relative to 1 across it;
 *   e1 = 1.0 - epsilon, rounded once.
 * FIT F_gicp(nn, pose = [R | t]), float64 on the exact float32 values, every operation rounded on its own.  Symmetric 3 x 3
 *   matrices keep the six entries uv = 00 01 02 11 12 22.  The pairs are the j < nb in ascending order with i = nn[j] >= 0;
 *   n_g of them (= num_corr of that association).  n_g < 3: the pose stays as it was.  m_j = y'_j of the association under
 *   the pose; c = (sum of m_j) / n_g.  Per pair:
 *   cov(v) for a 3-vector v: s = (v_0*v_0 + v_1*v_1) + v_2*v_2; f = e1 / s when s > 0, else 0; a_u = f * v_u;
 *     cov(v)_uv = I_uv - a_u * v_v (I_uv = 1.0 for u = v, else 0.0).  v is NON-ZERO iff s > 0.
 *   C_A = cov(n), n = the normal of anchor i.  C_B = cov(u), u_r = (R_r0*k_0 + R_r1*k_1) + R_r2*k_2 for k = the normal of
 *     positive j.  W_uv = C_A_uv + C_B_uv.
 *   cof_00 = W_11*W_22 - W_12*W_12; cof_01 = W_02*W_12 - W_01*W_22; cof_02 = W_01*W_12 - W_02*W_11;
 *     cof_11 = W_00*W_22 - W_02*W_02; cof_12 = W_01*W_02 - W_00*W_12; cof_22 = W_00*W_11 - W_01*W_01;
 *     det = (W_00*cof_00 + W_01*cof_01) + W_02*cof_02 (>= 8 epsilon^3 in exact arithmetic); M_uv = cof_uv / det, M_vu = M_uv.
 *   q = m_j - c and d = (double)x_i - m_j per axis.  The linearisation is F_plane's: a step s = (w, v) moves m_j by w x q + v,
 *     the columns of J being j_0 = (0, -q_2, q_1), j_1 = (q_2, 0, -q_0), j_2 = (-q_1, q_0, 0), j_3 = e_0, j_4 = e_1, j_5 = e_2.
 *   b_v = M j_v, written out per row r: b_0r = M_r2*q_1 - M_r1*q_2; b_1r = M_r0*q_2 - M_r2*q_0; b_2r = M_r1*q_0 - M_r0*q_1;
 *     b_3r = M_r0; b_4r = M_r1; b_5r = M_r2.
 *   h_uv = j_u . b_v for u <= v: u = 0: q_1*b_v2 - q_2*b_v1; u = 1: q_2*b_v0 - q_0*b_v2; u = 2: q_0*b_v1 - q_1*b_v0;
 *     u >= 3: b_v,u-3.  e_u = (b_u0*d_0 + b_u1*d_1) + b_u2*d_2.
 *   H_uv = sum of h_uv (u <= v, 21 sums), g_u = sum of e_u (6 sums).  Every sum (n_g's and c's three included): lane j % 256
 *   over its j in ascending order from 0; then within each 64-lane wave l_i = l_i + l_(i xor 32), then xor 16, 8, 4, 2, 1;
 *   then ((wave 0 + wave 1) + wave 2) + wave 3.
 *   H s = g by F_plane's Cholesky with its pivot refusal (not finite or <= 1e-12 * max_u H_uu) and its non-finite-s refusal;
 *   dR from w = s[0:3] and the new pose from dR, c and s[3:6] exactly as F_plane composes them.
 * OUTPUTS: Rt, nn, num_corr, fitness, rmse (point-to-point: the three methods compare) and valid as dh3d_icp_refine gives
 *   them; num_planar [P] int32 = the pairs of the last association with n and u both non-zero; rmse_gicp [P] float64 =
 *   sqrt(sum of z / num_corr) under the returned pose with y_r = (M_r0*d_0 + M_r1*d_1) + M_r2*d_2 and z = (d_0*y_0 + d_1*y_1)
 *   + d_2*y_2 (the sums in the fit's order), NaN when num_corr = 0.  A pair that is not valid comes back as from
 *   dh3d_icp_refine, with num_planar 0 and rmse_gicp NaN.  Every element is written.  Rt may be Rt0.
 * dh3d_icp_refine_gicp_ws_bytes (host only): the workspace, as dh3d_icp_refine_ws_bytes; the plan is dh3d_icp_plan.
 * SIDE EFFECTS: caller's stream, one launch after the other (no parallel branches), no host sync, no allocation, no
 *   floating-point atomics; graph-capturable.
 * STATUS: dh3d_icp_refine's, with NULL anchor_normals / positive_normals / num_planar / rmse_gicp, a normals stride below 3
 *   or an epsilon not in (0, 1] (NaN included) among the DH3D_ERR_INVALID_ARGUMENT cases.  NaN and infinite normals are
 *   outside the contract. */
size_t dh3d_icp_refine_gicp_ws_bytes(int P, int Na, int Nb);
int dh3d_icp_refine_gicp(const float *anchor, long long anchor_stride, const int32_t *anchor_count, const float *anchor_normals,
                         long long normals_stride, const float *positive_normals, long long positive_normals_stride,
                         const float *positive, long long positive_stride, const int32_t *positive_count, const double *Rt0,
                         const int32_t *valid0, int P, int Na, int Nb, double max_dist, int iterations, int path, double epsilon,
                         double *Rt, int32_t *nn, int32_t *num_corr, double *fitness, double *rmse, int32_t *valid,
                         int32_t *num_planar, double *rmse_gicp, void *workspace, size_t workspace_bytes, void *stream);

/* ISS keypoints (csrc/iss.hip) -- Intrinsic Shape Signatures, Zhong 2009, the model-free detector that Open3D offers as
 * compute_iss_keypoints: a point is salient where the scatter of ALL points within a radius has three well separated
 * eigenvalues, and a keypoint where no point within a second radius is more salient.  The rule follows Open3D 0.1x as
 * remembered, not as read from a source on this tree; what rests on memory alone is marked INFERRED:
 *   INFERRED  both radius tests are strict (d2 < r * r) and the point itself is a member of its own neighbourhoods;
 *   INFERRED  the covariance is (sum e e^T) / m - mean mean^T over the members, the point itself included;
 *   INFERRED  a point is salient iff l2 / l1 < gamma_21 and l3 / l2 < gamma_32 (here as products), its saliency being l3;
 *   INFERRED  both neighbourhoods need at least min_neighbors members.
 *   The project's own: ties of the suppression go to the lowest index (Open3D keeps both of two equal maxima, which gives
 *   twin keypoints on clouds with exact duplicates), and at most M keypoints come back, the most salient first.
 * INPUTS: point i of cloud p at xyz + (p*N + i) * stride (3 floats; the stride in elements, >= 3), finite below n =
 *   clamp(count[p], 0, N); a NULL count means N.  radii [P, 2] float32 on the DEVICE: r_s (salient radius) and r_n (non-max
 *   radius) of every cloud.  gamma_21, gamma_32 in (0, 1]; min_neighbors >= 1; 1 <= M <= 4096.
 * 1 MEMBERSHIP, float32, every operation rounded on its own (no fused multiply-add): d = x_j - x_i per axis, d2 = (dx*dx +
 *   dy*dy) + dz*dz; j is in S_i iff j < n and d2 < r_s * r_s (the product in float32), in T_i iff j < n and d2 < r_n * r_n.
 *   i is a member of both (d2 = 0).  A radius that is <= 0 or NaN has no members.  num_nbr[p, i] = (|S_i|, |T_i|).
 * 2 MOMENTS, float64: for j in S_i, e = (double)x_j - (double)x_i per axis (NOT the float32 d of step 1); S1 = sum of e,
 *   S2 = sum of e e^T, m = |S_i|; C = S2 / m - (S1 / m)(S1 / m)^T.  l1 >= l2 >= l3: the eigenvalues of C by the cyclic
 *   Jacobi of dh3d_estimate_normals (csrc/rigid_fit.h), sorted.  The order of the sums is not part of the rule: the
 *   eigenvalues carry an error of a few m * 2^-53 * r_s^2.
 * 3 SALIENCY, float32: s_i = (float)l3 if m >= min_neighbors and l2 < gamma_21 * l1 and l3 < gamma_32 * l2 and l3 > 0 (the
 *   products in float64), else +0.  Rows i >= n: 0.
 * 4 KEYPOINT: i < n is one iff s_i > 0 and |T_i| >= min_neighbors and no j in T_i, j != i, has s_j > s_i or (s_j == s_i and
 *   j < i).  A saliency that is <= 0 or NaN is never a candidate and never suppresses.
 * 5 OUTPUT: the keypoints by (s descending, index ascending), the first min(M, their number) of them: ids [P, M] int32, -1
 *   behind them; kp_count [P] = the number written.
 * saliency_in [P, N] float32 or NULL.  Given: steps 2 and 3 are skipped, s_i = saliency_in[p, i] for i < n (0 behind), the
 *   counts of step 1 are computed all the same, and lam, if asked for, is written as 0.
 * OUTPUTS: saliency [P, N] float32; num_nbr [P, N, 2] int32 (0 for rows i >= n); lam [P, N, 3] float64 or NULL: l1 l2 l3 of
 *   every row i < n with m >= 1, else 0; ids and kp_count.  Every element of every output is written, for n = 0 too.  A
 *   cloud's result does not depend on the batch, on the workspace's content or on the run.
 * dh3d_iss_keypoints_ws_bytes (host only; the shape alone): bytes of the caller-owned workspace (16-byte aligned, no clearing
 *   needed); 0 for a shape the call refuses.
 * SIDE EFFECTS: caller's stream, one launch after the other (pack, dh3d_spatial_sort_cells, moments, suppression, select; no
 *   parallel branches), no host sync, no allocation, no floating-point atomics; graph-capturable.
 * STATUS: NULL pointers (count, saliency_in and lam excepted), a stride below 3, P / N / M <= 0, min_neighbors < 1, a gamma
 *   not in (0, 1] (NaN included), a misaligned or too small workspace: DH3D_ERR_INVALID_ARGUMENT.  N > 16384 (the cell table),
 *   P > 65535, M > 4096: DH3D_ERR_UNSUPPORTED.  Both before any launch.  Non-finite coordinates below n are outside the
 *   contract. */
size_t dh3d_iss_keypoints_ws_bytes(int P, int N, int M);
int dh3d_iss_keypoints(const float *xyz, long long stride, const int32_t *count, const float *radii, const float *saliency_in,
                       int P, int N, double gamma_21, double gamma_32, int min_neighbors, int M, float *saliency,
                       int32_t *num_nbr, double *lam, int32_t *ids, int32_t *kp_count, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DH3D_HIP_H_ */
