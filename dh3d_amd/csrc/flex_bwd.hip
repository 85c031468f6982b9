// flex_conv backward in its FACTORISED form (gfx950), and the reference-layout (channels-first) fast paths built on
// the fused point-major kernels.
//
// Forward:  out = S @ Wcat,  S = [S0|Sx|Sy|Sz],  S0[n,i] = sum_k f[nk,i],  Sd[n,i] = sum_k (p[nk,d]-p[c(n),d]) f[nk,i],
//           Wcat = [bias; theta_x; theta_y; theta_z]  ([4*Din, Dout]).
// Backward: dWcat = S^T dOut            -> rows [0,Din) = grad_bias, rows [Din,4Din) = grad_theta   (MFMA, gemm.hip)
//           dS    = dOut Wcat^T         ([R, 4*Din], MFMA)
//           df[nk,i] += dS0[n,i] + sum_d (p[nk,d]-p[c(n),d]) dSd[n,i]                               (f32 atomics)
// -- 2*R*4Din*Dout*2 flop on the matrix pipe instead of the reference formulation's three 9*K*Din*Dout-flop VALU
// kernels (flex_conv_kernel_gpu.cu.cc:168-385), whose feature gradient is the same atomics scatter.
// Centre c(n): the point itself (GPU forward rule, :77-79) or the rank-0 neighbour (both reference backward paths,
// :196-202,314); identical under exact kNN.
#include "flex_common.h"

#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

namespace {

// S [R, 4*Din] (component-major columns).  One lane = (point, 4 channels).
__global__ __launch_bounds__(256) void flex_S_kernel(const float *__restrict__ feat, const float *__restrict__ xyz,
                                                    const int32_t *__restrict__ nbr, long long R, int N, int K,
                                                    int Din, int rank0, float *__restrict__ S) {
  const int lpr = Din / 4;
  const long long total = R * lpr;
  for (long long e = (long long)dh3d_xcd_remap(blockIdx.x, gridDim.x) * 256 + threadIdx.x; e < total;
       e += (long long)gridDim.x * 256) {
    const long long n = e / lpr;
    const int r4 = (int)(e - n * lpr) * 4;
    const long long cl0 = (n / N) * N;
    const int32_t *nb = nbr + n * K;
    const long long c = rank0 ? cl0 + nb[0] : n;
    const float px = xyz[c * 3], py = xyz[c * 3 + 1], pz = xyz[c * 3 + 2];
    float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), sx = s0, sy = s0, sz = s0;
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
      const long long g = cl0 + nb[k];
      const float4 f = *reinterpret_cast<const float4 *>(feat + g * Din + r4);
      const float dx = xyz[g * 3] - px, dy = xyz[g * 3 + 1] - py, dz = xyz[g * 3 + 2] - pz;
      s0.x += f.x; s0.y += f.y; s0.z += f.z; s0.w += f.w;
      sx.x = fmaf(dx, f.x, sx.x); sx.y = fmaf(dx, f.y, sx.y); sx.z = fmaf(dx, f.z, sx.z); sx.w = fmaf(dx, f.w, sx.w);
      sy.x = fmaf(dy, f.x, sy.x); sy.y = fmaf(dy, f.y, sy.y); sy.z = fmaf(dy, f.z, sy.z); sy.w = fmaf(dy, f.w, sy.w);
      sz.x = fmaf(dz, f.x, sz.x); sz.y = fmaf(dz, f.y, sz.y); sz.z = fmaf(dz, f.z, sz.z); sz.w = fmaf(dz, f.w, sz.w);
    }
    float *row = S + n * 4 * Din + r4;
    *reinterpret_cast<float4 *>(row) = s0;
    *reinterpret_cast<float4 *>(row + Din) = sx;
    *reinterpret_cast<float4 *>(row + 2 * Din) = sy;
    *reinterpret_cast<float4 *>(row + 3 * Din) = sz;
  }
}

// df[nk, :] += dS0[n, :] + dx dSx[n, :] + dy dSy[n, :] + dz dSz[n, :]
__global__ __launch_bounds__(256) void flex_scatter_kernel(const float *__restrict__ dS, const float *__restrict__ xyz,
                                                          const int32_t *__restrict__ nbr, long long R, int N, int K,
                                                          int Din, int rank0, float *__restrict__ dfeat) {
  const int lpr = Din / 4;
  const long long total = R * lpr;
  for (long long e = (long long)dh3d_xcd_remap(blockIdx.x, gridDim.x) * 256 + threadIdx.x; e < total;
       e += (long long)gridDim.x * 256) {
    const long long n = e / lpr;
    const int r4 = (int)(e - n * lpr) * 4;
    const long long cl0 = (n / N) * N;
    const int32_t *nb = nbr + n * K;
    const long long c = rank0 ? cl0 + nb[0] : n;
    const float px = xyz[c * 3], py = xyz[c * 3 + 1], pz = xyz[c * 3 + 2];
    const float *row = dS + n * 4 * Din + r4;
    const float4 d0 = *reinterpret_cast<const float4 *>(row), d1 = *reinterpret_cast<const float4 *>(row + Din),
                 d2 = *reinterpret_cast<const float4 *>(row + 2 * Din), d3 = *reinterpret_cast<const float4 *>(row + 3 * Din);
    for (int k = 0; k < K; ++k) {
      const long long g = cl0 + nb[k];
      const float dx = xyz[g * 3] - px, dy = xyz[g * 3 + 1] - py, dz = xyz[g * 3 + 2] - pz;
      float *dst = dfeat + g * Din + r4;
      unsafeAtomicAdd(dst, fmaf(dz, d3.x, fmaf(dy, d2.x, fmaf(dx, d1.x, d0.x))));
      unsafeAtomicAdd(dst + 1, fmaf(dz, d3.y, fmaf(dy, d2.y, fmaf(dx, d1.y, d0.y))));
      unsafeAtomicAdd(dst + 2, fmaf(dz, d3.z, fmaf(dy, d2.z, fmaf(dx, d1.z, d0.z))));
      unsafeAtomicAdd(dst + 3, fmaf(dz, d3.w, fmaf(dy, d2.w, fmaf(dx, d1.w, d0.w))));
    }
  }
}

// Every layout below: R = B * N point-major rows, each segment rounded up to 256 bytes.
struct PmBwdWs {
  float *S, *dS, *WT;
  PmBwdWs(Carve &c, size_t R, int Din, int Dout) {
    S = c.take<float>(R * 4 * Din, 256);
    dS = c.take<float>(R * 4 * Din, 256);
    WT = c.take<float>((size_t)Dout * 4 * Din, 256);  // Wcat^T [Dout, 4*Din]
  }
};

struct ConvFwdWs {
  PointMajor in{};
  void *wp;
  float *out, *S = nullptr;
  ConvFwdWs(Carve &c, size_t R, int K, int Din, int Dout, int kind) {
    in.f = c.take<float>(R * Din, 256);
    in.nbr = c.take<int32_t>(R * K, 256);
    in.xyz = c.take<float>(R * 3, 256);
    // the packed weight, 6 planes of [Din, Dout]; kind 2: Wcat = [bias; theta], 4 planes, and S [R, 4*Din]
    wp = c.take<float>((size_t)(kind == 2 ? 4 : 6) * Din * Dout, 256);
    out = c.take<float>(R * Dout, 256);
    if (kind == 2) S = c.take<float>(R * 4 * Din, 256);
  }
};

struct ConvBwdWs {
  PointMajor in{};
  float *df;
  // The nested call's workspace: dh3d_flex_conv_pm_bwd carves these bytes itself (PmBwdWs), so its own size query is
  // the one source of their extent (0 for a shape it refuses)
  char *pm;
  size_t pm_bytes;
  ConvBwdWs(Carve &c, int B, int N, int K, int Din, int Dout)
      : pm_bytes(dh3d_flex_conv_pm_bwd_workspace_bytes(B, N, Din, Dout)) {
    const size_t R = (size_t)B * N;
    in.f = c.take<float>(R * Din, 256);
    df = c.take<float>(R * Din, 256);
    in.nbr = c.take<int32_t>(R * K, 256);
    in.xyz = c.take<float>(R * 3, 256);
    in.g = c.take<float>(R * Dout, 256);
    pm = c.take<char>(pm_bytes);
  }
};

struct PoolFwdWs {
  PointMajor in{};
  float *out;
  int32_t *argmax;
  PoolFwdWs(Carve &c, size_t R, int K, int D) {
    in.f = c.take<float>(R * D, 256);
    out = c.take<float>(R * D, 256);
    argmax = c.take<int32_t>(R * D, 256);
    in.nbr = c.take<int32_t>(R * K, 256);
  }
};

// Reference-layout fast paths: user_ops tensors are channels-first ([B,C,N] features, [B,K,N] neighbourhoods,
// [B,3,N] positions).  A neighbour row in that layout is C scattered 4-byte reads (N*4 bytes apart), so the gather
// kernels want point-major rows: the inputs are transposed through LDS tiles into the caller's workspace (HBM-bound,
// ~2*size/5 TB/s each), the fused point-major kernel runs, and the result is transposed back.
// 1 = fused kernel (x6: the persistent bf16x6 one), 2 = any other channel counts that are multiples of four: the
// factorisation in two launches -- S = [S0|Sx|Sy|Sz] materialised by flex_S_kernel, then out = S @ [bias; theta] on the
// GEMM kernels (gemm.hip) -- instead of the reference formulation's 9*K*Din*Dout flop per point on the vector unit
// (flex_generic.hip: 3.4 ms at 64 -> 64, 8 x 8192, where this form takes ~0.1 ms); 0 = not served here, which
// includes a shape whose extents leave the kernels' 32-bit indices (the two guards below).
int fast_fwd_kind(int B, int N, int K, int Dp, int Din, int Dout, bool *x6) {
  *x6 = false;
  if (B <= 0 || N <= 1 || K <= 0 || Dp != 3) return 0;
  const size_t R = (size_t)B * N;
  *x6 = K == 8 && Dout == 64 && (Din == 32 || Din == 64);
  if (*x6) return R * Din * 4 < (1ull << 32) ? 1 : 0;
  static const int ok[][2] = {{32, 64}, {32, 128}, {64, 64}, {64, 128}, {64, 256}, {128, 128}, {128, 256}};
  for (auto &p : ok)
    if (p[0] == Din && p[1] == Dout) return 1;
  return (Din % 4 == 0 && Dout % 4 == 0 && R * 4 * Din < (1ull << 31)) ? 2 : 0;
}

}  // namespace

int dh3d_internal_flex_S(const float *feat, const float *xyz, const int32_t *nbr, long long R, int N, int K, int D,
                         int rank0, float *S, hipStream_t s) {
  hipLaunchKernelGGL(flex_S_kernel, dim3(flat_grid256(R * (D / 4), 8192)), dim3(256), 0, s, feat, xyz, nbr, R, N, K, D,
                     rank0, S);
  return dh3d_launch_status();
}

DH3D_API size_t dh3d_flex_conv_pm_bwd_workspace_bytes(int B, int N, int Din, int Dout) {
  if (B <= 0 || N <= 0 || Din <= 0 || Dout <= 0 || Din % 4 || Dout % 4) return 0;
  return carve_bytes<PmBwdWs>((size_t)B * N, Din, Dout);
}

DH3D_API int dh3d_flex_conv_pm_bwd(const float *features, const float *xyz, const int32_t *nbr, const float *theta,
                                   const float *bias, const float *grad_out, int B, int N, int K, int Din, int Dout,
                                   int center_rank0, void *workspace, size_t workspace_bytes, float *grad_features,
                                   float *grad_theta, float *grad_bias, void *stream) {
  DH3D_REQUIRE(features && xyz && nbr && theta && bias && grad_out && workspace && grad_theta && grad_bias);
  DH3D_REQUIRE(B > 0 && N > 0 && K > 0 && Din > 0 && Dout > 0);
  DH3D_SUPPORTED(Din % 4 == 0 && Dout % 4 == 0);
  const long long R = (long long)B * N;
  Carve c(workspace);
  const PmBwdWs w(c, (size_t)R, Din, Dout);
  DH3D_REQUIRE(workspace_bytes >= c.bytes());
  hipStream_t s = (hipStream_t)stream;
  const int KD = 4 * Din;
  int st = dh3d_internal_flex_S(features, xyz, nbr, R, N, K, Din, center_rank0, w.S, s);
  if (st != DH3D_OK) return st;
  // dWcat = S^T dOut: rows [0, Din) -> grad_bias, the rest -> grad_theta ([3, Din, Dout] is rows Din.. of Wcat)
  st = dh3d_internal_gemm(true, w.S, KD, grad_out, Dout, grad_bias, Dout, KD, Dout, (int)R, grad_theta, Din, false, s);
  if (st != DH3D_OK) return st;
  if (!grad_features) return DH3D_OK;
  st = dh3d_internal_transpose32(bias, w.WT, 1, Din, Dout, KD, 0, s);                     // columns [0, Din)
  if (st != DH3D_OK) return st;
  st = dh3d_internal_transpose32(theta, w.WT + Din, 3, Din, Dout, KD, Din, s);            // columns [(1+d)*Din, ...)
  if (st != DH3D_OK) return st;
  st = dh3d_internal_gemm(false, grad_out, Dout, w.WT, KD, w.dS, KD, (int)R, KD, Dout, nullptr, 0, false, s);
  if (st != DH3D_OK) return st;
  if (hipMemsetAsync(grad_features, 0, sizeof(float) * R * Din, s) != hipSuccess) return DH3D_ERR_LAUNCH;
  hipLaunchKernelGGL(flex_scatter_kernel, dim3(flat_grid256(R * (Din / 4), 8192)), dim3(256), 0, s, w.dS, xyz, nbr, R, N,
                     K, Din, center_rank0, grad_features);
  return dh3d_launch_status();
}

DH3D_API size_t dh3d_flex_conv_fwd_workspace_bytes(int B, int N, int K, int Dp, int Din, int Dout) {
  bool x6;
  const int kind = fast_fwd_kind(B, N, K, Dp, Din, Dout, &x6);
  return kind ? carve_bytes<ConvFwdWs>((size_t)B * N, K, Din, Dout, kind) : 0;
}

DH3D_API int dh3d_flex_conv_fwd_plan(int B, int N, int K, int Dp, int Din, int Dout) {
  bool x6;
  const int kind = fast_fwd_kind(B, N, K, Dp, Din, Dout, &x6);
  return kind && x6 ? 3 : kind;
}

DH3D_API int dh3d_flex_conv_fwd_ws(const float *features, const float *theta, const float *bias,
                                   const int32_t *neighborhood, const float *positions, int B, int N, int K, int Dp,
                                   int Din, int Dout, float *output, void *workspace, size_t workspace_bytes,
                                   void *stream) {
  DH3D_REQUIRE(features && theta && bias && neighborhood && positions && output && workspace);
  bool x6;
  const int kind = fast_fwd_kind(B, N, K, Dp, Din, Dout, &x6);
  DH3D_SUPPORTED(kind != 0);
  const size_t R = (size_t)B * N;
  Carve c(workspace);
  const ConvFwdWs w(c, R, K, Din, Dout, kind);
  DH3D_REQUIRE(workspace_bytes >= c.bytes());
  hipStream_t s = (hipStream_t)stream;
  int st = flex_to_point_major(w.in, features, neighborhood, positions, nullptr, B, N, K, Din, Dout, s);
  if (st != DH3D_OK) return st;
  if (kind == 2) {
    float *Wcat = static_cast<float *>(w.wp);
    if ((st = flex_build_wcat(bias, theta, Din, Dout, Wcat, s)) != DH3D_OK) return st;
    // centre = the point itself (the GPU forward's rule, flex_conv_kernel_gpu.cu.cc:77-79)
    if ((st = dh3d_internal_flex_S(w.in.f, w.in.xyz, w.in.nbr, (long long)R, N, K, Din, 0, w.S, s)) != DH3D_OK) return st;
    st = dh3d_internal_gemm(false, w.S, 4 * Din, Wcat, Dout, w.out, Dout, (int)R, Dout, 4 * Din, nullptr, 0, false, s);
  } else if (x6) {
    if ((st = dh3d_pack_flex_weight_x3(theta, bias, Din, Dout, w.wp, stream)) != DH3D_OK) return st;
    st = dh3d_flex_conv_pm_x6_fwd(w.in.f, w.in.xyz, w.in.nbr, w.wp, B, N, K, Din, Dout, nullptr, w.out, stream);
  } else {
    float *wp = static_cast<float *>(w.wp);
    if ((st = dh3d_pack_flex_weight(theta, bias, Din, Dout, wp, stream)) != DH3D_OK) return st;
    st = dh3d_flex_conv_pm_fwd(w.in.f, w.in.xyz, w.in.nbr, wp, B, N, K, Din, Dout, nullptr, w.out, stream);
  }
  if (st != DH3D_OK) return st;
  return dh3d_internal_transpose32(w.out, output, B, N, Dout, 0, 0, s);
}

DH3D_API size_t dh3d_flex_conv_bwd_workspace_bytes(int B, int N, int K, int Dp, int Din, int Dout) {
  if (B <= 0 || N <= 0 || K <= 0 || Dp != 3 || Din % 4 || Dout % 4) return 0;
  return carve_bytes<ConvBwdWs>(B, N, K, Din, Dout);
}

DH3D_API int dh3d_flex_conv_bwd_ws(const float *features, const float *theta, const float *bias,
                                   const int32_t *neighborhood, const float *positions, const float *topdiff, int B,
                                   int N, int K, int Dp, int Din, int Dout, float *grad_features, float *grad_theta,
                                   float *grad_bias, void *workspace, size_t workspace_bytes, void *stream) {
  DH3D_REQUIRE(features && theta && bias && neighborhood && positions && topdiff && grad_features && grad_theta &&
               grad_bias && workspace);
  DH3D_SUPPORTED(dh3d_flex_conv_bwd_workspace_bytes(B, N, K, Dp, Din, Dout) != 0);
  Carve c(workspace);
  const ConvBwdWs w(c, B, N, K, Din, Dout);
  DH3D_REQUIRE(workspace_bytes >= c.bytes());
  hipStream_t s = (hipStream_t)stream;
  int st = flex_to_point_major(w.in, features, neighborhood, positions, topdiff, B, N, K, Din, Dout, s);
  if (st != DH3D_OK) return st;
  // both reference backward paths centre on the rank-0 neighbour (flex_conv_kernel_gpu.cu.cc:196-202,314)
  st = dh3d_flex_conv_pm_bwd(w.in.f, w.in.xyz, w.in.nbr, theta, bias, w.in.g, B, N, K, Din, Dout, 1, w.pm,
                             w.pm_bytes, w.df, grad_theta, grad_bias, stream);
  if (st != DH3D_OK) return st;
  return dh3d_internal_transpose32(w.df, grad_features, B, N, Din, 0, 0, s);
}

DH3D_API size_t dh3d_flex_pool_fwd_workspace_bytes(int B, int N, int K, int D) {
  if (B <= 0 || N <= 0 || K <= 0 || D <= 0 || D % 4) return 0;
  return carve_bytes<PoolFwdWs>((size_t)B * N, K, D);
}

DH3D_API int dh3d_flex_pool_fwd_ws(const float *features, const int32_t *neighborhood, int B, int N, int K, int D,
                                   float *output, int32_t *argmax, void *workspace, size_t workspace_bytes,
                                   void *stream) {
  DH3D_REQUIRE(features && neighborhood && output && argmax && workspace);
  DH3D_SUPPORTED(dh3d_flex_pool_fwd_workspace_bytes(B, N, K, D) != 0);
  Carve c(workspace);
  const PoolFwdWs w(c, (size_t)B * N, K, D);
  DH3D_REQUIRE(workspace_bytes >= c.bytes());
  hipStream_t s = (hipStream_t)stream;
  int st;
  if ((st = flex_to_point_major(w.in, features, neighborhood, nullptr, nullptr, B, N, K, D, D, s)) != DH3D_OK) return st;
  if ((st = dh3d_flex_pool_pm_fwd(w.in.f, w.in.nbr, B, N, K, D, w.out, w.argmax, stream)) != DH3D_OK) return st;
  if ((st = dh3d_internal_transpose32(w.out, output, B, N, D, 0, 0, s)) != DH3D_OK) return st;
  return dh3d_internal_transpose32(w.argmax, argmax, B, N, D, 0, 0, s);
}
