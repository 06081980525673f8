// LayerNorm backward kernel and its launcher, shared by layernorm.hip (the plain instantiations) and layernorm_dp.hip
// (the stochastic-depth ones): one translation unit each, so the build parallelises.
#pragma once
#include "common.h"

namespace {

// The row-pipelined backward needs 187 VGPRs (2 waves per SIMD): 512 four-wave blocks are all
// resident at once on 256 CUs, and each wave walks ~25 rows (B/16 bs256: 123 vs 129 us isolated
// at 1024 blocks, +0.3% step; VIT_LN_BWD_BLOCKS overrides).
constexpr int LN_BWD_MAX_BLOCKS = 512;

// PATH: the stochastic-depth variant (vit_layernorm_bwd_drop_path, instantiated in layernorm_dp.hip): the bf16 copy and
// the dx column sums also carry the per-sample multiplier path.scale[mask row / rows per sample], loaded once per row
// with the row's statistics. The plain instantiations ignore `path`.
template <int NV, bool FULL, bool PATH>
__global__ void __launch_bounds__(256) ln_bwd_kernel(const void* __restrict__ dy, long lddy, int dy_f32,
                                                     const float* __restrict__ x, long ldx, const float* __restrict__ mean,
                                                     const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                     const float* __restrict__ dres, long lddres, float* __restrict__ dx,
                                                     long lddx, bf16_t* __restrict__ dxb, long lddxb,
                                                     float* __restrict__ partial, int rows, int D, DropDev drop,
                                                     PathDev path) {
  __shared__ float red[4][NV * 256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float4 pg[NV], pb[NV], ps[NV];
  float4 gm[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    pg[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    pb[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    ps[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    const int c = (k * 64 + lane) * 4;
    gm[k] = FULL || c < D ? *reinterpret_cast<const float4*>(gamma + c) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  // rows are software-pipelined: the next row's loads (dy, x, residual grad, stats) are issued
  // before this row's math and stores, so each wave keeps two rows of HBM reads in flight
  auto load_row = [&](int row, float4* d4, float4* x4, float4* r4, float& mu, float& rs) {
    mu = mean[row];
    rs = rstd[row];
    if constexpr (FULL) {
      // wave-uniform choices outside the chunk loops: each loop is straight-line, so the row's loads
      // issue together (a per-chunk branch made hipcc wait for each chunk's loads in turn)
      if (dy_f32) {
#pragma unroll
        for (int k = 0; k < NV; ++k)
          d4[k] = *reinterpret_cast<const float4*>((const float*)dy + (long)row * lddy + (k * 64 + lane) * 4);
      } else {
        uint2 u[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k)
          u[k] = *reinterpret_cast<const uint2*>((const bf16_t*)dy + (long)row * lddy + (k * 64 + lane) * 4);
#pragma unroll
        for (int k = 0; k < NV; ++k)
          d4[k] = make_float4(bf2f(u[k].x & 0xffff), bf2f(u[k].x >> 16), bf2f(u[k].y & 0xffff), bf2f(u[k].y >> 16));
      }
#pragma unroll
      for (int k = 0; k < NV; ++k) x4[k] = *reinterpret_cast<const float4*>(x + (long)row * ldx + (k * 64 + lane) * 4);
      if (dres) {
#pragma unroll
        for (int k = 0; k < NV; ++k)
          r4[k] = *reinterpret_cast<const float4*>(dres + (long)row * lddres + (k * 64 + lane) * 4);
      } else {
#pragma unroll
        for (int k = 0; k < NV; ++k) r4[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
      return;
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int c = (k * 64 + lane) * 4;
      if (FULL || c < D) {
        if (dy_f32) {
          d4[k] = *reinterpret_cast<const float4*>((const float*)dy + (long)row * lddy + c);
        } else {
          const uint2 u = *reinterpret_cast<const uint2*>((const bf16_t*)dy + (long)row * lddy + c);
          d4[k] = make_float4(bf2f(u.x & 0xffff), bf2f(u.x >> 16), bf2f(u.y & 0xffff), bf2f(u.y >> 16));
        }
        x4[k] = *reinterpret_cast<const float4*>(x + (long)row * ldx + c);
        r4[k] = dres ? *reinterpret_cast<const float4*>(dres + (long)row * lddres + c) : make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        d4[k] = x4[k] = r4[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
  };
  auto load_path = [&](int row) {  // the multiplier of the row's sample (mask row: the dropout descriptor's convention)
    return path.scale[path_sample(path, (uint32_t)(row * drop.row_mul + drop.row0))];
  };
  const int stride = gridDim.x * 4;
  float4 d4[NV], x4[NV], r4[NV];
  float mu = 0.f, rs = 0.f;
  float psc = 1.f;
  int row = blockIdx.x * 4 + wave;
  if (row < rows) {
    load_row(row, d4, x4, r4, mu, rs);
    if constexpr (PATH) psc = load_path(row);
  }
  for (; row < rows; row += stride) {
    float4 dn[NV], xn[NV], rn[NV];
    float mun = 0.f, rsn = 0.f;
    float psn = 1.f;
    if (row + stride < rows) {
      load_row(row + stride, dn, xn, rn, mun, rsn);
      if constexpr (PATH) psn = load_path(row + stride);
    }
    float4 xh[NV], g[NV];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      xh[k] = make_float4((x4[k].x - mu) * rs, (x4[k].y - mu) * rs, (x4[k].z - mu) * rs, (x4[k].w - mu) * rs);
      g[k] = make_float4(d4[k].x * gm[k].x, d4[k].y * gm[k].y, d4[k].z * gm[k].z, d4[k].w * gm[k].w);
      s1 += g[k].x + g[k].y + g[k].z + g[k].w;
      s2 += g[k].x * xh[k].x + g[k].y * xh[k].y + g[k].z * xh[k].z + g[k].w * xh[k].w;
      pg[k].x += d4[k].x * xh[k].x; pg[k].y += d4[k].y * xh[k].y; pg[k].z += d4[k].z * xh[k].z;
      pg[k].w += d4[k].w * xh[k].w;
      pb[k].x += d4[k].x; pb[k].y += d4[k].y; pb[k].z += d4[k].z; pb[k].w += d4[k].w;
    }
    const float m1 = wave_sum(s1) / D, m2 = wave_sum(s2) / D;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int c = (k * 64 + lane) * 4;
      if (FULL || c < D) {
        float4 o;
        o.x = rs * (g[k].x - m1 - xh[k].x * m2) + r4[k].x;
        o.y = rs * (g[k].y - m1 - xh[k].y * m2) + r4[k].y;
        o.z = rs * (g[k].z - m1 - xh[k].z * m2) + r4[k].z;
        o.w = rs * (g[k].w - m1 - xh[k].w * m2) + r4[k].w;
        *reinterpret_cast<float4*>(dx + (long)row * lddx + c) = o;
        if (drop.thr) {  // the copy / column sums feed the dropout-ed branch: gradient x mask
          float m8[8];
          drop_mult8(drop, row, c >> 3, m8);
          const bool hi = c & 4;
          o.x *= hi ? m8[4] : m8[0];
          o.y *= hi ? m8[5] : m8[1];
          o.z *= hi ? m8[6] : m8[2];
          o.w *= hi ? m8[7] : m8[3];
        }
        if constexpr (PATH) {  // ... x the sample's stochastic-depth multiplier
          o.x *= psc; o.y *= psc; o.z *= psc; o.w *= psc;
        }
        ps[k].x += o.x; ps[k].y += o.y; ps[k].z += o.z; ps[k].w += o.w;
        if (dxb) {
          uint2 u;
          u.x = pack2bf(o.x, o.y);
          u.y = pack2bf(o.z, o.w);
          *reinterpret_cast<uint2*>(dxb + (long)row * lddxb + c) = u;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      d4[k] = dn[k];
      x4[k] = xn[k];
      r4[k] = rn[k];
    }
    mu = mun;
    rs = rsn;
    if constexpr (PATH) psc = psn;
  }
  // block partials [dgamma | dbeta | dsum]: sum dy*xhat, sum dy, sum of the written dx (the
  // bias gradient of the linear layer that produced this residual stream)
#pragma unroll
  for (int q = 0; q < 3; ++q) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int c = (k * 64 + lane) * 4;
      *reinterpret_cast<float4*>(&red[wave][c]) = q == 0 ? pg[k] : (q == 1 ? pb[k] : ps[k]);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < D; c += 256)
      partial[(long)blockIdx.x * 3 * D + q * D + c] = red[0][c] + red[1][c] + red[2][c] + red[3][c];
    __syncthreads();
  }
}

inline int nv_for_bwd(int64_t D) { return (int)((D + 255) / 256); }

template <bool PATH>
int ln_bwd_run(const void* dy, int64_t lddy, int32_t dy_f32, const float* x, int64_t ldx,
                                 const float* mean, const float* rstd, const float* gamma, const float* dres,
                                 int64_t lddres, float* dx, int64_t lddx, void* dx_bf16, int64_t lddxb, float* partial,
                                 float* dgamma_dbeta, float* dx_colsum, int32_t accumulate_params, int64_t rows,
                                 int64_t D, const vit_dropout* dx_dropout, const PathDev path, vit_stream_t stream) {
  VIT_CHECK_ARG(dy && x && mean && rstd && gamma && dx && partial, "vit_layernorm_bwd: null pointer");
  const DropDev drop = make_drop(dx_dropout);
  VIT_CHECK_ARG(D > 0 && D % 4 == 0 && D <= 2048, "vit_layernorm_bwd: D=%lld unsupported", (long long)D);
  // every row is read and written in 16-B (f32) / 8-B (bf16) vectors
  VIT_CHECK_ARG(lddy % 4 == 0 && ldx % 4 == 0 && lddx % 4 == 0 && (!dres || lddres % 4 == 0) &&
                    (!dx_bf16 || lddxb % 4 == 0),
                "vit_layernorm_bwd: strides must be multiples of 4");
  if (rows <= 0) return VIT_OK;
  const int64_t nblk = vit_layernorm_bwd_blocks(rows);
  hipStream_t s = (hipStream_t)stream;
  switch (nv_for_bwd(D)) {
#define C(n)                                                                                                        \
  case n:                                                                                                           \
    if (D == n * 256)                                                                                               \
      hipLaunchKernelGGL((ln_bwd_kernel<n, true, PATH>), dim3((unsigned)nblk), dim3(256), 0, s, dy, (long)lddy, (int)dy_f32, \
                         x, (long)ldx, mean, rstd, gamma, dres, (long)lddres, dx, (long)lddx, (bf16_t*)dx_bf16,      \
                         (long)lddxb, partial, (int)rows, (int)D, drop, path);                                      \
    else                                                                                                            \
      hipLaunchKernelGGL((ln_bwd_kernel<n, false, PATH>), dim3((unsigned)nblk), dim3(256), 0, s, dy, (long)lddy,           \
                         (int)dy_f32, x, (long)ldx, mean, rstd, gamma, dres, (long)lddres, dx, (long)lddx,          \
                         (bf16_t*)dx_bf16, (long)lddxb, partial, (int)rows, (int)D, drop, path);                    \
    break;
    C(1) C(2) C(3) C(4) C(5) C(6) C(7) C(8)
#undef C
  }
  int st = vit::check_hip(hipGetLastError(), "vit_layernorm_bwd");
  if (st) return st;
  float* ws = partial + nblk * 3 * D;
  if (!dgamma_dbeta && !dx_colsum) return VIT_OK;
  if (D % 8 == 0)  // one reduction for [dgamma | dbeta | dx colsum]
    return vit_colsum3(partial, 0, nblk, D, 3 * D, ws, dgamma_dbeta, dgamma_dbeta ? dgamma_dbeta + D : nullptr,
                       dx_colsum, accumulate_params, stream);
  if (dgamma_dbeta) st = vit_colsum(partial, 0, nblk, 2 * D, 3 * D, ws, dgamma_dbeta, accumulate_params, stream);
  if (st) return st;
  if (dx_colsum) st = vit_colsum(partial + 2 * D, 0, nblk, D, 3 * D, ws, dx_colsum, accumulate_params, stream);
  return st;
}

}  // namespace
