// LayerNorm forward/backward (nn.LayerNorm(D), eps 1e-5, reference src/model.py:108,114,146).
// One wavefront per row, the row held in registers as float4 chunks (HBM-bound kernels: each
// row is read once and written once; 16-B loads per lane). Statistics in fp32.
#include "layernorm_bwd.h"

#include <cstdlib>

namespace {

// NV = float4 chunks per lane (D <= NV * 256).
// FULL: D == NV * 256, every chunk in range: no per-chunk guards, so a row's loads (and the gamma /
// beta loads) issue back to back instead of one guarded load and its wait at a time
template <int NV, bool FULL>
__global__ void __launch_bounds__(256) ln_fwd_kernel(const float* __restrict__ x, long ldx, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, void* __restrict__ y, long ldy,
                                                     int y_f32, float* __restrict__ mean, float* __restrict__ rstd,
                                                     int rows, int D, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + (long)row * ldx;
  float4 v[NV], gmv[NV], btv[NV];
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k) {  // gamma / beta requested with the row, not after its reductions
    const int c = (k * 64 + lane) * 4;
    if (FULL || c < D) {
      gmv[k] = *reinterpret_cast<const float4*>(gamma + c);
      btv[k] = *reinterpret_cast<const float4*>(beta + c);
    }
  }
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int c = (k * 64 + lane) * 4;
    if (FULL || c < D) {
      v[k] = *reinterpret_cast<const float4*>(xr + c);
      s += v[k].x + v[k].y + v[k].z + v[k].w;
    } else {
      v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  const float mu = wave_sum(s) / D;
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int c = (k * 64 + lane) * 4;
    if (FULL || c < D) {
      const float a = v[k].x - mu, b = v[k].y - mu, cc = v[k].z - mu, d = v[k].w - mu;
      ss += a * a + b * b + cc * cc + d * d;
    }
  }
  const float var = wave_sum(ss) / D;
  const float rs = rsqrtf(var + eps);
  if (lane == 0) {
    mean[row] = mu;
    rstd[row] = rs;
  }
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int c = (k * 64 + lane) * 4;
    if (FULL || c < D) {
      const float4 gm = gmv[k], bt = btv[k];
      const float o0 = (v[k].x - mu) * rs * gm.x + bt.x;
      const float o1 = (v[k].y - mu) * rs * gm.y + bt.y;
      const float o2 = (v[k].z - mu) * rs * gm.z + bt.z;
      const float o3 = (v[k].w - mu) * rs * gm.w + bt.w;
      if (y_f32) {
        *reinterpret_cast<float4*>((float*)y + (long)row * ldy + c) = make_float4(o0, o1, o2, o3);
      } else {
        uint2 u;
        u.x = pack2bf(o0, o1);
        u.y = pack2bf(o2, o3);
        *reinterpret_cast<uint2*>((bf16_t*)y + (long)row * ldy + c) = u;
      }
    }
  }
}

int nv_for(int64_t D) { return (int)((D + 255) / 256); }

}  // namespace

extern "C" int vit_layernorm_fwd(const float* x, int64_t ldx, const float* gamma, const float* beta, void* y,
                                 int64_t ldy, int32_t y_f32, float* mean, float* rstd, int64_t rows, int64_t D,
                                 float eps, vit_stream_t stream) {
  VIT_CHECK_ARG(x && gamma && beta && y && mean && rstd, "vit_layernorm_fwd: null pointer");
  VIT_CHECK_ARG(D > 0 && D % 4 == 0 && D <= 2048, "vit_layernorm_fwd: D=%lld unsupported", (long long)D);
  VIT_CHECK_ARG(ldx % 4 == 0 && ldy % 4 == 0, "vit_layernorm_fwd: strides must be multiples of 4");
  if (rows <= 0) return VIT_OK;
  dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  hipStream_t s = (hipStream_t)stream;
  switch (nv_for(D)) {
#define C(n)                                                                                                        \
  case n:                                                                                                           \
    if (D == n * 256)                                                                                               \
      hipLaunchKernelGGL((ln_fwd_kernel<n, true>), grid, block, 0, s, x, (long)ldx, gamma, beta, y, (long)ldy,       \
                         (int)y_f32, mean, rstd, (int)rows, (int)D, eps);                                           \
    else                                                                                                            \
      hipLaunchKernelGGL((ln_fwd_kernel<n, false>), grid, block, 0, s, x, (long)ldx, gamma, beta, y, (long)ldy,      \
                         (int)y_f32, mean, rstd, (int)rows, (int)D, eps);                                           \
    break;
    C(1) C(2) C(3) C(4) C(5) C(6) C(7) C(8)
#undef C
  }
  VIT_LAUNCH_CHECK("vit_layernorm_fwd");
}

static int64_t ln_bwd_blocks(int64_t rows) {
  static const int64_t cap = [] {
    const int k = vit::knob("VIT_LN_BWD_BLOCKS", 0);
    return k > 0 ? (int64_t)k : (int64_t)LN_BWD_MAX_BLOCKS;
  }();
  int64_t b = (rows + 3) / 4;
  if (b > cap) b = cap;
  return b < 1 ? 1 : b;
}

// rows of block partials the backward writes (the rows a deferred vit_colsum3 of them reduces)
extern "C" int64_t vit_layernorm_bwd_blocks(int64_t rows) { return ln_bwd_blocks(rows); }

// rows of 3*D floats the `partial` workspace must hold (block partials + their column reduction)
extern "C" int64_t vit_layernorm_bwd_partial_rows(int64_t rows) {
  const int64_t nb = ln_bwd_blocks(rows);
  return nb + vit_colsum_partial_rows(nb);
}

extern "C" int vit_layernorm_bwd(const void* dy, int64_t lddy, int32_t dy_f32, const float* x, int64_t ldx,
                                 const float* mean, const float* rstd, const float* gamma, const float* dres,
                                 int64_t lddres, float* dx, int64_t lddx, void* dx_bf16, int64_t lddxb, float* partial,
                                 float* dgamma_dbeta, float* dx_colsum, int32_t accumulate_params, int64_t rows,
                                 int64_t D, const vit_dropout* dx_dropout, vit_stream_t stream) {
  return ln_bwd_run<false>(dy, lddy, dy_f32, x, ldx, mean, rstd, gamma, dres, lddres, dx, lddx, dx_bf16, lddxb, partial,
                           dgamma_dbeta, dx_colsum, accumulate_params, rows, D, dx_dropout, PathDev{nullptr, 0u, 0u, 1},
                           stream);
}
