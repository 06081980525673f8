// Stochastic depth (timm.layers.drop_path, scale_by_keep): the per-sample multiplier table of a training forward and
// the standalone DropPath module's row scaling. The fused uses are the EPI_PATH GEMM epilogues (gemm_e10 / gemm_e11)
// and the PATH LayerNorm backward (layernorm_dp.hip).
#include "common.h"

namespace {

// per-site draw parameters (make_drop of dropout site 0x80000000 | s); the key and offset are shared
struct PathSitesDev {
  uint32_t thr[VIT_DROP_PATH_MAX_SITES];  // 0: rate 0, all ones
  float scale[VIT_DROP_PATH_MAX_SITES];   // 1 / (1 - p)
  uint32_t k0, k1, off;
};

// scale[s][b] = dropout multiplier of element (row b, col 0) of dropout site 0x80000000 | s
__global__ void __launch_bounds__(256) drop_path_scales_kernel(const PathSitesDev S, int B, float* __restrict__ out) {
  const int s = blockIdx.y;
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  float m = 1.0f;
  if (S.thr[s]) {
    const DropDev d = {S.thr[s], 0x80000000u | (uint32_t)s, S.k0, S.k1, S.off, S.scale[s], 0, 1};
    m = drop_mult1(d, b, 0);
  }
  out[(long)s * B + b] = m;
}

// out[r][c] = in[r][c] * scale[r / rps]; one thread per 4 columns (VEC) or per element
template <bool VEC>
__global__ void __launch_bounds__(256) row_scale_kernel(const float* __restrict__ in, float* __restrict__ out, long rows,
                                                        int cols, const float* __restrict__ scale, long rps) {
  const int per = VEC ? cols / 4 : cols;
  const long total = rows * per;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long r = i / per;
    const float m = scale[r / rps];
    if constexpr (VEC) {
      float4 v = reinterpret_cast<const float4*>(in)[i];
      v.x *= m; v.y *= m; v.z *= m; v.w *= m;
      reinterpret_cast<float4*>(out)[i] = v;
    } else {
      out[i] = in[i] * m;
    }
  }
}

}  // namespace

extern "C" int vit_drop_path_scales(const float* p_site, int32_t nsites, int64_t B, uint64_t seed, uint64_t offset,
                                    float* scale, vit_stream_t stream) {
  VIT_CHECK_ARG(p_site && scale && nsites >= 1 && nsites <= VIT_DROP_PATH_MAX_SITES && B >= 0 && B < (1L << 31),
                "vit_drop_path_scales: 1..%d sites, a rate per site and a table of nsites x B", VIT_DROP_PATH_MAX_SITES);
  PathSitesDev S{};
  for (int s = 0; s < nsites; ++s) {
    VIT_CHECK_ARG(p_site[s] >= 0.0f && p_site[s] < 1.0f, "vit_drop_path_scales: rate %g of site %d outside [0, 1)",
                  (double)p_site[s], s);
    const vit_dropout d = {p_site[s], 0x80000000u | (uint32_t)s, seed, offset, 1};
    const DropDev dv = make_drop(&d);  // the threshold and scale of nn.Dropout(p_site[s])
    S.thr[s] = dv.thr;
    S.scale[s] = dv.scale;
  }
  // make_drop's key and counter word (it leaves them zero for a site that is off)
  S.k0 = (uint32_t)seed;
  S.k1 = (uint32_t)(seed >> 32) ^ (uint32_t)(offset >> 32);
  S.off = (uint32_t)offset;
  if (B == 0) return VIT_OK;
  hipLaunchKernelGGL(drop_path_scales_kernel, dim3((unsigned)((B + 255) / 256), (unsigned)nsites), dim3(256), 0,
                     (hipStream_t)stream, S, (int)B, scale);
  VIT_LAUNCH_CHECK("vit_drop_path_scales");
}

extern "C" int vit_row_scale_f32(const float* in, float* out, int64_t rows, int64_t cols, const float* scale,
                                 int64_t rows_per_sample, vit_stream_t stream) {
  VIT_CHECK_ARG(in && out && scale && rows >= 0 && cols > 0 && cols < (1L << 31) && rows_per_sample >= 1,
                "vit_row_scale_f32: bad args");
  if (rows == 0) return VIT_OK;
  const bool vec = cols % 4 == 0 && (((uintptr_t)in | (uintptr_t)out) % 16) == 0;
  long blocks = (rows * (vec ? cols / 4 : cols) + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (vec)
    hipLaunchKernelGGL(row_scale_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, in, out,
                       (long)rows, (int)cols, scale, (long)rows_per_sample);
  else
    hipLaunchKernelGGL(row_scale_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, in, out,
                       (long)rows, (int)cols, scale, (long)rows_per_sample);
  VIT_LAUNCH_CHECK("vit_row_scale_f32");
}
