// LayerNorm backward with stochastic depth: the PATH instantiations of ln_bwd_kernel (layernorm_bwd.h).
#include "layernorm_bwd.h"

extern "C" int vit_layernorm_bwd_drop_path(const void* dy, int64_t lddy, int32_t dy_f32, const float* x, int64_t ldx,
                                           const float* mean, const float* rstd, const float* gamma, const float* dres,
                                           int64_t lddres, float* dx, int64_t lddx, void* dx_bf16, int64_t lddxb,
                                           float* partial, float* dgamma_dbeta, float* dx_colsum,
                                           int32_t accumulate_params, int64_t rows, int64_t D,
                                           const vit_dropout* dx_dropout, const vit_drop_path* dx_path,
                                           vit_stream_t stream) {
  if (!dx_path)
    return vit_layernorm_bwd(dy, lddy, dy_f32, x, ldx, mean, rstd, gamma, dres, lddres, dx, lddx, dx_bf16, lddxb, partial,
                             dgamma_dbeta, dx_colsum, accumulate_params, rows, D, dx_dropout, stream);
  VIT_CHECK_ARG(dx_path->scale && dx_path->rows_per_sample >= 1 && dx_path->rows_per_sample < (1L << 31),
                "vit_layernorm_bwd_drop_path: needs a scale table and rows_per_sample >= 1");
  const int64_t rs = dx_dropout && dx_dropout->row_stride > 1 ? dx_dropout->row_stride : 1;
  VIT_CHECK_ARG(rows * rs < (1L << 31), "vit_layernorm_bwd_drop_path: mask rows beyond 2^31");
  return ln_bwd_run<true>(dy, lddy, dy_f32, x, ldx, mean, rstd, gamma, dres, lddres, dx, lddx, dx_bf16, lddxb, partial,
                          dgamma_dbeta, dx_colsum, accumulate_params, rows, D, dx_dropout, make_path(dx_path), stream);
}
