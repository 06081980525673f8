// Instantiation unit: GEMM epilogue 4 with dropout and the stochastic-depth multiplier (84 = 4 | EPI_DROP | EPI_PATH),
// A K-contiguous.
#include "gemm_kernels.h"

template <> hipError_t vitg::launch_kk_x<84>(int cfg, const GemmDev& d, bool bk, int batch, int split, hipStream_t s) {
  return bk ? launch_cfg<84, true, true>(cfg, d, batch, split, s) : launch_cfg<84, true, false>(cfg, d, batch, split, s);
}
