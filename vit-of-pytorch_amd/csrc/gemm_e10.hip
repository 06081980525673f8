// Instantiation unit: GEMM epilogue 4 with the stochastic-depth multiplier (68 = 4 | EPI_PATH), A K-contiguous.
#include "gemm_kernels.h"

template <> hipError_t vitg::launch_kk_x<68>(int cfg, const GemmDev& d, bool bk, int batch, int split, hipStream_t s) {
  // (the out-projection reads the LinearGeneral weight [in][out] as it is: B M/N-contiguous)
  return bk ? launch_cfg<68, true, true>(cfg, d, batch, split, s) : launch_cfg<68, true, false>(cfg, d, batch, split, s);
}
