// Instantiation unit: every tile config and operand layout of GEMM epilogue 7.
#include "gemm_kernels.h"

template <> hipError_t vitg::launch_layout_x<7>(int cfg, const GemmDev& d, bool ak, bool bk, int batch, int split, hipStream_t s) {
  return launch_layout<7>(cfg, d, ak, bk, batch, split, s);
}

hipError_t vitg::launch_splitk_group(const GemmGroup& g, hipStream_t s) { return launch_pp2_group(g, s); }

hipError_t vitg::launch_group_table(const void* table, int n, int total, bool acc, hipStream_t s) {
  return acc ? launch_pp2_table<vitg::EPI_ACC>(table, n, total, s) : launch_pp2_table<0>(table, n, total, s);
}
