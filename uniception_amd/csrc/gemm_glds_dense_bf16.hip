// Dense direct-to-LDS GEMM kernels, epilogue family GLDS_EPI_BF16 (kernels: gemm_glds_kernel.h, epilogues: gemm_glds_epilogue.h, shared prologue pieces: gemm_glds_tile.h).
#include "gemm_glds_kernel.h"
void glds_launch_dense_bf16(const GldsParams& p, const GemmPlan& plan, hipStream_t st) { glds_launch_family<UC_A_DENSE, GLDS_EPI_BF16>(p, plan, st); }
