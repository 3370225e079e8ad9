// Implicit-GEMM 3x3 convolution kernels of the direct-to-LDS family (all epilogues: bf16 store with activation, residual drains; kernels: gemm_glds_kernel.h, epilogues: gemm_glds_epilogue.h, shared prologue pieces: gemm_glds_tile.h).
#include "gemm_glds_kernel.h"
void glds_launch_conv(const GldsParams& p, const GemmPlan& plan, hipStream_t st) {
    if (plan.epi == GLDS_EPI_RES16) glds_launch_family<UC_A_CONV3X3, GLDS_EPI_RES16>(p, plan, st);
    else glds_launch_family<UC_A_CONV3X3, GLDS_EPI_ALL>(p, plan, st);
}
