// fp16-operand instantiation of the implicit-GEMM 3x3 convolution kernels (the prediction heads' TF32-class mode; kernels: gemm_glds_kernel.h, epilogues: gemm_glds_epilogue.h, shared prologue pieces: gemm_glds_tile.h).
#include "gemm_glds_kernel.h"
void glds_launch_conv_f16(const GldsParams& p, const GemmPlan& plan, hipStream_t st) {
    if (plan.epi == GLDS_EPI_RES16) glds_launch_family<UC_A_CONV3X3, GLDS_EPI_RES16, true>(p, plan, st);
    else glds_launch_family<UC_A_CONV3X3, GLDS_EPI_ALL, true>(p, plan, st);
}
