// fp16-operand instantiation of the dense direct-to-LDS GEMM kernels (the prediction heads' TF32-class mode: 1x1 convolutions,
// ConvTranspose-as-GEMM, linear heads; kernels: gemm_glds_kernel.h, epilogues: gemm_glds_epilogue.h, shared prologue pieces: gemm_glds_tile.h).
#include "gemm_glds_kernel.h"
void glds_launch_dense_all_f16(const GldsParams& p, const GemmPlan& plan, hipStream_t st) { glds_launch_family<UC_A_DENSE, GLDS_EPI_ALL, true>(p, plan, st); }
