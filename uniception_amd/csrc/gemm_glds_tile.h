#pragma once
// What the direct-to-LDS GEMM kernels (gemm_glds_kernel.h) share around their K-loops.
//
// Only what leaves every kernel's generated code as it was lives here (profiles/gemm_glds_tile_codegen.txt).  hipcc simplifies a
// __forceinline__ function on its own BEFORE it inlines it, so a helper's body reaches the kernel in another canonical form than the
// same statements written in the kernel, and the kernel's instruction order and register assignment follow.  Tried as functions and
// found to change the product-build code of the kernels that would call them, hence still written out in each kernel:
//   * the grouped tile order (blockIdx -> tm, tn): the helper's product grp * GM * tiles_n is re-associated, one s_mul_i32 less, and
//     everything behind it is renumbered — in all five kernels;
//   * the wave's epilogue mode (vt_col0 / rope_cols -> 0 / 1 / 2): the compares come out with the other polarity;
//   * split-K slice and K range, fragment addressing (16- and eight-wave kernels);
//   * the drain (diagnostic sink, stamps, glds_epilogue_dispatch, trace record): glds_epilogue_dispatch is then simplified inside
//     the drain with unknown mode / ksplit before it meets the kernel's constants; identical for the GLDS_EPI_BS / _RES16 families,
//     other code for GLDS_EPI_ALL / _BF16 in every kernel.
// The 16-wave tile template also keeps its own start stagger and kernarg re-read: either helper changes its 128x128 and 32-deep
// instantiations.
#include "gemm_glds_epilogue.h"

// bounce space the epilogues use per wave: every kernel's LDS image must hold it once its K-loop is done (asserted next to each
// kernel's layout constants)
constexpr int GLDS_BOUNCE_BYTES = 8192;

// Experiment (UC_GEMM_STAGGER, off by default): de-phase the CUs.  Every tile of a launch costs the same, so all 256 CUs
// reach their epilogues together and the store / residual traffic hits HBM as one burst while the matrix pipes idle.
// The first round of workgroups (first_round of them: one per CU and co-resident workgroup) starts in 8 phase groups chosen by ROW
// PANEL tm, so the column tiles that share an A panel through their XCD's L2 stay in step; the offsets persist down each CU's chain
// of tiles.
__device__ __forceinline__ void glds_stagger(const GldsParams& p, int tm, unsigned first_round) {
    if (p.stagger > 0 && blockIdx.x < first_round) {
        const unsigned phase = (unsigned)tm & 7u;
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        const unsigned long long wait = (unsigned long long)phase * (unsigned)p.stagger;
        while (__builtin_amdgcn_s_memrealtime() - t0 < wait) __builtin_amdgcn_s_sleep(16);
    }
}

// The epilogue's parameters are re-read from the kernarg segment where the epilogue starts: `glds_pe_t pe = *glds_kernarg_params(p)`.
// Carried through the K-loop in SGPRs (some 60 of them: pointers, leading dimensions, option words) they overflowed the scalar file,
// the overflow went to VGPR lanes, and the 128-VGPR K-loop answered with scratch reloads of its DMA source pointers inside the loop.
// (Returned as a pointer: a returned reference carries `dereferenceable`, and the loads through it are then hoisted over the barrier.)
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((opencl_constant)) GldsParams* glds_pe_ptr_t;
#else
typedef const GldsParams* glds_pe_ptr_t;
#endif
__device__ __forceinline__ glds_pe_ptr_t glds_kernarg_params(const GldsParams& p) {
#if defined(__HIP_DEVICE_COMPILE__)
    glds_pe_ptr_t kp = (glds_pe_ptr_t)__builtin_amdgcn_kernarg_segment_ptr();   // explicit arguments start at offset 0
    asm volatile("" : "+s"(kp)::"memory");
    return kp;
#else
    return &p;
#endif
}
