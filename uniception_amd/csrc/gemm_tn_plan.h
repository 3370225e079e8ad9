// Routing of one uc_gemm_tn launch (the weight-gradient contraction dW = dY^T X): which kernel, tile counts, workgroup size, dynamic
// LDS and grid a descriptor gets, and the split_k the library recommends for its shape.
//
// Host-only, header-only and pure: no HIP header, no global state and no knob, so the system C++ compiler builds it
// (tests/test_gemm_tn_plan.py).  uc_gemm_tn validates, calls uc_gemm_tn_plan once and carries the plan out; uc_gemm_tn_query answers
// from the same two functions, so a caller's split_k and the launch can not disagree about the kernel.
#pragma once
#include <stdint.h>
#include "../../include/uc_hip.h"

// gemm_tn_kernel<BM, CONV>: BM x UC_TN_BN output tile, two stages of [64 t][BM i] + [64 t][UC_TN_BN j] bf16, BM * 4 threads
static constexpr int UC_TN_BN = 256;
static constexpr int UC_TN_NARROW_I = 128;   // I <= this: the half-height tile (BM = 128: no half-empty MFMA tiles), else BM = 256
static constexpr int uc_tn_lds_bytes(int bm) { return 2 * (64 * bm * 2 + 64 * UC_TN_BN * 2); }
// conv_dw_rows_kernel: one kernel row ky x UC_TN_ROWS_C output channels x UC_TN_ROWS_C input channels per workgroup, 64-pixel row
// segments; three stages of [64 t][128 i] + [68 pixels][128 c] bf16, 512 threads
static constexpr int UC_TN_ROWS_C = 128, UC_TN_ROWS_SEG = 64;
static constexpr int UC_TN_ROWS_LDS_BYTES = 3 * (64 * 256 + 68 * 256);
// the split rule fills this many compute units once.  The literal 256 (an unpartitioned MI355X), NOT the device's CU count: taking the
// count would change the launches on partitioned devices, which is a routing change and not this header's business.
static constexpr int UC_TN_FILL_CUS = 256;

enum GemmTnKernel {
    UC_TN_256_DENSE,    // gemm_tn_kernel<256, false>
    UC_TN_256_CONV,     // gemm_tn_kernel<256, true>: implicit im2col
    UC_TN_128_DENSE,    // gemm_tn_kernel<128, false>
    UC_TN_128_CONV,     // gemm_tn_kernel<128, true>
    UC_TN_CONV_ROWS,    // conv_dw_rows_kernel: row-walking conv weight gradient
};

struct GemmTnPlan {
    GemmTnKernel kernel;
    int tiles_i, tiles_j;   // output tiles; CONV_ROWS: tiles_j = Cin / 128, and 3 kernel rows on top
    int tiles;              // workgroups per K-slice
    int block;              // 1024 / 512
    int lds_bytes;          // 131072 / 98304 / 101376
    unsigned grid;          // tiles * d.split_k
};

// shapes the row-walking conv weight-gradient kernel takes (measured ahead of the implicit-im2col kernel on every one of them; every
// other conv: implicit im2col): stride 1, maps a multiple of 64 wide, whole 128-channel tiles of Cin and Cout (= I)
static inline bool uc_tn_conv_rows_ok(const uc_gemm_tn_desc& d) {
    return d.conv_B > 0 && d.conv_stride == 1 && d.conv_W % UC_TN_ROWS_SEG == 0 && d.conv_Cin % UC_TN_ROWS_C == 0 && d.I % UC_TN_ROWS_C == 0 &&
           d.conv_H > 0;
}

static inline GemmTnPlan uc_gemm_tn_plan(const uc_gemm_tn_desc& d) {
    GemmTnPlan p = {};
    if (uc_tn_conv_rows_ok(d)) {
        p.kernel = UC_TN_CONV_ROWS;
        p.tiles_i = (int)(d.I / UC_TN_ROWS_C); p.tiles_j = d.conv_Cin / UC_TN_ROWS_C;
        p.tiles = 3 * p.tiles_i * p.tiles_j;
        p.block = 512; p.lds_bytes = UC_TN_ROWS_LDS_BYTES;
    } else {
        const bool conv = d.conv_B > 0;
        const int bm = d.I <= UC_TN_NARROW_I ? 128 : 256;
        p.kernel = bm == 128 ? (conv ? UC_TN_128_CONV : UC_TN_128_DENSE) : (conv ? UC_TN_256_CONV : UC_TN_256_DENSE);
        p.tiles_i = (int)((d.I + bm - 1) / bm); p.tiles_j = (int)((d.J + UC_TN_BN - 1) / UC_TN_BN);
        p.tiles = p.tiles_i * p.tiles_j;
        p.block = bm * 4; p.lds_bytes = uc_tn_lds_bytes(bm);
    }
    p.grid = (unsigned)p.tiles * (unsigned)d.split_k;
    return p;
}

// Few output tiles, very long reduction: split it so that tiles * split_k just fills UC_TN_FILL_CUS once, with at least 512 rows of
// the reduction per slice.  (d.split_k is not read.)
static inline int uc_gemm_tn_auto_split_k(const uc_gemm_tn_desc& d) {
    const int64_t by_rows = d.T / 512, by_cus = UC_TN_FILL_CUS / uc_gemm_tn_plan(d).tiles;
    const int64_t sk = by_rows < by_cus ? by_rows : by_cus;
    return sk > 1 ? (int)sk : 1;
}
