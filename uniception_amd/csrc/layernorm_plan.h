// Routing of one uc_layernorm / uc_layernorm_twin launch (csrc/rope_norm.hip) and of one uc_layernorm_bwd launch (csrc/train.hip): which
// kernel, which exact-width instance, non-temporal loads or not, and the grid.
//
// Host-only, header-only and pure: no HIP header, no global state and no knob (the UC_LN_NT override is an argument), so the system C++
// compiler builds it (tests/layernorm_plan_driver.cpp).  launch_ln and uc_layernorm_bwd validate, call their plan once and carry it out.
//
// Pointers come in as addresses (0 = NULL); only their low four bits are read.  Both entry points take any element-aligned pointer: the
// vector kernels do 16-byte accesses (8-byte ones on bf16 rows) without a test of their own, so a launch that is not aligned for them
// takes the scalar / generic kernel.
#pragma once
#include <stdint.h>

// the register-resident kernels hold a row as UC_LN_MAXV float4 per lane: C <= 64 * 4 * UC_LN_MAXV
static constexpr int UC_LN_MAXV = 8;
static constexpr int UC_LN_MAX_VEC_C = 64 * 4 * UC_LN_MAXV;
// fp32 / bf16 rows above this many bytes are read once here and once two GEMMs later: streamed past the caches (half the Infinity Cache)
static constexpr int64_t UC_LN_NT_BYTES = (int64_t)128 << 20;
static constexpr int UC_LN_FWD_ROWS_PER_WG = 4;        // one wavefront per row, 256 threads
static constexpr int UC_LN_BWD_WIDE_ROWS_PER_WG = 8;   // layernorm_bwd_kernel: 512 threads, one row per wave and iteration
static constexpr int UC_LN_BWD_WIDE_GRID_CAP = 256;    // ... grid-stride above 2048 waves
static constexpr int UC_LN_BWD_C64_ROWS_PER_WG = 16;   // layernorm64_bwd_kernel: 256 threads, four rows per wave and iteration
static constexpr int UC_LN_BWD_C64_GRID_CAP = 1024;
static constexpr int UC_LN_BWD_GENERIC_ROWS_PER_WG = 4;

// the widths with an exact instance: C = 256 * nv.  0: none (1280 = 256 * 5 and 1792 = 256 * 7 have none)
static inline int uc_ln_exact_nv(int C) {
    if (C <= 0 || C % 256 != 0) return 0;
    const int nv = C / 256;
    return (nv == 1 || nv == 2 || nv == 3 || nv == 4 || nv == 6 || nv == 8) ? nv : 0;
}

static inline unsigned uc_ln_grid(int64_t rows, int per_wg, int64_t cap) {
    const int64_t g = (rows + per_wg - 1) / per_wg;
    return (unsigned)(cap > 0 && g > cap ? cap : g);
}

enum LnFwdKernel {
    UC_LN_FWD_EXACT,    // layernorm_exact_kernel<TI, TO, nv, nt>: C == 256 * nv, no predicates
    UC_LN_FWD_VEC,      // layernorm_vec_kernel<TI, TO>: C % 4 == 0, C <= 2048, predicated 16-byte chunks
    UC_LN_FWD_SCALAR,   // layernorm_scalar_kernel<TI, TO>: any C, any element-aligned pointer
};

struct LnFwdPlan {
    LnFwdKernel kernel;
    int nv;             // exact: 1 2 3 4 6 8; else 0
    bool nt;            // exact only: the NT = true instance
    int rows_per_wg;
    unsigned grid;
};

// ln_nt: the UC_LN_NT knob (< 0: the size policy, 0: never, > 0: always)
static inline LnFwdPlan uc_ln_fwd_plan(int64_t rows, int C, int x_elem_bytes, uintptr_t align_x, uintptr_t align_y, uintptr_t align_twin,
                                       uintptr_t align_gamma, uintptr_t align_beta, int ln_nt) {
    LnFwdPlan p = {};
    const bool vec = (C % 4 == 0) && (C <= UC_LN_MAX_VEC_C) && (align_x % 16 == 0) && (align_y % 16 == 0) && (align_twin % 8 == 0) &&
                     (align_gamma % 16 == 0) && (align_beta % 16 == 0);
    const int nv = vec ? uc_ln_exact_nv(C) : 0;
    p.kernel = nv ? UC_LN_FWD_EXACT : vec ? UC_LN_FWD_VEC : UC_LN_FWD_SCALAR;
    p.nv = nv;
    p.nt = nv != 0 && (ln_nt >= 0 ? ln_nt != 0 : rows * (int64_t)C * (int64_t)x_elem_bytes > UC_LN_NT_BYTES);
    p.rows_per_wg = UC_LN_FWD_ROWS_PER_WG;
    p.grid = uc_ln_grid(rows, p.rows_per_wg, 0);
    return p;
}

enum LnBwdKernel {
    UC_LN_BWD_WIDE,     // layernorm_bwd_kernel<TD, nv, TX>: C == 256 * nv, rows software-pipelined per wave
    UC_LN_BWD_C64,      // layernorm64_bwd_kernel<TD, TX>: C == 64 without dres and without the bf16 twin (qk-norm)
    UC_LN_BWD_GENERIC,  // layernorm_bwd_generic_kernel<TD, TX>: any C, any element-aligned pointer
};

struct LnBwdPlan {
    LnBwdKernel kernel;
    int nv;             // wide: 1 2 3 4 6 8; else 0
    int rows_per_wg;
    unsigned grid;      // rows above grid * rows_per_wg: further grid-stride iterations (wide, c64)
};

// x, dres and dx share x_elem_bytes (the stream's dtype); a lane's four elements are one access: 4 * elem bytes of alignment.
// dres / dx_bf16: pass 0 when absent.
static inline LnBwdPlan uc_ln_bwd_plan(int64_t rows, int C, bool has_dres, bool has_twin, int x_elem_bytes, int dy_elem_bytes, uintptr_t align_x,
                                       uintptr_t align_dy, uintptr_t align_dres, uintptr_t align_dx, uintptr_t align_twin, uintptr_t align_gamma) {
    LnBwdPlan p = {};
    const uintptr_t ax = 4 * (uintptr_t)x_elem_bytes, ad = 4 * (uintptr_t)dy_elem_bytes;
    const bool aligned = (align_x % ax == 0) && (align_dy % ad == 0) && (!has_dres || align_dres % ax == 0) && (align_dx % ax == 0) &&
                         (!has_twin || align_twin % 8 == 0) && (align_gamma % 16 == 0);
    const int nv = aligned ? uc_ln_exact_nv(C) : 0;
    if (aligned && C == 64 && !has_dres && !has_twin) {
        p.kernel = UC_LN_BWD_C64;
        p.rows_per_wg = UC_LN_BWD_C64_ROWS_PER_WG;
        p.grid = uc_ln_grid(rows, p.rows_per_wg, UC_LN_BWD_C64_GRID_CAP);
    } else if (nv) {
        p.kernel = UC_LN_BWD_WIDE;
        p.nv = nv;
        p.rows_per_wg = UC_LN_BWD_WIDE_ROWS_PER_WG;
        p.grid = uc_ln_grid(rows, p.rows_per_wg, UC_LN_BWD_WIDE_GRID_CAP);
    } else {
        p.kernel = UC_LN_BWD_GENERIC;
        p.rows_per_wg = UC_LN_BWD_GENERIC_ROWS_PER_WG;
        p.grid = uc_ln_grid(rows, p.rows_per_wg, 0);
    }
    return p;
}
