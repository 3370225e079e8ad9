// The two host-side choices of the DPT / MoGe heads' streaming kernels, and the grid caps of their grid-stride loops: which kernel one
// uc_bilinear_nhwc launch takes (csrc/elementwise.hip: one output row per work item, or R = 4 / 2 rows), which one uc_conv1x1_to4
// launch takes (the cooperative form with C8 = Cin / 8 lanes per pixel, or one thread per pixel), and the grids.
//
// Host-only, header-only and pure: no HIP header, no global state and no knob (UC_BILINEAR_ROWS2 is an argument), so the system C++
// compiler builds it (tests/stream_plan_driver.cpp).  The entry points validate, call their plan once and carry it out.
//
// Pointers come in as addresses; only their low four bits are read.
#pragma once
#include <stdint.h>

static constexpr int UC_STREAM_DT_F32 = 0, UC_STREAM_DT_BF16 = 1, UC_STREAM_DT_F16 = 2;     // UC_F32 / UC_BF16 / UC_F16 of include/uc_hip.h
static constexpr int UC_STREAM_WG = 256;                        // threads per workgroup of every streaming kernel
static constexpr int UC_EW_GRID_CAP = 65536 * 4;                // EW_GRID (vec_access.h): grid-stride kernels, one item per thread and iteration
static constexpr int UC_CONV1X1_COOP_GRID_CAP = 65536;          // conv1x1_to4_coop_kernel: 256 / C8 pixels per workgroup and iteration
static constexpr int UC_CONV1X1_BWD_GRID_CAP = 2048;            // conv1x1_to4_bwd_kernel: 256 / (Cin / 8) pixels per workgroup and iteration

static inline unsigned uc_stream_grid(int64_t items, int per_wg, int64_t cap) {
    const int64_t g = (items + per_wg - 1) / per_wg;
    return (unsigned)(cap > 0 && g > cap ? cap : g);
}

// ---- uc_bilinear_nhwc ------------------------------------------------------------------------------------------------------------
enum BilinearKernel {
    UC_BL_ONE_ROW,      // bilinear_kernel<Tag>: one output row per work item, any scale
    UC_BL_ROWS,         // bilinear_rows_kernel<Tag, R>: R output rows per work item, vertical scale <= 1/2
};

struct BilinearPlan {
    BilinearKernel kernel;
    int rows;           // R: 4 or 2; 1 for the one-row kernel
    float sy;           // vertical source step per output row: (Hi - 1) / (Ho - 1), 0 when Ho == 1
    unsigned grid_x, grid_y, grid_z;
};

static inline float uc_bilinear_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }

// rows2: the UC_BILINEAR_ROWS2 knob (rows per work item of the upsampling form: 4, 2, 0 = the one-row kernel).  The rows kernel is
// instantiated for (bf16, 4 or 2 rows) and (fp16, 4 rows): fp32 always takes the one-row kernel.  The widths decide nothing.
static inline BilinearPlan uc_bilinear_plan(int dtype, int Hi, int Ho, int crop_h, int crop_w, int C, int B, int rows2) {
    BilinearPlan p = {};
    p.sy = uc_bilinear_scale(Hi, Ho);
    const bool rows = rows2 != 0 && p.sy <= 0.5f && (dtype == UC_STREAM_DT_BF16 || dtype == UC_STREAM_DT_F16);
    p.kernel = rows ? UC_BL_ROWS : UC_BL_ONE_ROW;
    p.rows = !rows ? 1 : dtype == UC_STREAM_DT_F16 ? 4 : rows2 == 4 ? 4 : 2;
    p.grid_x = (unsigned)(((int64_t)crop_w * (C / 8) + UC_STREAM_WG - 1) / UC_STREAM_WG);
    p.grid_y = (unsigned)((crop_h + p.rows - 1) / p.rows);
    p.grid_z = (unsigned)B;
    return p;
}

// ---- uc_conv1x1_to4 / uc_conv1x1_to4_bwd -----------------------------------------------------------------------------------------
enum Conv1x1Kernel {
    UC_C1_COOP,         // conv1x1_to4_coop_kernel<Tag, C8>: C8 lanes share a pixel; reads the bias as one 16-byte vector
    UC_C1_PIXEL,        // conv1x1_to4_kernel<Tag>: one thread per pixel, any Cin % 8 == 0 up to 256, any bias alignment
};

struct Conv1x1Plan {
    Conv1x1Kernel kernel;
    int c8;             // coop: 1 2 4 8 16 32; else 0
    unsigned grid;
};

static inline Conv1x1Plan uc_conv1x1_to4_plan(int Cin, uintptr_t bias_ptr, int64_t npix) {
    Conv1x1Plan p = {};
    const int c8 = Cin / 8;
    const bool pow2 = Cin % 8 == 0 && (c8 == 1 || c8 == 2 || c8 == 4 || c8 == 8 || c8 == 16 || c8 == 32);
    if (bias_ptr % 16 == 0 && pow2) {
        p.kernel = UC_C1_COOP;
        p.c8 = c8;
        p.grid = uc_stream_grid(npix, UC_STREAM_WG / c8, UC_CONV1X1_COOP_GRID_CAP);
    } else {
        p.kernel = UC_C1_PIXEL;
        p.grid = uc_stream_grid(npix, UC_STREAM_WG, UC_EW_GRID_CAP);
    }
    return p;
}

// pixel lanes per workgroup = 256 / (Cin / 8); when 256 % (Cin / 8) != 0 the last threads of a workgroup own no pixel
static inline unsigned uc_conv1x1_to4_bwd_grid(int Cin, int64_t npix) {
    return uc_stream_grid(npix, UC_STREAM_WG / (Cin / 8), UC_CONV1X1_BWD_GRID_CAP);
}
