// Routing of one uc_gemm launch: which kernel, epilogue family, grid and launch options a descriptor gets.
//
// Host-only, header-only and pure: no HIP header and no global state, so the system C++ compiler builds it
// (tests/test_gemm_plan.py).  uc_gemm reads every knob once into a GemmKnobs snapshot and calls uc_gemm_plan once; the family
// launchers (gemm_glds_*.hip) carry the plan out and decide nothing.  A knob switched at run time therefore takes effect between
// launches, never inside one.
#pragma once
#include <stdint.h>
#include <algorithm>
#include "../../include/uc_hip.h"

static inline int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// hand-over buffer of the small-M path (fuse_split2): up to UC_FUSE_TILES 128x128 tiles of fp32 partials + one flag each
static constexpr int64_t UC_FUSE_TILES = 128;
static constexpr int64_t UC_FUSE_WS_FLOATS = UC_FUSE_TILES * 128 * 128;

// tiles of the register-staged (BM x BN) and fp32 VALU (FBM x FBN) kernels of gemm.hip
static constexpr int UC_REG_TILE = 128, UC_F32_TILE = 64;

// epilogue families of the direct-to-LDS kernels (one kernel instantiation per family, gemm_glds_kernel.h):
//   BF16: bf16 stores without residual;  F32: fp32 output (+ fp32 residuals, bf16 twin, row statistics);  BS: bf16 residual stream;
//   ALL: the generic drain (everything else, and every fp16-operand launch);  RES16: 3x3 convolution + 16-bit residual(s)
enum { GLDS_EPI_ALL = 0, GLDS_EPI_BF16 = 1, GLDS_EPI_F32 = 2, GLDS_EPI_BS = 3, GLDS_EPI_RES16 = 4 };

enum GemmKernel {
    UC_GK_REG,              // register-staged kernel (gemm_bf16_kernel), bf16 or f16 operands, 128x128 tiles
    UC_GK_F32,              // exact-fp32 VALU kernel (gemm_f32_kernel), 64x64 tiles
    // direct-to-LDS tile kernel gemm_bf16_glds_kernel<BM, BN, waves M, waves N, stages, ., BK, workgroups per CU>
    UC_GK_T128x128_S2,      // <128, 128, 2, 2, 2, ., 64, 1>
    UC_GK_T128x128_S3,      // <128, 128, 2, 2, 3, ., 64, 1>  latency regime: a 3-stage ring keeps two stages in flight
    UC_GK_T256x128_S2,      // <256, 128, 4, 2, 2, ., 64, 1>
    UC_GK_T256x128_S3,      // <256, 128, 4, 2, 3, ., 64, 1>
    UC_GK_T256x256,         // <256, 256, 4, 4, 2, ., 64, 1>
    UC_GK_T256x128_BK32,    // <256, 128, 4, 2, 3, ., 32, 2>  two co-resident workgroups per CU
    UC_GK_T128x64,          // <128, 64, 2, 1, 3, ., 64, 1>   dense bf16 only
    UC_GK_EIGHT_WAVE,       // gemm_bf16_glds8_kernel: 256x256, eight waves of 128x64 (dense bf16 only)
    UC_GK_FOUR_WAVE,        // gemm_bf16_glds4_kernel: 256x256, four waves of 128x128, AGPR accumulators (dense bf16 only)
    UC_GK_CONV_ROWS,        // conv3x3_rows_kernel: row-walking 3x3 convolution, 256 pixels x 128 channels
    UC_GK_CONV_ROWS8,       // conv3x3_rows8_kernel, segmented: 512 pixels of whole row segments x 128 channels
    UC_GK_CONV_ROWS8_FLAT,  // conv3x3_rows8_kernel, flat: 512 consecutive pixels, edge lanes zeroed in registers
};

// every knob the routing reads, read once per launch
struct GemmKnobs {
    int gemm_variant;    // -3 (or any negative but -1) automatic, -1 register-staged kernel, else the forced tile variant
    int small_m_split;   // smallest K the small-M path splits in two (0: never)
    int gemm_stagger;    // -1 launcher policy, >= 0 ticks per phase group
    int conv_rows;       // 0 never, 1 where they win, 2 the 256-pixel kernel / 3 the eight-wave kernel wherever the shape allows
    int conv_rows_flat;  // the eight-wave row kernel's flat form on maps whose rows do not tile 512 pixels: 1 / 0
    int gemm_group_m;    // row panels per L2-sharing tile group
    int gemm_4wave;      // four-wave kernel: 0 off, 1 bf16-store family, 2 + bf16 stream, 3 every family
    int cus;             // compute units of the device
    int dbg;             // diagnostics bits (UC_GEMM_DBG, diag build only; 0 in the release build)
};

struct GemmPlan {
    GemmKernel kernel;
    int epi;                   // GLDS_EPI_* family of a direct-to-LDS kernel
    int f16;                   // fp16 operands
    int relu_a;                // ReLU on load (selects the row kernels' instantiation)
    int64_t tiles_m, tiles_n;  // output tiles
    int slices;                // grid = tiles_m * tiles_n * slices (split-K slices, or the two halves of fuse_split2)
    int vec_ok;                // C / bias / residual / preact / dact_u are aligned for the 4-wide vector epilogues
    int stagger, nt_out, side_lds, fuse_split2;   // GldsParams launch options
};

// the four-wave kernel's shapes: whole 8-row groups, one mode per 128-column wave tile, no split-K, 32-bit row pitches
static inline bool glds4_ok(const uc_gemm_desc& d, int split_k) {
    return d.a_mode == UC_A_DENSE && d.M % 8 == 0 && d.N % 8 == 0 && d.M >= 8 && d.N >= 8 && split_k <= 1 && d.K >= 64 &&
           (d.vt_col0 < 0 || d.vt_col0 % 128 == 0) && (d.rope_cols <= 0 || d.rope_cols % 128 == 0) && d.lda * 2 < ((int64_t)1 << 31) &&
           d.K * 2 < ((int64_t)1 << 31) && d.M < ((int64_t)1 << 31) && d.N < ((int64_t)1 << 31);
}

// the 256-pixel row-walking conv kernel's shapes: stride 1, whole 64-channel chunks, 128-column tiles, maps 64 .. wide whose rows
// tile 256 pixels exactly (a tile = whole row segments of one image), 32-bit source windows
static inline bool conv_rows_ok(const uc_gemm_desc& d, int split_k) {
    if (d.a_mode != UC_A_CONV3X3 || d.conv_stride != 1 || d.conv_Cin % 64 != 0 || d.N % 128 != 0 || split_k > 1) return false;
    const int W = d.conv_W, H = d.conv_H;
    if (W < 64 || !(W % 256 == 0 || 256 % W == 0)) return false;
    const int R = W >= 256 ? 1 : 256 / W;
    if (H % R != 0 || d.M % 256 != 0) return false;
    return ((int64_t)(R + 3) * W + 4) * d.conv_Cin * 2 < ((int64_t)1 << 31) && d.N * d.K * 2 < ((int64_t)1 << 31) && d.M < ((int64_t)1 << 30);
}

// the eight-wave row-walking conv kernel's shapes: stride 1, whole 64-channel chunks (an even number of 32-channel super-steps),
// 128-column tiles, 32-bit source windows.  0: none; 1: the segmented form (maps 128 .. wide whose rows tile 512 pixels: no
// register masks); 2: the flat form (when `flat` is on: any map at least 16 wide, any pixel count, the last tile masked)
static inline int conv_rows8_ok(const uc_gemm_desc& d, int split_k, bool flat) {
    if (d.a_mode != UC_A_CONV3X3 || d.conv_stride != 1 || d.conv_Cin % 64 != 0 || d.N % 128 != 0 || split_k > 1) return 0;
    const int W = d.conv_W, H = d.conv_H;
    if (d.N * d.K * 2 >= ((int64_t)1 << 31) || d.M >= ((int64_t)1 << 30)) return 0;
    if (W >= 128 && (W % 512 == 0 || 512 % W == 0)) {
        const int R = W >= 512 ? 1 : 512 / W;
        if (H % R == 0 && d.M % 512 == 0 && ((int64_t)(R + 3) * W + 4) * d.conv_Cin * 2 < ((int64_t)1 << 31)) return 1;
    }
    if (W < 16 || !flat) return 0;
    return ((int64_t)(530 + 2 * W) * d.conv_Cin * 2 < ((int64_t)1 << 31)) ? 2 : 0;
}

// A convolution whose every tile takes the 16-bit residual epilogue: 16-bit output, one or two residuals of the same dtype laid
// out like it, bias or none, no activation — the residual conv units' second convolution.
static inline bool glds_res16_ok(const uc_gemm_desc& d, bool vec_ok, bool f16, int dbg) {
    const int out16 = f16 ? UC_F16 : UC_BF16;
    return d.a_mode == UC_A_CONV3X3 && vec_ok && d.N % 64 == 0 && d.split_k <= 1 && !d.preact_out && !d.dact_u && !(dbg & 16) &&
           d.out_dtype == out16 && d.residual && d.res_dtype == out16 && d.act == UC_ACT_NONE && !d.relu_a && !d.tail_out && !d.ln_stats &&
           !d.stats_out && !d.twin_out && (d.ldr & 7) == 0 && d.vt_col0 < 0 && d.rope_cols <= 0;
}

// dense operands the direct-to-LDS kernels take: K % 64 == 0, or — fp16 operands, which have no register-staged fallback kernel —
// K % 32 == 0 (the DPT's 96-channel ConvTranspose GEMM) on the 32-deep tile
static inline bool glds_dense32(const uc_gemm_desc& d) {
    return d.compute_dtype == UC_F16 && d.a_mode == UC_A_DENSE && d.K % 64 != 0 && d.K % 32 == 0 && !d.relu_a;
}
static inline bool glds_dense_ok(const uc_gemm_desc& d) { return d.a_mode == UC_A_DENSE && (d.K % 64 == 0 || glds_dense32(d)) && !d.relu_a; }

// tile kernel of a tile variant (0 = 128x128, 1 = 256x128, 2 = 256x256, 3 = 256x128x32 co-resident, 4 = 128x64, 6 = eight-wave,
// 7 = four-wave 256x256); what a family cannot run falls back to the 16-wave 256x256 / the 128x128 tile
static inline GemmKernel glds_tile_kernel(const uc_gemm_desc& d, int variant, bool f16, int split_k) {
    const int64_t sk = split_k;
    switch (variant) {
        case 1:   // latency regime (fewer workgroups than CUs: every K-step waits for its own DMA): a 3-stage ring
            return ceil_div64(d.M, 256) * ceil_div64(d.N, 128) * sk <= 256 ? UC_GK_T256x128_S3 : UC_GK_T256x128_S2;
        case 2: return UC_GK_T256x256;
        case 3: return UC_GK_T256x128_BK32;
        case 6:   // (its DMA addresses row groups of 8 uniformly: matrices whose last group is partial stay on the 16-wave kernel)
            return !f16 && d.a_mode == UC_A_DENSE && d.M % 8 == 0 && d.N % 8 == 0 ? UC_GK_EIGHT_WAVE : UC_GK_T256x256;
        case 7: return !f16 && glds4_ok(d, split_k) ? UC_GK_FOUR_WAVE : UC_GK_T256x256;
        case 4:   // the latency regime's small tile — launches whose 128x128 tiles cover at most half the CUs
            if (d.a_mode == UC_A_DENSE && !f16) return UC_GK_T128x64;
            [[fallthrough]];
        default: return ceil_div64(d.M, 128) * ceil_div64(d.N, 128) * sk <= 512 ? UC_GK_T128x128_S3 : UC_GK_T128x128_S2;
    }
}

static inline GemmPlan uc_gemm_plan(const uc_gemm_desc& d, const GemmKnobs& k) {
    GemmPlan plan = {};
    plan.f16 = d.compute_dtype == UC_F16;
    plan.relu_a = d.relu_a;
    plan.slices = 1;
    const bool f16 = plan.f16;
    if (d.compute_dtype == UC_F32) {
        plan.kernel = UC_GK_F32;
        plan.tiles_m = ceil_div64(d.M, UC_F32_TILE); plan.tiles_n = ceil_div64(d.N, UC_F32_TILE);
        return plan;
    }
    const bool conv = d.a_mode == UC_A_CONV3X3;
    const bool dense32 = glds_dense32(d), glds_dense = glds_dense_ok(d);
    // convolutions: Cin % 64 == 0 any tile, Cin % 32 == 0 (the DPT's 96-channel reassemble stage) the 32-deep K-step tile only; the
    // conv DMA addresses a tile's input window (the images its 256 output rows touch) with 32-bit byte offsets
    const int64_t conv_window_bytes = conv ? (256 / std::max<int64_t>(1, (int64_t)d.conv_Ho * d.conv_Wo) + 2) * (int64_t)d.conv_H * d.conv_W * d.conv_Cin * 2 : 0;
    const bool glds_conv = conv && d.conv_Cin % 32 == 0 && (int64_t)d.conv_B * d.conv_H * d.conv_W < (int64_t)1 << 30 &&
                           conv_window_bytes < (int64_t)1 << 31 && (int64_t)256 * d.K * 2 < (int64_t)1 << 31;
    if (!(glds_dense || glds_conv) || k.gemm_variant == -1) {
        plan.kernel = UC_GK_REG;
        plan.tiles_m = ceil_div64(d.M, UC_REG_TILE); plan.tiles_n = ceil_div64(d.N, UC_REG_TILE);
        return plan;
    }

    const int split_k = d.split_k > 1 ? d.split_k : 1;
    const int64_t sk = split_k;
    const bool c_ok = ((uintptr_t)d.C % 16 == 0) && (d.ldc % 8 == 0);
    const bool b_ok = !d.bias || ((uintptr_t)d.bias % 16 == 0);
    const bool r_ok = !d.residual || (((uintptr_t)d.residual % 16 == 0) && (d.ldr % 4 == 0) && (!d.residual2 || (uintptr_t)d.residual2 % 16 == 0));
    const bool x_ok = (!d.preact_out || (uintptr_t)d.preact_out % 16 == 0) && (!d.dact_u || (uintptr_t)d.dact_u % 8 == 0);
    plan.vec_ok = c_ok && b_ok && r_ok && x_ok && !d.tail_out;   // (the fused tail: never one of the single-family kernels)

    // tile variant: forced (gemm_variant >= 0) or the heuristic's
    const bool auto_variant = k.gemm_variant < 0;
    int variant = k.gemm_variant;
    if ((conv && d.conv_Cin % 64 != 0) || dense32) variant = 3;
    else if (variant < 0) {
        // the 256x256 tile (16 waves) has the best steady state (least LDS fill per flop) but needs enough tiles to cover the
        // 256 CUs; smaller problems fall back to 256x128 / 128x128 tiles
        const int64_t t256 = ceil_div64(d.M, 256) * ceil_div64(d.N, 256);
        const int64_t t256x128 = ceil_div64(d.M, 256) * ceil_div64(d.N, 128);
        variant = t256 * sk >= 192 ? 2 : (t256x128 * sk >= 160 ? 1 : 0);
        if (!conv) {
            // Dense launches of a few rounds of tiles (the batch sweep's 2 - 16 pairs): what matters is how many ROUNDS of
            // workgroups a tile size needs on the CUs, times what a round of that tile costs — measured per round at
            // K = 768 / 1024 (tools/scratch/bench_midsize_variants.py): 128x128 ~13 / 19 us, 256x128 ~16 / 23 us, 256x256 ~22 / 29 us,
            // i.e. 1 : 1.25 : 1.7.  The thresholds above missed the quantisation: 144 tiles of 256x256 beat 288 of 256x128 by
            // 38 % (decoder qkv at 4 pairs), 144 of 256x128 beat 288 of 128x128 by 47 % (at 2 pairs).
            const int64_t cus = k.cus;
            const int64_t t128 = ceil_div64(d.M, 128) * ceil_div64(d.N, 128);
            const double c0 = (double)ceil_div64(t128 * sk, cus), c1 = 1.25 * (double)ceil_div64(t256x128 * sk, cus),
                         c2 = 1.7 * (double)ceil_div64(t256 * sk, cus);
            variant = (c2 <= c1 && c2 <= c0) ? 2 : (c1 <= c0 ? 1 : 0);
        }
        // a 256-wide tile whose last column block is at most half full wastes a 128-column slab of MFMA work per row
        // panel (N = 128: half of every tile): take the 256x128 tile there
        const int64_t waste256 = ceil_div64(d.N, 256) * 256 - d.N, waste128 = ceil_div64(d.N, 128) * 128 - d.N;
        if (variant == 2 && waste256 - waste128 >= 128 && t256x128 * sk >= 160) variant = 1;
        // 256x128 tiles with enough workgroups for two per CU: the 32-deep K-step form (72 KiB of LDS, two co-resident
        // 8-wave workgroups) keeps 16 waves on a CU where the 64-deep form (96 KiB) leaves 8
        if (variant == 1 && t256x128 * sk >= 512) variant = 3;
    }
    if (d.tail_out && (variant == 2 || variant == 6)) variant = 1;    // the tail needs a tile that spans all 128 columns with two wave columns
    // Small-M path: a launch (dense or 3x3 conv) whose 128x128 tiles cover at most half the CUs is a chain of K / 64 dependent steps of
    // ~0.7 us on each of them (neither a smaller tile nor a deeper ring shortens it: measured) — split K in two across twice
    // the workgroups, hand-over inside the kernel (fuse_split2) through the caller's fuse_ws.  small_m_split = smallest K it is taken
    // for (0: never — the sum over K is then one chain whatever the batch size, and a pair's bits do not depend on its batch).
    const int64_t t128 = ceil_div64(d.M, 128) * ceil_div64(d.N, 128);
    plan.fuse_split2 = auto_variant && variant == 0 && d.split_k <= 1 && !d.tail_out && k.small_m_split > 0 && d.K >= k.small_m_split &&
                       d.K % 128 == 0 && 2 * t128 <= k.cus && t128 <= UC_FUSE_TILES && d.fuse_ws;
    // output (+ residual) streams of more than half the 256 MB Infinity Cache: non-temporal epilogue loads / stores
    // (bit 0: fp32 residual stream, 1: bf16 outputs, 2: bf16 RoPE (q, k) tiles)
    plan.nt_out = d.M * d.N * (d.out_dtype == UC_F32 ? 4 : 2) > ((int64_t)128 << 20) ? 7 : 0;
    plan.stagger = k.gemm_stagger;

    plan.epi = GLDS_EPI_ALL;
    if (f16 && (variant == 6 || variant == 7)) variant = 2;   // fp16 operands: the 16-wave / co-resident tiles only
    if (conv) {
        // row-walking kernels: the eight-wave 512-pixel form wherever its shape allows (conv_rows 3) or, by default, where the
        // launch has at least as many tiles as CUs (fewer: the latency-regime tiles — conv_rows 3 makes the kernel choice, and with
        // it the summation order, independent of the batch size).  Measured ahead of both other forms on every DPT-head shape
        // (DESIGN.md section 7).  The 256-pixel form where it wins over the implicit-GEMM tiles (conv_rows 1): 128 output channels
        // and >= 256 input channels — 256^2 256 -> 128: 850 -> 959 TFLOP/s (fp16 834 -> 926); with 256 output channels the 256x256
        // tile streams half the weights per MFMA and stays ahead.
        const int rows_mode = k.conv_rows;
        const int rows8 = conv_rows8_ok(d, split_k, k.conv_rows_flat != 0);
        const bool take_rows8 = rows8 && (rows_mode == 3 || (rows_mode == 1 && ((d.M + 511) / 512) * (d.N / 128) >= 256));
        const bool take_rows256 = rows_mode > 0 && rows_mode < 3 && conv_rows_ok(d, split_k) && (rows_mode >= 2 || (d.N == 128 && d.conv_Cin >= 256)) &&
                                  (d.M / 256) * (d.N / 128) >= 256;
        // the residual conv units' second convolution: its own family on the eight-wave row kernel or the 256x256 tile, else the
        // generic family's routing below
        if (glds_res16_ok(d, plan.vec_ok, f16, k.dbg) && (take_rows8 || (variant == 2 && !take_rows256))) plan.epi = GLDS_EPI_RES16;
        if (take_rows8) {
            plan.kernel = rows8 == 2 ? UC_GK_CONV_ROWS8_FLAT : UC_GK_CONV_ROWS8;
            plan.tiles_m = (d.M + 511) / 512; plan.tiles_n = d.N / 128;
            return plan;
        }
        if (take_rows256) {
            plan.kernel = UC_GK_CONV_ROWS;
            plan.tiles_m = d.M / 256; plan.tiles_n = d.N / 128;
            return plan;
        }
    } else if (!f16) {
        // a launch takes a single-family kernel only when EVERY wave of it takes that family's epilogue
        const bool plain = plan.vec_ok && d.N % 64 == 0 && d.split_k <= 1 && !d.preact_out && !d.dact_u && !(k.dbg & 16);
        // bf16 residual stream (out bf16 + bf16 residual and / or row statistics): the residual family's drain, 2 + 2 bytes per element
        const bool bf16_stream = plain && d.out_dtype == UC_BF16 && d.act == UC_ACT_NONE && d.vt_col0 < 0 && d.rope_cols <= 0 && !d.ln_stats &&
                                 !d.residual2 && ((d.residual && d.res_dtype == UC_BF16) || d.stats_out);
        const bool bf16_fam = plain && d.out_dtype == UC_BF16 && !d.residual && !bf16_stream;
        const bool f32_fam = plain && d.out_dtype == UC_F32 && (!d.residual || d.res_dtype == UC_F32) && d.act == UC_ACT_NONE && d.vt_col0 < 0;
        plan.epi = bf16_fam ? GLDS_EPI_BF16 : bf16_stream ? GLDS_EPI_BS : f32_fam ? GLDS_EPI_F32 : GLDS_EPI_ALL;
        // the heuristic's 256x256 tile: the eight-wave form for the bf16-store family (128x64 per wave, next K-chunk's fragments
        // register-resident) ...
        if (auto_variant && variant == 2 && d.M % 8 == 0 && d.N % 8 == 0 && bf16_fam) variant = 6;
        // ... or the four-wave form (128x128 wave tiles, accumulators in AGPRs, hand-scheduled K-loop) where it beats the 16-wave
        // kernel (K >= 2048)
        const int four = k.gemm_4wave;
        if (auto_variant && (variant == 2 || variant == 6) && four > 0 && d.K >= 2048 &&
            (four >= 3 || (bf16_fam && four >= 1) || (bf16_stream && four >= 2) || (f32_fam && four >= 3))) variant = 7;
        // The fp32 epilogues (residual read + fp32 store + bf16 twin) move 4-5x the bytes of a bf16 store and all CUs reach
        // them together: an HBM burst with idle matrix pipes.  Launches long enough to amortise the ramp (>= 6 tiles per CU)
        // start their first round of workgroups in 8 phase groups 1.5 us apart (by row panel, see the kernel):
        // encoder proj 480 -> 432 us, fc2 1095 -> 1043 us; neutral-to-worse for shorter launches, hence the threshold.
        // (bf16 residual stream, round 4: 4 bytes per element in the epilogue — the stagger measures 316 vs 322 us AGAINST it on the
        //  encoder's proj GEMM: off for that family)
        if ((f32_fam || bf16_stream) && plan.stagger < 0)
            plan.stagger = (!bf16_stream && (variant == 2 || variant == 6 || variant == 7) && ceil_div64(d.M, 256) * ceil_div64(d.N, 256) >= 6 * 256) ? 150 : 0;
    }
    plan.kernel = glds_tile_kernel(d, variant, f16, split_k);
    switch (plan.kernel) {
        case UC_GK_T128x128_S2: case UC_GK_T128x128_S3:
            plan.tiles_m = ceil_div64(d.M, 128); plan.tiles_n = ceil_div64(d.N, 128); break;
        case UC_GK_T128x64: plan.tiles_m = ceil_div64(d.M, 128); plan.tiles_n = ceil_div64(d.N, 64); break;
        case UC_GK_T256x128_S2: case UC_GK_T256x128_S3: case UC_GK_T256x128_BK32:
            plan.tiles_m = ceil_div64(d.M, 256); plan.tiles_n = ceil_div64(d.N, 128); break;
        default: plan.tiles_m = ceil_div64(d.M, 256); plan.tiles_n = ceil_div64(d.N, 256); break;
    }
    plan.slices = (plan.kernel == UC_GK_T128x128_S2 || plan.kernel == UC_GK_T128x128_S3) && plan.fuse_split2 ? 2 : split_k;
    // eight-wave kernel, bf16-store family with a finalized folded LayerNorm: the tile's row statistics / column sums / bias / RoPE
    // positions are DMA-staged into 8 KiB of LDS behind the ring at kernel start
    auto al16 = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
    plan.side_lds = plan.kernel == UC_GK_EIGHT_WAVE && plan.epi == GLDS_EPI_BF16 && d.ln_stats && d.ln_nblk <= 0 && d.ln_colsum && d.bias &&
                    split_k <= 1 && !(k.dbg & 16) && al16(d.ln_stats) && al16(d.ln_colsum) && al16(d.bias) &&
                    (d.rope_cols <= 0 || (d.rope_pos && al16(d.rope_pos)));
    return plan;
}
