// Routing of one attention forward / backward launch (uc_attention_fwd, uc_attention_bwd; bf16 and fp32, every head_dim, with and
// without dropout): whether the launch is served at all and, if it is, which kernel, grid and workgroup size it gets.  The plans are
// total: every descriptor that passed the entry points' null / shape / drop_p checks gets either a refusal reason or a launch, and
// nothing else in the library decides which dtype, head_dim, dropout and RoPE combinations exist.
//
// Host-only, header-only and pure: no HIP header and no global state, so the system C++ compiler builds it
// (tests/test_attention_plan.py, tests/test_attention_wide_plan.py).  The entry points read every knob once into an AttnKnobs
// snapshot and call the plan once; they carry it out and decide nothing.  A knob switched at run time (uc_tuning_set) therefore
// takes effect between launches, never inside one.  The head_dim > 64 kernels (attention_wide.hip, and the fp32 verification
// kernels at DMAX 96) read no knob: their plan is a function of the descriptor alone.
#pragma once
#include <stdint.h>
#include "../../include/uc_hip.h"

constexpr int UC_ATTN_WIDE_MAX_D = 96;   // the largest head_dim any kernel serves

// why a launch is refused; 0: it is served.  One message per reason (uc_attention_refusal_format).
enum AttnRefusal {
    UC_AR_SERVED = 0,
    UC_AR_DTYPE,         // dtype is neither UC_BF16 nor UC_F32
    UC_AR_BF16_HEAD_DIM, // bf16: head_dim must be 64, 80 or 96
    UC_AR_F32_HEAD_DIM,  // fp32: head_dim must be <= UC_ATTN_WIDE_MAX_D
    UC_AR_DROPOUT,       // attention dropout exists at head_dim <= 64 only
    UC_AR_ROPE_F32,      // backward RoPE positions: the fp32 backward has no inverse rotation
    UC_AR_ROPE_HEAD_DIM, // backward RoPE positions: the bf16 inverse rotation is head_dim 64 only
    UC_AR_BWD_GRID,      // bf16 backward: ceil(Nq / 128) H B or ceil(Nk / 128) H B does not fit a 1-D grid (>= 2^31)
};

// the message of a refusal as a printf format of (entry point's name, int): the int is the dtype for UC_AR_DTYPE, the head_dim otherwise
static inline const char* uc_attention_refusal_format(AttnRefusal r) {
    static const char* const TEXT[] = {
        "%s: served (head_dim %d)",
        "%s: unsupported dtype %d",
        "%s(bf16): head_dim must be 64, 80 or 96 (got %d)",
        "%s(f32): head_dim must be <= 96 (got %d)",
        "%s: attention dropout is not available at head_dim %d (head_dim <= 64 only)",
        "%s(f32): the fp32 backward takes no RoPE positions (head_dim %d)",
        "%s: the inverse RoPE is not available at head_dim %d (bf16 at head_dim 64 only)",
        "%s: too many 128-row tiles for one grid (head_dim %d)",
    };
    return TEXT[r];
}

enum AttnFwdKernel {
    UC_AF_REG128,        // attn_bf16_kernel: register-staged, 128 queries per workgroup, grid (query tiles, H, B)
    UC_AF_DMA4,          // attn_bf16_dma_kernel<4>: LDS-DMA staged, 128 queries per workgroup, 1-D grid
    UC_AF_DMA8,          // attn_bf16_dma_kernel<8>: 256 queries per workgroup
    UC_AF_RS8,           // attn_bf16_rs_kernel: the eight-wave kernel as role-split segments
    UC_AF_P64,           // attn_bf16_p64_kernel<false> (persistent, 64 queries per wave) + attn_bf16_fixup_kernel
    UC_AF_P64_TAIL,      // attn_bf16_p64_kernel<true>: the same with a partial last key tile
    UC_AF_REG128_DROP,   // attn_bf16_drop_kernel: attn_bf16_kernel with dropout of the probabilities
    UC_AF_F32_32,        // attn_f32_kernel<32>: fp32 verification kernel, head_dim <= 32
    UC_AF_F32_64,        // attn_f32_kernel<64>: head_dim <= 64
    UC_AF_F32_32_DROP,   // attn_f32_kernel<32, true>
    UC_AF_F32_64_DROP,   // attn_f32_kernel<64, true>
    UC_AF_DMA4_DBG,      // attn_bf16_dma_kernel<4, dbg>: diag build only (UC_ATTN_DBG, wrong results)
    UC_AF_BF16_80,       // attnw_fwd_kernel<80> (attention_wide.hip): four waves, 128 queries per workgroup, grid (query tiles, H, B)
    UC_AF_BF16_96,       // attnw_fwd_kernel<96>
    UC_AF_F32_96,        // attn_f32_kernel<96>: 64 < head_dim <= 96 (no dropout form)
};

enum AttnDqKernel {
    UC_AB_DQ32,          // attn_bwd_dq_kernel<false>: 128 queries (4 waves x 32) per workgroup
    UC_AB_DQ64,          // attn_bwd_dq64_kernel: persistent, 64 queries per wave
    UC_AB_DQ32_DROP,     // attn_bwd_dq_kernel<true>
    UC_AB_F32_DQ32,      // attn_bwd_dq_f32_kernel<32>: fp32 verification kernel (dropout a run-time test), head_dim <= 32, grid (query tiles, H, B)
    UC_AB_F32_DQ64,      // attn_bwd_dq_f32_kernel<64>: head_dim <= 64
    UC_AB_DQ80,          // attnw_bwd_dq_kernel<80> (attention_wide.hip): 128 queries per workgroup, 1-D grid
    UC_AB_DQ96,          // attnw_bwd_dq_kernel<96>
    UC_AB_F32_DQ96,      // attn_bwd_dq_f32_kernel<96>: 64 < head_dim <= 96
};

enum AttnDkvKernel {
    UC_AB_DKV32,         // attn_bwd_dkv_kernel<false>: 128 keys per workgroup
    UC_AB_DKV64,         // attn_bwd_dkv64_kernel: persistent, 64 keys per wave
    UC_AB_DKV32_DROP,    // attn_bwd_dkv_kernel<true>
    UC_AB_F32_DKV32,     // attn_bwd_dkv_f32_kernel<32>: grid (key tiles, H, B)
    UC_AB_F32_DKV64,     // attn_bwd_dkv_f32_kernel<64>
    UC_AB_DKV80,         // attnw_bwd_dkv_kernel<80> (attention_wide.hip): 128 keys per workgroup, 1-D grid
    UC_AB_DKV96,         // attnw_bwd_dkv_kernel<96>
    UC_AB_F32_DKV96,     // attn_bwd_dkv_f32_kernel<96>
};

// every knob the routing reads, read once per launch
struct AttnKnobs {
    int p64;          // persistent 64-queries-per-wave forward: 0 never, 1 where the launch has enough items, 2 wherever the shape allows
    int bwd64;        // 64-rows-per-wave backward kernels: 0 never, 1 where a workgroup's rows are mostly real, 2 always
    int role_split;   // eight-wave forward as role-split segments: 0 / 1
    int cus;          // compute units of the device
    int dbg;          // UC_ATTN_DBG anatomy switches (diag build only; 0 in the release build)
};

// (a refused plan — refused != 0 — has every other field zero)
struct AttnFwdPlan {
    AttnRefusal refused;
    AttnFwdKernel kernel;
    unsigned grid[3];   // x, y, z
    int block;          // threads per workgroup
    int nqt;            // query tiles per (batch, head) of the DMA kernels (AttnParams dGroup / dNq; bf16 without dropout, else 0)
    int fixup_grid;     // attn_bf16_fixup_kernel's grid (P64 / P64_TAIL)
    int dbg;            // the anatomy switches of UC_AF_DMA4_DBG
};

struct AttnBwdPlan {
    AttnRefusal refused;
    AttnDqKernel dq;
    AttnDkvKernel dkv;
    unsigned dq_grid[3], dkv_grid[3];   // x, y, z (bf16: 1-D)
    int block;                          // threads per workgroup of both launches
    unsigned delta_grid;                // fp32: attn_delta_f32_kernel's 1-D grid of 256 threads, launched first; else 0
};

// THE served set: which dtype, head_dim, dropout and backward-RoPE combinations have a kernel (rope: the backward got positions)
static inline AttnRefusal uc_attention_refusal(int dtype, int D, bool drop, bool rope) {
    if (dtype != UC_BF16 && dtype != UC_F32) return UC_AR_DTYPE;
    if (dtype == UC_BF16 && D != 64 && D != 80 && D != 96) return UC_AR_BF16_HEAD_DIM;
    if (dtype == UC_F32 && D > UC_ATTN_WIDE_MAX_D) return UC_AR_F32_HEAD_DIM;
    if (drop && D > 64) return UC_AR_DROPOUT;
    if (rope && dtype == UC_F32) return UC_AR_ROPE_F32;
    if (rope && D != 64) return UC_AR_ROPE_HEAD_DIM;
    return UC_AR_SERVED;
}

// (the plans read only the shape, strides, dtype, v_layout, the output's address, drop_p and — backward — whether there are RoPE
//  positions of the descriptor)
static inline AttnFwdPlan uc_attention_fwd_plan(const uc_attention_desc& d, const AttnKnobs& k) {
    AttnFwdPlan plan = {};
    plan.refused = uc_attention_refusal(d.dtype, d.D, d.drop_p != 0.f, false);
    if (plan.refused) return plan;
    plan.block = 256;
    // the grid of the register-staged and fp32 kernels: one workgroup per 128 queries of a (batch, head)
    plan.grid[0] = (unsigned)((d.Nq + 127) / 128); plan.grid[1] = (unsigned)d.H; plan.grid[2] = (unsigned)d.B;
    const bool drop = d.drop_p != 0.f;
    if (d.D > 64) {   // one workgroup per 128 queries here too; no knob is read
        plan.kernel = d.dtype == UC_F32 ? UC_AF_F32_96 : d.D == 80 ? UC_AF_BF16_80 : UC_AF_BF16_96;
        if (d.dtype == UC_F32) plan.block = 128;
        return plan;
    }
    if (d.dtype == UC_F32) {
        plan.kernel = d.D <= 32 ? (drop ? UC_AF_F32_32_DROP : UC_AF_F32_32) : (drop ? UC_AF_F32_64_DROP : UC_AF_F32_64);
        plan.block = 128;
        return plan;
    }
    if (drop) {   // bf16 with dropout: the register-staged kernel with the mask between the softmax and the second product
        plan.kernel = UC_AF_REG128_DROP;
        return plan;
    }
    const int Nq = d.Nq, Nk = d.Nk, H = d.H, B = d.B;
    const int npad = (Nk + 63) / 64 * 64;
    // eight waves per workgroup (256 queries share each K / VT tile) when that does not add a mostly empty query tile
    const int waste8 = (Nq + 255) / 256 * 256 - Nq, waste4 = (Nq + 127) / 128 * 128 - Nq;
    // (a launch whose 256-query tiles would not give every CU two workgroups takes 128-query tiles: one pair of 512 x 512 views is
    //  128 tiles of 256 queries — half the chip idle — or 256 of 128)
    const bool few8 = (int64_t)((Nq + 255) / 256) * H * B < 2 * (int64_t)k.cus;
    // (the diag build's anatomy switches exist in the four-wave kernel only)
    const int nw = !k.dbg && Nq >= 256 && waste8 - waste4 < 64 && !few8 ? 8 : 4;
    const int qtile = 32 * nw, nqt = (Nq + qtile - 1) / qtile;
    plan.nqt = nqt;
    // DMA-staged kernel: whole 64-key tiles, 32-bit byte offsets inside one (batch, head)'s K rows / VT rows
    const bool dma_ok = (int64_t)nqt * H * B < ((int64_t)1 << 31) && (uintptr_t)d.O % 16 == 0 && d.o_sb % 8 == 0 && d.o_sn % 8 == 0 && d.o_sh % 8 == 0 &&
                        (int64_t)32 * d.q_sn * 2 < ((int64_t)1 << 31) && (int64_t)Nk * d.k_sn * 2 < ((int64_t)1 << 31) &&
                        (int64_t)64 * npad * 2 < ((int64_t)1 << 31);
    if (!dma_ok) {
        plan.kernel = UC_AF_REG128;
        return plan;
    }
    plan.grid[0] = (unsigned)(nqt * H * B); plan.grid[1] = plan.grid[2] = 1;
    plan.block = 64 * nw;
    if (k.dbg) {
        plan.kernel = UC_AF_DMA4_DBG;
        plan.dbg = k.dbg;
        return plan;
    }
    // persistent 64-queries-per-wave kernel (attention_p64.h) + its fix-up scan: 32-bit DMA offsets as above, at least two key
    // tiles, and (policy) enough (batch, head, 256-query tile) items — one per workgroup of the 2 x 256 (measured break-even: 384 items
    // at 1024 keys, tools/bench_attention_ab.py; 256 items when an item is 64 key tiles long) —, a query count
    // that does not leave a quarter of the last tile empty.  (A wanted log-sum-exp is no obstacle: the kernel rounds scale * log2(e) * Q
    // to bf16, so its scores and LSE carry ~2^-9 of |q| |k| scale — and the backward's dQ kernel rounds Q the same way and recomputes
    // exactly these scores, the dK / dV kernel rounds K instead: the same noise class either way.)  The role-split kernel vetoes it.
    const int64_t p64_items = (int64_t)B * H * ((Nq + 255) / 256);
    const bool p64_ok = k.p64 && !k.role_split && Nk > 64 && p64_items < ((int64_t)1 << 28) && (int64_t)64 * d.q_sn * 2 < ((int64_t)1 << 31) &&
                        (int64_t)64 * d.o_sn * 2 < ((int64_t)1 << 31) &&
                        (k.p64 == 2 || ((p64_items >= 512 || (p64_items >= 256 && Nk >= 4096)) && waste8 * 4 <= Nq));
    if (p64_ok) {
        plan.kernel = Nk & 63 ? UC_AF_P64_TAIL : UC_AF_P64;
        // two workgroups per CU in whole groups of 8 (one per XCD), at least 8, at most the items rounded up to 8
        int64_t grid = 2 * k.cus / 8 * 8;
        if (grid < 8) grid = 8;
        const int64_t items8 = (p64_items + 7) / 8 * 8;
        if (grid > items8) grid = items8;
        plan.grid[0] = (unsigned)grid;
        plan.block = 256;
        const int64_t nblocks = (int64_t)B * H * ((Nq + 63) / 64), fblocks = (nblocks + 255) / 256;   // one thread per 64-query block
        plan.fixup_grid = (int)(fblocks < k.cus ? fblocks : k.cus);
        return plan;
    }
    plan.kernel = nw == 8 ? (k.role_split ? UC_AF_RS8 : UC_AF_DMA8) : UC_AF_DMA4;
    return plan;
}

static inline AttnBwdPlan uc_attention_bwd_plan(const uc_attention_bwd_desc& d, const AttnKnobs& k) {
    AttnBwdPlan plan = {};
    const int Nq = d.Nq, Nk = d.Nk, H = d.H, B = d.B;
    plan.refused = uc_attention_refusal(d.dtype, d.D, d.drop_p != 0.f, d.rope_qpos || d.rope_kpos);
    // every bf16 backward kernel takes its 128-row tiles from a 1-D grid (the persistent 64-row kernels count theirs from the same
    // product): it must fit one.  (Only the head_dim 80 / 96 entry used to test this; at head_dim 64 the product was cast to unsigned
    // unchecked.  A launch that large already fails in the runtime, so the rule refuses nothing that works.)
    if (!plan.refused && d.dtype == UC_BF16 &&
        ((int64_t)((Nq + 127) / 128) * H * B >= ((int64_t)1 << 31) || (int64_t)((Nk + 127) / 128) * H * B >= ((int64_t)1 << 31)))
        plan.refused = UC_AR_BWD_GRID;
    if (plan.refused) return plan;
    if (d.dtype == UC_F32) {   // one thread per query row (dQ) / per key row (dK, dV), 128 per workgroup, after the delta pass
        plan.dq = d.D <= 32 ? UC_AB_F32_DQ32 : d.D <= 64 ? UC_AB_F32_DQ64 : UC_AB_F32_DQ96;
        plan.dkv = d.D <= 32 ? UC_AB_F32_DKV32 : d.D <= 64 ? UC_AB_F32_DKV64 : UC_AB_F32_DKV96;
        plan.dq_grid[0] = (unsigned)((Nq + 127) / 128); plan.dkv_grid[0] = (unsigned)((Nk + 127) / 128);
        plan.dq_grid[1] = plan.dkv_grid[1] = (unsigned)H; plan.dq_grid[2] = plan.dkv_grid[2] = (unsigned)B;
        plan.block = 128;
        plan.delta_grid = (unsigned)(((int64_t)B * H * Nq + 255) / 256);
        return plan;
    }
    plan.block = 256;
    plan.dq_grid[1] = plan.dq_grid[2] = plan.dkv_grid[1] = plan.dkv_grid[2] = 1;
    plan.dq_grid[0] = (unsigned)(((Nq + 127) / 128) * H * B);
    plan.dkv_grid[0] = (unsigned)(((Nk + 127) / 128) * H * B);
    if (d.D > 64) {   // the head_dim 80 / 96 kernels: these grids, no knob
        plan.dq = d.D == 80 ? UC_AB_DQ80 : UC_AB_DQ96;
        plan.dkv = d.D == 80 ? UC_AB_DKV80 : UC_AB_DKV96;
        return plan;
    }
    if (d.drop_p != 0.f) {   // attention dropout: the 32-row kernels with the forward's mask re-evaluated per element
        plan.dq = UC_AB_DQ32_DROP;
        plan.dkv = UC_AB_DKV32_DROP;
        return plan;
    }
    // the persistent kernels: one workgroup per CU (in whole groups of 8: workgroup g on XCD g % 8), at most the items rounded up to 8
    auto persistent = [&](int64_t items) {
        const int64_t g = k.cus / 8 * 8, items8 = (items + 7) / 8 * 8;
        return (unsigned)(g < items8 ? g : items8);
    };
    const int64_t v_ext = ((int64_t)(B - 1) * d.v_sb + (int64_t)(H - 1) * d.v_sh + (int64_t)(Nk - 1) * d.v_sn + 64) * 2;
    // 64 queries per wave (attention_bwd64.h) when a 256-query workgroup is mostly real queries; the 32-query kernel otherwise
    const bool dq64 = Nk > 64 && v_ext < (int64_t)0xffffffffll &&
                      (k.bwd64 == 2 || (k.bwd64 == 1 && Nq >= 192 && ((Nq + 255) / 256) * 256 * 3 <= Nq * 4));
    plan.dq = dq64 ? UC_AB_DQ64 : UC_AB_DQ32;
    if (dq64) plan.dq_grid[0] = persistent((int64_t)((Nq + 255) / 256) * H * B);
    // 64 keys per wave (attention_bwd64.h) when a 256-key workgroup is mostly real keys; the 32-key kernel otherwise
    // (its Q / dO / scratch descriptors span the whole tensors: 32-bit byte offsets)
    const int64_t q_ext = ((int64_t)(B - 1) * d.q_sb + (int64_t)(H - 1) * d.q_sh + (int64_t)(Nq - 1) * d.q_sn + 64) * 2;
    const int64_t o_ext = ((int64_t)(B - 1) * d.o_sb + (int64_t)(H - 1) * d.o_sh + (int64_t)(Nq - 1) * d.o_sn + 64) * 2;
    const int64_t nq_pad = (Nq + 127) / 128 * 128;
    const bool fits32 = q_ext < (int64_t)0xffffffffll && o_ext < (int64_t)0xffffffffll && (int64_t)B * H * 2 * nq_pad * 4 < (int64_t)0xffffffffll;
    // query rows past Nq of a (batch, head) are read through those descriptors and must be FINITE (their P is exp2(-1e30 + s) = 0): true
    // when the next batch's rows follow directly (or the tensor ends: zero fill), not when a strided view leaves a gap of foreign memory
    // between batches — such views take the 32-key kernel, whose loads are bounded per (batch, head)
    const bool rows_follow = B == 1 || (d.q_sb == (int64_t)Nq * d.q_sn && d.o_sb == (int64_t)Nq * d.o_sn);
    const bool dkv64 = Nq > 64 && fits32 && rows_follow &&
                       (k.bwd64 == 2 || (k.bwd64 == 1 && Nk >= 192 && ((Nk + 255) / 256) * 256 * 3 <= Nk * 4));
    plan.dkv = dkv64 ? UC_AB_DKV64 : UC_AB_DKV32;
    if (dkv64) plan.dkv_grid[0] = persistent((int64_t)((Nk + 255) / 256) * H * B);
    return plan;
}
