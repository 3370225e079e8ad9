// Routing of one attention launch with head_dim > 64 (uc_attention_fwd, uc_attention_bwd): which kernel, grid and workgroup size.
// bf16: head_dim 80 and 96 (attention_wide.hip); fp32: 64 < head_dim <= 96 (the one-thread-per-row verification kernels at DMAX 96).
// Everything with head_dim <= 64 takes attention_plan.h; the entry points test D > 64 first.
//
// Host-only, header-only and pure, like attention_plan.h: no HIP header and no global state, so the system C++ compiler builds it
// (tests/test_attention_wide_plan.py).  The wide kernels read no tuning knob: a launch's plan is a function of its descriptor alone.
#pragma once
#include <stdint.h>
#include "../../include/uc_hip.h"

constexpr int UC_ATTN_WIDE_MAX_D = 96;

enum AttnWideFwdKernel {
    UC_AWF_BF16_80,   // attnw_fwd_kernel<80>: four waves, 128 queries per workgroup, grid (query tiles, H, B)
    UC_AWF_BF16_96,   // attnw_fwd_kernel<96>
    UC_AWF_F32_96,    // attn_f32_kernel<96>: fp32 verification kernel, 64 < head_dim <= 96
};
enum AttnWideDqKernel {
    UC_AWB_DQ_80,     // attnw_bwd_dq_kernel<80>: 128 queries per workgroup, 1-D grid
    UC_AWB_DQ_96,     // attnw_bwd_dq_kernel<96>
    UC_AWB_F32_DQ96,  // attn_bwd_dq_f32_kernel<96>, grid (query tiles, H, B)
};
enum AttnWideDkvKernel {
    UC_AWB_DKV_80,    // attnw_bwd_dkv_kernel<80>: 128 keys per workgroup, 1-D grid
    UC_AWB_DKV_96,    // attnw_bwd_dkv_kernel<96>
    UC_AWB_F32_DKV96, // attn_bwd_dkv_f32_kernel<96>, grid (key tiles, H, B)
};

struct AttnWideFwdPlan {
    AttnWideFwdKernel kernel;
    unsigned grid[3];
    int block;
};
struct AttnWideBwdPlan {
    AttnWideDqKernel dq;
    AttnWideDkvKernel dkv;
    unsigned dq_grid[3], dkv_grid[3];
    int block;
    unsigned delta_grid;   // fp32: attn_delta_f32_kernel's 1-D grid of 256 threads, launched first; else 0
};

// which head dims the wide path serves (the entry points refuse the others, naming the head_dim, before any launch)
static inline bool uc_attention_wide_supported(int dtype, int D) {
    if (dtype == UC_BF16) return D == 80 || D == 96;
    if (dtype == UC_F32) return D > 64 && D <= UC_ATTN_WIDE_MAX_D;
    return false;
}

static inline AttnWideFwdPlan uc_attention_wide_fwd_plan(const uc_attention_desc& d) {
    AttnWideFwdPlan plan = {};
    plan.grid[0] = (unsigned)((d.Nq + 127) / 128); plan.grid[1] = (unsigned)d.H; plan.grid[2] = (unsigned)d.B;
    if (d.dtype == UC_F32) {
        plan.kernel = UC_AWF_F32_96;
        plan.block = 128;
        return plan;
    }
    plan.kernel = d.D == 80 ? UC_AWF_BF16_80 : UC_AWF_BF16_96;
    plan.block = 256;
    return plan;
}

static inline AttnWideBwdPlan uc_attention_wide_bwd_plan(const uc_attention_bwd_desc& d) {
    AttnWideBwdPlan plan = {};
    const unsigned nqt = (unsigned)((d.Nq + 127) / 128), nkt = (unsigned)((d.Nk + 127) / 128);
    if (d.dtype == UC_F32) {
        plan.dq = UC_AWB_F32_DQ96;
        plan.dkv = UC_AWB_F32_DKV96;
        plan.dq_grid[0] = nqt; plan.dkv_grid[0] = nkt;
        plan.dq_grid[1] = plan.dkv_grid[1] = (unsigned)d.H; plan.dq_grid[2] = plan.dkv_grid[2] = (unsigned)d.B;
        plan.block = 128;
        plan.delta_grid = (unsigned)(((int64_t)d.B * d.H * d.Nq + 255) / 256);
        return plan;
    }
    plan.dq = d.D == 80 ? UC_AWB_DQ_80 : UC_AWB_DQ_96;
    plan.dkv = d.D == 80 ? UC_AWB_DKV_80 : UC_AWB_DKV_96;
    plan.dq_grid[0] = nqt * (unsigned)d.H * (unsigned)d.B;
    plan.dkv_grid[0] = nkt * (unsigned)d.H * (unsigned)d.B;
    plan.dq_grid[1] = plan.dq_grid[2] = plan.dkv_grid[1] = plan.dkv_grid[2] = 1;
    plan.block = 256;
    return plan;
}
