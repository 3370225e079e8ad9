// CPU driver of uc_attention_fwd_plan / uc_attention_bwd_plan (uniception_amd/csrc/attention_plan.h) for tests/test_attention_plan.py.
// stdin: one launch per line, `name=value` tokens — `fn=fwd` or `fn=bwd`, the uc_attention_desc / uc_attention_bwd_desc fields by their
// names (O as an integer address; `drop=1` sets a non-zero drop_p; `rope=1` gives the backward non-null RoPE positions; a backward
// without dtype / D is bf16 with head_dim 64) and the knob snapshot (p64, bwd64, role_split, cus, dbg).
// stdout: one line per launch, `refused <reason>` or, forward, `kernel grid_x grid_y grid_z block nqt fixup_grid`, backward
// `dq dq_grid dkv dkv_grid` (bf16, 1-D grids) or `dq dq_grid dkv dkv_grid block delta_grid` (fp32, grids as x,y,z).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include "attention_plan.h"

static const char* const FWD_KERNELS[] = {"reg128", "dma4", "dma8", "rs8", "p64", "p64_tail", "reg128_drop", "f32_32", "f32_64",
                                          "f32_32_drop", "f32_64_drop", "dma4_dbg", "bf16_80", "bf16_96", "f32_96"};
static const char* const DQ_KERNELS[] = {"dq32", "dq64", "dq32_drop", "f32_dq32", "f32_dq64", "dq80", "dq96", "f32_dq96"};
static const char* const DKV_KERNELS[] = {"dkv32", "dkv64", "dkv32_drop", "f32_dkv32", "f32_dkv64", "dkv80", "dkv96", "f32_dkv96"};
static const char* const REFUSALS[] = {"served", "dtype", "bf16_head_dim", "f32_head_dim", "dropout", "rope_f32", "rope_head_dim", "bwd_grid"};

static bool set_field(uc_attention_desc& f, uc_attention_bwd_desc& b, AttnKnobs& k, const std::string& n, const char* v) {
    const long long i = strtoll(v, nullptr, 0);
    if (n == "drop") {
        f.drop_p = b.drop_p = i ? 0.1f : 0.f;
        return true;
    }
    if (n == "rope") {
        static const int64_t POS[2] = {0, 0};
        b.rope_qpos = b.rope_kpos = i ? POS : nullptr;
        return true;
    }
#define FB(x) if (n == #x) { f.x = (decltype(f.x))i; b.x = (decltype(b.x))i; return true; }
#define F(x) if (n == #x) { f.x = (decltype(f.x))i; return true; }
#define K(x) if (n == #x) { k.x = (int)i; return true; }
    FB(dtype) FB(B) FB(H) FB(Nq) FB(Nk) FB(D) FB(q_sb) FB(q_sn) FB(q_sh) FB(k_sb) FB(k_sn) FB(k_sh) FB(v_sb) FB(v_sn) FB(v_sh)
    FB(o_sb) FB(o_sn) FB(o_sh) F(v_layout) F(O)
    K(p64) K(bwd64) K(role_split) K(cus) K(dbg)
#undef FB
#undef F
#undef K
    return false;
}

int main() {
    char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        uc_attention_desc f;
        uc_attention_bwd_desc b;
        memset(&f, 0, sizeof f);
        memset(&b, 0, sizeof b);
        b.dtype = UC_BF16;
        b.D = 64;
        AttnKnobs k = {1, 1, 0, 256, 0};   // the library's defaults on a 256-CU device
        bool bwd = false;
        for (char* t = strtok(line, " \t\n"); t; t = strtok(nullptr, " \t\n")) {
            char* eq = strchr(t, '=');
            const std::string n = eq ? std::string(t, eq - t) : std::string();
            if (eq && n == "fn" && (!strcmp(eq + 1, "fwd") || !strcmp(eq + 1, "bwd"))) {
                bwd = !strcmp(eq + 1, "bwd");
                continue;
            }
            if (!eq || !set_field(f, b, k, n, eq + 1)) {
                fprintf(stderr, "bad token %s\n", t);
                return 2;
            }
        }
        if (bwd) {
            const AttnBwdPlan p = uc_attention_bwd_plan(b, k);
            if (p.refused)
                printf("refused %s\n", REFUSALS[p.refused]);
            else if (b.dtype == UC_F32)
                printf("%s %u,%u,%u %s %u,%u,%u %d %u\n", DQ_KERNELS[p.dq], p.dq_grid[0], p.dq_grid[1], p.dq_grid[2], DKV_KERNELS[p.dkv],
                       p.dkv_grid[0], p.dkv_grid[1], p.dkv_grid[2], p.block, p.delta_grid);
            else
                printf("%s %u %s %u\n", DQ_KERNELS[p.dq], p.dq_grid[0], DKV_KERNELS[p.dkv], p.dkv_grid[0]);
        } else {
            const AttnFwdPlan p = uc_attention_fwd_plan(f, k);
            if (p.refused)
                printf("refused %s\n", REFUSALS[p.refused]);
            else
                printf("%s %u %u %u %d %d %d\n", FWD_KERNELS[p.kernel], p.grid[0], p.grid[1], p.grid[2], p.block, p.nqt, p.fixup_grid);
        }
    }
    return 0;
}
