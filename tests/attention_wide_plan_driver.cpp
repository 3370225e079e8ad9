// CPU driver of uc_attention_wide_fwd_plan / uc_attention_wide_bwd_plan (uniception_amd/csrc/attention_wide_plan.h) for
// tests/test_attention_wide_plan.py.
// stdin: one launch per line, `name=value` tokens as tests/attention_plan_driver.cpp takes them — `fn=fwd` or `fn=bwd` and the descriptor
// fields by their names; the knob tokens of that driver (p64, bwd64, role_split, cus, dbg) are accepted and ignored: the wide plan reads none.
// stdout: one line per launch.  A head_dim the wide path does not serve: `refused`.  Forward `kernel grid_x grid_y grid_z block`,
// backward `dq dq_grid dkv dkv_grid` (bf16, 1-D grids) or `dq x,y,z dkv x,y,z block delta_grid` (fp32).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include "attention_wide_plan.h"

static const char* const FWD_KERNELS[] = {"bf16_80", "bf16_96", "f32_96"};
static const char* const DQ_KERNELS[] = {"dq80", "dq96", "f32_dq96"};
static const char* const DKV_KERNELS[] = {"dkv80", "dkv96", "f32_dkv96"};

static bool set_field(uc_attention_desc& f, uc_attention_bwd_desc& b, const std::string& n, const char* v) {
    const long long i = strtoll(v, nullptr, 0);
    if (n == "drop") {
        f.drop_p = b.drop_p = i ? 0.1f : 0.f;
        return true;
    }
#define FB(x) if (n == #x) { f.x = (decltype(f.x))i; b.x = (decltype(b.x))i; return true; }
#define F(x) if (n == #x) { f.x = (decltype(f.x))i; return true; }
    FB(dtype) FB(B) FB(H) FB(Nq) FB(Nk) FB(D) FB(q_sb) FB(q_sn) FB(q_sh) FB(k_sb) FB(k_sn) FB(k_sh) FB(v_sb) FB(v_sn) FB(v_sh)
    FB(o_sb) FB(o_sn) FB(o_sh) F(v_layout) F(O)
#undef FB
#undef F
    return n == "p64" || n == "bwd64" || n == "role_split" || n == "cus" || n == "dbg";
}

int main() {
    char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        uc_attention_desc f;
        uc_attention_bwd_desc b;
        memset(&f, 0, sizeof f);
        memset(&b, 0, sizeof b);
        bool bwd = false;
        for (char* t = strtok(line, " \t\n"); t; t = strtok(nullptr, " \t\n")) {
            char* eq = strchr(t, '=');
            const std::string n = eq ? std::string(t, eq - t) : std::string();
            if (eq && n == "fn" && (!strcmp(eq + 1, "fwd") || !strcmp(eq + 1, "bwd"))) {
                bwd = !strcmp(eq + 1, "bwd");
                continue;
            }
            if (!eq || !set_field(f, b, n, eq + 1)) {
                fprintf(stderr, "bad token %s\n", t);
                return 2;
            }
        }
        if (!uc_attention_wide_supported(f.dtype, f.D)) {
            printf("refused\n");
        } else if (bwd) {
            const AttnWideBwdPlan p = uc_attention_wide_bwd_plan(b);
            if (b.dtype == UC_F32)
                printf("%s %u,%u,%u %s %u,%u,%u %d %u\n", DQ_KERNELS[p.dq], p.dq_grid[0], p.dq_grid[1], p.dq_grid[2], DKV_KERNELS[p.dkv],
                       p.dkv_grid[0], p.dkv_grid[1], p.dkv_grid[2], p.block, p.delta_grid);
            else
                printf("%s %u %s %u\n", DQ_KERNELS[p.dq], p.dq_grid[0], DKV_KERNELS[p.dkv], p.dkv_grid[0]);
        } else {
            const AttnWideFwdPlan p = uc_attention_wide_fwd_plan(f);
            printf("%s %u %u %u %d\n", FWD_KERNELS[p.kernel], p.grid[0], p.grid[1], p.grid[2], p.block);
        }
    }
    return 0;
}
