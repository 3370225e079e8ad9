// CPU driver of uc_ln_fwd_plan / uc_ln_bwd_plan (uniception_amd/csrc/layernorm_plan.h) for tests/test_layernorm_routes.py.
// stdin: one launch per line, `name=value` tokens: dir (fwd | bwd), rows, C, x_bytes, dy_bytes (element sizes), the pointers x y twin gamma
// beta dy dres dx as integer addresses (0 = NULL; twin is y_twin_bf16 / dx_bf16; has_dres / has_twin follow from dres / twin), ln_nt (the
// UC_LN_NT knob, default -1: the size policy).
// stdout: one line per launch, `fwd kernel nv nt rows_per_wg grid` or `bwd kernel nv rows_per_wg grid`.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include "layernorm_plan.h"

static const char* const FWD[] = {"exact", "vec", "scalar"};
static const char* const BWD[] = {"wide", "c64", "generic"};

struct Launch {
    bool bwd;
    long long rows, C, x_bytes, dy_bytes, x, y, twin, gamma, beta, dy, dres, dx, ln_nt;
};

static bool set_field(Launch& l, const std::string& n, const char* v) {
    if (n == "dir") {
        if (strcmp(v, "fwd") != 0 && strcmp(v, "bwd") != 0) return false;
        l.bwd = strcmp(v, "bwd") == 0;
        return true;
    }
    const long long i = strtoll(v, nullptr, 0);
#define I(f) if (n == #f) { l.f = i; return true; }
    I(rows) I(C) I(x_bytes) I(dy_bytes) I(x) I(y) I(twin) I(gamma) I(beta) I(dy) I(dres) I(dx) I(ln_nt)
#undef I
    return false;
}

int main() {
    char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        Launch l;
        memset(&l, 0, sizeof l);
        l.x_bytes = l.dy_bytes = 4;
        l.ln_nt = -1;
        for (char* t = strtok(line, " \t\n"); t; t = strtok(nullptr, " \t\n")) {
            char* eq = strchr(t, '=');
            if (!eq || !set_field(l, std::string(t, eq - t), eq + 1)) {
                fprintf(stderr, "bad token %s\n", t);
                return 2;
            }
        }
        if (l.bwd) {
            const LnBwdPlan p = uc_ln_bwd_plan(l.rows, (int)l.C, l.dres != 0, l.twin != 0, (int)l.x_bytes, (int)l.dy_bytes, (uintptr_t)l.x, (uintptr_t)l.dy,
                                               (uintptr_t)l.dres, (uintptr_t)l.dx, (uintptr_t)l.twin, (uintptr_t)l.gamma);
            printf("bwd %s %d %d %u\n", BWD[p.kernel], p.nv, p.rows_per_wg, p.grid);
        } else {
            const LnFwdPlan p = uc_ln_fwd_plan(l.rows, (int)l.C, (int)l.x_bytes, (uintptr_t)l.x, (uintptr_t)l.y, (uintptr_t)l.twin, (uintptr_t)l.gamma,
                                               (uintptr_t)l.beta, (int)l.ln_nt);
            printf("fwd %s %d %d %d %u\n", FWD[p.kernel], p.nv, (int)p.nt, p.rows_per_wg, p.grid);
        }
    }
    return 0;
}
