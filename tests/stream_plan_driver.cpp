// CPU driver of uc_bilinear_plan / uc_conv1x1_to4_plan / uc_conv1x1_to4_bwd_grid (uniception_amd/csrc/stream_plan.h) for
// tests/test_head_stream_routes.py.
// stdin: one launch per line, `name=value` tokens: op (bilinear | conv1x1 | conv1x1_bwd); bilinear: dtype (0 f32, 1 bf16, 2 f16), Hi, Ho,
// crop_h, crop_w, C, B, rows2 (the UC_BILINEAR_ROWS2 knob, default 4); conv1x1: Cin, bias (the pointer as an integer address), npix;
// conv1x1_bwd: Cin, npix.
// stdout: one line per launch, `bilinear one_row|rows R grid_x grid_y grid_z`, `conv1x1 coop|pixel c8 grid`, `conv1x1_bwd grid`.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include "stream_plan.h"

struct Launch {
    int op;
    long long dtype, Hi, Ho, crop_h, crop_w, C, B, rows2, Cin, bias, npix;
};

static bool set_field(Launch& l, const std::string& n, const char* v) {
    if (n == "op") {
        l.op = !strcmp(v, "bilinear") ? 0 : !strcmp(v, "conv1x1") ? 1 : !strcmp(v, "conv1x1_bwd") ? 2 : -1;
        return l.op >= 0;
    }
    const long long i = strtoll(v, nullptr, 0);
#define I(f) if (n == #f) { l.f = i; return true; }
    I(dtype) I(Hi) I(Ho) I(crop_h) I(crop_w) I(C) I(B) I(rows2) I(Cin) I(bias) I(npix)
#undef I
    return false;
}

int main() {
    char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        Launch l;
        memset(&l, 0, sizeof l);
        l.op = -1;
        l.rows2 = 4;
        for (char* t = strtok(line, " \t\n"); t; t = strtok(nullptr, " \t\n")) {
            char* eq = strchr(t, '=');
            if (!eq || !set_field(l, std::string(t, eq - t), eq + 1)) {
                fprintf(stderr, "bad token %s\n", t);
                return 2;
            }
        }
        if (l.op == 0) {
            const BilinearPlan p = uc_bilinear_plan((int)l.dtype, (int)l.Hi, (int)l.Ho, (int)l.crop_h, (int)l.crop_w, (int)l.C, (int)l.B, (int)l.rows2);
            printf("bilinear %s %d %u %u %u\n", p.kernel == UC_BL_ROWS ? "rows" : "one_row", p.rows, p.grid_x, p.grid_y, p.grid_z);
        } else if (l.op == 1) {
            const Conv1x1Plan p = uc_conv1x1_to4_plan((int)l.Cin, (uintptr_t)l.bias, l.npix);
            printf("conv1x1 %s %d %u\n", p.kernel == UC_C1_COOP ? "coop" : "pixel", p.c8, p.grid);
        } else if (l.op == 2) {
            printf("conv1x1_bwd %u\n", uc_conv1x1_to4_bwd_grid((int)l.Cin, l.npix));
        } else {
            fprintf(stderr, "no op\n");
            return 2;
        }
    }
    return 0;
}
