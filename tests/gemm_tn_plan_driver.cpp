// CPU driver of uc_gemm_tn_plan / uc_gemm_tn_auto_split_k (uniception_amd/csrc/gemm_tn_plan.h) for tests/test_gemm_tn_plan.py.
// stdin: one launch per line, `name=value` tokens — uc_gemm_tn_desc fields by their names (pointers as integer addresses, 0 = NULL).
// stdout: one line per launch, `kernel tiles_i tiles_j tiles block lds_bytes grid auto_split_k`.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include "gemm_tn_plan.h"

static const char* const KERNELS[] = {"256_dense", "256_conv", "128_dense", "128_conv", "conv_rows"};

static bool set_field(uc_gemm_tn_desc& d, const std::string& n, const char* v) {
    const long long i = strtoll(v, nullptr, 0);
#define I(f) if (n == #f) { d.f = (decltype(d.f))i; return true; }
#define PTR(f) if (n == #f) { d.f = (decltype(d.f))(uintptr_t)i; return true; }
    PTR(A) I(lda) PTR(B) I(ldb) I(T) I(I) I(J) I(conv_B) I(conv_H) I(conv_W) I(conv_Cin) I(conv_stride) I(relu_b) PTR(C) PTR(colsum_a)
    I(colsum_atomic) I(split_k)
#undef I
#undef PTR
    return false;
}

int main() {
    char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        uc_gemm_tn_desc d;
        memset(&d, 0, sizeof d);
        d.split_k = 1;
        for (char* t = strtok(line, " \t\n"); t; t = strtok(nullptr, " \t\n")) {
            char* eq = strchr(t, '=');
            if (!eq || !set_field(d, std::string(t, eq - t), eq + 1)) {
                fprintf(stderr, "bad token %s\n", t);
                return 2;
            }
        }
        const GemmTnPlan p = uc_gemm_tn_plan(d);
        printf("%s %d %d %d %d %d %u %d\n", KERNELS[p.kernel], p.tiles_i, p.tiles_j, p.tiles, p.block, p.lds_bytes, p.grid, uc_gemm_tn_auto_split_k(d));
    }
    return 0;
}
