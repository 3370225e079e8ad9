// CPU driver of uc_gemm_plan (uniception_amd/csrc/gemm_plan.h) for tests/test_gemm_plan.py.
// stdin: one launch per line, `name=value` tokens — uc_gemm_desc fields by their names (pointers as integer addresses, 0 = NULL)
// and the knob snapshot (gemm_variant, small_m_split, gemm_stagger, conv_rows, conv_rows_flat, gemm_4wave, cus, dbg).
// stdout: one line per launch, `kernel epi tiles_m tiles_n slices stagger nt_out side_lds fuse_split2 vec_ok relu_a`.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include "gemm_plan.h"

static const char* const KERNELS[] = {"reg", "f32", "t128x128_s2", "t128x128_s3", "t256x128_s2", "t256x128_s3", "t256x256", "t256x128_bk32",
                                      "t128x64", "eight_wave", "four_wave", "conv_rows", "conv_rows8", "conv_rows8_flat"};
static const char* const EPIS[] = {"all", "bf16", "f32", "bs", "res16"};

static bool set_field(uc_gemm_desc& d, GemmKnobs& k, const std::string& n, const char* v) {
    const long long i = strtoll(v, nullptr, 0);
    const void* p = (const void*)(uintptr_t)i;
#define I(f) if (n == #f) { d.f = (decltype(d.f))i; return true; }
#define PTR(f) if (n == #f) { d.f = (decltype(d.f))p; return true; }
#define K(f) if (n == #f) { k.f = (int)i; return true; }
    I(compute_dtype) I(a_mode) I(relu_a) I(lda) I(M) I(N) I(K) I(conv_B) I(conv_H) I(conv_W) I(conv_Cin) I(conv_stride) I(conv_Ho) I(conv_Wo)
    I(act) I(res_dtype) I(ldr) I(rope_cols) I(rope_npos) I(vt_col0) I(vt_ntok) I(vt_npad) I(split_k) I(dact_act) I(out_dtype) I(ldc) I(ldt)
    I(ln_nblk)
    if (n == "ln_eps") { d.ln_eps = strtof(v, nullptr); return true; }
    PTR(A) PTR(W) PTR(bias) PTR(residual) PTR(residual2) PTR(rope_pos) PTR(rope_table) PTR(vt_out) PTR(preact_out) PTR(dact_u) PTR(C)
    PTR(twin_out) PTR(stats_out) PTR(ln_stats) PTR(ln_colsum) PTR(tail_w) PTR(tail_b) PTR(tail_out) PTR(fuse_ws) PTR(sat_flag)
    K(gemm_variant) K(small_m_split) K(gemm_stagger) K(conv_rows) K(conv_rows_flat) K(gemm_group_m) K(gemm_4wave) K(cus) K(dbg)
#undef I
#undef PTR
#undef K
    return false;
}

int main() {
    char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        uc_gemm_desc d;
        memset(&d, 0, sizeof d);
        d.vt_col0 = -1;
        GemmKnobs k = {-3, 2048, -1, 1, 1, 4, 3, 256, 0};   // the library's defaults on a 256-CU device
        for (char* t = strtok(line, " \t\n"); t; t = strtok(nullptr, " \t\n")) {
            char* eq = strchr(t, '=');
            if (!eq || !set_field(d, k, std::string(t, eq - t), eq + 1)) {
                fprintf(stderr, "bad token %s\n", t);
                return 2;
            }
        }
        if (d.a_mode == UC_A_CONV3X3) {   // derived geometry, as the callers fill it in
            if (!d.conv_stride) d.conv_stride = 1;
            d.conv_Ho = (d.conv_H - 1) / d.conv_stride + 1;
            d.conv_Wo = (d.conv_W - 1) / d.conv_stride + 1;
            d.M = (int64_t)d.conv_B * d.conv_Ho * d.conv_Wo;
            d.K = (int64_t)9 * d.conv_Cin;
        }
        const GemmPlan p = uc_gemm_plan(d, k);
        printf("%s %s %lld %lld %d %d %d %d %d %d %d\n", KERNELS[p.kernel], EPIS[p.epi], (long long)p.tiles_m, (long long)p.tiles_n, p.slices,
               p.stagger, p.nt_out, p.side_lds, p.fuse_split2, p.vec_ok, p.relu_a);
    }
    return 0;
}
