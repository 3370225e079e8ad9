"""CPU: uc_gemm's routing (uniception_amd/csrc/gemm_plan.h) — which kernel, epilogue family, grid and launch options a launch gets.

tests/gemm_plan_driver.cpp is compiled with the system C++ compiler against the host-only header and fed one descriptor + knob
snapshot per line.  Expected plans: `kernel epi tiles_m tiles_n slices stagger nt_out side_lds fuse_split2 vec_ok relu_a`, as the
routing had them when it was spread over uc_gemm and the family launchers; the bench rows agree with the forward's kernel trace.
Pointers are integer addresses: 4096 is 256-byte aligned, 4100 / 4104 are 4- / 8-byte aligned."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every distinct uc_gemm launch of the bench configurations, recorded from bench.py: {config: [[descriptor row, expected plan], ...]}
with open(os.path.join(ROOT, "tests", "golden", "gemm_plan_bench.json")) as _f:
    BENCH = json.load(_f)
BF16, F16, F32 = 1, 2, 0
BF = BF16


def dense(M, N, K, cd=BF16, out=BF16, **kw):
    row = dict(compute_dtype=cd, M=M, N=N, K=K, lda=K, ldc=N, out_dtype=out, A=4096, W=4096, C=4096)
    row.update(kw)
    return row


def conv(B, H, W, Cin, N, cd=BF16, out=BF16, **kw):
    row = dict(compute_dtype=cd, a_mode=1, conv_B=B, conv_H=H, conv_W=W, conv_Cin=Cin, conv_stride=1, N=N, ldc=N, out_dtype=out,
               A=4096, W=4096, C=4096)
    row.update(kw)
    return row


# one row on each side of every rule
RULES = {
 # tile heuristic: rounds x cost, waste-256, co-resident
 "dense_cost_256x256_f16": (dense(262144, 3072, 1024, cd=F16, out=F16),
     "t256x256 all 1024 12 1 -1 7 0 0 1 0"),
 "dense_cost_256x256_eight_wave": (dense(16384, 1024, 1024, act=1),
     "eight_wave bf16 64 4 1 -1 0 0 0 1 0"),
 "dense_cost_256x128": (dense(8192, 1024, 1024, act=1),
     "t256x128_s3 bf16 32 8 1 -1 0 0 0 1 0"),
 "dense_cost_128x128": (dense(4096, 1024, 1024, act=1),
     "t128x128_s3 bf16 32 8 1 -1 0 0 0 1 0"),
 "dense_waste256_coresident": (dense(262144, 384, 1024, act=1),
     "t256x128_bk32 bf16 1024 3 1 -1 7 0 0 1 0"),
 "dense_coresident_off": (dense(65536, 128, 1024, act=1),
     "t256x128_s3 bf16 256 1 1 -1 0 0 0 1 0"),
 "dense_coresident_on": (dense(131072, 128, 1024, act=1),
     "t256x128_bk32 bf16 512 1 1 -1 0 0 0 1 0"),
 # eight-wave / four-wave upgrades
 "bf16_fam_eight_wave": (dense(262144, 3072, 1024),
     "eight_wave bf16 1024 12 1 -1 7 0 0 1 0"),
 "bf16_fam_eight_wave_m_odd": (dense(262148 - 2, 3072, 1024),
     "t256x256 bf16 1025 12 1 -1 7 0 0 1 0"),
 "bf16_fam_four_wave": (dense(262144, 1024, 4096),
     "four_wave bf16 1024 4 1 -1 7 0 0 1 0"),
 "bf16_fam_four_wave_k_below": (dense(262144, 1024, 1984),
     "eight_wave bf16 1024 4 1 -1 7 0 0 1 0"),
 "f32_fam_four_wave_stagger": (dense(262144, 1024, 4096, out=F32, residual=4096, res_dtype=F32, ldr=1024),
     "four_wave f32 1024 4 1 150 7 0 0 1 0"),
 "f32_fam_stagger_below": (dense(16384, 1024, 1024, out=F32, residual=4096, res_dtype=F32, ldr=1024),
     "t256x256 f32 64 4 1 0 0 0 0 1 0"),
 "f32_fam_stagger_knob": (dense(262144, 1024, 4096, out=F32, residual=4096, res_dtype=F32, ldr=1024, gemm_stagger=300),
     "four_wave f32 1024 4 1 300 7 0 0 1 0"),
 "bs_fam": (dense(262144, 1024, 4096, residual=4096, res_dtype=BF, ldr=1024, stats_out=4096),
     "four_wave bs 1024 4 1 0 7 0 0 1 0"),
 "bs_fam_four1": (dense(262144, 1024, 4096, residual=4096, res_dtype=BF, ldr=1024, gemm_4wave=1),
     "t256x256 bs 1024 4 1 0 7 0 0 1 0"),
 "bs_fam_four2": (dense(262144, 1024, 4096, residual=4096, res_dtype=BF, ldr=1024, gemm_4wave=2),
     "four_wave bs 1024 4 1 0 7 0 0 1 0"),
 "bf16_fam_four0": (dense(262144, 1024, 4096, gemm_4wave=0),
     "eight_wave bf16 1024 4 1 -1 7 0 0 1 0"),
 "all_fam_four1": (dense(262144, 1024, 4096, act=1, residual=4096, res_dtype=F32, ldr=1024, gemm_4wave=1),
     "t256x256 all 1024 4 1 -1 7 0 0 1 0"),
 "all_fam_four3": (dense(262144, 1024, 4096, act=1, residual=4096, res_dtype=F32, ldr=1024),
     "four_wave all 1024 4 1 -1 7 0 0 1 0"),
 "vec_misaligned": (dense(262144, 3072, 1024, C=4104),
     "t256x256 all 1024 12 1 -1 7 0 0 0 0"),
 "side_lds": (dense(262144, 3072, 1024, ln_stats=4096, ln_colsum=4096, bias=4096),
     "eight_wave bf16 1024 12 1 -1 7 1 0 1 0"),
 "side_lds_partial": (dense(262144, 3072, 1024, ln_stats=4096, ln_colsum=4096, bias=4096, ln_nblk=16, ln_eps=1e-6),
     "eight_wave bf16 1024 12 1 -1 7 0 0 1 0"),
 "side_lds_stats_align8": (dense(262144, 3072, 1024, ln_stats=4104, ln_colsum=4096, bias=4096),
     "eight_wave bf16 1024 12 1 -1 7 0 0 1 0"),
 "nt_out_below": (dense(65536, 1024, 1024),
     "eight_wave bf16 256 4 1 -1 0 0 0 1 0"),
 # small-M in-kernel split
 "small_m_split": (dense(2048, 1024, 4096, fuse_ws=4096),
     "t128x128_s3 bf16 16 8 2 -1 0 0 1 1 0"),
 "small_m_no_ws": (dense(2048, 1024, 4096),
     "t128x128_s3 bf16 16 8 1 -1 0 0 0 1 0"),
 "small_m_knob0": (dense(2048, 1024, 4096, fuse_ws=4096, small_m_split=0),
     "t128x128_s3 bf16 16 8 1 -1 0 0 0 1 0"),
 "small_m_k_below": (dense(2048, 1024, 1024, fuse_ws=4096),
     "t128x128_s3 bf16 16 8 1 -1 0 0 0 1 0"),
 "small_m_too_many_tiles": (dense(4096, 1024, 4096, fuse_ws=4096),
     "t128x128_s3 bf16 32 8 1 -1 0 0 0 1 0"),
 "small_m_forced_0": (dense(2048, 1024, 4096, fuse_ws=4096, gemm_variant=0),
     "t128x128_s3 bf16 16 8 1 -1 0 0 0 1 0"),
 "small_m_cus": (dense(2048, 1024, 4096, fuse_ws=4096, cus=128),
     "t128x128_s3 bf16 16 8 1 -1 0 0 0 1 0"),
 # training forms
 "train_preact": (dense(131072, 4096, 1024, act=1, preact_out=4096, bias=4096),
     "t256x256 all 512 16 1 -1 7 0 0 1 0"),
 "train_dact_u": (dense(131072, 1024, 4096, dact_u=4096, dact_act=1),
     "four_wave all 512 4 1 -1 7 0 0 1 0"),
 "train_split_k": (dense(1024, 4096, 131072, out=F32, split_k=16),
     "t256x256 all 4 16 16 -1 0 0 0 1 0"),
 # fp16 operands
 "f16_dense32": (dense(131072, 96, 96, cd=F16, out=F16),
     "t256x128_bk32 all 512 1 1 -1 0 0 0 1 0"),
 "f16_forced_6": (dense(262144, 3072, 1024, cd=F16, out=F16, gemm_variant=6),
     "t256x256 all 1024 12 1 -1 7 0 0 1 0"),
 "f16_forced_7": (dense(262144, 3072, 1024, cd=F16, out=F16, gemm_variant=7),
     "t256x256 all 1024 12 1 -1 7 0 0 1 0"),
 "f16_forced_4": (dense(262144, 3072, 1024, cd=F16, out=F16, gemm_variant=4),
     "t128x128_s2 all 2048 24 1 -1 7 0 0 1 0"),
 # register-staged and fp32 kernels
 "reg_forced": (dense(262144, 3072, 1024, gemm_variant=-1),
     "reg all 2048 24 1 0 0 0 0 0 0"),
 "reg_k_not_64": (dense(4096, 1024, 1000),
     "reg all 32 8 1 0 0 0 0 0 0"),
 "reg_relu_a": (dense(4096, 1024, 1024, relu_a=1),
     "reg all 32 8 1 0 0 0 0 0 1"),
 "fp32_vaLU": (dense(4096, 1024, 1000, cd=F32, out=F32),
     "f32 all 64 16 1 0 0 0 0 0 0"),
 # convolutions: row kernels
 "conv_rows8_seg": (conv(2, 256, 256, 256, 128),
     "conv_rows8 all 256 1 1 -1 0 0 0 1 0"),
 "conv_rows8_seg_relu": (conv(2, 256, 256, 256, 128, relu_a=1),
     "conv_rows8 all 256 1 1 -1 0 0 0 1 1"),
 "conv_rows8_too_few_tiles": (conv(1, 256, 256, 256, 128),
     "conv_rows all 256 1 1 -1 0 0 0 1 0"),
 "conv_rows8_forced_mode3": (conv(1, 256, 256, 256, 128, conv_rows=3),
     "conv_rows8 all 128 1 1 -1 0 0 0 1 0"),
 "conv_rows256_mode2": (conv(2, 256, 256, 256, 128, conv_rows=2),
     "conv_rows all 512 1 1 -1 0 0 0 1 0"),
 "conv_rows_off": (conv(2, 256, 256, 256, 128, conv_rows=0),
     "t256x128_bk32 all 512 1 1 -1 0 0 0 1 0"),
 "conv_rows8_flat_296": (conv(2, 296, 296, 128, 128),
     "conv_rows8_flat all 343 1 1 -1 0 0 0 1 0"),
 "conv_rows8_flat_off_296": (conv(2, 296, 296, 128, 128, conv_rows_flat=0),
     "t256x128_bk32 all 685 1 1 -1 0 0 0 1 0"),
 "conv_stride2": (conv(8, 256, 256, 256, 128, conv_stride=2),
     "t256x128_bk32 all 512 1 1 -1 0 0 0 1 0"),
 "conv_cin96": (conv(8, 128, 128, 96, 256),
     "t256x128_bk32 all 512 2 1 -1 0 0 0 1 0"),
 "conv_cin96_forced_2": (conv(8, 128, 128, 96, 256, gemm_variant=2),
     "t256x128_bk32 all 512 2 1 -1 0 0 0 1 0"),
 "conv_f16_rows8": (conv(2, 256, 256, 256, 128, cd=F16, out=F16),
     "conv_rows8 all 256 1 1 -1 0 0 0 1 0"),
 # convolutions: 16-bit residual family
 "conv_res16_rows8": (conv(8, 128, 128, 256, 256, residual=4096, res_dtype=BF, ldr=256),
     "conv_rows8 res16 256 2 1 -1 0 0 0 1 0"),
 "conv_res16_tile": (conv(8, 128, 128, 256, 256, residual=4096, res_dtype=BF, ldr=256, conv_rows=0),
     "t256x256 res16 512 1 1 -1 0 0 0 1 0"),
 "conv_res16_small": (conv(2, 128, 128, 256, 256, residual=4096, res_dtype=BF, ldr=256),
     "t256x128_s3 all 128 2 1 -1 0 0 0 1 0"),
 "conv_res16_rows256_wins": (conv(8, 128, 128, 256, 128, residual=4096, res_dtype=BF, ldr=128, conv_rows=2),
     "conv_rows all 512 1 1 -1 0 0 0 1 0"),
 "conv_res16_f16": (conv(8, 128, 128, 256, 256, cd=F16, out=F16, residual=4096, res_dtype=F16, ldr=256, conv_rows=0),
     "t256x256 res16 512 1 1 -1 0 0 0 1 0"),
 "conv_res16_f16_forced_7": (conv(8, 128, 128, 256, 256, cd=F16, out=F16, residual=4096, res_dtype=F16, ldr=256, conv_rows=0, gemm_variant=7),
     "t256x256 res16 512 1 1 -1 0 0 0 1 0"),
 "conv_res16_bf16_forced_7": (conv(8, 128, 128, 256, 256, residual=4096, res_dtype=BF, ldr=256, conv_rows=0, gemm_variant=7),
     "t256x256 all 512 1 1 -1 0 0 0 1 0"),
 "conv_cost_model_dense_only": (conv(2, 96, 96, 256, 256, conv_rows=0),
     "t128x128_s3 all 144 2 1 -1 0 0 0 1 0"),
 "conv_rows256_cin_below": (conv(1, 256, 256, 128, 128),
     "t256x128_s3 all 256 1 1 -1 0 0 0 1 0"),
 "conv_res16_rows256_n256": (conv(8, 128, 128, 256, 256, residual=4096, res_dtype=BF, ldr=256, conv_rows=2),
     "conv_rows all 512 2 1 -1 0 0 0 1 0"),
 # fused tail
 "conv_tail_forced_2": (conv(2, 128, 128, 128, 128, tail_out=4096, tail_w=4096, C=0, conv_rows=0, act=2, gemm_variant=2),
     "t256x128_s3 all 128 1 1 -1 0 0 0 0 0"),
 "conv_tail_forced_6": (conv(2, 128, 128, 128, 128, tail_out=4096, tail_w=4096, C=0, conv_rows=0, act=2, gemm_variant=6),
     "t256x128_s3 all 128 1 1 -1 0 0 0 0 0"),
 "conv_tail": (conv(8, 256, 256, 128, 128, tail_out=4096, tail_w=4096, C=0, conv_rows=0, act=2),
     "t256x128_bk32 all 2048 1 1 -1 0 0 0 0 0"),
 "conv_tail_rows8": (conv(8, 256, 256, 128, 128, tail_out=4096, tail_w=4096, C=0, act=2),
     "conv_rows8 all 1024 1 1 -1 0 0 0 0 0"),
}
FORCED = {   # every forced gemm_variant: no upgrades, no small-M split, no waste / co-resident rule
    0: ("t128x128_s2 bf16 2048 24 1 -1 7 0 0 1 0", "t128x128_s3 all 256 2 1 -1 0 0 0 1 0"),
    1: ("t256x128_s2 bf16 1024 24 1 -1 7 0 0 1 0", "t256x128_s3 all 128 2 1 -1 0 0 0 1 0"),
    2: ("t256x256 bf16 1024 12 1 -1 7 0 0 1 0", "t256x256 all 128 1 1 -1 0 0 0 1 0"),
    3: ("t256x128_bk32 bf16 1024 24 1 -1 7 0 0 1 0", "t256x128_bk32 all 128 2 1 -1 0 0 0 1 0"),
    4: ("t128x64 bf16 2048 48 1 -1 7 0 0 1 0", "t128x128_s3 all 256 2 1 -1 0 0 0 1 0"),
    6: ("eight_wave bf16 1024 12 1 -1 7 0 0 1 0", "t256x256 all 128 1 1 -1 0 0 0 1 0"),
    7: ("four_wave bf16 1024 12 1 -1 7 0 0 1 0", "t256x256 all 128 1 1 -1 0 0 0 1 0"),
}


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler is needed to build tests/gemm_plan_driver.cpp"
    exe = str(tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "uniception_amd", "csrc"), os.path.join(ROOT, "tests", "gemm_plan_driver.cpp"), "-o", exe])

    def run(rows):
        lines = [" ".join(f"{k}={v}" for k, v in row.items()) for row in rows]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(rows)
        return out
    return run


def check(plan, cases):
    got = plan([row for row, _ in cases.values()])
    wrong = {name: (want, g) for (name, (_, want)), g in zip(cases.items(), got) if g != want}
    assert not wrong, "\n".join(f"{n}: want {w!r}, got {g!r}" for n, (w, g) in wrong.items())


def test_every_rule_on_both_sides(plan):
    check(plan, RULES)


def test_forced_variants(plan):
    cases = {}
    for v, (want_dense, want_conv) in FORCED.items():
        cases[f"dense {v}"] = (dense(262144, 3072, 1024, gemm_variant=v), want_dense)
        cases[f"conv {v}"] = (conv(2, 128, 128, 256, 256, gemm_variant=v, conv_rows=0), want_conv)
    check(plan, cases)


@pytest.mark.parametrize("config", sorted(BENCH))
def test_bench_launches(plan, config):
    """Every distinct uc_gemm launch of the bench configurations (default forward: ViT-L/16 + 12-block decoder + DPT heads at
    512^2, 128 pairs; the batch sweep's 2 / 4 / 16 pairs; the 224^2 linear head; the training step)."""
    check(plan, {f"{config}[{i}]": case for i, case in enumerate(BENCH[config])})
