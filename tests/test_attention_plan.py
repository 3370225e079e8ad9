"""CPU: the attention routing (uniception_amd/csrc/attention_plan.h) — whether a forward or backward launch is served and which
kernel, grid and workgroup size it gets.

tests/attention_plan_driver.cpp is compiled with the system C++ compiler against the host-only header (tests/attention_routes.py
build_driver) and fed one descriptor + knob snapshot per line.  Expected plans: `refused <reason>`, or forward
`kernel grid_x grid_y grid_z block nqt fixup_grid`, backward `dq dq_grid dkv dkv_grid`, as the routing had them when it was written
inline in uc_attention_fwd, attention_bwd_impl and attention_bwd_f32_impl (head_dim <= 64) and in the head_dim > 64 entry functions;
the bench rows agree with the kernel traces of the bench configurations.  O is an integer address: 4096 is 256-byte aligned, 4104
8-byte aligned."""
import json
import os

import pytest

from tests import attention_routes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every distinct bf16 attention launch of the bench configurations, recorded from their ABI calls: {config: [[row, expected plan], ...]}
with open(os.path.join(ROOT, "tests", "golden", "attention_plan_bench.json")) as _f:
    BENCH = json.load(_f)
F32, BF16 = 0, 1


def fwd(B, H, Nq, Nk=None, dtype=BF16, D=64, **kw):
    """q / k / O as contiguous [B, N, H, D], V packed (bf16) or row-major (fp32) like k"""
    Nk = Nq if Nk is None else Nk
    row = dict(fn="fwd", dtype=dtype, v_layout=1 if dtype == BF16 else 0, B=B, H=H, Nq=Nq, Nk=Nk, D=D,
               q_sb=Nq * H * D, q_sn=H * D, q_sh=D, k_sb=Nk * H * D, k_sn=H * D, k_sh=D, o_sb=Nq * H * D, o_sn=H * D, o_sh=D, O=4096)
    if dtype == F32:
        row.update(v_sb=Nk * H * D, v_sn=H * D, v_sh=D)
    row.update(kw)
    return row


def bwd(B, H, Nq, Nk=None, **kw):
    """q / O / dO as contiguous [B, Nq, H, 64], k / v as contiguous [B, Nk, H, 64]; bf16 unless dtype / D say otherwise"""
    Nk = Nq if Nk is None else Nk
    row = dict(fn="bwd", B=B, H=H, Nq=Nq, Nk=Nk, q_sb=Nq * H * 64, q_sn=H * 64, q_sh=64, k_sb=Nk * H * 64, k_sn=H * 64, k_sh=64,
               v_sb=Nk * H * 64, v_sn=H * 64, v_sh=64, o_sb=Nq * H * 64, o_sn=H * 64, o_sh=64)
    row.update(kw)
    return row


# one row on each side of every rule
FWD_RULES = {
 # persistent kernel: policy items (>= 512, or >= 256 at >= 4096 keys), the waste of the last 256-query tile, its grids
 "p64_headline": (fwd(128, 16, 1024), "p64 512 1 1 256 4 128"),
 "p64_items_512": (fwd(8, 16, 1024), "p64 512 1 1 256 4 8"),
 "p64_items_448": (fwd(7, 16, 1024), "dma4 896 1 1 256 8 0"),
 "p64_items_256_keys_4096": (fwd(1, 16, 4096), "p64 256 1 1 256 32 4"),
 "p64_items_256_keys_4032": (fwd(1, 16, 4096, 4032), "dma4 512 1 1 256 32 0"),
 "p64_tail_ragged_keys": (fwd(32, 16, 1370), "p64_tail 512 1 1 256 11 44"),
 "p64_waste_quarter_ok": (fwd(64, 16, 640), "p64 512 1 1 256 5 40"),
 "p64_waste_quarter_over": (fwd(64, 16, 600), "dma4 5120 1 1 256 5 0"),
 "p64_knob0": (fwd(128, 16, 1024, p64=0), "dma8 8192 1 1 512 4 0"),
 "p64_knob2_small": (fwd(2, 16, 1024, p64=2), "p64 128 1 1 256 8 2"),
 "p64_knob2_one_key_tile": (fwd(2, 16, 1024, 64, p64=2), "dma4 256 1 1 256 8 0"),
 "p64_knob2_tail": (fwd(2, 16, 1024, 65, p64=2), "p64_tail 128 1 1 256 8 2"),
 "p64_q_offset_32bit": (fwd(128, 16, 1024, q_sn=16777216 - 8), "p64 512 1 1 256 4 128"),
 "p64_q_offset_over": (fwd(128, 16, 1024, q_sn=16777216), "dma8 8192 1 1 512 4 0"),
 "p64_o_offset_over": (fwd(128, 16, 1024, o_sn=16777216), "dma8 8192 1 1 512 4 0"),
 "p64_items_below_2p28": (fwd(65535, 4096, 128, p64=2), "p64 512 1 1 256 1 256"),
 "p64_items_2p28": (fwd(65535, 4097, 128, p64=2), "dma4 268496895 1 1 256 1 0"),
 # role split: vetoes the persistent kernel, eight-wave launches only
 "role_split_eight_wave": (fwd(128, 16, 1024, role_split=1), "rs8 8192 1 1 512 4 0"),
 "role_split_four_wave": (fwd(2, 16, 1024, role_split=1), "dma4 256 1 1 256 8 0"),
 # eight / four waves: 256-query tiles only where every CU gets two workgroups and the last tile is not mostly empty
 "few8_default_cus": (fwd(4, 16, 1024), "dma4 512 1 1 256 8 0"),
 "few8_128_cus": (fwd(4, 16, 1024, cus=128), "dma8 256 1 1 512 4 0"),
 "waste8_equal": (fwd(64, 16, 1200, p64=0), "dma8 5120 1 1 512 5 0"),
 "waste8_over": (fwd(64, 16, 1100, p64=0), "dma4 9216 1 1 256 9 0"),
 "nq_below_256": (fwd(256, 16, 196), "dma4 8192 1 1 256 2 0"),
 # persistent grids: 2 per CU in groups of 8, at least 8; fix-up at most one workgroup per CU
 "p64_cus_128": (fwd(128, 16, 1024, cus=128), "p64 256 1 1 256 4 128"),
 "p64_cus_80": (fwd(128, 16, 1024, cus=80), "p64 160 1 1 256 4 80"),
 "p64_cus_2": (fwd(128, 16, 1024, cus=2), "p64 8 1 1 256 4 2"),
 # LDS-DMA eligibility: the register-staged kernel takes the rest
 "dma_o_misaligned": (fwd(128, 16, 1024, O=4104), "reg128 8 16 128 256 4 0"),
 "dma_o_strides_4": (fwd(2, 3, 300, 260, o_sb=300 * 204, o_sn=204, o_sh=68), "reg128 3 3 2 256 3 0"),   # (test_ops_gpu.py)
 "dma_k_offset_32bit": (fwd(1, 1, 256, 65472, k_sn=16384, k_sb=65472 * 16384), "dma4 2 1 1 256 2 0"),
 "dma_k_offset_over": (fwd(1, 1, 256, 65536, k_sn=16384, k_sb=65536 * 16384), "reg128 2 1 1 256 2 0"),
 "dma_q_offset_over": (fwd(1, 1, 256, q_sn=33554432), "reg128 2 1 1 256 2 0"),
 "dma_vt_row_32bit": (fwd(1, 1, 128, 16777216 - 64, k_sn=8, k_sh=8, k_sb=0), "dma4 1 1 1 256 1 0"),
 "dma_vt_row_over": (fwd(1, 1, 128, 16777216, k_sn=8, k_sh=8, k_sb=0), "reg128 1 1 1 256 1 0"),
 "dma_grid_over": (fwd(65535, 65535, 128), "reg128 1 65535 65535 256 1 0"),
 # diag build: the four-wave DMA kernel wherever it may run
 "dbg": (fwd(128, 16, 1024, dbg=1), "dma4_dbg 16384 1 1 256 8 0"),
 "dbg_o_misaligned": (fwd(128, 16, 1024, dbg=2, O=4104), "reg128 8 16 128 256 8 0"),
 # dropout and fp32
 "drop_bf16": (fwd(128, 16, 1024, drop=1), "reg128_drop 8 16 128 256 0 0"),
 "f32_d32": (fwd(2, 4, 300, dtype=F32, D=32), "f32_32 3 4 2 128 0 0"),
 "f32_d33": (fwd(2, 4, 300, dtype=F32, D=33), "f32_64 3 4 2 128 0 0"),
 "f32_d32_drop": (fwd(2, 4, 300, dtype=F32, D=32, drop=1), "f32_32_drop 3 4 2 128 0 0"),
 "f32_d64_drop": (fwd(2, 4, 300, dtype=F32, drop=1), "f32_64_drop 3 4 2 128 0 0"),
 # the served set.  fp32: every head_dim up to 96, the DMAX 96 instantiation above 64
 "f32_d64": (fwd(2, 4, 300, dtype=F32, D=64), "f32_64 3 4 2 128 0 0"),
 "f32_d65": (fwd(2, 4, 300, dtype=F32, D=65), "f32_96 3 4 2 128 0 0"),
 "f32_d96": (fwd(2, 4, 300, dtype=F32, D=96), "f32_96 3 4 2 128 0 0"),
 "f32_d97": (fwd(2, 4, 300, dtype=F32, D=97), "refused f32_head_dim"),
 # bf16: head_dim 64, 80 or 96; 80 / 96 take one workgroup per 128 queries of a (batch, head)
 "bf16_d64": (fwd(2, 4, 300), "dma4 24 1 1 256 3 0"),
 "bf16_d72": (fwd(2, 4, 300, D=72), "refused bf16_head_dim"),
 "bf16_d80": (fwd(2, 4, 300, D=80), "bf16_80 3 4 2 256 0 0"),
 "bf16_d96": (fwd(2, 4, 300, D=96), "bf16_96 3 4 2 256 0 0"),
 "bf16_d112": (fwd(2, 4, 300, D=112), "refused bf16_head_dim"),
 "dtype_f16": (fwd(2, 4, 300, dtype=2), "refused dtype"),
 # dropout: head_dim <= 64 only (served: drop_bf16, f32_d64_drop above)
 "drop_bf16_d80": (fwd(2, 4, 300, D=80, drop=1), "refused dropout"),
 "drop_f32_d80": (fwd(2, 4, 300, dtype=F32, D=80, drop=1), "refused dropout"),
 # the head_dim > 64 plans read no knob
 "bf16_d80_knobs_ignored": (fwd(2, 4, 300, D=80, p64=2, bwd64=2, role_split=1, cus=8), "bf16_80 3 4 2 256 0 0"),
}
BWD_RULES = {
 "train_step": (bwd(64, 16, 1024), "dq64 256 dkv64 256"),
 "mostly_real_over": (bwd(2, 16, 300), "dq32 96 dkv32 96"),
 "mostly_real_384": (bwd(2, 16, 384), "dq64 64 dkv64 64"),
 "dq64_dkv32": (bwd(2, 16, 1024, 300), "dq64 128 dkv32 96"),
 "knob0": (bwd(64, 16, 1024, bwd64=0), "dq32 8192 dkv32 8192"),
 "knob2_small": (bwd(2, 16, 100, bwd64=2), "dq64 32 dkv64 32"),
 "knob2_one_tile": (bwd(2, 16, 64, bwd64=2), "dq32 32 dkv32 32"),
 "cus_128": (bwd(64, 16, 1024, cus=128), "dq64 128 dkv64 128"),
 "cus_100": (bwd(64, 16, 1024, cus=100), "dq64 96 dkv64 96"),
 # query rows past Nq must be followed by the next batch's rows (not by a gap of foreign memory)
 "rows_follow_q_gap": (bwd(2, 16, 1024, q_sb=1025 * 1024), "dq64 128 dkv32 256"),
 "rows_follow_o_gap": (bwd(2, 16, 1024, o_sb=1025 * 1024), "dq64 128 dkv32 256"),
 "rows_follow_one_batch": (bwd(1, 16, 1024, q_sb=1025 * 1024, o_sb=1025 * 1024), "dq64 64 dkv64 64"),
 # 32-bit byte offsets of the persistent kernels' descriptors
 "fits32_q": (bwd(1, 16, 1024, q_sn=2097152, q_sb=1024 * 2097152), "dq64 64 dkv64 64"),
 "fits32_q_over": (bwd(1, 16, 1025, 1024, q_sn=2097152, q_sb=1025 * 2097152), "dq64 80 dkv32 128"),
 "fits32_o_over": (bwd(1, 16, 1025, 1024, o_sn=2097152, o_sb=1025 * 2097152), "dq64 80 dkv32 128"),
 "fits32_scratch": (bwd(1, 65535, 8192, 256, q_sn=8, q_sh=8, o_sn=8, o_sh=8), "dq64 256 dkv64 256"),
 "fits32_scratch_over": (bwd(1, 65535, 8320, 256, q_sn=8, q_sh=8, o_sn=8, o_sh=8), "dq64 256 dkv32 131070"),
 "v_ext_over": (bwd(1, 16, 1024, 1025, v_sn=2097152, v_sb=1025 * 2097152), "dq32 128 dkv64 80"),
 "drop": (bwd(64, 16, 1024, drop=1), "dq32_drop 8192 dkv32_drop 8192"),
 # fp32: one workgroup of 128 rows per (row tile, head, batch), the head_dim <= 32 or <= 64 instantiation, the delta pass first
 "f32_d32": (bwd(2, 4, 300, 200, dtype=F32, D=32), "f32_dq32 3,4,2 f32_dkv32 2,4,2 128 10"),
 "f32_d33": (bwd(2, 4, 300, 200, dtype=F32, D=33), "f32_dq64 3,4,2 f32_dkv64 2,4,2 128 10"),
 "f32_d64_drop": (bwd(2, 4, 300, 200, dtype=F32, drop=1), "f32_dq64 3,4,2 f32_dkv64 2,4,2 128 10"),
 "f32_knobs_ignored": (bwd(1, 1, 1, 129, dtype=F32, D=1, bwd64=2, cus=8), "f32_dq32 1,1,1 f32_dkv32 2,1,1 128 1"),
 # the served set.  fp32: every head_dim up to 96, the DMAX 96 instantiations above 64
 "f32_d64": (bwd(2, 4, 300, 200, dtype=F32, D=64), "f32_dq64 3,4,2 f32_dkv64 2,4,2 128 10"),
 "f32_d65": (bwd(2, 4, 300, 200, dtype=F32, D=65), "f32_dq96 3,4,2 f32_dkv96 2,4,2 128 10"),
 "f32_d96": (bwd(2, 4, 300, 200, dtype=F32, D=96), "f32_dq96 3,4,2 f32_dkv96 2,4,2 128 10"),
 "f32_d97": (bwd(2, 4, 300, 200, dtype=F32, D=97), "refused f32_head_dim"),
 # bf16: head_dim 64, 80 or 96; 80 / 96 take one workgroup per 128 queries / keys of a (batch, head) from 1-D grids
 "bf16_d64": (bwd(2, 4, 300, 200, D=64), "dq32 24 dkv64 8"),      # (200 keys: a 256-key workgroup is mostly real)
 "bf16_d72": (bwd(2, 4, 300, 200, D=72), "refused bf16_head_dim"),
 "bf16_d80": (bwd(2, 4, 300, 200, D=80), "dq80 24 dkv80 16"),
 "bf16_d96": (bwd(2, 4, 300, 200, D=96), "dq96 24 dkv96 16"),
 "bf16_d112": (bwd(2, 4, 300, 200, D=112), "refused bf16_head_dim"),
 "dtype_f16": (bwd(2, 4, 300, 200, dtype=2), "refused dtype"),
 # dropout: head_dim <= 64 only (served: drop, f32_d64_drop above)
 "drop_bf16_d80": (bwd(2, 4, 300, 200, D=80, drop=1), "refused dropout"),
 "drop_f32_d80": (bwd(2, 4, 300, 200, dtype=F32, D=80, drop=1), "refused dropout"),
 # RoPE positions (the inverse rotation in the kernels' epilogues): bf16 at head_dim 64 only, and no other routing
 "rope_bf16_d64": (bwd(64, 16, 1024, rope=1), "dq64 256 dkv64 256"),
 "rope_bf16_d96": (bwd(2, 4, 300, 200, D=96, rope=1), "refused rope_head_dim"),
 "rope_f32_d64": (bwd(2, 4, 300, 200, dtype=F32, D=64, rope=1), "refused rope_f32"),
 # bf16: ceil(Nq / 128) H B and ceil(Nk / 128) H B fit a 1-D grid (65535 x 32768 = 2^31 - 32768)
 "grid_below_2p31": (bwd(65535, 32768, 128, bwd64=0), "dq32 2147450880 dkv32 2147450880"),
 "grid_2p31_queries": (bwd(65535, 32769, 128, bwd64=0), "refused bwd_grid"),
 "grid_2p31_keys": (bwd(65535, 16385, 128, 256, bwd64=0), "refused bwd_grid"),
 "grid_below_2p31_d80": (bwd(65535, 32768, 128, D=80), "dq80 2147450880 dkv80 2147450880"),
 "grid_2p31_d80": (bwd(65535, 32769, 128, D=80), "refused bwd_grid"),
 "grid_f32_no_limit": (bwd(65535, 32769, 128, dtype=F32, D=32), "f32_dq32 1,32769,65535 f32_dkv32 1,32769,65535 128 1073758208"),
 # the head_dim > 64 plans read no knob
 "bf16_d80_knobs_ignored": (bwd(2, 4, 300, 200, D=80, p64=2, bwd64=2, role_split=1, cus=8), "dq80 24 dkv80 16"),
}


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return attention_routes.build_driver(tmp_path_factory.mktemp("attention_plan"))


def check(plan, cases):
    got = plan([row for row, _ in cases.values()])
    wrong = {name: (want, g) for (name, (_, want)), g in zip(cases.items(), got) if g != want}
    assert not wrong, "\n".join(f"{n}: want {w!r}, got {g!r}" for n, (w, g) in wrong.items())


def test_forward_rules_on_both_sides(plan):
    check(plan, FWD_RULES)


def test_backward_rules_on_both_sides(plan):
    check(plan, BWD_RULES)


def test_header_is_pure():
    """no HIP header and no environment: the knobs come in as a snapshot"""
    with open(os.path.join(ROOT, "uniception_amd", "csrc", "attention_plan.h")) as f:
        src = f.read()
    assert "hip_runtime" not in src and "getenv" not in src and "g_uc_" not in src


@pytest.mark.parametrize("config", sorted(BENCH))
def test_bench_launches(plan, config):
    """Every distinct attention launch of the bench configurations (the forward at 512^2 with 128 pairs, the batch sweep's 1 - 16
    pairs, 224^2 at 64 / 256 pairs, DINOv2-518 at 32 pairs, 1024^2 at 8 pairs, the training step at 64 pairs): the persistent kernel
    at 512^2 (+ its ragged form at 518^2), the four-wave DMA kernel at 224^2 and at small batches, the 64-row backward kernels."""
    check(plan, {f"{config}[{i}]": tuple(case) for i, case in enumerate(BENCH[config])})
