"""engine.attention_route: the one place that decides which pipeline an inference attention sub-layer runs.  No device, and the
library is not loaded: the function takes plain values.

The expected routes were worked by hand from the three copies of the choice this function replaced (engine.py of commit 5903ccd):
  R1  fused routes need bf16 operands                      self_attention l.682/686/693, cross_attention l.788/794/800
  R2  ... and head_dim 64; bf16 with another one raises    same lines; the raise: l.700-701, l.808-809, l.829-830
  R3  ... and no rope or the native one                    `native`, l.681 and l.787
  R4  ... and no qk_norm                                   folded into `native` at l.681; tested first at l.777
  R5  ... and value tokens that are the key tokens         l.777 (cross_attention only: self-attention has no separate values)
  R6  fp8 when attention_precision("fp8") outside autograd l.682, l.788 with _fp8_attention, l.129-130; it goes before R7
  R7  vt_pack when keys % 4 != 0 and VT_PACK_ODD           l.686, l.794 with VT_PACK_ODD, l.665
  R8  vt_epilogue otherwise                                l.693, l.800
"""
import pytest
import torch

from uniception_amd import engine
from uniception_amd._lib import UcHipError

BF16, F32 = torch.bfloat16, torch.float32


def route(dtype=BF16, head_dim=64, native_rope=True, qk_norm=False, separate_v=False, n_keys=1024):
    with torch.no_grad():
        return engine.attention_route(dtype, head_dim, native_rope, qk_norm, separate_v, n_keys)


def test_both_sides_of_every_rule():
    assert route() == "vt_epilogue"                                  # the fused side of R1-R5, the off side of R6 and R7: R8
    assert route(dtype=F32) == "unfused"                             # R1
    assert route(dtype=torch.float16) == "unfused"                   # R1: the test is for bf16, not for "a 16-bit type"
    assert route(dtype=F32, head_dim=48) == "unfused"                # R2: fp32 takes any head_dim
    assert route(native_rope=False) == "unfused"                     # R3
    assert route(qk_norm=True) == "unfused"                          # R4
    assert route(separate_v=True) == "unfused"                       # R5
    for n, want in ((1024, "vt_epilogue"), (196, "vt_epilogue"), (1370, "vt_pack"), (1369, "vt_pack"), (1371, "vt_pack")):
        assert route(n_keys=n) == want, n                            # R7 / R8
    saved = engine.VT_PACK_ODD
    try:
        engine.VT_PACK_ODD = False
        assert route(n_keys=1370) == "vt_epilogue"                   # R7: the switch
    finally:
        engine.VT_PACK_ODD = saved


def test_fp8_mode_is_asked_first_and_only_outside_autograd():
    with engine.attention_precision("fp8"):
        assert route() == "fp8"                                      # R6
        assert route(n_keys=1370) == "fp8"                           # R6 before R7
        with torch.enable_grad():
            assert engine.attention_route(BF16, 64, True, False, False, 1024) == "vt_epilogue"     # R6: inference only
        # the mode changes nothing for what the fused routes do not carry
        assert route(dtype=F32) == route(qk_norm=True) == route(separate_v=True) == route(native_rope=False) == "unfused"
    assert route() == "vt_epilogue"


def test_bf16_needs_head_dim_64_whatever_else_is_asked():
    for kw in ({}, {"qk_norm": True}, {"separate_v": True}, {"native_rope": False}, {"n_keys": 1370}):
        with pytest.raises(UcHipError, match=r"bf16 attention needs head_dim 64 \(got 32\)"):
            route(head_dim=32, **kw)
    with engine.attention_precision("fp8"), pytest.raises(UcHipError, match="bf16 attention needs head_dim 64"):
        route(head_dim=128)


def test_routes_of_the_bench_legs():
    # ViT-L/16 encoder at 512 x 512: 1024 tokens, 16 heads of 64, native RoPE-2D, bf16
    assert route(BF16, 1024 // 16, True, False, False, 1024) == "vt_epilogue"
    # decoder cross-attention on the other view's 1024 tokens: width 768, 12 heads of 64, keys = values
    assert route(BF16, 768 // 12, True, False, False, 1024) == "vt_epilogue"
    # --encoder dinov2 (ViT-L/14 at 518 x 518): 37 * 37 + 1 = 1370 tokens, no rope (learned positions)
    assert route(BF16, 1024 // 16, True, False, False, 37 * 37 + 1) == "vt_pack"
    # --img 1024 --attention fp8: 4096 tokens
    with engine.attention_precision("fp8"):
        assert route(BF16, 64, True, False, False, 4096) == "fp8"
        assert route(BF16, 768 // 12, True, False, False, 4096) == "fp8"
    # precision("bf16x3"): fp32 tensors — the rotation and both products ride in the split-operand attention of the unfused route
    with engine.precision("bf16x3"):
        assert engine.compute_dtype() == F32
        assert route(engine.compute_dtype(), 64, True, False, False, 1024) == "unfused"
