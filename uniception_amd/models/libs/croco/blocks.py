"""CroCo encoder blocks (reference: libs/croco/blocks.py:37-161) on the HIP kernel library.

The nn.Linear / nn.LayerNorm children are parameter containers (identical state_dict keys, shapes and init);
`forward` never calls them — it hands their weights to the fused pipelines in uniception_amd.engine:
    LN -> [QKV GEMM + bias + RoPE-2D + V-transpose epilogue] -> flash attention -> [proj GEMM + bias + residual]
    LN -> [fc1 GEMM + bias + erf-GELU] -> [fc2 GEMM + bias + residual]
"""
import collections.abc
from itertools import repeat

import torch
import torch.nn as nn

from .... import autograd, engine
from ...utils import sublayers
from ...utils.config import use_fused_attn
from ...utils.sublayers import as_dt

use_torch_attn = use_fused_attn()


def _ntuple(n):
    def parse(x):
        if isinstance(x, collections.abc.Iterable) and not isinstance(x, str):
            return x
        return tuple(repeat(x, n))

    return parse


to_2tuple = _ntuple(2)


class DropPath(nn.Module):
    """Stochastic depth; identity in eval / at rate 0, which is all the HIP inference path supports."""

    def __init__(self, drop_prob: float = 0.0, scale_by_keep: bool = True):
        super().__init__()
        self.drop_prob = drop_prob
        self.scale_by_keep = scale_by_keep

    def forward(self, x):
        if self.drop_prob == 0.0 or not self.training:
            return x
        # (in training the blocks apply it inside their sub-layer Functions: autograd.make_drops / uc_mask_scale)
        raise engine.UcHipError("DropPath with drop_prob > 0 is applied by the blocks' training path; called on its own (or without "
                                "gradients in train mode) it has no HIP form")

    def extra_repr(self):
        return f"drop_prob={round(self.drop_prob, 3):0.3f}"


def _as_2d(x):
    B, N, C = x.shape
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise engine.UcHipError(f"token dtype {x.dtype} not supported (fp32 or bf16)")
    return engine.carry_ln(x, x.reshape(B * N, C)) if x.is_contiguous() else x.contiguous().view(B * N, C)


class Mlp(nn.Module):
    """fc1 -> act -> fc2 (blocks.py:64-86)."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, bias=True, drop=0.0):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        bias = to_2tuple(bias)
        drop_probs = to_2tuple(drop)
        self.fc1 = nn.Linear(in_features, hidden_features, bias=bias[0])
        self.act = act_layer()
        self.drop1 = nn.Dropout(drop_probs[0])
        self.fc2 = nn.Linear(hidden_features, out_features, bias=bias[1])
        self.drop2 = nn.Dropout(drop_probs[1])

    def forward(self, x):
        engine.require_inference(x, self.fc1.weight)
        sublayers.refuse_drops(self.training, False, self.drop1.p, self.drop2.p)
        dt = engine.compute_dtype()
        shp = x.shape
        h = as_dt(x.reshape(-1, shp[-1]).contiguous(), dt)
        return engine.mlp(h, self.fc1, self.fc2, engine.act_name(self.act), None, dt).view(*shp[:-1], -1)


class Attention(nn.Module):
    """MHSA with RoPE on q,k (blocks.py:89-130)."""

    def __init__(self, dim, rope=None, num_heads=8, qkv_bias=False, attn_drop=0.0, proj_drop=0.0, torch_attn=use_torch_attn):
        super().__init__()
        self.num_heads = num_heads
        head_dim = dim // num_heads
        self.scale = head_dim**-0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        self.rope = rope
        self.torch_attn = torch_attn
        self.dropout_p = attn_drop

    def forward(self, x, xpos):
        engine.require_inference(x, self.qkv.weight)
        sublayers.refuse_drops(self.training, False, self.dropout_p, self.proj_drop.p)
        B, N, C = x.shape
        dt = engine.compute_dtype()
        return engine.self_attention(as_dt(_as_2d(x), dt), B, N, self.qkv, self.proj, self.num_heads, self.rope, xpos, self.scale,
                                     None, dt).view(B, N, C)


class Block(nn.Module):
    """x += attn(norm1(x)); x += mlp(norm2(x)) (blocks.py:133-161)."""

    def __init__(self, dim, num_heads, mlp_ratio=4.0, qkv_bias=False, drop=0.0, attn_drop=0.0, drop_path=0.0,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm, rope=None):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, rope=rope, num_heads=num_heads, qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=drop)
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.norm2 = norm_layer(dim)
        mlp_hidden_dim = int(dim * mlp_ratio)
        self.mlp = Mlp(in_features=dim, hidden_features=mlp_hidden_dim, act_layer=act_layer, drop=drop)

    def forward_tokens(self, x2d, B, N, xpos, dt):
        """[B*N, C] residual stream in, new residual stream out (same dtype)."""
        sa, mlp, training = self.attn, self.mlp, self.training
        train = autograd.grad_needed(x2d, *self.parameters())
        # the masks, in this block's generator order: the attention kernels' seed, proj_drop + DropPath, the Mlp's drops + DropPath
        ad = sublayers.attn_drop_for(training, train, sa.dropout_p)
        d1 = sublayers.drops_for(training, train, x2d, B, N, sa.proj_drop.p, self.drop_path)
        d2 = sublayers.drops_for(training, train, x2d, B, N, mlp.drop2.p, self.drop_path, mlp.drop1.p, mlp.fc1.out_features)
        x2d = sublayers.self_attn(x2d, self.norm1, sa.qkv, sa.proj, B, N, sa.num_heads, sa.rope, xpos, sa.scale, dt, train=train,
                                  drops=d1, attn_drop=ad)
        return sublayers.mlp(x2d, self.norm2, mlp.fc1, mlp.fc2, mlp.act, dt, train=train, drops=d2)

    def forward(self, x, xpos):
        B, N, C = x.shape
        return self.forward_tokens(_as_2d(x), B, N, xpos, engine.compute_dtype()).view(B, N, C)
