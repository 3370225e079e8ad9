"""Decoder transformer blocks (reference: utils/transformer_blocks.py:38-89, 136-412, 517-647) on the HIP kernels.

CrossAttentionBlock.forward(x, y, xpos, ypos):
    x += proj(SDPA(rope(q), rope(k), v))              q,k,v = qkv(norm1(x))
    x += proj(SDPA(rope(projq(norm2(x)), xpos), rope(projk(norm_y(y)), ypos), projv(norm_y(y))))
    x += fc2(gelu(fc1(norm3(x))))
Each line is: LayerNorm kernel -> GEMM(s) with fused bias/RoPE/VT epilogues -> flash attention ->
GEMM with fused bias+residual.  K and V of the other view share one GEMM (weights concatenated once).
"""
import math
from typing import Callable, Optional

import torch
import torch.nn as nn

from ... import autograd, engine
from ..libs.croco.blocks import DropPath, Mlp, _as_2d, to_2tuple  # noqa: F401
from . import sublayers
from .config import use_fused_attn
from .sublayers import as_dt


def _std_mlp(mlp):
    if not isinstance(mlp, Mlp):
        raise engine.UcHipError("only the standard Mlp layer has a fused HIP pipeline")
    return mlp


def _softmax_scale_multiplier(module, n_tokens: int) -> float:
    """The reference's optional q-scalings are scalar multipliers of q, i.e. of the softmax scale
    (transformer_blocks.py:231-241, 360-370)."""
    m = 1.0
    if module.use_scalable_softmax:
        m *= math.log(n_tokens)
    if module.use_entropy_scaling:
        m *= math.sqrt(module.entropy_scaling_growth_factor * math.log(n_tokens)
                       / math.log(module.base_token_count_for_entropy_scaling))
    return m


class Attention(nn.Module):
    "Self-Attention Layer"

    def __init__(self, dim: int, latent_attn_dim: Optional[int] = None, num_heads: int = 8, qkv_bias: bool = False,
                 qk_norm: bool = False, attn_drop: float = 0.0, proj_drop: float = 0.0, norm_layer: nn.Module = nn.LayerNorm,
                 custom_positional_encoding: Callable = None, use_scalable_softmax: bool = False,
                 use_entropy_scaling: bool = False, base_token_count_for_entropy_scaling: int = 444,
                 entropy_scaling_growth_factor: float = 1.4):
        super().__init__()
        assert dim % num_heads == 0, "dim should be divisible by num_heads"
        # latent attention (utils/transformer_blocks.py:178-199; round 6): q / k / v live in `latent_attn_dim` channels, proj maps back
        if latent_attn_dim is not None:
            assert latent_attn_dim % num_heads == 0, "latent_attn_dim should be divisible by num_heads"
            self.latent_attn_dim = latent_attn_dim
            self.latent_attn = True
        else:
            self.latent_attn = False
        self.num_heads = num_heads
        self.head_dim = dim // num_heads if not self.latent_attn else latent_attn_dim // num_heads
        self.scale = self.head_dim**-0.5
        self.fused_attn = use_fused_attn()
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias) if not self.latent_attn else nn.Linear(dim, latent_attn_dim * 3, bias=qkv_bias)
        self.q_norm = norm_layer(self.head_dim) if qk_norm else nn.Identity()
        self.k_norm = norm_layer(self.head_dim) if qk_norm else nn.Identity()
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim) if not self.latent_attn else nn.Linear(latent_attn_dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        self.custom_positional_encoding = custom_positional_encoding
        self.use_scalable_softmax = use_scalable_softmax
        self.use_entropy_scaling = use_entropy_scaling
        self.base_token_count_for_entropy_scaling = base_token_count_for_entropy_scaling
        self.entropy_scaling_growth_factor = entropy_scaling_growth_factor

    def forward(self, x: torch.Tensor, xpos: torch.Tensor = None) -> torch.Tensor:
        engine.require_inference(x, self.qkv.weight)
        sublayers.refuse_drops(self.training, False, self.attn_drop.p, self.proj_drop.p)
        if self.custom_positional_encoding is not None:
            assert xpos is not None, "Positions of tokens (xpos) are a required input when using custom positional encoding"
        B, N, C = x.shape
        dt = engine.compute_dtype()
        return engine.self_attention(as_dt(_as_2d(x), dt), B, N, self.qkv, self.proj, self.num_heads, self.custom_positional_encoding, xpos,
                                     self.scale * _softmax_scale_multiplier(self, N), None, dt, q_norm=self.q_norm,
                                     k_norm=self.k_norm).view(B, N, C)


class CrossAttention(nn.Module):
    "Cross-Attention Layer"

    def __init__(self, dim: int, num_heads: int = 8, qkv_bias: bool = False, qk_norm: bool = False, attn_drop: float = 0.0,
                 proj_drop: float = 0.0, norm_layer: nn.Module = nn.LayerNorm, custom_positional_encoding: Callable = None,
                 use_scalable_softmax: bool = False, use_entropy_scaling: bool = False,
                 base_token_count_for_entropy_scaling: int = 444, entropy_scaling_growth_factor: float = 1.4):
        super().__init__()
        assert dim % num_heads == 0, "dim should be divisible by num_heads"
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.scale = self.head_dim**-0.5
        self.fused_attn = use_fused_attn()
        self.projq = nn.Linear(dim, dim, bias=qkv_bias)
        self.projk = nn.Linear(dim, dim, bias=qkv_bias)
        self.projv = nn.Linear(dim, dim, bias=qkv_bias)
        self.q_norm = norm_layer(self.head_dim) if qk_norm else nn.Identity()
        self.k_norm = norm_layer(self.head_dim) if qk_norm else nn.Identity()
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        self.custom_positional_encoding = custom_positional_encoding
        self.use_scalable_softmax = use_scalable_softmax
        self.use_entropy_scaling = use_entropy_scaling
        self.base_token_count_for_entropy_scaling = base_token_count_for_entropy_scaling
        self.entropy_scaling_growth_factor = entropy_scaling_growth_factor

    def forward(self, query, key, value, qpos=None, kpos=None):
        engine.require_inference(query, key, value, self.projq.weight)
        sublayers.refuse_drops(self.training, False, self.attn_drop.p, self.proj_drop.p)
        if self.custom_positional_encoding is not None:
            assert qpos is not None, "Positions of queries (qpos) are a required input when using custom positional encoding"
            assert kpos is not None, "Positions of keys (kpos) are a required input when using custom positional encoding"
        B, Nq, C = query.shape
        Nk = key.shape[1]
        dt = engine.compute_dtype()
        hq, hk = as_dt(_as_2d(query), dt), as_dt(_as_2d(key), dt)
        hv = None
        if value is not key:      # (utils/transformer_blocks.py:341-348: projv runs on its own tokens)
            assert value.shape[1] == Nk, "key and value must have the same number of tokens"
            hv = as_dt(_as_2d(value), dt)
        return engine.cross_attention(hq, hk, B, Nq, Nk, self.projq, self.projk, self.projv, self.proj, self.num_heads,
                                      self.custom_positional_encoding, qpos, kpos, self.scale * _softmax_scale_multiplier(self, Nq), None, dt,
                                      q_norm=self.q_norm, k_norm=self.k_norm, hv2d=hv).view(B, Nq, C)


class LayerScale(nn.Module):
    """Per-channel scale; parameter container only.  The blocks fold it into the preceding linear's weights
    (gamma * (x W^T + b) = x (gamma W)^T + gamma b: no kernel work); in training the folded weight's gradient is unfolded into
    d W, d b and d gamma (autograd._unfold_layerscale).  SelfAttentionBlock since round 2, CrossAttentionBlock since round 6."""

    def __init__(self, dim: int, init_values: float = 1e-5, inplace: bool = False):
        super().__init__()
        self.inplace = inplace
        self.gamma = nn.Parameter(init_values * torch.ones(dim))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        raise engine.UcHipError("LayerScale is folded into the block's proj / fc2 weights; it is not callable on its own in the HIP path")


class SelfAttentionBlock(nn.Module):
    """x += ls1(attn(norm1(x))); x += ls2(mlp(norm2(x)))  (reference: utils/transformer_blocks.py:415-514) — the block of the
    global / alternating multi-view transformers.  Same fused pipeline as the CroCo encoder block: LayerNorm folded into the
    QKV / fc1 GEMMs, RoPE + V-transpose in the QKV epilogue, residual adds in the proj / fc2 epilogues."""

    def __init__(self, dim: int, num_heads: int, latent_attn_dim: Optional[int] = None, mlp_ratio: float = 4.0,
                 qkv_bias: bool = False, qk_norm: bool = False, proj_drop: float = 0.0, attn_drop: float = 0.0,
                 init_values: Optional[float] = None, drop_path: float = 0.0, act_layer: nn.Module = nn.GELU,
                 norm_layer: nn.Module = nn.LayerNorm, mlp_layer: nn.Module = Mlp, custom_positional_encoding: Callable = None,
                 use_scalable_softmax: bool = False, use_entropy_scaling: bool = False,
                 base_token_count_for_entropy_scaling: int = 444, entropy_scaling_growth_factor: float = 1.4):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, latent_attn_dim=latent_attn_dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_norm=qk_norm,
                              attn_drop=attn_drop, proj_drop=proj_drop, norm_layer=norm_layer,
                              custom_positional_encoding=custom_positional_encoding, use_scalable_softmax=use_scalable_softmax,
                              use_entropy_scaling=use_entropy_scaling,
                              base_token_count_for_entropy_scaling=base_token_count_for_entropy_scaling,
                              entropy_scaling_growth_factor=entropy_scaling_growth_factor)
        self.ls1 = LayerScale(dim, init_values=init_values) if init_values else nn.Identity()
        self.drop_path1 = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.norm2 = norm_layer(dim)
        self.mlp = mlp_layer(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=proj_drop)
        self.ls2 = LayerScale(dim, init_values=init_values) if init_values else nn.Identity()
        self.drop_path2 = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.custom_positional_encoding = custom_positional_encoding

    def forward_tokens(self, x2d, B, N, xpos, dt):
        """[B*N, C] fp32 residual stream in, new residual stream out; attention spans the N tokens of each of the B sequences."""
        sa, mlp, training = self.attn, _std_mlp(self.mlp), self.training
        if self.custom_positional_encoding is not None:
            assert xpos is not None, "Positions of tokens (xpos) are a required input when using custom positional encoding"
        train = autograd.grad_needed(x2d, *self.parameters())
        # the masks, in this block's generator order: the attention kernels' seed, proj_drop + DropPath, the Mlp's drops + DropPath
        ad = sublayers.attn_drop_for(training, train, sa.attn_drop.p)
        d1 = sublayers.drops_for(training, train, x2d, B, N, sa.proj_drop.p, self.drop_path1)
        d2 = sublayers.drops_for(training, train, x2d, B, N, mlp.drop2.p, self.drop_path2, mlp.drop1.p, mlp.fc1.out_features)
        x2d = sublayers.self_attn(x2d, self.norm1, sa.qkv, sa.proj, B, N, sa.num_heads, sa.custom_positional_encoding, xpos,
                                  sa.scale * _softmax_scale_multiplier(sa, N), dt, train=train, gamma=sublayers.gamma_of(self.ls1),
                                  q_norm=sa.q_norm, k_norm=sa.k_norm, drops=d1, attn_drop=ad)
        return sublayers.mlp(x2d, self.norm2, mlp.fc1, mlp.fc2, mlp.act, dt, train=train, gamma=sublayers.gamma_of(self.ls2), drops=d2)

    def forward(self, x: torch.Tensor, xpos: torch.Tensor = None) -> torch.Tensor:
        B, N, C = x.shape
        x2 = _as_2d(x)
        if x2.dtype != torch.float32:
            x2 = x2.float()
        return self.forward_tokens(x2, B, N, xpos, engine.compute_dtype()).view(B, N, C)


class CrossAttentionBlock(nn.Module):
    "Cross-Attention Block"

    def __init__(self, dim: int, num_heads: int, mlp_ratio: float = 4.0, qkv_bias: bool = False, qk_norm: bool = False,
                 proj_drop: float = 0.0, attn_drop: float = 0.0, init_values: Optional[float] = None, drop_path: float = 0.0,
                 act_layer: nn.Module = nn.GELU, norm_layer: nn.Module = nn.LayerNorm, mlp_layer: nn.Module = Mlp,
                 custom_positional_encoding: Callable = None, norm_cross_tokens: bool = True,
                 use_scalable_softmax: bool = False, use_entropy_scaling: bool = False,
                 base_token_count_for_entropy_scaling: int = 444, entropy_scaling_growth_factor: float = 1.4):
        super().__init__()
        akw = dict(num_heads=num_heads, qkv_bias=qkv_bias, qk_norm=qk_norm, attn_drop=attn_drop, proj_drop=proj_drop,
                   norm_layer=norm_layer, custom_positional_encoding=custom_positional_encoding,
                   use_scalable_softmax=use_scalable_softmax, use_entropy_scaling=use_entropy_scaling,
                   base_token_count_for_entropy_scaling=base_token_count_for_entropy_scaling,
                   entropy_scaling_growth_factor=entropy_scaling_growth_factor)
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, **akw)
        self.ls1 = LayerScale(dim, init_values=init_values) if init_values else nn.Identity()
        self.drop_path1 = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.norm_y = norm_layer(dim) if norm_cross_tokens else nn.Identity()
        self.custom_positional_encoding = custom_positional_encoding
        self.norm2 = norm_layer(dim)
        self.cross_attn = CrossAttention(dim, **akw)
        self.ls2 = LayerScale(dim, init_values=init_values) if init_values else nn.Identity()
        self.drop_path2 = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.norm3 = norm_layer(dim)
        self.mlp = mlp_layer(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=proj_drop)
        self.ls3 = LayerScale(dim, init_values=init_values) if init_values else nn.Identity()
        self.drop_path3 = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()

    def forward_tokens(self, x2d, y2d, B, Nx, Ny, xpos, ypos, dt):
        """x2d [B*Nx, C] residual stream, y2d [B*Ny, C] other-view tokens (previous depth) -> new x2d."""
        sa, ca, mlp, training = self.attn, self.cross_attn, _std_mlp(self.mlp), self.training
        rope = self.custom_positional_encoding
        if rope is not None:
            assert xpos is not None, "Positions of tokens (xpos) are a required input when using custom positional encoding"
            assert ypos is not None, "Positions of cross tokens (ypos) are a required input when using custom positional encoding"
        train = autograd.grad_needed(x2d, y2d, *self.parameters())
        # the masks, in this block's generator order: both attention seeds, then the three sub-layers' output masks
        ad1 = sublayers.attn_drop_for(training, train, sa.attn_drop.p)
        ad2 = sublayers.attn_drop_for(training, train, ca.attn_drop.p)
        d1 = sublayers.drops_for(training, train, x2d, B, Nx, sa.proj_drop.p, self.drop_path1)
        d2 = sublayers.drops_for(training, train, x2d, B, Nx, ca.proj_drop.p, self.drop_path2)
        d3 = sublayers.drops_for(training, train, x2d, B, Nx, mlp.drop2.p, self.drop_path3, mlp.drop1.p, mlp.fc1.out_features)
        x2d = sublayers.self_attn(x2d, self.norm1, sa.qkv, sa.proj, B, Nx, sa.num_heads, rope, xpos,
                                  sa.scale * _softmax_scale_multiplier(sa, Nx), dt, train=train, gamma=sublayers.gamma_of(self.ls1),
                                  q_norm=sa.q_norm, k_norm=sa.k_norm, drops=d1, attn_drop=ad1)
        x2d = sublayers.cross_attn(x2d, y2d, self.norm2, self.norm_y, ca, B, Nx, Ny, rope, xpos, ypos,
                                   ca.scale * _softmax_scale_multiplier(ca, Nx), dt, train=train, gamma=sublayers.gamma_of(self.ls2),
                                   drops=d2, attn_drop=ad2)
        return sublayers.mlp(x2d, self.norm3, mlp.fc1, mlp.fc2, mlp.act, dt, train=train, gamma=sublayers.gamma_of(self.ls3), drops=d3)

    def forward(self, x, y, xpos=None, ypos=None):
        B, Nx, C = x.shape
        Ny = y.shape[1]
        out = self.forward_tokens(_as_2d(x), _as_2d(y), B, Nx, Ny, xpos, ypos, engine.compute_dtype())
        return out.view(B, Nx, C)


# ---- differential attention (reference: utils/transformer_blocks.py:657-1045; arXiv 2410.05258) ----------------------------------
class RMSNorm(nn.Module):
    """Parameter container of the differential layers' `subln` (reference :658-679).  Inside DiffAttention / DiffCrossAttention the
    normalisation runs in the epilogue of the fused attention kernel; on its own the module is plain PyTorch arithmetic, as written in
    the reference (it is not on any hot path)."""

    def __init__(self, dim: int, eps: float = 1e-6, elementwise_affine=True, memory_efficient=False):
        super().__init__()
        self.dim = dim
        self.eps = eps
        self.elementwise_affine = elementwise_affine
        if self.elementwise_affine:
            self.weight = nn.Parameter(torch.ones(dim))
        else:
            self.register_parameter("weight", None)

    def _norm(self, x):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + self.eps)

    def forward(self, x):
        output = self._norm(x.float()).type_as(x)
        if self.weight is not None:
            output = output * self.weight
        return output

    def extra_repr(self) -> str:
        return f"dim={self.dim}, eps={self.eps}, elementwise_affine={self.elementwise_affine}"


def lambda_init_fn(depth):
    return 0.8 - 0.6 * math.exp(-0.3 * depth)


def _diff_params(module, depth: int):
    "the DiffTransformer-specific parameters, in the reference's registration order (:733-740)"
    module.lambda_init = lambda_init_fn(depth)
    for name in ("lambda_q1", "lambda_k1", "lambda_q2", "lambda_k2"):
        setattr(module, name, nn.Parameter(torch.zeros(module.head_dim, dtype=torch.float32).normal_(mean=0, std=0.1)))
    module.subln = RMSNorm(2 * module.head_dim, eps=1e-5, elementwise_affine=True)


def _in_dt(x: torch.Tensor, dt: torch.dtype) -> torch.Tensor:
    x2 = _as_2d(x)
    return x2 if x2.dtype == dt else autograd.convert(x2, dt)


class DiffAttention(nn.Module):
    """Differential Self-Attention Layer (reference :686-804): two softmaxes over q / k heads of head_dim = dim / num_heads / 2 and one
    shared v of twice that width, subtracted with the learned lambda, RMS-normalised and scaled by 1 - lambda_init — one fused HIP
    kernel (engine.diff_self_attention), trainable."""

    def __init__(self, dim: int, depth: int, num_heads: int = 8, qkv_bias: bool = False, qk_norm: bool = False, attn_drop: float = 0.0,
                 proj_drop: float = 0.0, norm_layer: nn.Module = nn.LayerNorm, custom_positional_encoding: Callable = None):
        super().__init__()
        assert dim % num_heads == 0, "dim should be divisible by num_heads"
        self.num_heads = num_heads
        self.head_dim = dim // num_heads // 2
        self.scale = self.head_dim**-0.5
        self.fused_attn = use_fused_attn()
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.q_norm = norm_layer(self.head_dim) if qk_norm else nn.Identity()
        self.k_norm = norm_layer(self.head_dim) if qk_norm else nn.Identity()
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        self.custom_positional_encoding = custom_positional_encoding
        _diff_params(self, depth)

    def forward(self, x: torch.Tensor, xpos: torch.Tensor = None) -> torch.Tensor:
        B, N, C = x.shape
        if self.custom_positional_encoding is not None:
            assert xpos is not None, "Positions of tokens (xpos) are a required input when using custom positional encoding"
        if self.proj_drop.p > 0.0 and self.training:
            raise engine.UcHipError("proj_drop > 0 on a stand-alone differential attention layer has no HIP path; use the block")
        engine.check_diff_layer(self)
        dt = engine.compute_dtype()
        # the reference reshapes its [B, H, N, 2 head_dim] result to [B, N, C] WITHOUT transposing heads and tokens back (:796-800);
        # the arithmetic is reproduced as written: the kernel stores that memory order (autograd.diff_self_attn_core, head_major)
        return engine.diff_self_attention(self, _in_dt(x, dt), B, N, xpos, dt).view(B, N, C)


class DiffCrossAttention(nn.Module):
    "Differential Cross-Attention Layer (reference :807-945) on the fused HIP kernel (engine.diff_cross_attention), trainable."

    def __init__(self, dim: int, depth: int, num_heads: int = 8, qkv_bias: bool = False, qk_norm: bool = False, attn_drop: float = 0.0,
                 proj_drop: float = 0.0, norm_layer: nn.Module = nn.LayerNorm, custom_positional_encoding: Callable = None):
        super().__init__()
        assert dim % num_heads == 0, "dim should be divisible by num_heads"
        self.num_heads = num_heads
        self.head_dim = dim // num_heads // 2
        self.scale = self.head_dim**-0.5
        self.fused_attn = use_fused_attn()
        self.projq = nn.Linear(dim, dim, bias=qkv_bias)
        self.projk = nn.Linear(dim, dim, bias=qkv_bias)
        self.projv = nn.Linear(dim, dim, bias=qkv_bias)
        self.q_norm = norm_layer(self.head_dim) if qk_norm else nn.Identity()
        self.k_norm = norm_layer(self.head_dim) if qk_norm else nn.Identity()
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        _diff_params(self, depth)
        self.custom_positional_encoding = custom_positional_encoding

    def lambda_init_fn(self, depth):
        return lambda_init_fn(depth)

    def forward(self, query, key, value, qpos=None, kpos=None):
        B, Nq, C = query.shape
        Nk = key.shape[1]
        assert value.shape[1] == Nk, "key and value must have the same number of tokens"
        if self.custom_positional_encoding is not None:
            assert qpos is not None, "Positions of queries (qpos) are a required input when using custom positional encoding"
            assert kpos is not None, "Positions of keys (kpos) are a required input when using custom positional encoding"
        if self.proj_drop.p > 0.0 and self.training:
            raise engine.UcHipError("proj_drop > 0 on a stand-alone differential attention layer has no HIP path; use the block")
        engine.check_diff_layer(self)
        dt = engine.compute_dtype()
        hk = _in_dt(key, dt)
        hv = hk if value is key else _in_dt(value, dt)
        return engine.diff_cross_attention(self, _in_dt(query, dt), hk, hv, B, Nq, Nk, qpos, kpos, dt).view(B, Nq, C)


class DiffSelfAttentionBlock(SelfAttentionBlock):
    "Differential Self-Attention Block (reference :948-994): SelfAttentionBlock whose attention is DiffAttention."

    def __init__(self, dim: int, depth: int, num_heads: int, mlp_ratio: float = 4.0, qkv_bias: bool = False, qk_norm: bool = False,
                 proj_drop: float = 0.0, attn_drop: float = 0.0, init_values: Optional[float] = None, drop_path: float = 0.0,
                 act_layer: nn.Module = nn.GELU, norm_layer: nn.Module = nn.LayerNorm, mlp_layer: nn.Module = Mlp,
                 custom_positional_encoding: Callable = None):
        super().__init__(dim=dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_norm=qk_norm, proj_drop=proj_drop,
                         attn_drop=attn_drop, init_values=init_values, drop_path=drop_path, act_layer=act_layer, norm_layer=norm_layer,
                         mlp_layer=mlp_layer, custom_positional_encoding=custom_positional_encoding)
        self.attn = DiffAttention(dim, depth, num_heads=num_heads, qkv_bias=qkv_bias, qk_norm=qk_norm, attn_drop=attn_drop,
                                  proj_drop=proj_drop, norm_layer=norm_layer, custom_positional_encoding=custom_positional_encoding)

    def forward_tokens(self, x2d, B, N, xpos, dt):
        sa, mlp, training = self.attn, _std_mlp(self.mlp), self.training
        engine.check_diff_layer(sa)
        if self.custom_positional_encoding is not None:
            assert xpos is not None, "Positions of tokens (xpos) are a required input when using custom positional encoding"
        train = autograd.grad_needed(x2d, *self.parameters())
        d1 = sublayers.drops_for(training, train, x2d, B, N, sa.proj_drop.p, self.drop_path1)
        d2 = sublayers.drops_for(training, train, x2d, B, N, mlp.drop2.p, self.drop_path2, mlp.drop1.p, mlp.fc1.out_features)
        x2d = autograd.diff_self_attn_sublayer(x2d, self.norm1, sa, B, N, sa.custom_positional_encoding, xpos, dt,
                                               gamma=sublayers.gamma_of(self.ls1), drops=d1)
        return sublayers.mlp(x2d, self.norm2, mlp.fc1, mlp.fc2, mlp.act, dt, train=train, gamma=sublayers.gamma_of(self.ls2), drops=d2)


class DiffCrossAttentionBlock(CrossAttentionBlock):
    """Differential Cross-Attention Block (reference :997-1045): CrossAttentionBlock whose cross-attention is DiffCrossAttention.  The
    plain self-attention (head_dim = dim / num_heads: 64 where the differential layer has 32 | 64) and the Mlp are the runners'
    sub-layers (sublayers.self_attn / sublayers.mlp); the differential sub-layer is LayerNorm -> q / k / v GEMMs -> uc_rope2d -> the fused kernel -> proj."""

    def __init__(self, dim: int, depth: int, num_heads: int, mlp_ratio: float = 4.0, qkv_bias: bool = False, qk_norm: bool = False,
                 proj_drop: float = 0.0, attn_drop: float = 0.0, init_values: Optional[float] = None, drop_path: float = 0.0,
                 act_layer: nn.Module = nn.GELU, norm_layer: nn.Module = nn.LayerNorm, mlp_layer: nn.Module = Mlp,
                 custom_positional_encoding: Callable = None, norm_cross_tokens: bool = True):
        super().__init__(dim=dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_norm=qk_norm, proj_drop=proj_drop,
                         attn_drop=attn_drop, init_values=init_values, drop_path=drop_path, act_layer=act_layer, norm_layer=norm_layer,
                         mlp_layer=mlp_layer, custom_positional_encoding=custom_positional_encoding, norm_cross_tokens=norm_cross_tokens)
        self.cross_attn = DiffCrossAttention(dim, depth, num_heads=num_heads, qkv_bias=qkv_bias, qk_norm=qk_norm, attn_drop=attn_drop,
                                             proj_drop=proj_drop, norm_layer=norm_layer,
                                             custom_positional_encoding=custom_positional_encoding)

    def forward_tokens(self, x2d, y2d, B, Nx, Ny, xpos, ypos, dt):
        sa, ca, mlp, training = self.attn, self.cross_attn, _std_mlp(self.mlp), self.training
        engine.check_diff_layer(ca)      # (before the plain self-attention: an unsupported geometry is reported as the differential layer's)
        rope = self.custom_positional_encoding
        if rope is not None:
            assert xpos is not None, "Positions of tokens (xpos) are a required input when using custom positional encoding"
            assert ypos is not None, "Positions of cross tokens (ypos) are a required input when using custom positional encoding"
        train = autograd.grad_needed(x2d, y2d, *self.parameters())
        # the masks, in this block's generator order: the differential sub-layer's first, then the attention seed and the other two
        d2 = sublayers.drops_for(training, train, x2d, B, Nx, ca.proj_drop.p, self.drop_path2)
        ad1 = sublayers.attn_drop_for(training, train, sa.attn_drop.p)
        d1 = sublayers.drops_for(training, train, x2d, B, Nx, sa.proj_drop.p, self.drop_path1)
        d3 = sublayers.drops_for(training, train, x2d, B, Nx, mlp.drop2.p, self.drop_path3, mlp.drop1.p, mlp.fc1.out_features)
        x2d = sublayers.self_attn(x2d, self.norm1, sa.qkv, sa.proj, B, Nx, sa.num_heads, rope, xpos,
                                  sa.scale * _softmax_scale_multiplier(sa, Nx), dt, train=train, gamma=sublayers.gamma_of(self.ls1),
                                  q_norm=sa.q_norm, k_norm=sa.k_norm, drops=d1, attn_drop=ad1)
        lny = None if isinstance(self.norm_y, nn.Identity) else self.norm_y
        x2d = autograd.diff_cross_attn_sublayer(x2d, y2d, self.norm2, lny, ca, B, Nx, Ny, rope, xpos, ypos, dt,
                                                gamma=sublayers.gamma_of(self.ls2), drops=d2)
        return sublayers.mlp(x2d, self.norm3, mlp.fc1, mlp.fc2, mlp.act, dt, train=train, gamma=sublayers.gamma_of(self.ls3), drops=d3)
