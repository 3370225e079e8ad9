"""Differential multi-view cross-attention transformer (reference: info_sharing/diff_cross_attention_transformer.py:22-475).

The plain transformer's token-stream core (cross_attention_transformer.py: Jacobi update over the views, two streams for two views,
intermediate features) with DiffCrossAttentionBlock branches: block i is built with depth=i (its lambda_init) and num_heads // 2 heads,
so the differential cross-attention has Q / K head_dim = dim / num_heads and V head_dim twice that, and the block's plain
self-attention head_dim 2 dim / num_heads.  The HIP kernels cover dim / num_heads = 32 (e.g. dim 192 with 6 heads, 768 with 24);
the reference's default 768 / 12 needs head_dim-128 attention and raises UcHipError when it is called.
"""
from copy import deepcopy
from functools import partial
from typing import Callable, List, Optional, Type, Union

import torch
import torch.nn as nn

from ..utils.intermediate_feature_return import IntermediateFeatureReturner
from ..utils.positional_encoding import PositionGetter
from ..utils.transformer_blocks import DiffCrossAttentionBlock, Mlp
from .base import UniCeptionInfoSharingBase
from .cross_attention_transformer import MultiViewCrossAttentionTransformer, MultiViewCrossAttentionTransformerIFR


class DifferentialMultiViewCrossAttentionTransformer(MultiViewCrossAttentionTransformer):
    "Differential cross-attention transformer with one branch of blocks per view (https://arxiv.org/abs/2410.05258)."

    def __init__(self, name: str, input_embed_dim: int, num_views: int, size: Optional[str] = None, depth: int = 12,
                 dim: int = 768, num_heads: int = 12, mlp_ratio: float = 4.0, qkv_bias: bool = True, qk_norm: bool = False,
                 proj_drop: float = 0.0, attn_drop: float = 0.0, init_values: Optional[float] = None, drop_path: float = 0.0,
                 act_layer: Type[nn.Module] = nn.GELU,
                 norm_layer: Union[Type[nn.Module], Callable[..., nn.Module]] = partial(nn.LayerNorm, eps=1e-6),
                 mlp_layer: Type[nn.Module] = Mlp, custom_positional_encoding: Optional[Callable] = None,
                 norm_cross_tokens: bool = True, pretrained_checkpoint_path: Optional[str] = None,
                 gradient_checkpointing: bool = False, *args, **kwargs):
        UniCeptionInfoSharingBase.__init__(self, name=name, size=size, *args, **kwargs)
        self.input_embed_dim = input_embed_dim
        self.num_views = num_views
        self.depth = depth
        self.dim = dim
        self.num_heads = num_heads
        self.mlp_ratio = mlp_ratio
        self.qkv_bias = qkv_bias
        self.qk_norm = qk_norm
        self.proj_drop = proj_drop
        self.attn_drop = attn_drop
        self.init_values = init_values
        self.drop_path = drop_path
        self.act_layer = act_layer
        self.norm_layer = norm_layer
        self.mlp_layer = mlp_layer
        self.custom_positional_encoding = custom_positional_encoding
        self.norm_cross_tokens = norm_cross_tokens
        self.pretrained_checkpoint_path = pretrained_checkpoint_path
        self.gradient_checkpointing = gradient_checkpointing

        self.proj_embed = nn.Linear(input_embed_dim, dim, bias=True) if input_embed_dim != dim else nn.Identity()
        assert num_heads % 2 == 0, "Number of heads must be divisible by 2 for differential cross-attention."
        branch = nn.ModuleList([
            DiffCrossAttentionBlock(depth=i, dim=dim, num_heads=num_heads // 2, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_norm=qk_norm,
                                    proj_drop=proj_drop, attn_drop=attn_drop, init_values=init_values, drop_path=drop_path,
                                    act_layer=act_layer, norm_layer=norm_layer, mlp_layer=mlp_layer,
                                    custom_positional_encoding=custom_positional_encoding, norm_cross_tokens=norm_cross_tokens)
            for i in range(depth)])
        # per-view weights: every further view starts as a copy of view 0's branch (:131-135)
        self.multi_view_branches = nn.ModuleList([branch])
        for _ in range(1, num_views):
            self.multi_view_branches.append(deepcopy(branch))
        self.norm = norm_layer(dim)
        if custom_positional_encoding is not None:
            self.position_getter = PositionGetter()
        self.initialize_weights()
        if pretrained_checkpoint_path is not None:
            print(f"Loading pretrained differential multi-view cross-attention transformer weights from {pretrained_checkpoint_path} ...")
            ckpt = torch.load(pretrained_checkpoint_path, weights_only=False)
            print(self.load_state_dict(ckpt["model"]))
        if self.gradient_checkpointing:
            # (the reference refers to a missing attribute at :148-150 and raises; here the blocks are wrapped as in the plain transformer)
            for br in self.multi_view_branches:
                for i, block in enumerate(br):
                    br[i] = self.wrap_module_with_gradient_checkpointing(block)


class DifferentialMultiViewCrossAttentionTransformerIFR(DifferentialMultiViewCrossAttentionTransformer, IntermediateFeatureReturner):
    "Same transformer, also returning the features after the blocks in `indices` (:262-475)."

    def __init__(self, name: str, input_embed_dim: int, num_views: int, size: Optional[str] = None, depth: int = 12,
                 dim: int = 768, num_heads: int = 12, mlp_ratio: float = 4.0, qkv_bias: bool = True, qk_norm: bool = False,
                 proj_drop: float = 0.0, attn_drop: float = 0.0, init_values: Optional[float] = None, drop_path: float = 0.0,
                 act_layer: nn.Module = nn.GELU, norm_layer: nn.Module = partial(nn.LayerNorm, eps=1e-6),
                 mlp_layer: nn.Module = Mlp, custom_positional_encoding: Callable = None, norm_cross_tokens: bool = True,
                 pretrained_checkpoint_path: str = None, indices: Optional[Union[int, List[int]]] = None,
                 norm_intermediate: bool = True, intermediates_only: bool = False, gradient_checkpointing: bool = False,
                 *args, **kwargs):
        DifferentialMultiViewCrossAttentionTransformer.__init__(
            self, name=name, input_embed_dim=input_embed_dim, num_views=num_views, size=size, depth=depth, dim=dim,
            num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_norm=qk_norm, proj_drop=proj_drop,
            attn_drop=attn_drop, init_values=init_values, drop_path=drop_path, act_layer=act_layer, norm_layer=norm_layer,
            mlp_layer=mlp_layer, custom_positional_encoding=custom_positional_encoding, norm_cross_tokens=norm_cross_tokens,
            pretrained_checkpoint_path=pretrained_checkpoint_path, gradient_checkpointing=gradient_checkpointing, *args, **kwargs)
        IntermediateFeatureReturner.__init__(self, indices=indices, norm_intermediate=norm_intermediate,
                                             intermediates_only=intermediates_only)

    forward = MultiViewCrossAttentionTransformerIFR.forward
