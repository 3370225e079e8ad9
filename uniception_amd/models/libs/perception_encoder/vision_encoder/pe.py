"""Perception Encoder vision tower (reference: libs/perception_encoder/vision_encoder/pe.py:33-562) on the HIP kernels.

A pre-LN ViT with optional LayerScale, erf-GELU MLP and 2-D RoPE.  Parameter names, shapes and state_dict order are the reference's
(including `proj`, `attn_pool.*` and `class_embedding`, which the feature path never reads).

RoPE.  The reference (vision_encoder/rope.py:281-323) rotates the INTERLEAVED pairs (2i, 2i+1) of a head; the first half of the head
carries the x angle, the second the y angle; angle = pos * 10000^(-i / (D/4)); with a class token the patches sit at (y+1, x+1) and
the class token at (0, 0).  The kernels of this package (uc_rope2d, the QKV GEMM's epilogue, the attention backward's inverse
rotation) rotate CroCo's layout: y half then x half, pairs (i, i + D/4).  A fixed permutation of the channels inside each head maps
one onto the other, and q.k^T does not change when q and k are permuted alike, so the permutation is applied to the ROWS of
in_proj_weight / in_proj_bias of q and k (rope_row_permutation) and every RoPE-fused route serves this model unchanged with
RoPE2D(freq=10000).  Stored parameters stay in the reference's order.

Stem.  ln_pre(cat(class_embedding, conv1(x)) + resampled positional_embedding) is patch gather + GEMM, then one kernel
(uc_vit_stem; autograd.vit_stem with its own backward in training).
"""
from collections import OrderedDict
from dataclasses import asdict
from functools import partial
from typing import Callable, List, Literal, Optional, Union

import torch
import torch.nn as nn
from torch.nn.init import constant_, xavier_uniform_

from ..... import autograd, engine, ops
from ....libs.croco.pos_embed import RoPE2D
from ....utils import sublayers
from .config import PE_VISION_CONFIG

HEAD_DIM = 64          # what the bf16 attention kernels take


def head_channel_permutation(head_dim: int) -> torch.Tensor:
    """perm[n] = the reference's channel of a head that lands on channel n of the layout the RoPE kernels rotate:
    y half, n = r D/4 + i -> D/2 + 2i + r;  x half, n = D/2 + r D/4 + i -> 2i + r   (i < D/4, r in {0, 1})."""
    q = head_dim // 4
    n = torch.arange(head_dim // 2)
    r, i = n // q, n % q
    return torch.cat([head_dim // 2 + 2 * i + r, 2 * i + r])


def rope_row_permutation(width: int, heads: int) -> torch.Tensor:
    "rows of in_proj_weight [3 width, width] in the order the kernels want: q and k permuted inside each head, v untouched"
    D = width // heads
    per_head = (torch.arange(heads)[:, None] * D + head_channel_permutation(D)[None, :]).reshape(-1)
    return torch.cat([per_head, width + per_head, 2 * width + torch.arange(width)])


class LayerScale(nn.Module):
    def __init__(self, dim, init_values=1e-5, inplace=False):
        super().__init__()
        self.inplace = inplace
        self.dim = dim
        self.init_values = init_values

    def init_tensors(self):
        self.gamma = nn.Parameter(self.init_values * torch.ones(self.dim))


class AttentionPooling(nn.Module):
    "Parameters of the CLIP pooling head (loaded and saved, never run: VisionTransformer.forward)."

    def __init__(self, embed_dim: int, num_heads: int, num_probe: int = 1, mlp_ratio: int = 4, act_layer: Callable = nn.GELU,
                 norm_layer: Callable = nn.LayerNorm):
        super().__init__()
        self.embed_dim = embed_dim
        self.num_heads = num_heads
        assert self.embed_dim % num_heads == 0, "embed_dim must be divisible by num_heads"
        self.probe = nn.Parameter(torch.randn(1, num_probe, self.embed_dim))
        self.attn = nn.MultiheadAttention(self.embed_dim, self.num_heads, batch_first=True)
        self.layernorm = norm_layer(embed_dim)
        self.mlp_width = int(embed_dim * mlp_ratio)
        self.mlp = nn.Sequential(OrderedDict([("c_fc", nn.Linear(self.embed_dim, self.mlp_width)), ("gelu", act_layer()),
                                              ("c_proj", nn.Linear(self.mlp_width, self.embed_dim))]))


class _InProj:
    "What the attention routes read of an nn.Linear (weight, bias, out_features), around the packed q | k | v projection."

    def __init__(self, weight, bias):
        self.weight, self.bias, self.out_features = weight, bias, weight.shape[0]


class SelfAttention(nn.Module):
    "Parameters of the packed self-attention under nn.MultiheadAttention's names; `rope` is the shared RoPE2D or None."

    def __init__(self, embed_dim: int, num_heads: int, rope: Optional[nn.Module] = None):
        super().__init__()
        self.embed_dim = embed_dim
        self.num_heads = num_heads
        self.head_dim = embed_dim // num_heads
        assert self.head_dim * num_heads == self.embed_dim, "embed_dim must be divisible by num_heads"
        self.in_proj_weight = nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        self.in_proj_bias = nn.Parameter(torch.empty(3 * embed_dim))
        self.out_proj = nn.Linear(embed_dim, embed_dim, bias=True)
        object.__setattr__(self, "rope", rope)          # shared, and no entry of this module's tree (the reference's Rope2D is no nn.Module)
        self.scale = self.head_dim ** (-0.5)

    def init_tensors(self):
        xavier_uniform_(self.in_proj_weight)
        constant_(self.in_proj_bias, 0.0)
        constant_(self.out_proj.bias, 0.0)

    def _rows(self):
        w = self.in_proj_weight
        return engine.prepared(self, ("rope_rows", w.device), (), lambda: rope_row_permutation(self.embed_dim, self.num_heads).to(w.device))

    def in_proj(self, train: bool) -> _InProj:
        """The q | k | v projection as the attention routes take it.  Without a rope: the parameters themselves.  With one: rows of q and
        k in the kernels' channel order — inference: a copy cached per version of the parameters (every prepared weight derived from it
        hangs on that copy's holder and goes with it); training: a differentiable gather, so the gradients arrive in the stored order."""
        w, b = self.in_proj_weight, self.in_proj_bias
        if self.rope is None:
            return _InProj(w, b)
        rows = self._rows()
        if train:
            return _InProj(w.index_select(0, rows), b.index_select(0, rows))
        return engine.prepared(self, "in_proj_perm", (w, b),
                               lambda: _InProj(w.detach().index_select(0, rows).contiguous(), b.detach().index_select(0, rows).contiguous()))


class ResidualAttentionBlock(nn.Module):
    "x += ls_1(attn(ln_1(x))); x += ls_2(mlp(ln_2(x)))  — parameter container; the fused pipeline is in forward_tokens."

    def __init__(self, d_model: int, n_head: int, mlp_ratio: float = 4.0, ls_init_value: float = None, act_layer: Callable = nn.GELU,
                 norm_layer: Callable = nn.LayerNorm, drop_path: float = 0.0, rope: Optional[nn.Module] = None):
        super().__init__()
        if drop_path > 0.0:
            raise engine.UcHipError("drop_path > 0 has no HIP path in the Perception Encoder blocks (every published config has 0)")
        # (the reference takes nn.MultiheadAttention without a rope: the same parameter names, the same route here)
        self.attn = SelfAttention(d_model, n_head, rope=rope)
        self.ls_1 = LayerScale(d_model, ls_init_value) if ls_init_value is not None else nn.Identity()
        self.ls_2 = LayerScale(d_model, ls_init_value) if ls_init_value is not None else nn.Identity()
        self.ln_1 = norm_layer(d_model)
        self.ln_2 = norm_layer(d_model)
        self.drop_path1 = nn.Identity()
        self.drop_path2 = nn.Identity()
        mlp_width = int(d_model * mlp_ratio)
        self.mlp = nn.Sequential(OrderedDict([("c_fc", nn.Linear(d_model, mlp_width)), ("gelu", act_layer()),
                                              ("c_proj", nn.Linear(mlp_width, d_model))]))

    def forward_tokens(self, x2d, B, N, dt, pos=None):
        a, mlp = self.attn, self.mlp
        train = autograd.grad_needed(x2d, *self.parameters())
        x2d = sublayers.self_attn(x2d, self.ln_1, a.in_proj(train), a.out_proj, B, N, a.num_heads, a.rope, pos, a.scale, dt, train=train,
                                  gamma=sublayers.gamma_of(self.ls_1))
        return sublayers.mlp(x2d, self.ln_2, mlp.c_fc, mlp.c_proj, mlp.gelu, dt, train=train, gamma=sublayers.gamma_of(self.ls_2))


class Transformer(nn.Module):
    def __init__(self, width: int, layers: int, heads: int, mlp_ratio: float = 4.0, ls_init_value: float = None, act_layer: Callable = nn.GELU,
                 norm_layer: Callable = nn.LayerNorm, drop_path: float = 0.0, rope: Optional[nn.Module] = None):
        super().__init__()
        self.width = width
        self.layers = layers
        self.grad_checkpointing = False
        self.resblocks = nn.ModuleList([ResidualAttentionBlock(width, heads, mlp_ratio, ls_init_value=ls_init_value, act_layer=act_layer,
                                                               norm_layer=norm_layer, drop_path=drop_path, rope=rope) for _ in range(layers)])

    def set_grad_checkpointing(self, enable=True):
        "re-compute every block in the backward pass (models/utils/checkpointing.py); False restores the plain blocks"
        from ....utils.checkpointing import wrap_module_with_gradient_checkpointing
        self.grad_checkpointing = enable
        for blk in self.resblocks:
            if enable:
                wrap_module_with_gradient_checkpointing(blk)
            elif getattr(blk.__class__, "_restore_cls", None) is not None:
                blk.__class__ = blk.__class__._restore_cls

    def truncate(self, layer_idx: int):
        "Delete layers so the last layer is the given layer index (the reference's arithmetic: truncate(k) leaves ((layers + k) % layers) + 1)."
        self.layers = ((self.layers + layer_idx) % self.layers) + 1
        self.resblocks = nn.ModuleList(self.resblocks[: self.layers])


class VisionTransformer(nn.Module):
    def __init__(self, patch_size: int, width: int, layers: int, heads: int, mlp_ratio: float, act_layer: Callable = nn.GELU,
                 norm_layer: Callable = partial(nn.LayerNorm, eps=1e-5), use_ln_pre: bool = True, use_ln_post: bool = True,
                 ls_init_value: float = None, drop_path: float = 0.0, image_size: int = 448, use_abs_posemb: bool = True,
                 use_rope2d: bool = True, use_cls_token: bool = False, output_dim: Optional[int] = 1280, attn_pooler_heads: int = 8,
                 pool_type: Literal["attn", "tok", "avg", "none"] = "attn"):
        super().__init__()
        assert pool_type in ("attn", "tok", "avg", "none")
        if width % heads != 0 or width // heads != HEAD_DIM:
            raise engine.UcHipError(f"Perception Encoder with width {width} and {heads} heads has head_dim {width // heads}: the head_dim-{HEAD_DIM} "
                                    "attention kernels do not serve it (the giant models, width 1536 with 16 heads, are not supported)")
        self.pool_type = pool_type
        self.patch_size = patch_size
        self.output_dim = output_dim or width
        self.proj_dim = output_dim
        self.heads = heads
        self.width = width
        self.layers = layers
        self.use_abs_posemb = use_abs_posemb
        self.use_cls_token = use_cls_token
        self.use_rope2d = use_rope2d
        self.image_size = image_size

        self.conv1 = nn.Conv2d(in_channels=3, out_channels=width, kernel_size=patch_size, stride=patch_size, bias=False)
        # the kernels' RoPE-2D at the reference's base; kept out of the module tree and the state_dict, like the reference's Rope2D
        object.__setattr__(self, "rope", RoPE2D(freq=10000.0, F0=1.0) if use_rope2d else None)
        self.ln_pre = norm_layer(width) if use_ln_pre else nn.Identity()
        self.ln_post = norm_layer(self.width) if use_ln_post else nn.Identity()
        self.transformer = Transformer(width, layers, heads, mlp_ratio, ls_init_value=ls_init_value, act_layer=act_layer,
                                       norm_layer=norm_layer, drop_path=drop_path, rope=self.rope)
        if pool_type == "attn":
            self.attn_pool = AttentionPooling(embed_dim=width, num_heads=attn_pooler_heads, act_layer=act_layer, norm_layer=norm_layer)
        else:
            self.attn_pool = None
        self._pos_cache = {}
        self.init_tensors()

    def init_tensors(self):
        def init_submodule_tensors(module):
            for _, child in module.named_children():
                if hasattr(child, "init_tensors"):
                    child.init_tensors()
                init_submodule_tensors(child)

        init_submodule_tensors(self)
        init_scale = self.width ** -0.5
        if self.use_cls_token:
            self.class_embedding = nn.Parameter(init_scale * torch.randn(self.width))
        if self.use_abs_posemb:
            self.posemb_grid_size = self.image_size // self.patch_size
            self.positional_embedding = nn.Parameter(init_scale * torch.randn(int(self.use_cls_token) + self.posemb_grid_size ** 2, self.width))
        if self.proj_dim is not None:
            self.proj = nn.Parameter(init_scale * torch.randn(self.width, self.proj_dim))

    # ---- checkpoints, configs ----------------------------------------------------------------------------------------------------
    def load_ckpt(self, ckpt_path: str):
        _sd = torch.load(ckpt_path, weights_only=True)
        if "state_dict" in _sd:
            _sd = _sd["state_dict"]
        elif "weights" in _sd:
            _sd = _sd["weights"]
        _sd = {k.replace("module.", ""): v for k, v in _sd.items()}
        if any(k.startswith("visual.") for k in _sd):
            _sd = {k.replace("visual.", ""): v for k, v in _sd.items() if "visual" in k}
        self.load_state_dict(_sd, strict=True)

    def truncate(self, layer_idx: int):
        self.transformer.truncate(layer_idx)
        self.layers = self.transformer.layers

    @classmethod
    def from_config(cls, name: str, pretrained: bool = False, checkpoint_path: Optional[str] = None, **kwdargs):
        if name not in PE_VISION_CONFIG:
            raise RuntimeError(f"{name} not found in configs.")
        args = asdict(PE_VISION_CONFIG[name])
        args.update(kwdargs)
        model = cls(**args)
        if pretrained:
            if not checkpoint_path or checkpoint_path.startswith("hf://"):
                raise engine.UcHipError(f"{name}: pretrained=True needs checkpoint_path, a local file (nothing is downloaded here)")
            model.load_ckpt(checkpoint_path)
        return model

    @classmethod
    def available_configs(cls):
        return list(PE_VISION_CONFIG.keys())

    def set_grad_checkpointing(self, enable=True):
        self.transformer.set_grad_checkpointing(enable=enable)

    # ---- position table and RoPE positions -------------------------------------------------------------------------------------------
    def _sample_abs_posemb(self, grid_h: int, grid_w: int) -> torch.Tensor:
        """[ncls + grid_h grid_w, C] fp32: the table itself at the native grid, else its patch rows resized bilinearly
        (align_corners=False: uc_resize_bilinear_nhwc) behind the untouched class row.  Differentiable when the table asks for it;
        otherwise cached per grid and per version of the table."""
        pe, g, ncls = self.positional_embedding, self.posemb_grid_size, int(self.use_cls_token)

        def build(resize, table):
            table = table.float()
            if (g, g) == (grid_h, grid_w):
                return table.contiguous()
            rows = resize(table[ncls:].reshape(1, g, g, self.width).contiguous(), grid_h, grid_w, False).reshape(grid_h * grid_w, self.width)
            return torch.cat([table[:ncls], rows], 0) if ncls else rows

        if autograd.grad_needed(pe):
            return build(autograd.resize_bilinear, pe)
        return engine.prepared(self, ("posemb", grid_h, grid_w), (pe,), lambda: build(ops.resize_bilinear_nhwc, pe.detach()))

    def rope_positions(self, B: int, grid_h: int, grid_w: int, device) -> torch.Tensor:
        "int64 [B, N, 2] (y, x) per token, cached per grid: patches at (y + 1, x + 1) behind a class token at (0, 0), else at (y, x)"
        key = (B, grid_h, grid_w, str(device))
        pos = self._pos_cache.get(key)
        if pos is None:
            off = int(self.use_cls_token)
            yx = torch.cartesian_prod(torch.arange(grid_h), torch.arange(grid_w)) + off
            if off:
                yx = torch.cat([torch.zeros(1, 2, dtype=yx.dtype), yx], 0)
            if len(self._pos_cache) > 16:
                self._pos_cache.clear()
            pos = self._pos_cache[key] = yx[None].repeat(B, 1, 1).contiguous().to(device)
        return pos

    # ---- token stream --------------------------------------------------------------------------------------------------------------------
    def _stem(self, x: torch.Tensor, grid_h: int, grid_w: int):
        "image -> (ln_pre(cat(class_embedding, conv1(x)) + posemb) [B, T, C] in the stream dtype, compute dtype)"
        ops._need_gpu(x)
        P, B, hw = self.patch_size, x.shape[0], grid_h * grid_w
        K = 3 * P * P
        dt = engine.compute_dtype()
        sdt = engine.stream_dtype(dt, self.width)
        img = x if (x.dtype == torch.float32 and x.is_contiguous()) else x.float().contiguous()
        cls = self.class_embedding if self.use_cls_token else None
        pos = self._sample_abs_posemb(grid_h, grid_w) if self.use_abs_posemb else None
        if autograd.grad_needed(x, *self.parameters()):
            tok = autograd.patch_embed(img, self.conv1, P, dt if K % 8 == 0 else torch.float32)
            return autograd.vit_stem(tok.view(B, hw, self.width), cls, pos, self.ln_pre, sdt), dt
        if dt == torch.bfloat16 and K % 64 != 0:      # patch 14: K = 588 zero-padded to 640 for the MFMA kernel (as the DINOv2 encoder)
            kpad = (K + 63) // 64 * 64
            cols = ops.patch_gather(img, P, torch.bfloat16)
            colsp = torch.zeros((cols.shape[0], kpad), dtype=torch.bfloat16, device=cols.device)
            colsp[:, :K] = cols
            w, b = engine.patch_weights_padded(self.conv1, torch.bfloat16, kpad)
            tok = ops.gemm(colsp, w, b, out_dtype=torch.float32)
        else:
            w, b = engine.patch_weights(self.conv1, dt)
            tok = ops.gemm(ops.patch_gather(img, P, dt), w, b, out_dtype=torch.float32)
        return autograd.vit_stem(tok.view(B, hw, self.width), cls, pos, self.ln_pre, sdt), dt

    def _blocks(self, x: torch.Tensor, taps):
        "run the blocks on the image x up to the last tapped one; returns ([B T, C] stream after each tapped block, B, T)"
        B, _, h, w = x.shape
        grid_h, grid_w = h // self.patch_size, w // self.patch_size
        x3, dt = self._stem(x, grid_h, grid_w)
        T = x3.shape[1]
        pos = self.rope_positions(B, grid_h, grid_w, x3.device) if self.use_rope2d else None
        x2d, outs, last = x3.view(B * T, self.width), [], max(taps)
        for i, blk in enumerate(self.transformer.resblocks):
            x2d = blk.forward_tokens(x2d, B, T, dt, pos)
            if i in taps:
                outs.append(x2d)
            if i == last:
                break
        return outs, B, T

    def _finish(self, x2d, B, T, norm: bool, strip_cls_token: bool):
        "-> fp32 [B, T or T - 1, C]: ln_post when asked for and present, the class row dropped when asked for and present"
        if norm and isinstance(self.ln_post, nn.LayerNorm):
            x2d = engine.layernorm(x2d, self.ln_post, torch.float32)
        elif x2d.dtype != torch.float32:
            x2d = autograd.convert(x2d, torch.float32) if x2d.requires_grad else ops.convert(x2d, torch.float32)
        x3 = x2d.view(B, T, self.width)
        if strip_cls_token and self.use_cls_token:
            x3 = x3[:, 1:, :] if x3.requires_grad else ops.token_slice(x3, 1, T - 1)
        return x3

    def forward_features(self, x: torch.Tensor, norm: bool = False, layer_idx: int = -1, strip_cls_token: bool = False):
        n = len(self.transformer.resblocks)
        outs, B, T = self._blocks(x, [(n + layer_idx) % n])
        return self._finish(outs[0], B, T, norm, strip_cls_token)

    def get_intermediate_layers(self, x: torch.Tensor, n: Union[int, List[int]] = 1, norm: bool = True, strip_cls_token: bool = False):
        "n: a list of block indices, or an integer — the reference then returns the SINGLE layer len(blocks) - n, not the last n"
        nblk = len(self.transformer.resblocks)
        taps = [nblk - n] if isinstance(n, int) else [i for i in range(nblk) if i in n]
        if not taps:
            return []
        outs, B, T = self._blocks(x, taps)
        return [self._finish(o, B, T, norm, strip_cls_token) for o in outs]

    def forward(self, x: torch.Tensor, **kwargs):
        raise engine.UcHipError("the pooled CLIP embedding (attention pooling with head_dim width / 8, then `proj`) has no HIP path: use "
                                "forward_features / get_intermediate_layers, as the encoder wrappers do")
