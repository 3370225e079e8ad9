"""Pixio encoder (reference: encoders/pixio.py:335-598) on the HIP kernels: a plain pre-LN ViT with `n_cls_tokens` class tokens, a
learned position table resized bicubically to other grids, fused qkv with bias and an erf-GELU Mlp; no RoPE, no qk_norm, no LayerScale.
The published sizes have head_dim 64 (B/16, L/16, 1B/16), 80 (H/16, the reference's default) and 96 (5B/16): the last two run the
wide-head attention kernels (csrc/attention_wide.hip) in bf16.

Kernel mapping: patch gather + GEMM with bias -> uc_assemble_prefix ([cls + pos | tok + pos] in the stream's dtype, one pass) -> per
block the sub-layer runners of models/utils/sublayers.py (self_attn + mlp) -> final LayerNorm (applied once: the reference applies it
after every block and keeps the last) -> the patch tokens as BCHW.
Training: the blocks are HIP forward + backward sub-layers, the patch embedding autograd.patch_embed; the class rows, the (resized)
table and the token assembly are a handful of torch ops (slices, adds, one cat) whose adjoints autograd provides.

Nothing is downloaded: the reference's constructor fetches `hf_model_name` from the hub; here the name is kept as an attribute and
weights come from `pretrained_checkpoint_path` (a plain state_dict file with `blocks.N.*` keys, as the published .pth files have).
"""
from functools import partial
from typing import Callable, Optional, Type, Union

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.utils.checkpoint import checkpoint

from ... import autograd, engine, ops
from ..utils import sublayers
from ..utils.checkpointing import has_random_masks
from .base import UniCeptionViTEncoderBase, ViTEncoderInput, ViTEncoderOutput


class SelfAttention(nn.Module):
    "parameter container of the reference's SelfAttention (encoders/pixio.py:99-176) as PixioEncoder builds it: qkv with bias, no norms"

    def __init__(self, dim: int, num_heads: int = 8, qkv_bias: bool = False, proj_bias: bool = True):
        super().__init__()
        assert dim % num_heads == 0, "dim should be divisible by num_heads"
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.scale = self.head_dim ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim, bias=proj_bias)


class Mlp(nn.Module):
    "fc1 -> GELU(erf) -> fc2 (encoders/pixio.py:178-218; drop 0, no norm)"

    def __init__(self, in_features: int, hidden_features: int, bias: bool = True):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features, bias=bias)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden_features, in_features, bias=bias)


class PatchEmbed(nn.Module):
    "2D Image to Patch Embedding (encoders/pixio.py:221-256): parameter container; the gather + GEMM is in PixioEncoder._tokens"

    def __init__(self, img_size: int = 224, patch_size: int = 16, in_chans: int = 3, embed_dim: int = 768):
        super().__init__()
        self.patch_size = (patch_size, patch_size)
        self.img_size = (img_size, img_size)
        self.grid_size = (img_size // patch_size, img_size // patch_size)
        self.num_patches = self.grid_size[0] * self.grid_size[1]
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size, bias=True)


class SelfAttentionBlock(nn.Module):
    "x += attn(norm1(x)); x += mlp(norm2(x)) (encoders/pixio.py:258-333) — parameter container; the pipeline is in forward_tokens"

    def __init__(self, dim: int, num_heads: int, mlp_ratio: float = 4.0, qkv_bias: bool = False, norm_layer=nn.LayerNorm):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.attn = SelfAttention(dim, num_heads=num_heads, qkv_bias=qkv_bias)
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))

    def forward_tokens(self, x2d, B, N, dt):
        a, m = self.attn, self.mlp
        train = autograd.grad_needed(x2d, *self.parameters())
        x2d = sublayers.self_attn(x2d, self.norm1, a.qkv, a.proj, B, N, a.num_heads, None, None, a.scale, dt, train=train)
        return sublayers.mlp(x2d, self.norm2, m.fc1, m.fc2, m.act, dt, train=train)


class _CheckpointingWrapper(nn.Module):
    """The reference's wrapper (encoders/pixio.py:411-422): the block becomes the sub-module `inner`, so its keys are `blocks.N.inner.*`.
    The re-computation is the project's checkpointing of the HIP sub-layers (models/utils/checkpointing.py): their Functions save through
    ctx.save_for_backward, which the non-reentrant checkpoint's hooks see.  Without a requested gradient the wrapper is transparent."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward_tokens(self, x2d, *args):
        if not torch.is_grad_enabled() or not autograd.grad_needed(x2d, *self.parameters()):
            return self.inner.forward_tokens(x2d, *args)
        return checkpoint(self.inner.forward_tokens, x2d, *args, use_reentrant=False,
                          preserve_rng_state=self.training and has_random_masks(self.inner))


class PixioEncoder(UniCeptionViTEncoderBase):
    "UniCeption Pixio Encoder (encoders/pixio.py:335-502)"

    def __init__(
        self,
        name: str,
        data_norm_type: str,
        img_size: int = 256,
        patch_size: int = 16,
        embed_dim: int = 1280,
        depth: int = 32,
        in_chans: int = 3,
        num_heads: int = 16,
        mlp_ratio: float = 4.0,
        n_cls_tokens: int = 8,
        norm_layer: Union[Type[nn.Module], Callable[..., nn.Module]] = partial(
            nn.LayerNorm, eps=1e-6
        ),
        hf_model_name: str = "facebook/pixio-vith16",
        gradient_checkpointing: bool = True,
        pretrained_checkpoint_path: Optional[str] = None,
        *args,
        **kwargs,
    ):
        super().__init__(name=name, data_norm_type=data_norm_type, patch_size=patch_size, *args, **kwargs)
        if in_chans != 3:
            raise engine.UcHipError("PixioEncoder: the forward takes 3-channel images (encoders/pixio.py:464)")
        self.n_cls_tokens = n_cls_tokens
        self.patch_size = patch_size
        self.enc_embed_dim = embed_dim
        self.hf_model_name = hf_model_name
        self.patch_embed = PatchEmbed(img_size, patch_size, in_chans, self.enc_embed_dim)
        self.cls_token = nn.Parameter(torch.zeros(1, n_cls_tokens, self.enc_embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, self.patch_embed.num_patches + n_cls_tokens, self.enc_embed_dim))
        self.blocks = nn.ModuleList([SelfAttentionBlock(self.enc_embed_dim, num_heads, mlp_ratio, qkv_bias=True, norm_layer=norm_layer)
                                     for _ in range(depth)])
        self.norm = norm_layer(self.enc_embed_dim)
        if pretrained_checkpoint_path:
            print(f"Loading pretrained Pixio Encoder from {pretrained_checkpoint_path} ...")
            ckpt = torch.load(pretrained_checkpoint_path, weights_only=False)
            print(self.load_state_dict(ckpt, strict=False))
        if gradient_checkpointing:
            for i in range(len(self.blocks)):
                self.blocks[i] = self.wrap_module_with_gradient_checkpointing(self.blocks[i])

    def wrap_module_with_gradient_checkpointing(self, module: nn.Module):
        return _CheckpointingWrapper(module)

    def get_pth_file(self, repo_id: str) -> str:
        raise engine.UcHipError(f"PixioEncoder downloads nothing ({repo_id}): pass the weights as pretrained_checkpoint_path "
                                "(a state_dict file with blocks.N.* keys)")

    # ---- position table ---------------------------------------------------------------------------
    def _resized_patch_rows(self, pe: torch.Tensor, H: int, W: int) -> torch.Tensor:
        "[H W, C]: the patch rows of the table pe [1, n_cls + pt pt, C], resized bicubically unless pt == H == W (encoders/pixio.py:424-456)"
        rows = pe[0, self.n_cls_tokens:]
        pt = int(rows.shape[0] ** 0.5)
        if pt == H == W:
            return rows
        grid = rows.reshape(1, pt, pt, -1).permute(0, 3, 1, 2)
        grid = F.interpolate(grid, size=(H, W), mode="bicubic", align_corners=False)
        return grid.permute(0, 2, 3, 1).reshape(H * W, -1)

    def _interpolate_pos_emb(self, x):
        "Interpolate the positional embeddings to match the input x: [1, n_cls + H W, C] (the class rows pass through)"
        ph, pw = self.patch_embed.patch_size
        assert x.shape[-2] % ph == 0, f"height {x.shape[-2]} must be divisible by patch size {ph}"
        assert x.shape[-1] % pw == 0, f"width {x.shape[-1]} must be divisible by patch size {pw}"
        H, W = x.shape[-2] // ph, x.shape[-1] // pw
        pt = int((self.pos_embed.shape[1] - self.n_cls_tokens) ** 0.5)
        if pt == H == W:
            return self.pos_embed
        return torch.cat((self.pos_embed[:, :self.n_cls_tokens], self._resized_patch_rows(self.pos_embed, H, W)[None]), dim=1)

    # ---- token stream -----------------------------------------------------------------------------
    def _tokens(self, image, h, w):
        P, n = self.patch_size, self.n_cls_tokens
        dt = engine.compute_dtype()
        B = image.shape[0]
        img = image.float().contiguous() if (image.dtype != torch.float32 or not image.is_contiguous()) else image
        conv = self.patch_embed.proj
        if autograd.grad_needed(image, *self.parameters()):
            tok = autograd.patch_embed(img, conv, P, dt).view(B, h * w, -1)
            pe = self.pos_embed.float()
            prefix = (self.cls_token.float() + pe[:, :n]).expand(B, -1, -1)
            return torch.cat((prefix, tok + self._resized_patch_rows(pe, h, w)), dim=1).contiguous(), dt
        wgt, bias = engine.patch_weights(conv, dt)
        tok = ops.gemm(ops.patch_gather(img, P, dt), wgt, bias, out_dtype=torch.float32).view(B, h * w, -1)
        prefix = engine.prepared(self, "prefix", (self.cls_token, self.pos_embed),
                                 lambda: (self.cls_token.detach().float() + self.pos_embed.detach().float()[:, :n])[0].contiguous())
        rows = engine.prepared(self, ("pos", h, w), (self.pos_embed,),
                               lambda: self._resized_patch_rows(self.pos_embed.detach().float(), h, w).contiguous())
        return ops.assemble_prefix(tok, prefix, rows, engine.stream_dtype(dt, self.enc_embed_dim)), dt

    @staticmethod
    def _as_bchw(feat, B, h, w):
        "[B, h w, C] patch tokens -> BCHW: plain (differentiable) views in training, else the channels-last view the heads consume"
        if feat.requires_grad:
            return feat.reshape(B, h, w, -1).permute(0, 3, 1, 2)
        return engine.nlc_as_bchw(feat.reshape(B * h * w, -1), B, h, w)

    def forward(self, encoder_input: ViTEncoderInput) -> ViTEncoderOutput:
        assert isinstance(encoder_input.image, torch.Tensor), "Input must be a torch.Tensor"
        assert encoder_input.image.ndim == 4, "Input must be of shape (B, C, H, W)"
        B, channels, height, width = encoder_input.image.shape
        assert channels == 3, "Input must have 3 channels"
        assert height % self.patch_size == 0 and width % self.patch_size == 0, f"Input shape must be divisible by patch size: {self.patch_size}"
        h, w = height // self.patch_size, width // self.patch_size
        x, dt = self._tokens(encoder_input.image, h, w)
        Nt, C = x.shape[1], x.shape[2]
        x2d = x.view(B * Nt, C)
        for blk in self.blocks:
            x2d = blk.forward_tokens(x2d, B, Nt, dt)
        xn = engine.layernorm(x2d, self.norm, torch.float32).view(B, Nt, C)
        n = self.n_cls_tokens
        feats = xn[:, n:] if xn.requires_grad else ops.token_slice(xn, n, h * w)
        return ViTEncoderOutput(features=self._as_bchw(feats, B, h, w))


def _factory(pretrained, **kw):
    # (the reference's factories omit `name` and `data_norm_type`, which its constructor requires; they are supplied here)
    model = PixioEncoder(name="pixio", data_norm_type="pixio", img_size=256, patch_size=16, mlp_ratio=4, n_cls_tokens=8,
                         norm_layer=partial(nn.LayerNorm, eps=1e-6), **kw)
    if pretrained:
        model.load_state_dict(torch.load(pretrained, map_location="cpu", weights_only=False))
    return model


def pixio_vitb16(pretrained=None):
    return _factory(pretrained, embed_dim=768, depth=12, num_heads=12)


def pixio_vitl16(pretrained=None):
    return _factory(pretrained, embed_dim=1024, depth=24, num_heads=16)


def pixio_vith16(pretrained=None):
    return _factory(pretrained, embed_dim=1280, depth=32, num_heads=16)


def pixio_vit1b16(pretrained=None):
    return _factory(pretrained, embed_dim=1536, depth=48, num_heads=24)


def pixio_vit5b16(pretrained=None):
    return _factory(pretrained, embed_dim=3072, depth=48, num_heads=32)
