"""Patch embedder for any spatial input [B, C, H, W] (reference: encoders/patch_embedder.py:30-181) on the HIP kernels.

forward: patch gather + GEMM (autograd.patch_embed: the k = s = P convolution) -> LN(tokens) + position table -> LN, the last three
in one pass over the token rows (uc_ln_pe_ln).  The learned position table is resized to other grids the way DINOv2Encoder does it:
F.interpolate(mode="bicubic") on the small [M, M, C] table, on the device and differentiable (pos_embed is a Parameter here); without
a graph the resized table is cached per grid and per version of pos_embed.  The returned BCHW features are a channels-last view of
the fp32 [B*N, C] token matrix, like CroCoEncoder's."""
import math
from functools import partial
from typing import Callable, Optional, Tuple, Union

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.init import trunc_normal_

from ... import autograd, engine, ops
from ..._lib import UcHipError
from .base import UniCeptionViTEncoderBase, ViTEncoderInput, ViTEncoderNonImageInput, ViTEncoderOutput


def make_2tuple(x):
    if isinstance(x, tuple):
        assert len(x) == 2
        return x
    assert isinstance(x, int)
    return (x, x)


def build_norm(factory: Optional[Callable], dim: int, what: str) -> nn.Module:
    "norm_layer(dim), or Identity for None; anything but an affine nn.LayerNorm has no HIP path and is refused at construction"
    if not factory:
        return nn.Identity()
    norm = factory(dim)
    if not isinstance(norm, nn.LayerNorm) or norm.weight is None or norm.bias is None or tuple(norm.normalized_shape) != (dim,):
        raise UcHipError(f"{what}={type(norm).__name__} has no HIP path (supported: nn.LayerNorm with weight and bias, or None)")
    return norm


def resize_pos_table(table: torch.Tensor, npatch: int, height: int, width: int, patch_size: int, offset: float, antialias: bool) -> torch.Tensor:
    """table [1, N, C] (N = M * M) -> [1, npatch, C] for an input of height x width pixels (patch_embedder.py:90-132): the table itself
    on its native square grid, else its bicubic resize — by scale factor (height0 + offset) / M when offset is non-zero, by output size
    otherwise.  Runs on the table's device and is differentiable."""
    N = table.shape[1]
    if npatch == N and height == width:
        return table
    dim = table.shape[-1]
    height0, width0 = height // patch_size, width // patch_size
    M = int(math.sqrt(N))  # Recover the number of patches in each dimension
    assert N == M * M
    if offset:
        kwargs = {"scale_factor": (float(height0 + offset) / M, float(width0 + offset) / M)}
    else:
        kwargs = {"size": (height0, width0)}
    grid = F.interpolate(table.float().reshape(1, M, M, dim).permute(0, 3, 1, 2), mode="bicubic", antialias=antialias, **kwargs)
    assert (height0, width0) == grid.shape[-2:]
    return grid.permute(0, 2, 3, 1).reshape(1, -1, dim)


def pos_rows(module: nn.Module, table: torch.Tensor, npatch: int, height: int, width: int) -> torch.Tensor:
    """fp32 [npatch, C] rows of `module`'s position table for this input: recomputed under autograd when the table takes a gradient,
    else cached per (grid, squareness) and per version of the table (engine.prepared)."""
    args = (npatch, height, width, module.patch_size, module.interpolate_offset, module.interpolate_antialias)
    if autograd.grad_needed(table):
        return resize_pos_table(table, *args)[0].float()
    key = ("pos", height // module.patch_size, width // module.patch_size, height == width)
    return engine.prepared(module, key, (table,), lambda: resize_pos_table(table.detach(), *args)[0].float().contiguous())


def spatial_input(encoder, encoder_input, what: str, in_chans: Optional[int] = None) -> torch.Tensor:
    "the [B, C, H, W] tensor of either input dataclass, with the reference's checks"
    if isinstance(encoder_input, ViTEncoderInput):
        encoder._check_data_normalization_type(encoder_input.data_norm_type)
        input_data = encoder_input.image
    elif isinstance(encoder_input, ViTEncoderNonImageInput):
        input_data = encoder_input.data
    else:
        raise ValueError(f"Unsupported input type for {what}.")
    assert isinstance(input_data, torch.Tensor), "Input must be a torch.Tensor"
    assert input_data.ndim == 4, "Input must be of shape (B, C, H, W)"
    assert in_chans is None or input_data.shape[1] == in_chans, f"Input channels must be {in_chans}"
    height, width = input_data.shape[-2:]
    assert (
        height % encoder.patch_size == 0 and width % encoder.patch_size == 0
    ), f"Input shape must be divisible by patch size: {encoder.patch_size}"
    ops._need_gpu(input_data)
    return input_data


class PatchEmbedder(UniCeptionViTEncoderBase):
    "UniCeption Patch Embedder"

    def __init__(
        self,
        name: str,
        data_norm_type: str = "patch_embedder",
        input_size: Union[int, Tuple[int, int]] = 518,
        patch_size: int = 14,
        in_chans: int = 3,
        enc_embed_dim: int = 1024,
        norm_layer: Optional[Callable] = None,
        post_pe_norm_layer: Optional[Callable] = partial(nn.LayerNorm, eps=1e-6),
        interpolate_antialias: bool = False,
        interpolate_offset: float = 0.1,
        pretrained_checkpoint_path: str = None,
        *args,
        **kwargs,
    ):
        super().__init__(name=name, data_norm_type=data_norm_type, patch_size=patch_size, *args, **kwargs)
        patch_HW = make_2tuple(patch_size)
        self.input_size = make_2tuple(input_size)
        self.patches_resolution = (self.input_size[0] // patch_HW[0], self.input_size[1] // patch_HW[1])
        self.num_patches = self.patches_resolution[0] * self.patches_resolution[1]
        self.in_chans = in_chans
        self.enc_embed_dim = enc_embed_dim

        self.proj = nn.Conv2d(in_chans, enc_embed_dim, kernel_size=patch_HW, stride=patch_HW)
        self.norm = build_norm(norm_layer, enc_embed_dim, "norm_layer")

        # learnable positional encodings
        self.pos_embed = nn.Parameter(torch.zeros(1, self.num_patches, self.enc_embed_dim))
        trunc_normal_(self.pos_embed, std=0.02)
        self.interpolate_antialias = interpolate_antialias
        self.interpolate_offset = interpolate_offset

        self.post_pe_norm = build_norm(post_pe_norm_layer, enc_embed_dim, "post_pe_norm_layer")

        self.pretrained_checkpoint_path = pretrained_checkpoint_path
        if self.pretrained_checkpoint_path:
            print(f"Loading custom pretrained Patch Embedder checkpoint from {self.pretrained_checkpoint_path} ...")
            ckpt = torch.load(self.pretrained_checkpoint_path, weights_only=False)
            print(self.load_state_dict(ckpt["model"]))

    def interpolate_pos_encoding(self, features, height, width):
        "the position table [1, N, C] for `features` [B, N, C] of an input of height x width pixels, in features' dtype"
        return resize_pos_table(self.pos_embed, features.shape[1], height, width, self.patch_size, self.interpolate_offset,
                                self.interpolate_antialias).to(features.dtype)

    def forward(self, encoder_input: Union[ViTEncoderInput, ViTEncoderNonImageInput]) -> ViTEncoderOutput:
        input_data = spatial_input(self, encoder_input, "Patch Embedder")
        B, C, height, width = input_data.shape
        P = self.patch_size
        h, w = height // P, width // P
        dt = engine.compute_dtype()
        pdt = dt if (C * P * P) % 8 == 0 else torch.float32       # (the bf16 GEMM's operand rows are 16-byte aligned)
        img = input_data if (input_data.dtype == torch.float32 and input_data.is_contiguous()) else input_data.float().contiguous()
        tokens = autograd.patch_embed(img, self.proj, P, pdt)                                   # fp32 [B h w, E]
        pe = pos_rows(self, self.pos_embed, h * w, height, width)
        y = autograd.ln_pe_ln(tokens, B, h * w, self.norm, pe, self.post_pe_norm, torch.float32)
        return ViTEncoderOutput(features=engine.nlc_as_bchw(y, B, h, w))
