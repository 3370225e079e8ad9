"""Dense representation encoder (reference: encoders/dense_rep_encoder.py:31-287) on the HIP kernels: ray maps, depth maps and other
per-pixel inputs as patch tokens.

  unshuffle    nn.PixelUnshuffle(P) written straight as the NHWC operand of conv_in (uc_unshuffle_rows), C P^2 columns zero-padded to 64;
  conv_in      zero-padded 3x3 convolution (uc_gemm's implicit GEMM) on padded channel counts;
  block        conv1 -> act (uc_act on the stored pre-activation) -> conv2 with the shortcut (a 1x1 GEMM, or the input) added in its
               epilogue -> act (uc_act: uc_gemm's epilogues apply an activation BEFORE the residual, the block needs it after);
  projection   the last 1x1 convolution as a dense GEMM with fp32 output;
  tail         LN(tokens) + resized sinusoid table -> LN in one pass (uc_ln_pe_ln).
Every intermediate channel count is zero-padded to a multiple of 64 in the prepared weights and in the activations (the default
588 runs as 640); zero weight rows, zero bias entries and act(0) = 0 keep the padded channels exactly zero, and the state_dict holds
the reference's shapes only.  Training and inference launch the same kernels: the same bits."""
from functools import partial
from typing import Callable, List, Optional, Tuple, Type, Union

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import autograd, engine, ops
from ..._lib import UcHipError
from .base import UniCeptionViTEncoderBase, ViTEncoderInput, ViTEncoderNonImageInput, ViTEncoderOutput
from .patch_embedder import build_norm, make_2tuple, pos_rows, resize_pos_table, spatial_input


def build_act(act_layer) -> Tuple[nn.Module, str]:
    "act_layer() and its kernel name; anything but nn.GELU (exact erf) or nn.ReLU has no HIP path and is refused at construction"
    act = act_layer()
    if isinstance(act, nn.GELU) and getattr(act, "approximate", "none") == "none":
        return act, "gelu"
    if isinstance(act, nn.ReLU):
        return act, "relu"
    raise UcHipError(f"act_layer={type(act).__name__} has no HIP path (supported: nn.GELU with the exact erf, nn.ReLU)")


class ResidualBlock(nn.Module):
    "Residual block for Dense Representation Encoder: act(conv2(act(conv1(x))) + shortcut(x))"

    def __init__(self, in_channels: int, out_channels: int, act_layer: Type[nn.Module] = nn.GELU):
        super(ResidualBlock, self).__init__()
        self.conv1 = nn.Conv2d(in_channels, out_channels, kernel_size=3, stride=1, padding=1)
        self.act, self._act_name = build_act(act_layer)
        self.conv2 = nn.Conv2d(out_channels, out_channels, kernel_size=3, stride=1, padding=1)
        self.shortcut = (
            nn.Conv2d(in_channels, out_channels, kernel_size=1, stride=1, padding=0)
            if in_channels != out_channels
            else nn.Identity()
        )

    def forward_tokens(self, x: torch.Tensor) -> torch.Tensor:
        "the block on an NHWC map [B, h, w, pad64(in_channels)] in the compute dtype -> [B, h, w, pad64(out_channels)]"
        B, h, w, cin_pad = x.shape
        cout_pad = autograd.head_pad(self.conv1.out_channels, autograd.ENC_PAD)
        if isinstance(self.shortcut, nn.Identity):
            identity = x
        else:
            identity = autograd.head_linear(x.reshape(-1, cin_pad), (self.shortcut,), x.dtype, npad=cout_pad).view(B, h, w, cout_pad)
        out = autograd.act(autograd.conv3x3_padded(x, self.conv1, cout_pad), self._act_name)
        out = autograd.conv3x3_padded(out, self.conv2, cout_pad, residual=identity)
        return autograd.act(out, self._act_name)

    def forward(self, x):
        "x [B, in_channels, h, w] -> fp32 [B, out_channels, h, w]"
        ops._need_gpu(x)
        cin = self.conv1.in_channels
        nhwc = engine.bchw_to_nhwc(x, engine.compute_dtype())
        y = self.forward_tokens(F.pad(nhwc, (0, autograd.head_pad(cin, autograd.ENC_PAD) - cin)))
        return autograd.convert(y[..., :self.conv1.out_channels].contiguous(), torch.float32).permute(0, 3, 1, 2)


class DenseRepresentationEncoder(UniCeptionViTEncoderBase):
    "UniCeption Dense Representation Encoder"

    def __init__(
        self,
        name: str,
        in_chans: int = 3,
        enc_embed_dim: int = 1024,
        apply_pe: bool = True,
        input_size_for_pe: Union[int, Tuple[int, int]] = 518,
        patch_size: int = 14,
        intermediate_dims: List[int] = [588, 768, 1024],
        data_norm_type: str = "dense_rep_encoder",
        act_layer: Type[nn.Module] = nn.GELU,
        norm_layer: Optional[Callable] = partial(nn.LayerNorm, eps=1e-6),
        post_pe_norm_layer: Optional[Callable] = partial(nn.LayerNorm, eps=1e-6),
        interpolate_antialias: bool = False,
        interpolate_offset: float = 0.1,
        pretrained_checkpoint_path: str = None,
        *args,
        **kwargs,
    ):
        super().__init__(name=name, data_norm_type=data_norm_type, patch_size=patch_size, *args, **kwargs)
        self.in_chans = in_chans
        self.enc_embed_dim = enc_embed_dim
        self.intermediate_dims = intermediate_dims
        self.apply_pe = apply_pe
        build_act(act_layer)          # (refused here even when there is no residual block to refuse it)

        # pixel unshuffle and a conv projection patchify the input
        self.unshuffle = nn.PixelUnshuffle(self.patch_size)
        self.conv_in = nn.Conv2d(self.in_chans * (self.patch_size**2), self.intermediate_dims[0], 3, 1, 1)

        layers = []
        for intermediate_idx in range(len(self.intermediate_dims) - 1):
            layers.append(
                ResidualBlock(
                    in_channels=self.intermediate_dims[intermediate_idx],
                    out_channels=self.intermediate_dims[intermediate_idx + 1],
                    act_layer=act_layer,
                )
            )
        # final projection to the encoder embedding dim
        layers.append(nn.Conv2d(in_channels=self.intermediate_dims[-1], out_channels=self.enc_embed_dim, kernel_size=1, stride=1, padding=0))
        self.encoder = nn.Sequential(*layers)

        self.norm_layer = build_norm(norm_layer, enc_embed_dim, "norm_layer")
        if isinstance(self.norm_layer, nn.LayerNorm):
            nn.init.constant_(self.norm_layer.bias, 0)
            nn.init.constant_(self.norm_layer.weight, 1.0)

        if self.apply_pe:
            patch_HW = make_2tuple(patch_size)
            self.input_size_for_pe = make_2tuple(input_size_for_pe)
            self.patches_resolution = (
                self.input_size_for_pe[0] // patch_HW[0],
                self.input_size_for_pe[1] // patch_HW[1],
            )
            self.num_patches = self.patches_resolution[0] * self.patches_resolution[1]
            # sinusoidal positional encodings
            self.register_buffer("pos_embed", self._get_sinusoid_encoding_table(self.num_patches, self.enc_embed_dim, 70007))
            self.interpolate_antialias = interpolate_antialias
            self.interpolate_offset = interpolate_offset
            self.post_pe_norm = build_norm(post_pe_norm_layer, enc_embed_dim, "post_pe_norm_layer")
            if isinstance(self.post_pe_norm, nn.LayerNorm):
                nn.init.constant_(self.post_pe_norm.bias, 0)
                nn.init.constant_(self.post_pe_norm.weight, 1.0)

        self.pretrained_checkpoint_path = pretrained_checkpoint_path
        if self.pretrained_checkpoint_path:
            print(
                f"Loading custom pretrained Dense Representation Encoder checkpoint from {self.pretrained_checkpoint_path} ..."
            )
            ckpt = torch.load(self.pretrained_checkpoint_path, weights_only=False)
            print(self.load_state_dict(ckpt["model"]))

        if self.gradient_checkpointing:
            for i in range(len(self.encoder) - 1):
                self.encoder[i] = self.wrap_module_with_gradient_checkpointing(self.encoder[i])

    def _get_sinusoid_encoding_table(self, n_position, d_hid, base):
        "Sinusoid position encoding table: angle(pos, j) = pos / base^(2 (j // 2) / d_hid), sin on even and cos on odd columns (float64, stored fp32)"
        j = np.arange(d_hid)
        table = np.arange(n_position, dtype=np.float64)[:, None] / np.power(base, 2 * (j // 2) / d_hid)[None, :]
        table[:, 0::2] = np.sin(table[:, 0::2])
        table[:, 1::2] = np.cos(table[:, 1::2])
        return torch.FloatTensor(table)

    def interpolate_pos_encoding(self, features, height, width):
        "the position table [1, N, C] for `features` [B, N, C] of an input of height x width pixels, in features' dtype"
        return resize_pos_table(self.pos_embed.unsqueeze(0), features.shape[1], height, width, self.patch_size, self.interpolate_offset,
                                self.interpolate_antialias).to(features.dtype)

    def forward(self, encoder_input: Union[ViTEncoderInput, ViTEncoderNonImageInput]) -> ViTEncoderOutput:
        input_data = spatial_input(self, encoder_input, "Dense Representation Encoder", self.in_chans)
        B, C, height, width = input_data.shape
        P, E = self.patch_size, self.enc_embed_dim
        h, w = height // P, width // P
        dt = engine.compute_dtype()
        pad = lambda n: autograd.head_pad(n, autograd.ENC_PAD)      # noqa: E731
        x = autograd.unshuffle_rows(input_data, P, pad(C * P * P), dt).view(B, h, w, -1)
        x = autograd.conv3x3_padded(x, self.conv_in, pad(self.intermediate_dims[0]))
        for block in self.encoder[:-1]:
            x = block.forward_tokens(x)
        tokens = autograd.head_linear(x.reshape(B * h * w, -1), (self.encoder[-1],), dt, out_dtype=torch.float32, npad=pad(E))
        if tokens.shape[1] != E:
            tokens = tokens[:, :E].contiguous()
        if self.apply_pe:
            pe = pos_rows(self, self.pos_embed.unsqueeze(0), h * w, height, width)
            y = autograd.ln_pe_ln(tokens, B, h * w, self.norm_layer, pe, self.post_pe_norm, torch.float32)
        else:
            y = autograd.ln_pe_ln(tokens, B, h * w, self.norm_layer, None, None, torch.float32)
        return ViTEncoderOutput(features=engine.nlc_as_bchw(y, B, h, w))
