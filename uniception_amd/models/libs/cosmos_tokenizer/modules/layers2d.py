"""2D layers of the continuous image tokenizer (reference: modules/layers2d.py) on the HIP kernels.

Maps are channels-last (NHWC) in one dtype between the patcher and the unpatcher:
  ResnetBlock   x' + conv2(silu(gn2(conv1(silu(gn1(x)))))): GroupNorm + SiLU is one pass (uc_group_norm_silu_nhwc), the 3x3 convolutions
                are uc_gemm's implicit GEMM with the skip added in conv2's epilogue, the 1x1 nin_shortcut is a GEMM;
  AttnBlock     GroupNorm -> q | k | v as ONE GEMM over the row-concatenated weights -> autograd.wide_attention (one head over all pixels,
                head_dim = channels) -> proj_out with the input added in its epilogue;
  Downsample    rows gathered with the right / bottom zero pad (uc_down2_gather) -> dense GEMM;
  Upsample      uc_upsample2_nhwc -> 3x3 convolution;
  Encoder       Patcher (48 coefficients zero-padded to 64 channels) -> conv_in -> levels -> mid -> norm_out + SiLU -> conv_out;
  Decoder       conv_in -> mid -> levels in reverse -> norm_out + SiLU -> conv_out (fp32) -> UnPatcher.
Narrow channel counts (z_channels = 16, the 48 coefficients) travel zero-padded to 64 / a multiple of 8; the zero rows / columns are
built into the prepared weights.  Module forward() keeps the reference's BCHW interface; forward_nhwc() is what the pipelines call.
Nothing reads a device value on the host."""
import math

import torch
import torch.nn as nn

from ..... import autograd, engine
from ....._lib import UcHipError
from .patching import Patcher, UnPatcher
from .utils import Normalize

LATENT_PAD = 64      # channel count the 16-channel latent maps travel with (zeros beyond z_channels): the GEMM routes' K granule


def _bchw(fn, x: torch.Tensor) -> torch.Tensor:
    "a forward_nhwc as the reference's BCHW forward, in the engine's compute dtype"
    y = fn(engine.bchw_to_nhwc(x, engine.compute_dtype()))
    return autograd.convert(y, torch.float32).permute(0, 3, 1, 2)


class Upsample(nn.Module):
    def __init__(self, in_channels: int):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, in_channels, kernel_size=3, stride=1, padding=1)

    def forward_nhwc(self, x: torch.Tensor) -> torch.Tensor:
        return autograd.conv3x3(autograd.upsample2(x), self.conv)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return _bchw(self.forward_nhwc, x)


class Downsample(nn.Module):
    def __init__(self, in_channels: int):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, in_channels, kernel_size=3, stride=2, padding=0)

    def forward_nhwc(self, x: torch.Tensor) -> torch.Tensor:
        return autograd.down2_conv(x, self.conv)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return _bchw(self.forward_nhwc, x)


class ResnetBlock(nn.Module):
    def __init__(self, *, in_channels: int, out_channels: int = None, dropout: float, **kwargs):
        super().__init__()
        self.in_channels = in_channels
        out_channels = in_channels if out_channels is None else out_channels
        self.norm1 = Normalize(in_channels)
        self.conv1 = nn.Conv2d(in_channels, out_channels, kernel_size=3, stride=1, padding=1)
        self.norm2 = Normalize(out_channels)
        self.dropout = nn.Dropout(dropout)
        self.conv2 = nn.Conv2d(out_channels, out_channels, kernel_size=3, stride=1, padding=1)
        self.nin_shortcut = (nn.Conv2d(in_channels, out_channels, kernel_size=1, stride=1, padding=0)
                             if in_channels != out_channels else nn.Identity())

    def check_supported(self) -> None:
        "what has no HIP path, said before any tensor is touched"
        if self.dropout.p > 0:
            raise UcHipError(f"ResnetBlock: dropout={self.dropout.p} has no HIP path (supported: 0.0)")
        for gn in (self.norm1, self.norm2):
            autograd.check_group_size(gn.num_channels, gn.num_groups, "ResnetBlock", group4=True)

    def forward_nhwc(self, x: torch.Tensor) -> torch.Tensor:
        h = autograd.conv3x3(autograd.group_norm_silu(x, self.norm1), self.conv1)
        h = autograd.group_norm_silu(h, self.norm2)
        skip = x
        if not isinstance(self.nin_shortcut, nn.Identity):
            B, H, W, C = x.shape
            skip = autograd.head_linear(x.reshape(-1, C), (self.nin_shortcut,), x.dtype).view(B, H, W, -1)
        return autograd.conv3x3(h, self.conv2, residual=skip)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        self.check_supported()
        return _bchw(self.forward_nhwc, x)


class AttnBlock(nn.Module):
    def __init__(self, in_channels: int):
        super().__init__()
        self.norm = Normalize(in_channels)
        self.q = nn.Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.k = nn.Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.v = nn.Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.proj_out = nn.Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)

    def check_supported(self) -> None:
        autograd.check_group_size(self.norm.num_channels, self.norm.num_groups, "AttnBlock")
        if self.norm.num_channels % 64:
            raise UcHipError(f"AttnBlock: {self.norm.num_channels} channels: the attention's products need a multiple of 64")

    def forward_nhwc(self, x: torch.Tensor, panel: int = autograd.WIDE_ATTN_PANEL) -> torch.Tensor:
        B, H, W, C = x.shape
        dt = x.dtype
        h = autograd.group_norm(x, self.norm, relu=False).reshape(B * H * W, C)
        qkv = autograd.head_linear(h, (self.q, self.k, self.v), dt)
        o = autograd.wide_attention(qkv, B, H * W, int(C) ** (-0.5), panel)
        return autograd.head_linear(o, (self.proj_out,), dt, residual=x.reshape(B * H * W, C)).view(B, H, W, C)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        self.check_supported()
        return _bchw(self.forward_nhwc, x)


def _check_tree(module: nn.Module) -> None:
    for m in module.modules():
        if isinstance(m, (ResnetBlock, AttnBlock, Patcher, UnPatcher)):
            m.check_supported()


def _mid(block_in: int, dropout: float) -> nn.Module:
    mid = nn.Module()
    mid.block_1 = ResnetBlock(in_channels=block_in, out_channels=block_in, dropout=dropout)
    mid.attn_1 = AttnBlock(block_in)
    mid.block_2 = ResnetBlock(in_channels=block_in, out_channels=block_in, dropout=dropout)
    return mid


def _level(c_in: int, c_out: int, n_blocks: int, dropout: float, with_attn: bool) -> nn.Module:
    "n_blocks residual blocks (the first one changes the width), each followed by an attention block when with_attn"
    level = nn.Module()
    level.block = nn.ModuleList([ResnetBlock(in_channels=c_in if i == 0 else c_out, out_channels=c_out, dropout=dropout) for i in range(n_blocks)])
    level.attn = nn.ModuleList([AttnBlock(c_out) for _ in range(n_blocks)] if with_attn else [])
    return level


def _run_level(level: nn.Module, h: torch.Tensor) -> torch.Tensor:
    for i, block in enumerate(level.block):
        h = block.forward_nhwc(h)
        if len(level.attn) > 0:
            h = level.attn[i].forward_nhwc(h)
    return h


class Encoder(nn.Module):
    def __init__(self, in_channels: int, channels: int, channels_mult: list, num_res_blocks: int, attn_resolutions: list, dropout: float,
                 resolution: int, z_channels: int, spatial_compression: int, **ignore_kwargs):
        super().__init__()
        self.num_resolutions = len(channels_mult)
        self.num_res_blocks = num_res_blocks
        patch_size = ignore_kwargs.get("patch_size", 1)
        self.patcher = Patcher(patch_size, ignore_kwargs.get("patch_method", "rearrange"))
        in_channels = in_channels * patch_size * patch_size
        self.num_downsamples = int(math.log2(spatial_compression)) - int(math.log2(patch_size))
        assert self.num_downsamples <= self.num_resolutions, f"{self.num_downsamples} Downsamples do not fit {self.num_resolutions} levels"
        self.conv_in = nn.Conv2d(in_channels, channels, kernel_size=3, stride=1, padding=1)
        # state_dict layout: down.L.block.i / down.L.attn.i (only where the level's map size is in attn_resolutions) / down.L.downsample
        self.in_ch_mult = (1,) + tuple(channels_mult)
        widths = [channels * m for m in self.in_ch_mult]          # width entering level L, widths[L + 1] leaving it
        size = resolution // patch_size                            # the level's map size at the config's nominal resolution
        self.down = nn.ModuleList()
        for lv in range(self.num_resolutions):
            self.down.append(_level(widths[lv], widths[lv + 1], num_res_blocks, dropout, size in attn_resolutions))
            if lv < self.num_downsamples:
                self.down[lv].downsample = Downsample(widths[lv + 1])
                size //= 2
        self.mid = _mid(widths[-1], dropout)
        self.norm_out = Normalize(widths[-1])
        self.conv_out = nn.Conv2d(widths[-1], z_channels, kernel_size=3, stride=1, padding=1)

    def check_supported(self) -> None:
        _check_tree(self)
        autograd.check_group_size(self.norm_out.num_channels, self.norm_out.num_groups, "Encoder.norm_out", group4=True)
        if self.conv_in.in_channels > LATENT_PAD or self.conv_out.out_channels > LATENT_PAD:
            raise UcHipError(f"Encoder: {self.conv_in.in_channels} patch coefficients / {self.conv_out.out_channels} latent channels exceed "
                             f"the padded width {LATENT_PAD}")

    def forward_nhwc(self, img: torch.Tensor, dt: torch.dtype) -> torch.Tensor:
        "fp32 NCHW image -> NHWC latent map [B, h, w, LATENT_PAD] in dt (z_channels real channels, zeros beyond)"
        self.check_supported()
        h = self.patcher.forward_nhwc(img, dt, LATENT_PAD)
        h = autograd.conv3x3_padded(h, self.conv_in, self.conv_in.out_channels)
        for i_level, level in enumerate(self.down):
            h = _run_level(level, h)
            if i_level < self.num_downsamples:
                h = level.downsample.forward_nhwc(h)
        h = self.mid.block_2.forward_nhwc(self.mid.attn_1.forward_nhwc(self.mid.block_1.forward_nhwc(h)))
        h = autograd.group_norm_silu(h, self.norm_out)
        return autograd.conv3x3_padded(h, self.conv_out, LATENT_PAD)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        y = self.forward_nhwc(x, engine.compute_dtype())[..., :self.conv_out.out_channels]
        return autograd.convert(y, torch.float32).permute(0, 3, 1, 2)


class Decoder(nn.Module):
    def __init__(self, out_channels: int, channels: int, channels_mult: list, num_res_blocks: int, attn_resolutions: list, dropout: float,
                 resolution: int, z_channels: int, spatial_compression: int, **ignore_kwargs):
        super().__init__()
        self.num_resolutions = len(channels_mult)
        self.num_res_blocks = num_res_blocks
        self.out_channels = out_channels
        patch_size = ignore_kwargs.get("patch_size", 1)
        self.unpatcher = UnPatcher(patch_size, ignore_kwargs.get("patch_method", "rearrange"))
        out_ch = out_channels * patch_size * patch_size
        self.num_upsamples = int(math.log2(spatial_compression)) - int(math.log2(patch_size))
        assert self.num_upsamples <= self.num_resolutions, f"{self.num_upsamples} Upsamples do not fit {self.num_resolutions} levels"
        n = self.num_resolutions
        widths = [channels * m for m in channels_mult]             # width leaving level L (the forward walks L = n - 1 .. 0)
        size = (resolution // patch_size) >> (n - 1)               # the deepest level's map size at the config's nominal resolution
        self.z_shape = (1, z_channels, size, size)
        self.conv_in = nn.Conv2d(z_channels, widths[-1], kernel_size=3, stride=1, padding=1)
        self.mid = _mid(widths[-1], dropout)
        # state_dict layout: up.L.block.i / up.L.attn.i / up.L.upsample, L the level's index
        levels, c_in = [None] * n, widths[-1]
        for lv in reversed(range(n)):
            levels[lv] = _level(c_in, widths[lv], num_res_blocks + 1, dropout, size in attn_resolutions)
            if lv >= n - self.num_upsamples:
                levels[lv].upsample = Upsample(widths[lv])
                size *= 2
            c_in = widths[lv]
        self.up = nn.ModuleList(levels)
        self.norm_out = Normalize(widths[0])
        self.conv_out = nn.Conv2d(widths[0], out_ch, kernel_size=3, stride=1, padding=1)

    def check_supported(self) -> None:
        _check_tree(self)
        autograd.check_group_size(self.norm_out.num_channels, self.norm_out.num_groups, "Decoder.norm_out", group4=True)
        if self.conv_in.in_channels > LATENT_PAD or self.conv_out.out_channels % 8:
            raise UcHipError(f"Decoder: {self.conv_in.in_channels} latent channels exceed the padded width {LATENT_PAD}, or the "
                             f"{self.conv_out.out_channels} output coefficients are not a multiple of 8")

    def forward_nhwc(self, z: torch.Tensor) -> torch.Tensor:
        "NHWC latent map [B, h, w, LATENT_PAD] (z_channels real channels, zeros beyond) -> fp32 NCHW image [B, out_channels, H, W]"
        self.check_supported()
        h = autograd.conv3x3_padded(z, self.conv_in, self.conv_in.out_channels)
        h = self.mid.block_2.forward_nhwc(self.mid.attn_1.forward_nhwc(self.mid.block_1.forward_nhwc(h)))
        for i_level in reversed(range(self.num_resolutions)):
            h = _run_level(self.up[i_level], h)
            if i_level >= self.num_resolutions - self.num_upsamples:
                h = self.up[i_level].upsample.forward_nhwc(h)
        h = autograd.group_norm_silu(h, self.norm_out)
        h = autograd.conv3x3_padded(h, self.conv_out, self.conv_out.out_channels, out_dtype=torch.float32)
        return self.unpatcher.forward_nhwc(h, self.out_channels)

    def forward(self, z: torch.Tensor) -> torch.Tensor:
        return self.forward_nhwc(pad_latent(engine.bchw_to_nhwc(z, engine.compute_dtype())))


def pad_latent(z: torch.Tensor) -> torch.Tensor:
    "NHWC latent map with zero channels appended up to LATENT_PAD"
    return z if z.shape[-1] == LATENT_PAD else torch.nn.functional.pad(z, (0, LATENT_PAD - z.shape[-1]))
