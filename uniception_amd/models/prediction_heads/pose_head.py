"""Pose regression head (reference: prediction_heads/pose_head.py:18-159, after Reloc3r / MaRePo): a 1x1-conv projection, residual
blocks of three 1x1 convolutions, the mean over the tokens, two Linear + ReLU layers and the translation / rotation outputs.

On the token matrix every layer is one uc_gemm with bias, ReLU and (third convolution of a block) the residual in its epilogue; the
mean is uc_token_pool; fc_t and fc_rot are one GEMM on their row-concatenated weights.  Hidden widths are padded to 64 columns inside
(autograd.head_linear); parameters, state_dict and outputs have the reference's shapes."""
import copy

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import autograd, engine
from .base import PredictionHeadInput, SummaryTaskOutput


def _tokens(feat: torch.Tensor, dt: torch.dtype, granule: int) -> torch.Tensor:
    "BCHW -> [B h w, C] rows in dt (engine.bchw_to_nhwc), the channel axis zero-padded to `granule` columns where it is not one already."
    B, C, h, w = feat.shape
    tok = engine.bchw_to_nhwc(feat, dt).reshape(B * h * w, C)
    return tok if C % granule == 0 else F.pad(tok, (0, autograd.head_pad(C, granule) - C))


class ResConvBlock(nn.Module):
    "head_skip(res) + relu(conv3(relu(conv2(relu(conv1(res)))))), all 1x1 (reference: pose_head.py:18-47)."

    def __init__(self, in_channels: int, out_channels: int, *args, **kwargs):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.head_skip = (nn.Identity() if self.in_channels == self.out_channels
                          else nn.Conv2d(self.in_channels, self.out_channels, 1, 1, 0))
        self.res_conv1 = nn.Conv2d(self.in_channels, self.out_channels, 1, 1, 0)
        self.res_conv2 = nn.Conv2d(self.out_channels, self.out_channels, 1, 1, 0)
        self.res_conv3 = nn.Conv2d(self.out_channels, self.out_channels, 1, 1, 0)

    def forward_tokens(self, tok, dt, out_dtype=None, pool=None):
        """The block on token rows [M, padded in_channels] -> [M, padded out_channels]; pool = (B, T): the fp32 [B, padded
        out_channels] mean over each sample's rows instead (the block's output is then not handed out)."""
        x = autograd.head_linear(tok, (self.res_conv1,), dt, relu=True)
        x = autograd.head_linear(x, (self.res_conv2,), dt, relu=True)
        skip = tok if isinstance(self.head_skip, nn.Identity) else autograd.head_linear(tok, (self.head_skip,), dt)
        return autograd.head_linear(x, (self.res_conv3,), dt, out_dtype, relu=True, residual=skip, pool=pool)

    def forward(self, res):
        B, C, h, w = res.shape
        assert C == self.in_channels, f"Input channels {C} do not match expected {self.in_channels}"
        dt = engine.head_dtype()
        tok = _tokens(res, dt, autograd.HEAD_PAD if isinstance(self.head_skip, nn.Identity) else 8)
        y = self.forward_tokens(tok, dt, out_dtype=torch.float32)
        return y[:, :self.out_channels].view(B, h, w, self.out_channels).permute(0, 3, 1, 2)


def summary_trunk(head, feat: torch.Tensor, dt: torch.dtype) -> torch.Tensor:
    "proj -> res_conv blocks -> mean over the tokens -> more_mlps of a PoseHead / GlobalHead: [B, padded 4 P^2] rows in dt."
    B, _, h, w = feat.shape
    x = autograd.head_linear(_tokens(feat, dt, 8), (head.proj,), dt)
    n = head.num_resconv_block
    for i in range(n):
        x = head.res_conv[i].forward_tokens(x, dt, pool=(B, h * w) if i == n - 1 else None)
    if n == 0:
        x = autograd.token_pool(x, B, h * w)
    x = autograd.head_linear(x, (head.more_mlps[0],), dt, relu=True)
    return autograd.head_linear(x, (head.more_mlps[2],), dt, relu=True)


class PoseHead(nn.Module):
    "Pose regression head: decoded_channels [B, 3 + rot_representation_dim] (translation | rotation); needs an adaptor on top."

    def __init__(self, patch_size: int, input_feature_dim: int, num_resconv_block: int = 2, rot_representation_dim: int = 4,
                 pretrained_checkpoint_path: str = None, *args, **kwargs):
        super().__init__()
        self.patch_size = patch_size
        self.input_feature_dim = input_feature_dim
        self.num_resconv_block = num_resconv_block
        self.rot_representation_dim = rot_representation_dim
        self.pretrained_checkpoint_path = pretrained_checkpoint_path
        self.output_dim = 4 * (self.patch_size**2)
        self.proj = nn.Conv2d(in_channels=self.input_feature_dim, out_channels=self.output_dim, kernel_size=1, stride=1, padding=0,
                              bias=True)
        self.res_conv = nn.ModuleList(
            [copy.deepcopy(ResConvBlock(self.output_dim, self.output_dim)) for _ in range(self.num_resconv_block)])
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.more_mlps = nn.Sequential(nn.Linear(self.output_dim, self.output_dim), nn.ReLU(),
                                       nn.Linear(self.output_dim, self.output_dim), nn.ReLU())
        self.fc_t = nn.Linear(self.output_dim, 3)
        self.fc_rot = nn.Linear(self.output_dim, self.rot_representation_dim)
        if self.pretrained_checkpoint_path is not None:
            print(f"Loading pretrained pose head from {self.pretrained_checkpoint_path}")
            ckpt = torch.load(self.pretrained_checkpoint_path, weights_only=False)
            print(self.load_state_dict(ckpt["model"]))

    def forward(self, feature_input: PredictionHeadInput):
        feat = feature_input.last_feature  # (B, C, H, W)
        assert (
            feat.shape[1] == self.input_feature_dim
        ), f"Input feature dimension {feat.shape[1]} does not match expected dimension {self.input_feature_dim}"
        dt = engine.head_dtype()
        x = summary_trunk(self, feat, dt)
        n = 3 + self.rot_representation_dim
        out = autograd.head_linear(x, (self.fc_t, self.fc_rot), dt, torch.float32, npad=autograd.head_pad(n, 8))
        return SummaryTaskOutput(decoded_channels=out[:, :n])
