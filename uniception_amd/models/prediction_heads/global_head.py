"""Global quantity regression head (reference: prediction_heads/global_head.py:16-120): the PoseHead's trunk with one output layer."""
import copy

import torch
import torch.nn as nn

from ... import autograd, engine
from .base import PredictionHeadInput, SummaryTaskOutput
from .pose_head import ResConvBlock, summary_trunk


class GlobalHead(nn.Module):
    "Global quantity regression head: decoded_channels [B, output_representation_dim]; needs an adaptor on top."

    def __init__(self, patch_size: int, input_feature_dim: int, num_resconv_block: int = 2, output_representation_dim: int = 1,
                 pretrained_checkpoint_path: str = None, *args, **kwargs):
        super().__init__()
        self.patch_size = patch_size
        self.input_feature_dim = input_feature_dim
        self.num_resconv_block = num_resconv_block
        self.output_representation_dim = output_representation_dim
        self.pretrained_checkpoint_path = pretrained_checkpoint_path
        self.output_dim = 4 * (self.patch_size**2)
        self.proj = nn.Conv2d(in_channels=self.input_feature_dim, out_channels=self.output_dim, kernel_size=1, stride=1, padding=0,
                              bias=True)
        self.res_conv = nn.ModuleList(
            [copy.deepcopy(ResConvBlock(self.output_dim, self.output_dim)) for _ in range(self.num_resconv_block)])
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.more_mlps = nn.Sequential(nn.Linear(self.output_dim, self.output_dim), nn.ReLU(),
                                       nn.Linear(self.output_dim, self.output_dim), nn.ReLU())
        self.fc_output = nn.Linear(self.output_dim, self.output_representation_dim)
        if self.pretrained_checkpoint_path is not None:
            print(f"Loading pretrained global head from {self.pretrained_checkpoint_path}")
            ckpt = torch.load(self.pretrained_checkpoint_path, weights_only=False)
            print(self.load_state_dict(ckpt["model"]))

    def forward(self, feature_input: PredictionHeadInput):
        feat = feature_input.last_feature  # (B, C, H, W)
        assert (
            feat.shape[1] == self.input_feature_dim
        ), f"Input feature dimension {feat.shape[1]} does not match expected dimension {self.input_feature_dim}"
        dt = engine.head_dtype()
        x = summary_trunk(self, feat, dt)
        n = self.output_representation_dim
        out = autograd.head_linear(x, (self.fc_output,), dt, torch.float32, npad=autograd.head_pad(n, 8))
        return SummaryTaskOutput(decoded_channels=out[:, :n])
