"""MLP head (reference: prediction_heads/mlp_head.py:13-92): tokens [B, C, T] -> proj -> num_mlp_layers x (Linear + ReLU) ->
output_proj -> [B, output_dim, T].  Each layer is one uc_gemm over the B T token rows; the hidden width (196 by default, no
multiple of 8) is padded to 64 columns by zeros in the prepared weights (autograd.head_linear)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import autograd, engine
from .base import PredictionHeadTokenInput, SummaryTaskOutput


class MLPHead(nn.Module):
    "MLP head converting tokens to the target representation."

    def __init__(self, input_feature_dim: int, output_dim: int, num_mlp_layers: int = 2, hidden_dim: int = 196,
                 pretrained_checkpoint_path: str = None, *args, **kwargs):
        super().__init__()
        self.input_feature_dim = input_feature_dim
        self.num_mlp_layers = num_mlp_layers
        self.hidden_dim = hidden_dim
        self.proj = nn.Linear(self.input_feature_dim, hidden_dim)
        self.mlp = nn.ModuleList()
        for _ in range(self.num_mlp_layers):
            self.mlp.append(nn.Sequential(nn.Linear(self.hidden_dim, self.hidden_dim), nn.ReLU()))
        self.output_proj = nn.Linear(self.hidden_dim, output_dim)
        if pretrained_checkpoint_path:
            print(f"Loading pretrained mlp head from {pretrained_checkpoint_path}")
            ckpt = torch.load(pretrained_checkpoint_path, weights_only=False)
            print(self.load_state_dict(ckpt["model"]))

    def forward(self, feature_input: PredictionHeadTokenInput):
        feat = feature_input.last_feature  # (B, C, T)
        assert feat.ndim == 3, f"Input feature tensor must have 3 dimensions (B, C, T), got {feat.ndim}"
        assert (
            feat.shape[1] == self.input_feature_dim
        ), f"Input feature dimension {feat.shape[1]} does not match expected dimension {self.input_feature_dim}"
        B, C, T = feat.shape
        dt = engine.head_dtype()
        # [B, C, T] as a BCHW map of height T and width 1: its channels-last rows are the B T tokens
        x = engine.bchw_to_nhwc(feat.unsqueeze(-1), dt).reshape(B * T, C)
        if C % 8:
            x = F.pad(x, (0, autograd.head_pad(C, 8) - C))
        x = autograd.head_linear(x, (self.proj,), dt)
        for layer in self.mlp:
            x = autograd.head_linear(x, (layer[0],), dt, relu=True)
        n = self.output_proj.out_features
        out = autograd.head_linear(x, (self.output_proj,), dt, torch.float32, npad=autograd.head_pad(n, 8))
        return SummaryTaskOutput(decoded_channels=out[:, :n].reshape(B, T, n).permute(0, 2, 1))  # (B, C, T)
