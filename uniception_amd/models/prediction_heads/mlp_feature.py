"""Linear head with an MLP in front (reference: prediction_heads/mlp_feature.py:17-110): Mlp (fc1 -> GELU -> fc2) on the token rows,
then LinearFeature's 1x1 convolution and pixel shuffle.  fc1 carries GELU in its epilogue, the data-gradient GEMM of fc2 GELU'
(autograd.MlpFn: MlpSubLayerFn without the LayerNorm and the residual)."""
from typing import Union

import torch
import torch.nn as nn

from ... import autograd, engine
from ..._lib import UcHipError
from .base import PixelTaskOutput, PredictionHeadInput


class Mlp(nn.Module):
    "parameter holder with the reference's layout (utils/transformer_blocks.py:66-89); MLPFeature runs it through autograd.mlp"

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, bias=True, drop=0.0):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        bias = bias if isinstance(bias, (tuple, list)) else (bias, bias)
        drop_probs = drop if isinstance(drop, (tuple, list)) else (drop, drop)
        self.fc1 = nn.Linear(in_features, hidden_features, bias=bias[0])
        self.act = act_layer()
        self.drop1 = nn.Dropout(drop_probs[0])
        self.fc2 = nn.Linear(hidden_features, out_features, bias=bias[1])
        self.drop2 = nn.Dropout(drop_probs[1])


class MLPFeature(nn.Module):
    "Patch features -> Mlp -> Conv2d 1x1 (C -> output_dim * P^2) -> pixel_shuffle(P)."

    def __init__(self, input_feature_dim: Union[int, str], patch_size: int, output_dim: int, mlp_ratio: int = 4, act_layer=nn.GELU,
                 bias=True, drop=0.0, pretrained_checkpoint_path: str = None, *args, **kwargs):
        super().__init__(*args, **kwargs)
        if isinstance(input_feature_dim, str):
            input_feature_dim = eval(input_feature_dim)
        self.input_feature_dim = input_feature_dim
        self.output_dim = output_dim
        self.patch_size = patch_size
        self.pretrained_checkpoint_path = pretrained_checkpoint_path
        self.act_layer = act_layer
        self.mlp = Mlp(in_features=self.input_feature_dim, hidden_features=int(mlp_ratio * self.input_feature_dim), act_layer=act_layer,
                       drop=drop, bias=bias)
        self.linear = nn.Conv2d(in_channels=self.input_feature_dim, out_channels=self.output_dim * (self.patch_size**2), kernel_size=1,
                                stride=1, padding=0, bias=True)
        if self.pretrained_checkpoint_path is not None:
            print(f"Loading pretrained linear dense feature head from {self.pretrained_checkpoint_path}")
            ckpt = torch.load(self.pretrained_checkpoint_path, weights_only=False)
            print(self.load_state_dict(ckpt["model"]))

    def forward(self, feature_input: PredictionHeadInput):
        x = feature_input.last_feature
        assert x.shape[1] == self.input_feature_dim, f"Input feature dimension mismatch: {x.shape[1]} != {self.input_feature_dim}"
        if not (isinstance(self.mlp.act, nn.GELU) and getattr(self.mlp.act, "approximate", "none") == "none"):
            raise UcHipError(f"MLPFeature: act_layer={type(self.mlp.act).__name__} has no HIP path (supported: nn.GELU)")
        B, C, h, w = x.shape
        dt = engine.head_dtype()
        tok = engine.bchw_to_nhwc(x, dt).reshape(B * h * w, C)
        hidden = self.mlp.fc1.out_features
        drops = autograd.make_drops(self.training, x.device, B, h * w, C, p_out=self.mlp.drop2.p, hidden=hidden, p_mid=self.mlp.drop1.p)
        y = autograd.mlp(tok, self.mlp.fc1, self.mlp.fc2, "gelu", dt, drops)
        y = autograd.linear(y, self.linear.weight, self.linear.bias, self.linear, dt, torch.float32)
        return PixelTaskOutput(decoded_channels=autograd.pixel_shuffle(y, B, h, w, self.patch_size, self.output_dim))
