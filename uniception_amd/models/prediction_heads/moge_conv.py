"""MoGe convolutional decoder (reference: prediction_heads/moge_conv.py:18-246, after microsoft/MoGe moge/model/v1.py).

The head runs on channels-last maps in engine.head_dtype():
  projection   the sum of the 1x1 `projects` is ONE uc_gemm over the K-concatenated features (weights concatenated along K, biases
               summed; autograd.sum_linear);
  stage        [x | uv | 0] -> ConvTranspose2d(k = s = 2) as GEMM + scatter (the channel axis zero-padded to 64: 514 -> 576, the
               zero columns built into the prepared weight) -> replicate-padded 3x3 convolution -> ResidualConvBlocks;
  block        GroupNorm + ReLU (uc_group_norm_nhwc) -> conv -> GroupNorm + ReLU -> conv (+ skip, added in the crop pass);
  conv         padding_mode="replicate" = replicate pad -> uc_gemm's zero-padded 3x3 convolution on the (H + 2) x (W + 2) map -> crop:
               the interior of that output is the replicate-padded convolution exactly;
  output       half-pixel bilinear resize to the image size -> [x | uv | 0] (66 -> 96 channels) -> per output block a 3x3
               convolution (its ReLU applied in the crop pass that produces the last convolution's operand), the optional blocks and
               the last convolution, which writes fp32.
The reference's torch.utils.checkpoint calls change no number and are not reproduced.  Nothing reads a device value on the host."""
import math
from typing import List, Literal, Optional, Union

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import autograd, engine
from ..._lib import UcHipError
from .base import PixelTaskOutput, PredictionHeadLayeredInput


class ResidualConvBlock(nn.Module):
    "x + conv(relu(gn(conv(relu(gn(x)))))), the skip through a 1x1 convolution when the channel count changes (moge_conv.py:18-65)."

    # activation name -> module factory; only "relu" has a HIP path (check_supported), the others are kept so that a checkpoint's
    # module tree can be built and inspected
    ACTIVATIONS = {"relu": (nn.ReLU, {}), "leaky_relu": (nn.LeakyReLU, {"negative_slope": 0.2}), "silu": (nn.SiLU, {}), "elu": (nn.ELU, {})}

    def __init__(self, in_channels: int, out_channels: Optional[int] = None, hidden_channels: Optional[int] = None,
                 padding_mode: str = "replicate", activation: Literal["relu", "leaky_relu", "silu", "elu"] = "relu",
                 norm: Literal["group_norm", "layer_norm"] = "group_norm"):
        super().__init__()
        if activation not in self.ACTIVATIONS:
            raise ValueError(f"Unsupported activation function: {activation}")
        act_cls, act_kw = self.ACTIVATIONS[activation]
        c_in, c_out, c_mid = in_channels, out_channels or in_channels, hidden_channels or in_channels
        self.activation = activation
        self.padding_mode = padding_mode
        # state_dict layout: layers.{0,3} the two GroupNorms (one group over the input; 32-channel groups, or one group for
        # norm="layer_norm", over the hidden map), layers.{2,5} the two 3x3 convolutions, skip_connection a 1x1 convolution when needed
        groups = (1, c_mid // 32 if norm == "group_norm" else 1)
        widths = (c_in, c_mid, c_out)
        stack = []
        for i in range(2):
            stack += [nn.GroupNorm(groups[i], widths[i]), act_cls(inplace=True, **act_kw),
                      nn.Conv2d(widths[i], widths[i + 1], kernel_size=3, padding=1, padding_mode=padding_mode)]
        self.layers = nn.Sequential(*stack)
        self.skip_connection = nn.Identity() if c_in == c_out else nn.Conv2d(c_in, c_out, kernel_size=1)

    def check_supported(self) -> None:
        "what has no HIP path, said before any tensor is touched"
        if self.activation != "relu":
            raise UcHipError(f"ResidualConvBlock: activation={self.activation!r} has no HIP path (the GroupNorm kernel fuses ReLU only)")
        if self.padding_mode != "replicate":
            raise UcHipError(f"ResidualConvBlock: padding_mode={self.padding_mode!r} has no HIP path (supported: 'replicate')")
        for gn in (self.layers[0], self.layers[3]):
            autograd.check_group_size(gn.num_channels, gn.num_groups, "ResidualConvBlock")

    def forward_nhwc(self, x: torch.Tensor, relu_out: bool = False) -> torch.Tensor:
        "the block on an NHWC map in the head dtype; relu_out: a ReLU on the block's output, applied in its last pass"
        h = autograd.group_norm(x, self.layers[0], relu=True)
        h = autograd.conv3x3_replicate(h, self.layers[2])
        h = autograd.group_norm(h, self.layers[3], relu=True)
        skip = x if isinstance(self.skip_connection, nn.Identity) else autograd.conv1x1(x, self.skip_connection)
        return autograd.conv3x3_replicate(h, self.layers[5], residual=skip, relu_out=relu_out)

    def forward(self, x):
        self.check_supported()
        y = self.forward_nhwc(engine.bchw_to_nhwc(x, engine.head_dtype()))
        return autograd.convert(y, torch.float32).permute(0, 3, 1, 2)


def normalized_view_plane_uv(width: int, height: int, aspect_ratio: Optional[float] = None, dtype: Optional[torch.dtype] = None,
                             device: Optional[torch.device] = None) -> torch.Tensor:
    """[height, width, 2] = (u, v) of every pixel centre on a view plane whose half-diagonal is 1: with a = aspect_ratio
    (default width / height) the plane spans +-a / sqrt(1 + a^2) horizontally and +-1 / sqrt(1 + a^2) vertically, and pixel i of n along
    an axis sits at half_span * (2 i + 1 - n) / n.  Evaluated in float64 and rounded once to `dtype`."""
    a = width / height if aspect_ratio is None else float(aspect_ratio)
    diag = math.hypot(a, 1.0)

    def centres(n: int, half_span: float) -> torch.Tensor:
        return (2.0 * torch.arange(n, dtype=torch.float64) + (1 - n)) * (half_span / n)

    uv = torch.empty((height, width, 2), dtype=torch.float64)
    uv[..., 0] = centres(width, a / diag)[None, :]
    uv[..., 1] = centres(height, 1.0 / diag)[:, None]
    return uv.to(dtype=dtype or torch.get_default_dtype(), device=device)


_uv_cache = {}


def _uv_tail(h: int, w: int, aspect: float, npad: int, dt: torch.dtype, device) -> torch.Tensor:
    "[h, w, 2 + npad]: the UV channels (host, float64, rounded once to dt) followed by npad zero channels; cached"
    key = (h, w, float(aspect), npad, dt, str(device))
    t = _uv_cache.get(key)
    if t is None:
        if len(_uv_cache) > 64:
            _uv_cache.clear()
        uv = normalized_view_plane_uv(width=w, height=h, aspect_ratio=aspect, dtype=torch.float64)
        t = _uv_cache[key] = F.pad(uv, (0, npad)).to(dt).to(device)
    return t


def _with_uv(x: torch.Tensor, aspect: float, granule: int) -> torch.Tensor:
    "[x | uv | 0]: the two UV channels appended to an NHWC map, the channel count zero-padded to a multiple of `granule`"
    B, h, w, C = x.shape
    tail = _uv_tail(h, w, aspect, autograd.head_pad(C + 2, granule) - (C + 2), x.dtype, x.device)
    return torch.cat([x, tail.unsqueeze(0).expand(B, -1, -1, -1)], dim=-1)


def _upsampler(c_in: int, c_out: int) -> nn.Sequential:
    "x2: ConvTranspose2d(k = s = 2) whose four taps start out equal (nearest-neighbour upsampling of a 1x1 convolution), then a 3x3 convolution"
    up = nn.ConvTranspose2d(c_in, c_out, kernel_size=2, stride=2)
    with torch.no_grad():
        up.weight.copy_(up.weight[:, :, :1, :1].expand_as(up.weight).clone())
    return nn.Sequential(up, nn.Conv2d(c_out, c_out, kernel_size=3, padding=1, padding_mode="replicate"))


def _output_block(c_in: int, c_out: int, hidden: int, n_blocks: int, width: int, last_size: int, norm: str) -> nn.Sequential:
    "3x3 convolution to `width` channels, n_blocks residual blocks, ReLU, the last convolution (last_size x last_size) to c_out channels"
    blocks = [ResidualConvBlock(width, width, hidden * width, activation="relu", norm=norm) for _ in range(n_blocks)]
    return nn.Sequential(nn.Conv2d(c_in, width, kernel_size=3, padding=1, padding_mode="replicate"), *blocks, nn.ReLU(inplace=True),
                         nn.Conv2d(width, c_out, kernel_size=last_size, padding=last_size // 2, padding_mode="replicate"))


class MoGeConvFeature(nn.Module):
    "Multi-feature projection -> three x2 upsampling stages of residual conv blocks -> resize to the image -> output blocks."

    def __init__(self, patch_size: int, num_features: int, input_feature_dims: Union[int, List[int]], dim_out: List[int],
                 dim_proj: int = 512, dim_upsample: List[int] = [256, 128, 64], dim_times_res_block_hidden: int = 2,
                 num_res_blocks: int = 2, res_block_norm: Literal["group_norm", "layer_norm"] = "group_norm", last_res_blocks: int = 0,
                 last_conv_channels: int = 32, last_conv_size: int = 1, pretrained_checkpoint_path: Optional[str] = None, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.patch_size = patch_size
        if isinstance(input_feature_dims, int):
            input_feature_dims = [input_feature_dims] * num_features
        self.input_feature_dims = input_feature_dims
        self.dim_out = list(dim_out)
        # state_dict layout: projects.i | upsample_blocks.i.0.{0: transposed conv, 1: 3x3 conv}, upsample_blocks.i.j: residual blocks |
        # output_block.i.{0: 3x3 conv, 1..: residual blocks, then ReLU, last conv}
        hidden = dim_times_res_block_hidden
        self.projects = nn.ModuleList([nn.Conv2d(c, dim_proj, kernel_size=1) for c in self.input_feature_dims[:num_features]])
        stages, width = [], dim_proj
        for out_ch in dim_upsample:
            blocks = [ResidualConvBlock(out_ch, out_ch, hidden * out_ch, activation="relu", norm=res_block_norm) for _ in range(num_res_blocks)]
            stages.append(nn.Sequential(_upsampler(width + 2, out_ch), *blocks))          # (+ 2: the UV channels)
            width = out_ch
        self.upsample_blocks = nn.ModuleList(stages)
        self.output_block = nn.ModuleList([_output_block(width + 2, n, hidden, last_res_blocks, last_conv_channels, last_conv_size, res_block_norm)
                                           for n in dim_out])
        self.pretrained_checkpoint_path = pretrained_checkpoint_path
        if self.pretrained_checkpoint_path is not None:
            print(f"Loading pretrained DPT dense feature head from {self.pretrained_checkpoint_path}")
            ckpt = torch.load(self.pretrained_checkpoint_path, weights_only=False)
            print(self.load_state_dict(ckpt["model"]))

    def check_supported(self) -> None:
        for m in self.modules():
            if isinstance(m, ResidualConvBlock):
                m.check_supported()
        if sum(self.input_feature_dims) % 8 != 0:
            raise UcHipError(f"MoGeConvFeature: the input feature dims {self.input_feature_dims} must add up to a multiple of 8")
        for ob in self.output_block:
            if ob[-1].kernel_size not in ((1, 1), (3, 3)):
                raise UcHipError(f"MoGeConvFeature: last_conv_size={ob[-1].kernel_size[0]} has no HIP path (supported: 1, 3)")

    def _output(self, block: nn.Sequential, xp: torch.Tensor, dt: torch.dtype) -> torch.Tensor:
        "one output block on the replicate-padded [x | uv | 0] map (padded once for all blocks): fp32 [B, H, W, dim_out]"
        first, res, last = block[0], list(block[1:-2]), block[-1]
        y = autograd.conv3x3_replicate(xp, first, relu_out=not res, padded=True)        # (the block's ReLU: in the pass that writes the last conv's operand)
        for i, rb in enumerate(res):
            y = rb.forward_nhwc(y, relu_out=i == len(res) - 1)
        if last.kernel_size == (1, 1):
            o = autograd.out_conv1x1(y, last, dt, autograd.head_pad(last.out_channels, 8))
        else:
            o = autograd.conv3x3_replicate(y, last, out_dtype=torch.float32)
        return o[..., :last.out_channels]

    def forward(self, head_input: PredictionHeadLayeredInput) -> PixelTaskOutput:
        self.check_supported()
        img_h, img_w = head_input.target_output_shape
        feats = head_input.list_features
        assert len(feats) == len(self.projects), f"expected {len(self.projects)} feature maps, got {len(feats)}"
        for f, c in zip(feats, self.input_feature_dims):
            assert f.shape[1] == c, f"Input feature dimension mismatch: {f.shape[1]} != {c}"
        B, _, h, w = feats[0].shape
        dt = engine.head_dtype()
        aspect = img_w / img_h
        toks = [engine.bchw_to_nhwc(f, dt).reshape(B * h * w, f.shape[1]) for f in feats]
        x = autograd.sum_linear(toks[0] if len(toks) == 1 else torch.cat(toks, dim=1), self.projects, dt).view(B, h, w, -1)
        # (patch_h, patch_w) -> x2 -> x4 -> x8
        for block in self.upsample_blocks:
            x = _with_uv(x, aspect, 64)            # UV coordinates: awareness of the image aspect ratio
            x = autograd.conv_transpose_padded(x, block[0][0])
            x = autograd.conv3x3_replicate(x, block[0][1])
            for rb in list(block)[1:]:
                x = rb.forward_nhwc(x)
        x = autograd.resize_bilinear(x, img_h, img_w, False)
        xp = autograd.replicate_pad(_with_uv(x, aspect, 32))       # the first convolutions of all output blocks read this one map
        out = [self._output(block, xp, dt) for block in self.output_block]
        out = out[0] if len(out) == 1 else torch.cat(out, dim=-1)
        return PixelTaskOutput(decoded_channels=out.permute(0, 3, 1, 2))
