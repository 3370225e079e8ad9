"""Cosmos decoder head (reference: prediction_heads/cosmos.py): one decoder of the continuous image tokenizer per output channel.

CosmosSingleChannel   latent [B, 16, h, w] -> 1x1 post_quant_conv -> convolutional decoder (libs/cosmos_tokenizer/modules/layers2d.py) ->
                      Haar unpatcher -> [B, 3, h P, w P] in fp32;
CosmosFeature         optional 1x1 `linear` (input_feature_dim -> 16 output_dim, ONE GEMM, fp32 output) -> 16-channel groups, one
                      CosmosSingleChannel each -> mean over each decoder's 3 channels -> x output_scaling + output_bias.
                      Returns (PixelTaskOutput(decoded_channels), x_split) like the reference.
The maps are channels-last in engine.head_dtype(); the 16-channel latents travel zero-padded to 64 channels.  The channel mean and the
affine output map are three elementwise torch ops on the [B, output_dim, H, W] result."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import autograd, engine
from ..._lib import UcHipError
from ..libs.cosmos_tokenizer.modules import DecoderType
from ..libs.cosmos_tokenizer.modules.layers2d import LATENT_PAD, pad_latent
from ..libs.cosmos_tokenizer.networks import TokenizerConfigs
from .base import PixelTaskOutput, PredictionHeadInput

COSMOS_LATENT_CHANNELS = 16


class CosmosSingleChannel(nn.Module):
    "A single Cosmos decoder: 16-channel latent features -> a 3-channel image in about [-1, 1]."

    def __init__(self, patch_size: int, pretrained_checkpoint_path: str = None, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.patch_size = patch_size
        assert self.patch_size in (8, 16), f"patch_size must be 8 or 16, got {self.patch_size}"
        tokenizer_config = TokenizerConfigs["CI"].value.copy()
        tokenizer_config.update(dict(spatial_compression=self.patch_size))
        z_channels = tokenizer_config.pop("z_channels")
        latent_channels = tokenizer_config.pop("latent_channels")
        decoder_name = tokenizer_config.get("decoder", DecoderType.Default.name)
        self.decoder = DecoderType[decoder_name].value(z_channels=z_channels, **tokenizer_config)
        self.post_quant_conv = torch.nn.Conv2d(latent_channels, z_channels, 1)
        if pretrained_checkpoint_path is not None:
            print(f"CosmosSingleChannel: weights from {pretrained_checkpoint_path}")
            ckpt = torch.load(pretrained_checkpoint_path, weights_only=False)
            print(self.load_state_dict(ckpt["model"]))

    def check_supported(self) -> None:
        "what has no HIP path, said before any tensor is touched"
        if not isinstance(self.decoder, DecoderType.Default.value):
            raise UcHipError(f"CosmosSingleChannel: decoder type {type(self.decoder).__name__} has no HIP path (supported: 'Default')")
        self.decoder.check_supported()

    def forward_nhwc(self, z: torch.Tensor) -> torch.Tensor:
        "NHWC latent [B, h, w, LATENT_PAD] in the head dtype (16 real channels, zeros beyond) -> fp32 image [B, 3, h P, w P]"
        B, h, w, _ = z.shape
        x = autograd.head_linear(z.reshape(B * h * w, LATENT_PAD), (self.post_quant_conv,), z.dtype, npad=LATENT_PAD)
        return self.decoder.forward_nhwc(x.view(B, h, w, LATENT_PAD))

    def forward(self, x: torch.Tensor):
        self.check_supported()
        assert x.shape[1] == self.post_quant_conv.in_channels, f"expected {self.post_quant_conv.in_channels} latent channels, got {x.shape[1]}"
        return self.forward_nhwc(pad_latent(engine.bchw_to_nhwc(x, engine.head_dtype())))


class CosmosFeature(nn.Module):
    "Low-resolution patch features -> pixel-wise features through one Cosmos decoder per output channel."

    def __init__(self, input_feature_dim: int, output_dim: int, patch_size: int, skip_linear: bool = False, single_channel_ckpt: str = None,
                 pretrained_checkpoint_path: str = None, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.input_feature_dim = input_feature_dim
        self.output_dim = output_dim
        self.patch_size = patch_size
        self.skip_linear = skip_linear
        self.pretrained_checkpoint_path = pretrained_checkpoint_path
        assert self.patch_size in (8, 16), f"patch_size must be 8 or 16, got {self.patch_size}"
        if not self.skip_linear:
            self.linear = nn.Conv2d(in_channels=self.input_feature_dim, out_channels=self.output_dim * COSMOS_LATENT_CHANNELS, kernel_size=1,
                                    stride=1, padding=0, bias=True)
        self.cosmos_decoders = nn.ModuleList([CosmosSingleChannel(patch_size=self.patch_size, pretrained_checkpoint_path=single_channel_ckpt,
                                                                  *args, **kwargs) for _ in range(self.output_dim)])
        self.output_scaling = nn.Parameter(torch.ones(1, self.output_dim, 1, 1))
        self.output_bias = nn.Parameter(torch.zeros(1, self.output_dim, 1, 1))
        if self.pretrained_checkpoint_path is not None:
            print(f"CosmosFeature: weights from {self.pretrained_checkpoint_path}")
            ckpt = torch.load(self.pretrained_checkpoint_path, weights_only=False)
            print(self.load_state_dict(ckpt["model"]))

    def check_supported(self) -> None:
        for dec in self.cosmos_decoders:
            dec.check_supported()

    def forward(self, feature_input: PredictionHeadInput):
        self.check_supported()
        x = feature_input.last_feature
        assert x.shape[1] == self.input_feature_dim, f"CosmosFeature: {x.shape[1]} input channels, built for {self.input_feature_dim}"
        assert self.skip_linear is False or x.shape[1] >= self.output_dim * COSMOS_LATENT_CHANNELS, "too few channels for the decoders"
        B, _, h, w = x.shape
        dt = engine.head_dtype()
        L = COSMOS_LATENT_CHANNELS
        if not self.skip_linear:
            rows = engine.bchw_to_nhwc(x, dt).reshape(B * h * w, -1)
            kp = autograd.head_pad(rows.shape[1])
            rows = rows if kp == rows.shape[1] else F.pad(rows, (0, kp - rows.shape[1]))
            lat = autograd.head_linear(rows, (self.linear,), dt, out_dtype=torch.float32).view(B, h, w, -1)     # fp32: it is an output
            x = lat[..., :self.output_dim * L].permute(0, 3, 1, 2)
        else:
            lat = x.permute(0, 2, 3, 1)
        x_split = list(torch.split(x, L, dim=1))
        output = []
        for i, decoder in enumerate(self.cosmos_decoders):
            z = pad_latent(autograd.convert(lat[..., i * L:(i + 1) * L], dt))
            output.append(torch.mean(decoder.forward_nhwc(z), dim=1, keepdim=True))
        x = torch.cat(output, dim=1)
        x = x * self.output_scaling + self.output_bias
        return PixelTaskOutput(decoded_channels=x), x_split
