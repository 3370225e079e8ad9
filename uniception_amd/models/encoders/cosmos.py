"""Cosmos encoder (reference: encoders/cosmos.py): the encoder half of the continuous image tokenizer (CI 8x8 / 16x16) as a feature
extractor, on the HIP kernels.

image [B, 3, H, W] (fp32, range [-1, 1]) -> Haar patcher -> convolutional encoder (libs/cosmos_tokenizer/modules/layers2d.py) -> 1x1
quant_conv -> identity formulation -> features [B, 16, H / patch_size, W / patch_size] in fp32.  The maps are channels-last in
engine.compute_dtype() (engine.precision(...)); GroupNorm statistics, the attention's softmax and the Haar arithmetic are fp32 in every
mode.  Forward and backward both run: gradients reach every parameter and the image."""
import torch

from ... import autograd, engine
from ..._lib import UcHipError
from ..libs.cosmos_tokenizer.modules import ContinuousFormulation, EncoderType
from ..libs.cosmos_tokenizer.modules.distributions import IdentityDistribution
from ..libs.cosmos_tokenizer.modules.layers2d import LATENT_PAD
from ..libs.cosmos_tokenizer.networks import TokenizerConfigs
from .base import UniCeptionViTEncoderBase, ViTEncoderInput, ViTEncoderOutput


class CosmosEncoder(UniCeptionViTEncoderBase):
    "Uniception Cosmos Encoder"

    def __init__(self, name: str, data_norm_type: str = "cosmos", patch_size: int = 8, pretrained_checkpoint_path: str = None, *args, **kwargs):
        super().__init__(name=name, data_norm_type=data_norm_type, patch_size=patch_size, *args, **kwargs)
        tokenizer_config = TokenizerConfigs["CI"].value.copy()
        tokenizer_config.update(dict(spatial_compression=self.patch_size))
        z_factor = tokenizer_config.pop("z_factor")
        z_channels = tokenizer_config.pop("z_channels")
        latent_channels = tokenizer_config.pop("latent_channels")
        encoder_name = kwargs.get("encoder", EncoderType.Default.name)
        self.encoder = EncoderType[encoder_name].value(z_channels=z_factor * z_channels, **tokenizer_config)
        self.quant_conv = torch.nn.Conv2d(z_factor * z_channels, z_factor * latent_channels, 1)
        formulation_name = kwargs.get("formulation", ContinuousFormulation.AE.name)
        self.distribution = ContinuousFormulation[formulation_name].value()
        if pretrained_checkpoint_path is not None:
            print(f"CosmosEncoder: weights from {pretrained_checkpoint_path}")
            ckpt = torch.load(pretrained_checkpoint_path, weights_only=False)
            print(self.load_state_dict(ckpt["model"]))

    def check_supported(self) -> None:
        "what has no HIP path, said before any tensor is touched"
        if not isinstance(self.distribution, IdentityDistribution):
            raise UcHipError(f"CosmosEncoder: formulation {type(self.distribution).__name__} has no HIP path (supported: 'AE')")
        if not isinstance(self.encoder, EncoderType.Default.value):
            raise UcHipError(f"CosmosEncoder: encoder type {type(self.encoder).__name__} has no HIP path (supported: 'Default')")
        self.encoder.check_supported()

    def encode(self, input_tensor: torch.Tensor):
        "image [B, 3, H, W], range [-1, 1] -> (latent [B, 16, h, w] fp32,)"
        self.check_supported()
        dt = engine.compute_dtype()
        img = input_tensor if input_tensor.dtype == torch.float32 else input_tensor.float()
        x = self.encoder.forward_nhwc(img, dt)                       # [B, h, w, LATENT_PAD], zeros beyond z_channels
        B, h, w, _ = x.shape
        n = self.quant_conv.out_channels
        lat = autograd.head_linear(x.reshape(B * h * w, LATENT_PAD), (self.quant_conv,), dt, out_dtype=torch.float32, npad=LATENT_PAD)
        output_latent = self.distribution(lat.view(B, h, w, LATENT_PAD)[..., :n].permute(0, 3, 1, 2))
        return output_latent[:-1]

    def forward(self, encoder_input: ViTEncoderInput) -> ViTEncoderOutput:
        self._check_data_normalization_type(encoder_input.data_norm_type)
        image = encoder_input.image
        assert isinstance(image, torch.Tensor) and image.ndim == 4 and image.shape[1] == 3, "CosmosEncoder: the image must be a [B, 3, H, W] tensor"
        assert image.shape[2] % self.patch_size == 0 and image.shape[3] % self.patch_size == 0, \
            f"CosmosEncoder: image size {tuple(image.shape[2:])} is not a multiple of patch_size {self.patch_size}"
        return ViTEncoderOutput(features=self.encode(image)[0].contiguous())
