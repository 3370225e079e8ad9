"""The continuous image tokenizer's default config (reference: networks/configs.py:continuous_image)."""
from ..modules import ContinuousFormulation, DecoderType, EncoderType

continuous_image = dict(
    attn_resolutions=[32],             # map sizes at which the levels carry attention blocks
    channels=128,                      # base width
    channels_mult=[2, 4, 4],           # width multiplier per level
    dropout=0.0,
    in_channels=3,
    spatial_compression=16,            # overwritten by the wrappers' patch_size (8 | 16)
    num_res_blocks=2,
    out_channels=3,
    resolution=1024,
    patch_size=4,                      # of the Haar patcher: two levels
    patch_method="haar",
    latent_channels=16,
    z_channels=16,
    z_factor=1,
    name="CI",
    formulation=ContinuousFormulation.AE.name,
    encoder=EncoderType.Default.name,
    decoder=DecoderType.Default.name,
)
