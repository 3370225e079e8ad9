"""Encoder factory, restricted to the encoders with a HIP path (reference: encoders/__init__.py:32-140)."""
from .base import (EncoderGlobalRepInput, EncoderGlobalRepOutput, EncoderInput, EncoderOutput, UniCeptionEncoderBase,  # noqa: F401
                   UniCeptionViTEncoderBase, ViTEncoderInput, ViTEncoderNonImageInput, ViTEncoderOutput)
from .cosmos import CosmosEncoder
from .croco import CroCoEncoder, CroCoIntermediateFeatureReturner
from .dense_rep_encoder import DenseRepresentationEncoder, ResidualBlock  # noqa: F401
from .dinov2 import DINOv2Encoder, DINOv2IntermediateFeatureReturner
from .dinov3 import (DINOv3ConvNextEncoder, DINOv3ConvNextIntermediateFeatureReturner, DINOv3Encoder,  # noqa: F401
                     DINOv3IntermediateFeatureReturner)
from .global_rep_encoder import GlobalRepresentationEncoder
from .image_normalizations import IMAGE_NORMALIZATION_DICT  # noqa: F401
from .patch_embedder import PatchEmbedder
from .perception_encoder import PerceptionEncoder, PerceptionEncoderIntermediateFeatureReturner
from .pixio import PixioEncoder

ENCODER_CONFIGS = {
    "cosmos": {"class": CosmosEncoder, "supported_models": ["Cosmos-Tokenizer CI8x8", "Cosmos-Tokenizer CI16x16"]},
    "croco": {"class": CroCoEncoder, "intermediate_feature_returner_class": CroCoIntermediateFeatureReturner,
              "supported_models": ["CroCov2", "DUSt3R", "MASt3R"]},
    "dense_rep_encoder": {"class": DenseRepresentationEncoder, "supported_models": ["Dense-Representation-Encoder"]},
    "dinov2": {"class": DINOv2Encoder, "intermediate_feature_returner_class": DINOv2IntermediateFeatureReturner,
               "supported_models": ["DINOv2", "DINOv2-Registers", "DINOv2-Depth-Anythingv2"]},
    "dinov3": {"class": DINOv3Encoder, "intermediate_feature_returner_class": DINOv3IntermediateFeatureReturner,
               "supported_models": ["DINOv3-ViT"]},
    "dinov3_convnext": {"class": DINOv3ConvNextEncoder, "intermediate_feature_returner_class": DINOv3ConvNextIntermediateFeatureReturner,
                        "supported_models": ["DINOv3-ConvNext"]},
    "global_rep_encoder": {"class": GlobalRepresentationEncoder, "supported_models": ["Global-Representation-Encoder"]},
    "patch_embedder": {"class": PatchEmbedder, "supported_models": ["Patch-Embedder"]},
    "perception_encoder": {"class": PerceptionEncoder, "intermediate_feature_returner_class": PerceptionEncoderIntermediateFeatureReturner,
                           "supported_models": ["Perception Encoder Core", "Preception Encoder Spatial"]},
    "pixio": {"class": PixioEncoder, "supported_models": ["Pixio-Encoder"]},
}


def encoder_factory(encoder_str: str, **kwargs):
    "encoder_factory('croco', name=..., data_norm_type=..., ...) -> CroCoEncoder"
    if encoder_str not in ENCODER_CONFIGS:
        raise ValueError(f"Unknown encoder: {encoder_str}. For valid encoder_str options, please use print_available_encoder_models()")
    return ENCODER_CONFIGS[encoder_str]["class"](**kwargs)


def feature_returner_encoder_factory(encoder_str: str, **kwargs):
    if encoder_str not in ENCODER_CONFIGS:
        raise ValueError(f"Unknown encoder: {encoder_str}. For valid encoder_str options, please use print_available_encoder_models()")
    return ENCODER_CONFIGS[encoder_str]["intermediate_feature_returner_class"](**kwargs)


def get_available_encoders():
    return list(ENCODER_CONFIGS.keys())


def print_available_encoder_models():
    for name, cfg in ENCODER_CONFIGS.items():
        print(f"{name}: {', '.join(cfg['supported_models'])}")
