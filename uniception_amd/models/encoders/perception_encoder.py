"""Perception Encoder wrappers (reference: encoders/perception_encoder.py:14-223) around the HIP vision tower
(models/libs/perception_encoder/vision_encoder/pe.py).

The reference downloads the published weights in its constructor; here nothing is fetched: the architecture is built from the config
table and the weights come from `pretrained_checkpoint_path` (a {"model": state_dict} file with the reference's names under "model.",
tools/convert_checkpoint.py --mode perception_encoder writes one from an original PE checkpoint) or stay at their initialisation.
Built: core/base, core/large, lang/large.  The giant models (head_dim 96) raise UcHipError; lang/base raises the reference's
RuntimeError (its table names a config that does not exist).  The returned BCHW features are a channels-last view of the token rows
(the reference materialises a contiguous NCHW copy): the same values.
"""
from typing import List, Optional, Union

import torch

from ... import engine
from ..libs.perception_encoder.vision_encoder import pe
from ..utils.intermediate_feature_return import IntermediateFeatureReturner
from .base import UniCeptionViTEncoderBase, ViTEncoderInput, ViTEncoderOutput

_EMBED_DIM = {"small": 384, "base": 768, "large": 1024, "giant": 1536}
MODEL_CKPT_DICT = {        # (checkpoint_type, size) -> config name, as the reference has it ("PE-Lang-B16-224" is no config there either)
    ("core", "base"): "PE-Core-B16-224",
    ("core", "large"): "PE-Core-L14-336",
    ("core", "giant"): "PE-Core-G14-448",
    ("lang", "base"): "PE-Lang-B16-224",
    ("lang", "large"): "PE-Lang-L14-448",
    ("lang", "giant"): "PE-Lang-G14-448",
    ("spatial", "giant"): "PE-Spatial-G14-448",
}


class PerceptionEncoder(UniCeptionViTEncoderBase):
    "UniCeption Perception Encoder (encoders/perception_encoder.py:14-123)"

    def __init__(self, name: str, data_norm_type: str = "perception_encoder", patch_size: int = 14, size: str = "large",
                 checkpoint_type: str = "core", pretrained_checkpoint_path: str = None, gradient_checkpointing: bool = False,
                 keep_first_n_layers: Optional[int] = None, *args, **kwargs):
        super().__init__(name=name, data_norm_type=data_norm_type, size=size, patch_size=patch_size,
                         gradient_checkpointing=gradient_checkpointing, *args, **kwargs)
        self.enc_embed_dim = _EMBED_DIM[size]
        model_str = MODEL_CKPT_DICT.get((checkpoint_type, size), None)
        if model_str is None:
            raise ValueError(f"Unsupported combination of checkpoint_type '{checkpoint_type}' and size '{size}'.")
        self.model = pe.VisionTransformer.from_config(model_str, pretrained=False)
        if keep_first_n_layers is not None:
            self.model.truncate(keep_first_n_layers)
        self.model.set_grad_checkpointing(gradient_checkpointing)       # (models/utils/checkpointing.py around every kept block)
        if pretrained_checkpoint_path:
            print(f"Loading custom pretrained Perception Encoder checkpoint from {pretrained_checkpoint_path}")
            ckpt = torch.load(pretrained_checkpoint_path, weights_only=False)
            print(self.load_state_dict(ckpt["model"]))

    def _check(self, encoder_input):
        self._check_data_normalization_type(encoder_input.data_norm_type)
        assert isinstance(encoder_input.image, torch.Tensor), "Input must be a torch.Tensor"
        assert encoder_input.image.ndim == 4, "Input must be of shape (B, C, H, W)"
        B, C, H, W = encoder_input.image.shape
        assert C == 3, "Input must have 3 channels"
        assert H % self.patch_size == 0 and W % self.patch_size == 0, \
            f"Input shape must be divisible by patch size: {self.patch_size}"
        return B, H // self.patch_size, W // self.patch_size

    @staticmethod
    def _as_bchw(feat, B, h, w):
        "[B, h w, C] patch tokens -> BCHW: plain (differentiable) views in training, else the channels-last view the heads consume"
        if feat.requires_grad:
            return feat.reshape(B, h, w, -1).permute(0, 3, 1, 2)
        return engine.nlc_as_bchw(feat.reshape(B * h * w, -1), B, h, w)

    def forward(self, encoder_input: ViTEncoderInput) -> ViTEncoderOutput:
        B, h, w = self._check(encoder_input)
        feats = self.model.forward_features(encoder_input.image, norm=True, strip_cls_token=True)
        return ViTEncoderOutput(features=self._as_bchw(feats, B, h, w))


class PerceptionEncoderIntermediateFeatureReturner(PerceptionEncoder, IntermediateFeatureReturner):
    "Intermediate Feature Returner for UniCeption Perception Encoder (encoders/perception_encoder.py:126-223)"

    def __init__(self, name: str, data_norm_type: str = "perception_encoder", patch_size: int = 14, size: str = "large",
                 checkpoint_type: str = "core", pretrained_checkpoint_path: str = None, gradient_checkpointing: bool = False,
                 keep_first_n_layers: Optional[int] = None, indices: Optional[Union[int, List[int]]] = 1, norm_intermediate: bool = True,
                 *args, **kwargs):
        PerceptionEncoder.__init__(self, name=name, data_norm_type=data_norm_type, patch_size=patch_size, size=size,
                                   checkpoint_type=checkpoint_type, pretrained_checkpoint_path=pretrained_checkpoint_path,
                                   gradient_checkpointing=gradient_checkpointing, keep_first_n_layers=keep_first_n_layers, *args, **kwargs)
        IntermediateFeatureReturner.__init__(self, indices=indices, norm_intermediate=norm_intermediate)

    def forward(self, encoder_input: ViTEncoderInput) -> List[ViTEncoderOutput]:
        B, h, w = self._check(encoder_input)
        if self.indices is None:
            self.indices = range(len(self.model.transformer.resblocks))
        feats = self.model.get_intermediate_layers(x=encoder_input.image, n=self.indices, norm=self.norm_intermediate, strip_cls_token=True)
        return [ViTEncoderOutput(features=self._as_bchw(f, B, h, w)) for f in feats]
