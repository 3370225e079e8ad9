"""Vision tower configurations of the Perception Encoder (reference: vision_encoder/config.py:29-156), restated.  There is no
checkpoint download here: weights come from a local file (VisionTransformer.from_config(..., checkpoint_path=...))."""
from dataclasses import dataclass, replace
from typing import Optional


@dataclass
class PEConfig:
    "Vision Tower Config."
    patch_size: int
    width: int
    layers: int
    heads: int
    mlp_ratio: float
    output_dim: Optional[int]

    ls_init_value: float = None
    drop_path: float = 0.0

    image_size: int = (224,)          # (the reference's default is this 1-tuple; every entry below sets it)
    use_abs_posemb: bool = True
    use_cls_token: bool = False
    use_rope2d: bool = True

    pool_type: str = "attn"
    attn_pooler_heads: int = 8

    use_ln_pre: bool = True
    use_ln_post: bool = True


def _lang(core: PEConfig, **kw) -> PEConfig:
    "PE Lang / Spatial: the Core tower without pooling, projection and ln_post, with LayerScale"
    return replace(core, image_size=448, pool_type="none", use_ln_post=False, output_dim=None, ls_init_value=0.1, **kw)


PE_VISION_CONFIG = {}
PE_VISION_CONFIG["PE-Core-G14-448"] = PEConfig(image_size=448, patch_size=14, width=1536, layers=50, heads=16, mlp_ratio=8960 / 1536,
                                               pool_type="attn", output_dim=1280, use_cls_token=False)
PE_VISION_CONFIG["PE-Core-L14-336"] = PEConfig(image_size=336, patch_size=14, width=1024, layers=24, heads=16, mlp_ratio=4.0,
                                               pool_type="attn", output_dim=1024, use_cls_token=True)
PE_VISION_CONFIG["PE-Core-B16-224"] = PEConfig(image_size=224, patch_size=16, width=768, layers=12, heads=12, mlp_ratio=4.0,
                                               pool_type="attn", output_dim=1024, use_cls_token=True)
PE_VISION_CONFIG["PE-Lang-G14-448"] = _lang(PE_VISION_CONFIG["PE-Core-G14-448"], layers=47)
PE_VISION_CONFIG["PE-Lang-L14-448"] = _lang(PE_VISION_CONFIG["PE-Core-L14-336"], layers=23)
PE_VISION_CONFIG["PE-Spatial-G14-448"] = _lang(PE_VISION_CONFIG["PE-Core-G14-448"])
