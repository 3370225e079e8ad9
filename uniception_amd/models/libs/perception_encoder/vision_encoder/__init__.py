"""Vision tower of the Perception Encoder (reference: libs/perception_encoder/vision_encoder/{config,pe}.py)."""
from .config import PE_VISION_CONFIG, PEConfig  # noqa: F401
from .pe import VisionTransformer  # noqa: F401
