"""Prediction heads of the pointmap path (reference: prediction_heads/__init__.py)."""
from .base import (AdaptorInput, AdaptorOutput, PixelTaskOutput, PredictionHeadInput, PredictionHeadLayeredInput,  # noqa: F401
                   PredictionHeadOutput, RegressionAdaptorOutput, RegressionWithConfidenceAdaptorOutput,
                   UniCeptionAdaptorBase, UniCeptionPredictionHeadBase)
from .base import PredictionHeadTokenInput, SummaryTaskOutput  # noqa: F401,E402
from .global_head import GlobalHead  # noqa: F401,E402
from .mlp_head import MLPHead  # noqa: F401,E402
from .pose_head import PoseHead, ResConvBlock  # noqa: F401,E402
from .mlp_feature import MLPFeature  # noqa: F401,E402
from .moge_conv import MoGeConvFeature, ResidualConvBlock, normalized_view_plane_uv  # noqa: F401,E402
from .cosmos import COSMOS_LATENT_CHANNELS, CosmosFeature, CosmosSingleChannel  # noqa: F401,E402
