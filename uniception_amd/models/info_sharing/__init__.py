"""Info-sharing registry (reference: info_sharing/__init__.py:23-37): the cross-attention transformer of the DUSt3R path and the
global / alternating self-attention transformers built from the same kernels, and the differential cross-attention variant on the
fused differential-attention kernel."""
from .alternating_attention_transformer import (MultiViewAlternatingAttentionTransformer,
                                                MultiViewAlternatingAttentionTransformerIFR)
from .base import MultiViewTransformerInput, MultiViewTransformerOutput, UniCeptionInfoSharingBase  # noqa: F401
from .cross_attention_transformer import MultiViewCrossAttentionTransformer, MultiViewCrossAttentionTransformerIFR
from .diff_cross_attention_transformer import (DifferentialMultiViewCrossAttentionTransformer,
                                               DifferentialMultiViewCrossAttentionTransformerIFR)
from .global_attention_transformer import MultiViewGlobalAttentionTransformer, MultiViewGlobalAttentionTransformerIFR

INFO_SHARING_CLASSES = {
    "cross_attention": (MultiViewCrossAttentionTransformer, MultiViewCrossAttentionTransformerIFR),
    "alternating_attention": (MultiViewAlternatingAttentionTransformer, MultiViewAlternatingAttentionTransformerIFR),
    "global_attention": (MultiViewGlobalAttentionTransformer, MultiViewGlobalAttentionTransformerIFR),
}

# (the differential transformer is exported by name; the registry keeps the three keys tests/test_host_logic.py pins)
__all__ = ["INFO_SHARING_CLASSES", "MultiViewTransformerInput", "DifferentialMultiViewCrossAttentionTransformer",
           "DifferentialMultiViewCrossAttentionTransformerIFR"]
