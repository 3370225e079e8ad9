"""Names the wrappers look up (reference: libs/cosmos_tokenizer/modules/__init__.py): the 2D encoder / decoder and the two continuous
formulations."""
from enum import Enum

from .distributions import GaussianDistribution, IdentityDistribution
from .layers2d import Decoder, Encoder


class EncoderType(Enum):
    Default = Encoder


class DecoderType(Enum):
    Default = Decoder


class ContinuousFormulation(Enum):
    VAE = GaussianDistribution
    AE = IdentityDistribution
