"""Tokenizer config table (reference: networks/__init__.py); only the continuous image tokenizer is on this path."""
from enum import Enum

from .configs import continuous_image as continuous_image_dict


class TokenizerConfigs(Enum):
    CI = continuous_image_dict
