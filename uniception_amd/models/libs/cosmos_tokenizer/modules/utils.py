"""Normalize and the swish non-linearity of the tokenizer layers (reference: modules/utils.py).  On the HIP path the two are one pass:
autograd.group_norm_silu."""
import torch


def Normalize(in_channels: int, num_groups: int = 32) -> torch.nn.GroupNorm:
    return torch.nn.GroupNorm(num_groups=num_groups, num_channels=in_channels, eps=1e-6, affine=True)
