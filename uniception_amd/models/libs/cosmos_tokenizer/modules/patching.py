"""Patcher / UnPatcher (reference: modules/patching.py): log2(patch_size) levels of the 2x2 Haar transform applied to every channel,
sub-bands concatenated as [ll | lh | hl | hh].  The HIP path evaluates the two levels of patch_size = 4 in one pass (uc_haar_patch /
uc_haar_unpatch) and works on channels-last maps; the buffers are kept (non-persistent, as in the reference) for attribute parity."""
import math

import torch

from ..... import autograd, engine
from ....._lib import UcHipError

_WAVELETS = {"haar": torch.tensor([0.7071067811865476, 0.7071067811865476]), "rearrange": torch.tensor([1.0, 1.0])}


class _PatchBase(torch.nn.Module):
    def __init__(self, patch_size: int = 1, patch_method: str = "haar"):
        super().__init__()
        self.patch_size = patch_size
        self.patch_method = patch_method
        self.register_buffer("wavelets", _WAVELETS[patch_method].clone(), persistent=False)
        self.range = range(int(math.log2(patch_size)))
        self.register_buffer("_arange", torch.arange(2), persistent=False)

    def check_supported(self) -> None:
        "what has no HIP path, said before any tensor is touched"
        if self.patch_method != "haar" or self.patch_size != 4:
            raise UcHipError(f"{type(self).__name__}: patch_method={self.patch_method!r} with patch_size={self.patch_size} has no HIP path "
                             "(supported: 'haar' with patch_size 4)")


class Patcher(_PatchBase):
    def forward_nhwc(self, img: torch.Tensor, dt: torch.dtype, ld=None) -> torch.Tensor:
        "fp32 NCHW image -> NHWC coefficients [B, H/4, W/4, ld] in dt (16 C real channels, zeros beyond)"
        self.check_supported()
        if img.shape[-2] % 4 or img.shape[-1] % 4:
            raise UcHipError(f"Patcher: image size {tuple(img.shape[-2:])} must be a multiple of 4")
        return autograd.haar_patch(img, dt, ld)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.forward_nhwc(x, torch.float32).permute(0, 3, 1, 2)


class UnPatcher(_PatchBase):
    def forward_nhwc(self, rows: torch.Tensor, out_channels: int) -> torch.Tensor:
        "NHWC coefficients [B, h, w, >= 16 out_channels] -> fp32 NCHW image [B, out_channels, 4h, 4w]"
        self.check_supported()
        return autograd.haar_unpatch(rows, out_channels)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        self.check_supported()
        if x.shape[1] % 16:
            raise UcHipError(f"UnPatcher: {x.shape[1]} channels are not 16 sub-bands of whole channels")
        return self.forward_nhwc(engine.bchw_to_nhwc(x, torch.float32), x.shape[1] // 16)
