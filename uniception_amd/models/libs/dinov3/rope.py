"""Axial RoPE of the DINOv3 ViT (published `RopePositionEmbedding` + `rope_apply`; same arithmetic as transformers'
DINOv3ViTRopePositionEmbedding / apply_rotary_pos_emb, modeling_dinov3_vit.py:96-121,153-268), host side.

The coordinates are the patch centres normalised per axis to [-1, 1] (c = 2 (i + 0.5) / n - 1), the angle of frequency j is
2 pi c base^(-4j/D), a head's channels are laid out [y | x | y | x] (each D/4 wide), channel j pairs with j + D/2, and the class and
register tokens are not rotated.  uc_rope_axial does the rotation and computes no trigonometry: `RoPEAxial.tables` builds the two
(cos, sin) tables — [h, D/4, 2] for the rows, [w, D/4, 2] for the columns — in fp32 in the reference's order of operations, so on the
same device the table entries are the reference's cos / sin bit for bit.  In training mode the coordinates are augmented first
(shift, jitter, rescale: one random affine map per axis per call, the reference's distributions and draw order), which only changes
the two tiny tables.

`RoPEAxial` is a plain object — no parameters, not in the module tree, not in the state_dict (like the Perception Encoder's rope).
`bind` fixes the tables of one forward pass; the bound object is what the attention sub-layers take as their `rope`
(engine.is_axial_rope) — every block of a forward, the re-computation under gradient checkpointing and the backward's inverse
rotation see the same tables.
"""
import math
from typing import Optional

import numpy as np
import torch

from .... import engine, ops


class BoundRoPEAxial:
    "The axial RoPE of ONE token grid with its tables fixed: rotate_(q, k) in place (engine.self_attention, autograd.self_attn_sublayer)."
    _uc_axial_rope = True

    def __init__(self, prefix: int, grid_h: int, grid_w: int, table_y: torch.Tensor, table_x: torch.Tensor):
        self.prefix, self.grid_h, self.grid_w = prefix, grid_h, grid_w
        self.table_y, self.table_x = table_y, table_x

    def rotate_(self, q: torch.Tensor, k: Optional[torch.Tensor] = None, inverse: bool = False) -> None:
        "q, k: [B, prefix + grid_h * grid_w, H, D] views (stride(3) == 1); inverse: the gradient path"
        ops.rope_axial_(q, k, self.table_y, self.table_x, self.prefix, self.grid_h, self.grid_w, inverse=inverse)

    def __call__(self, *args, **kwargs):
        raise engine.UcHipError("the axial RoPE is not a positional-encoding callable: it serves the self-attention sub-layers "
                                "(sublayers.self_attn) only")


class RoPEAxial:
    """base: the period base (100); shift / jitter / rescale: the training-mode coordinate augmentation (None: off) — shift adds
    U(-shift, shift) per axis, jitter multiplies by exp(U(-log jitter, log jitter)) per axis, rescale by exp(U(-log rescale, log rescale))
    for both axes."""

    def __init__(self, head_dim: int, base: float = 100.0, shift: Optional[float] = None, jitter: Optional[float] = None,
                 rescale: Optional[float] = None):
        if head_dim % 4 != 0:
            raise engine.UcHipError(f"the axial RoPE needs head_dim % 4 == 0 (got {head_dim})")
        self.head_dim, self.base = head_dim, float(base)
        self.shift, self.jitter, self.rescale = shift, jitter, rescale
        # (built once on the host, like the reference's buffer: the device copies are bit copies of it)
        self.inv_freq = 1 / self.base ** torch.arange(0, 1, 4 / head_dim, dtype=torch.float32)       # [D/4]

    @property
    def augments(self) -> bool:
        return self.shift is not None or self.jitter is not None or self.rescale is not None

    @staticmethod
    def centres(n: int, device) -> torch.Tensor:
        "[n] fp32: the patch centres of one axis in [-1, 1]"
        c = torch.arange(0.5, n, dtype=torch.float32, device=device) / n
        return 2.0 * c - 1.0

    def augmented(self, cy: torch.Tensor, cx: torch.Tensor):
        "the training-mode affine map of the coordinates (device-side draws from PyTorch's generator, no host sync)"
        dev, dt = cy.device, cy.dtype
        if self.shift is not None:
            s = torch.empty((1, 2), device=dev, dtype=dt).uniform_(-self.shift, self.shift)
            cy, cx = cy + s[0, 0], cx + s[0, 1]
        if self.jitter is not None:
            r = float(np.log(self.jitter))
            j = torch.empty((1, 2), device=dev, dtype=dt).uniform_(-r, r).exp()
            cy, cx = cy * j[0, 0], cx * j[0, 1]
        if self.rescale is not None:
            r = float(np.log(self.rescale))
            m = torch.empty(1, device=dev, dtype=dt).uniform_(-r, r).exp()
            cy, cx = cy * m, cx * m
        return cy, cx

    def _table(self, c: torch.Tensor) -> torch.Tensor:
        ang = 2 * math.pi * c[:, None] * self.inv_freq.to(c.device)[None, :]
        return torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1).contiguous()                      # [n, D/4, 2]

    def _build(self, h: int, w: int, device, augment: bool):
        cy, cx = self.centres(h, device), self.centres(w, device)
        if augment:
            cy, cx = self.augmented(cy, cx)
        return self._table(cy), self._table(cx)

    def tables(self, h: int, w: int, device, training: bool = False):
        """(table_y [h, D/4, 2], table_x [w, D/4, 2]) fp32 (cos, sin).  Eval (or no augmentation configured): cached per (h, w, device);
        training with augmentation: rebuilt per call."""
        device = torch.device(device)
        if training and self.augments:
            with torch.no_grad():
                return self._build(h, w, device, True)
        return engine.prepared(self, ("axial", h, w, str(device)), (), lambda: self._build(h, w, device, False))

    def bind(self, prefix: int, h: int, w: int, device, training: bool = False) -> BoundRoPEAxial:
        return BoundRoPEAxial(prefix, h, w, *self.tables(h, w, device, training))
