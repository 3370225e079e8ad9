"""The arithmetic of uc_rope_axial written out in torch (any dtype, CPU or GPU): the model of the kernel's indexing the CPU test holds
against transformers' apply_rotary_pos_emb, and the fp64 evaluation (with its per-element rounding bound) the GPU test holds the
kernel against.  Both read the same fp32 (cos, sin) tables the kernel reads."""
import torch


def rope_axial_model(t, table_y, table_x, prefix, grid_h, grid_w, inverse=False, with_bound=False):
    """t [B, N, H, D], N == prefix + grid_h * grid_w; tables [grid, D/4, 2].  Channel j of [0, D/4) pairs with j + D/2 under table_y of
    the token's row, channel D/4 + j with D/4 + j + D/2 under table_x of its column; tokens [0, prefix) pass through.  Returns the
    rotated tensor in t's dtype arithmetic (pass fp64 in for the reference), and with_bound the per-element |u c| + |v s|."""
    B, N, H, D = t.shape
    Q = D // 4
    assert N == prefix + grid_h * grid_w and D % 4 == 0
    p = torch.arange(N - prefix, device=t.device)
    ty, tx = table_y.to(t.dtype)[p // grid_w], table_x.to(t.dtype)[p % grid_w]          # [hw, Q, 2]
    cos = torch.cat([ty[..., 0], tx[..., 0]], dim=-1)[None, :, None, :]                  # [1, hw, 1, 2Q]: the [y | x] half
    sin = torch.cat([ty[..., 1], tx[..., 1]], dim=-1)[None, :, None, :]
    if inverse:
        sin = -sin
    u, v = t[:, prefix:, :, :2 * Q], t[:, prefix:, :, 2 * Q:]
    out = t.clone()
    out[:, prefix:, :, :2 * Q] = u * cos - v * sin
    out[:, prefix:, :, 2 * Q:] = v * cos + u * sin
    if not with_bound:
        return out
    mag = torch.zeros_like(t)
    mag[:, prefix:, :, :2 * Q] = (u * cos).abs() + (v * sin).abs()
    mag[:, prefix:, :, 2 * Q:] = (v * cos).abs() + (u * sin).abs()
    return out, mag
