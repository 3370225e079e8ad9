"""Plain-PyTorch statements of the formulas behind the Cosmos tokenizer kernels (include/uc_hip.h), in whatever dtype the inputs have
(float64 as the reference of the GPU tests, bfloat16 / float16 as the same-dtype yardstick).  test_cosmos.py checks each of them against
torch.nn.functional on the CPU; test_cosmos_gpu.py checks the kernels against them."""
import torch


# ---- Haar patcher: NCHW [B, C, H, W] <-> NCHW [B, 16 C, H/4, W/4], channel index s2 * 4C + s1 * C + c ----
def haar_level(x):
    a, b, c, d = x[..., 0::2, 0::2], x[..., 0::2, 1::2], x[..., 1::2, 0::2], x[..., 1::2, 1::2]
    return torch.cat([a + b + c + d, a + b - c - d, a - b + c - d, a - b - c + d], dim=1) / 4


def haar_unlevel(p):
    ll, lh, hl, hh = p.chunk(4, dim=1)
    B, C, h, w = ll.shape
    x = p.new_empty((B, C, 2 * h, 2 * w))
    x[..., 0::2, 0::2] = ll + lh + hl + hh
    x[..., 0::2, 1::2] = ll + lh - hl - hh
    x[..., 1::2, 0::2] = ll - lh + hl - hh
    x[..., 1::2, 1::2] = ll - lh - hl + hh
    return x


def haar_patch(x):
    return haar_level(haar_level(x))


def haar_unpatch(p):
    return haar_unlevel(haar_unlevel(p))


# ---- GroupNorm + SiLU on an NHWC map ----
def _group_stats(x, G, eps):
    B, H, W, C = x.shape
    xg = x.reshape(B, H * W, G, C // G)
    mean = xg.mean(dim=(1, 3))
    rstd = 1.0 / torch.sqrt(xg.var(dim=(1, 3), unbiased=False) + eps)
    return mean, rstd


def _per_channel(v, C):
    "[B, G] -> [B, 1, 1, C]"
    return v.repeat_interleave(C // v.shape[1], dim=1)[:, None, None, :]


def group_norm_silu(x, gamma, beta, G, eps):
    "(y, mean [B, G], rstd [B, G]): y = z sigmoid(z), z = (x - mean) rstd gamma + beta"
    C = x.shape[-1]
    mean, rstd = _group_stats(x, G, eps)
    z = (x - _per_channel(mean, C)) * _per_channel(rstd, C) * gamma + beta
    return z * torch.sigmoid(z), mean, rstd


def group_norm_silu_bwd(dy, x, gamma, beta, G, eps):
    "(dx, dgamma, dbeta): g = dy silu'(z), silu'(z) = s (1 + z (1 - s)), then GroupNorm's backward with its two group sums"
    B, H, W, C = x.shape
    mean, rstd = _group_stats(x, G, eps)
    xh = (x - _per_channel(mean, C)) * _per_channel(rstd, C)
    z = xh * gamma + beta
    s = torch.sigmoid(z)
    g = dy * s * (1 + z * (1 - s))
    m = H * W * (C // G)
    gg = (g * gamma).reshape(B, H * W, G, C // G)
    s1 = gg.sum(dim=(1, 3)) / m
    s2 = (gg * xh.reshape(B, H * W, G, C // G)).sum(dim=(1, 3)) / m
    dx = _per_channel(rstd, C) * (g * gamma - _per_channel(s1, C) - xh * _per_channel(s2, C))
    return dx, (g * xh).sum(dim=(0, 1, 2)), g.sum(dim=(0, 1, 2))


# ---- Downsample operand rows: NHWC [B, H, W, C] -> [B (H/2) (W/2), 9 C], K ordered (ky, kx, c); row H and column W read as zero ----
def down2_rows(x):
    B, H, W, C = x.shape
    xp = x.new_zeros((B, H + 1, W + 1, C))
    xp[:, :H, :W] = x
    taps = [xp[:, ky:ky + H:2, kx:kx + W:2] for ky in range(3) for kx in range(3)]          # each [B, H/2, W/2, C]
    return torch.stack(taps, dim=3).reshape(B * (H // 2) * (W // 2), 9 * C)


def down2_rows_adjoint(drows, B, H, W):
    C = drows.shape[1] // 9
    d = drows.reshape(B, H // 2, W // 2, 3, 3, C)
    dxp = drows.new_zeros((B, H + 1, W + 1, C))
    for ky in range(3):
        for kx in range(3):
            dxp[:, ky:ky + H:2, kx:kx + W:2] += d[:, :, :, ky, kx]
    return dxp[:, :H, :W]


def down2_conv(x, weight, bias):
    "the Downsample on an NHWC map with an OIHW weight: rows times the (ky, kx, c)-ordered weight matrix"
    B, H, W, C = x.shape
    w2 = weight.permute(0, 2, 3, 1).reshape(weight.shape[0], -1)
    return (down2_rows(x) @ w2.t() + bias).reshape(B, H // 2, W // 2, -1)


# ---- nearest x2 upsample on an NHWC map ----
def upsample2(x):
    return x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def upsample2_adjoint(dy):
    return ((dy[:, 0::2, 0::2] + dy[:, 0::2, 1::2]) + dy[:, 1::2, 0::2]) + dy[:, 1::2, 1::2]


# ---- row softmax ----
def softmax_rows(s, scale):
    t = s * scale
    e = torch.exp(t - t.max(dim=1, keepdim=True).values)
    return e / e.sum(dim=1, keepdim=True)


def softmax_rows_bwd(p, dp, scale):
    return scale * p * (dp - (dp * p).sum(dim=1, keepdim=True))


# ---- single-head attention over all pixels: qkv [B N, 3C] -> [B N, C] ----
def wide_attention(qkv, B, N, scale):
    C = qkv.shape[1] // 3
    q, k, v = (qkv[:, i * C:(i + 1) * C].reshape(B, N, C) for i in range(3))
    p = softmax_rows((q @ k.transpose(1, 2)).reshape(B * N, N), scale).reshape(B, N, N)
    return (p @ v).reshape(B * N, C)
