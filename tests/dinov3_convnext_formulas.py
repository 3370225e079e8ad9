"""fp64 models of the DINOv3 ConvNeXt kernels (csrc/dwconv.hip), written from the contract in include/uc_hip.h and from nothing else:
uc_dwconv7x7_nhwc (both `flip` values), uc_dwconv7x7_nhwc_wgrad, uc_patch2_gather_nhwc and its adjoint.  Each returns the reference
and the magnitude its error bound is taken of.  Shared by tests/test_dinov3_convnext.py (the models against torch, planted defects)
and tests/test_dinov3_convnext_gpu.py (the kernels against the models, every element).

Bounds, derived and not measured.  Forward: 49 products and 50 additions in fp32 in a fixed order (bias first), so
|fp32 result - exact| <= gamma_50 * (|b| + sum |w x|), gamma_n = n u / (1 - n u), u = 2^-24 (Higham, Accuracy and Stability of Numerical
Algorithms, Lemma 3.1 / eq. 3.5 — a fused multiply-add rounds once, which only helps).  Storing rounds to nearest in the output
format: half an ulp more, taken at |reference| + the arithmetic bound (the stored value may sit one binade above the reference).
Weight gradient: one sum of B H W products per output, joined by `merge depth` further additions, whatever the tree:
gamma_(B H W + merge depth) * sum |dy x|; fp32 outputs, so no storage term."""
import torch

U32 = 2.0 ** -24
DEFECTS = ("tap_order_transposed", "padding_2", "bias_dropped", "flip_rows_only", "right_halo_not_zeroed")
# (B, H, W, C): height under 7 — every output misses tap rows; a map inside the halo radius; one pixel; a tile seam in both directions
# for any tile up to 16, channels no multiple of 16; more than two tiles down, channels a multiple of 64
WITNESS_SHAPES = [(2, 5, 9, 24), (1, 2, 3, 96), (1, 1, 1, 8), (2, 17, 19, 40), (1, 33, 18, 64)]


def gamma(n: int) -> float:
    return n * U32 / (1.0 - n * U32)


def half_ulp(x, dtype):
    "half a unit in the last place of `dtype` at magnitude x (fp64 tensor); 0 for fp32 — the fp32 roundings are the arithmetic bound"
    if dtype == torch.float32:
        return torch.zeros_like(x)
    bits, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    e = torch.frexp(x.abs().clamp_min(2.0 ** emin).cpu())[1].double() - 1     # floor(log2 x) exactly, clamped to the smallest normal
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - bits - 1).to(x.device)


def forward_bound(ref, mag, dtype):
    arith = gamma(50) * mag
    return arith + half_ulp(ref.abs() + arith, dtype)


def _padded(x, before: int, after: int, right_fill=None):
    "x [B,H,W,C] with `before` zero rows / columns in front and `after` behind; right_fill: what the columns right of the map hold"
    B, H, W, C = x.shape
    xp = x.new_zeros(B, H + before + after, W + before + after, C)
    xp[:, before:before + H, before:before + W] = x
    if right_fill is not None:
        xp[:, before:before + H, before + W:] = right_fill
    return xp


def dwconv7x7_model(x, w49, bias=None, flip=False, defect=None):
    """(y, mag) in fp64: y[b,i,j,c] = bias[c] + sum_(ky,kx) w49[t][c] x[b, i+ky-3, j+kx-3, c], t = ky 7 + kx (48 - t with flip), zero
    outside the map; mag = |bias| + sum |w x|.  defect: one of DEFECTS, planted into the evaluation (the tests show each is caught)."""
    assert defect is None or defect in DEFECTS
    x, w49 = x.double(), w49.double()
    B, H, W, C = x.shape
    before = 2 if defect == "padding_2" else 3
    xp = _padded(x, before, 6 - before, x[:, :, -1:, :] if defect == "right_halo_not_zeroed" else None)
    y = x.new_zeros(B, H, W, C)
    mag = x.new_zeros(B, H, W, C)
    if bias is not None and defect != "bias_dropped":
        y = y + bias.double()
        mag = mag + bias.double().abs()
    for ky in range(7):
        for kx in range(7):
            t = kx * 7 + ky if defect == "tap_order_transposed" else ky * 7 + kx
            if flip:
                t = (6 - t // 7) * 7 + t % 7 if defect == "flip_rows_only" else 48 - t
            term = w49[t] * xp[:, ky:ky + H, kx:kx + W]
            y = y + term
            mag = mag + term.abs()
    return y, mag


def dwconv7x7_wgrad_model(x, dy):
    "(dw [49, C], db [C], mag_w [49, C], mag_b [C]) in fp64: dw[t][c] = sum_(b,i,j) dy[b,i,j,c] x[b, i+ky-3, j+kx-3, c], db = sum dy"
    x, dy = x.double(), dy.double()
    B, H, W, C = x.shape
    xp = _padded(x, 3, 3)
    dw, mw = x.new_zeros(49, C), x.new_zeros(49, C)
    for ky in range(7):
        for kx in range(7):
            term = dy * xp[:, ky:ky + H, kx:kx + W]
            dw[ky * 7 + kx] = term.sum((0, 1, 2))
            mw[ky * 7 + kx] = term.abs().sum((0, 1, 2))
    return dw, dy.sum((0, 1, 2)), mw, dy.abs().sum((0, 1, 2))


def patch2_gather_model(x):
    "rows [B (H//2) (W//2), 4 C]: rows[(b,i,j)][(ky 2 + kx) C + c] = x[b, 2i+ky, 2j+kx, c]; an odd last row / column is not read"
    B, H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    return x[:, :2 * Ho, :2 * Wo].reshape(B, Ho, 2, Wo, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B * Ho * Wo, 4 * C)


def patch2_gather_bwd_model(drows, B, H, W):
    "the adjoint: dx [B, H, W, C], zero in an odd last row / column"
    Ho, Wo = H // 2, W // 2
    C = drows.shape[1] // 4
    dx = drows.new_zeros(B, H, W, C)
    dx[:, :2 * Ho, :2 * Wo] = drows.reshape(B, Ho, Wo, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * Ho, 2 * Wo, C)
    return dx


def patch2_weight(weight):
    "[Cout, Cin, 2, 2] -> the GEMM weight [Cout, 4 Cin], K ordered (ky, kx, c)"
    return weight.permute(0, 2, 3, 1).reshape(weight.shape[0], -1)
