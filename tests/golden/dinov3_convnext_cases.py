"""DINOv3 ConvNeXt cases pinned to an independent implementation (HuggingFace transformers' DINOv3ConvNextModel) — shared by the golden
generator (make_golden_dinov3_convnext_hf.py), the CPU test and the GPU test.  A tiny configuration that still takes every branch:
stage widths 96, 128, 192, 256 (96 is no multiple of 64: the GEMM routes of the tiny / small sizes' first stage), depths 1, 1, 2, 1,
LayerScale `gamma` drawn away from 1 (0.1 N(0,1), the name-keyed filler's 1-D rule), NON-SQUARE images — 64x96 and 96x64, whose last
stage is 2x3 / 3x2: smaller than the stencil's radius — and 48x80, whose maps are 12x20, 6x10, 3x5, 1x2: an odd map goes through the
floor of the stride-2 gather.  The weights are held under transformers' names; the tests put them through
uniception_amd.tools.convert_checkpoint (--mode dinov3_convnext), which exercises the key map."""
import torch

HIDDEN_SIZES, DEPTHS = [96, 128, 192, 256], [1, 1, 2, 1]
DINOV3_CONVNEXT_CASES = {
    "64x96": dict(hw=(64, 96), B=2, seed=41),
    "96x64": dict(hw=(96, 64), B=2, seed=42),
    "48x80": dict(hw=(48, 80), B=1, seed=43),
}
# cases that also carry gradients (transformers' autograd): loss = <features, Wf>, seeded cotangent
DINOV3_CONVNEXT_GRAD_CASES = ("64x96", "48x80")
# 48x80 is divisible by 16, the wrapper's default patch_size; every case is divisible by the stem's 4
PATCH_SIZE = 16


def convnext_size():
    "the `size` dict DINOv3ConvNextEncoder takes for this configuration"
    return dict(hidden_sizes=list(HIDDEN_SIZES), depths=list(DEPTHS))


def convnext_hf_config_kwargs():
    "keyword arguments of transformers' DINOv3ConvNextConfig for this configuration"
    return dict(num_channels=3, hidden_sizes=list(HIDDEN_SIZES), depths=list(DEPTHS), hidden_act="gelu", layer_norm_eps=1e-6,
                layer_scale_init_value=1e-6, drop_path_rate=0.0)


def convnext_image(c):
    g = torch.Generator().manual_seed(c["seed"])
    return torch.randn(c["B"], 3, *c["hw"], generator=g)


def convnext_hf_shapes():
    "key -> shape of a transformers DINOv3ConvNextModel state_dict of this configuration"
    W, shapes = HIDDEN_SIZES, {}
    for i in range(4):
        s = f"model.stages.{i}."
        if i == 0:
            down = [("0.weight", (W[0], 3, 4, 4)), ("0.bias", (W[0],)), ("1.weight", (W[0],)), ("1.bias", (W[0],))]
        else:
            down = [("0.weight", (W[i - 1],)), ("0.bias", (W[i - 1],)), ("1.weight", (W[i], W[i - 1], 2, 2)), ("1.bias", (W[i],))]
        for n, shp in down:
            shapes[s + "downsample_layers." + n] = shp
        for j in range(DEPTHS[i]):
            p, C = s + f"layers.{j}.", W[i]
            for n, shp in [("gamma", (C,)), ("depthwise_conv.weight", (C, 1, 7, 7)), ("depthwise_conv.bias", (C,)), ("layer_norm.weight", (C,)),
                           ("layer_norm.bias", (C,)), ("pointwise_conv1.weight", (4 * C, C)), ("pointwise_conv1.bias", (4 * C,)),
                           ("pointwise_conv2.weight", (C, 4 * C)), ("pointwise_conv2.bias", (C,))]:
                shapes[p + n] = shp
    shapes["layer_norm.weight"] = (W[-1],)
    shapes["layer_norm.bias"] = (W[-1],)
    return shapes


def convnext_hf_state_dict():
    "Parameters under transformers' DINOv3ConvNextModel names, filled by the name-keyed filler (one set of weights for every case)."
    from oracle import dust3r_oracle as O
    sd = {k: torch.empty(*shp) for k, shp in convnext_hf_shapes().items()}
    O.fill_state_dict_(sd)
    return sd


def convnext_grad_weights(name, f_shape):
    g = torch.Generator().manual_seed(sum(map(ord, name)) + 5113)
    return torch.randn(*f_shape, generator=g)
