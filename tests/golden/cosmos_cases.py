"""Cases of the Cosmos encoder (CosmosEncoder) and decoder head (CosmosSingleChannel, CosmosFeature), shared by the golden generator
(make_golden_cosmos.py) and the tests.  Weights come from the oracle's name-keyed filler (GroupNorm weights 1 + 0.1 N(0, 1), biases
0.1 N(0, 1)); inputs and cotangents are seeded.  The shapes are the smallest at which the code can still go wrong: one and two
Downsamples / Upsamples, non-square maps, 20 / 12 / 6 attention rows, two decoders (group indexing), the skipped linear layer."""
from tests.golden.moge_heads_cases import grad_errors, keys_of, signature  # noqa: F401  (the same lines, key lists and error normalisation)

GAIN = 1.0

# name -> (class, constructor arguments, input shape)
CASES = {
    "enc_p8": ("CosmosEncoder", dict(name="cosmos", patch_size=8), (2, 3, 32, 40)),
    "enc_p16": ("CosmosEncoder", dict(name="cosmos", patch_size=16), (2, 3, 64, 48)),
    "single_p8": ("CosmosSingleChannel", dict(patch_size=8), (2, 16, 4, 5)),
    "feature_p16": ("CosmosFeature", dict(input_feature_dim=24, output_dim=2, patch_size=16), (1, 24, 2, 3)),
    "feature_skip": ("CosmosFeature", dict(input_feature_dim=32, output_dim=2, patch_size=8, skip_linear=True), (1, 32, 4, 5)),
}
MODULE_OF = {"CosmosEncoder": "encoders.cosmos", "CosmosSingleChannel": "prediction_heads.cosmos", "CosmosFeature": "prediction_heads.cosmos"}
NSAMP = 32       # samples per parameter gradient (88 .. 226 parameters per case)


def fill(model):
    from oracle import dust3r_oracle as O
    O.fill_state_dict_(dict(model.state_dict()), gain=GAIN)


def input_of(name):
    import torch
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    return torch.randn(*CASES[name][2], generator=g)


def cotangent(name, shape):
    import torch
    g = torch.Generator().manual_seed(7 + sum(map(ord, name)))
    return torch.randn(*shape, generator=g)


def run(name, model, x, encoder_input, head_input):
    """call the module of case `name` on the tensor x; returns the list of output tensors (CosmosFeature: decoded_channels, then the
    x_split pieces — inputs of the decoders, which the cotangent leaves alone)"""
    kind = CASES[name][0]
    if kind == "CosmosEncoder":
        return [model(encoder_input(image=x, data_norm_type="cosmos")).features]
    if kind == "CosmosSingleChannel":
        return [model(x)]
    out, x_split = model(head_input(last_feature=x))
    return [out.decoded_channels] + list(x_split)


def last_conv(model, kind):
    "the module whose terms the cancellation ratio of the fixture is taken over"
    if kind == "CosmosEncoder":
        return model.quant_conv
    return (model if kind == "CosmosSingleChannel" else model.cosmos_decoders[0]).decoder.conv_out
