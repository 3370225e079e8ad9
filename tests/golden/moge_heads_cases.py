"""Cases of the MoGe convolutional head (MoGeConvFeature, ResidualConvBlock) and MLPFeature, shared by the golden generator
(make_golden_moge_heads.py) and the tests.  Weights come from the oracle's name-keyed filler; `fill` then moves every GroupNorm
weight to 1 + 0.1 N(0, 1) (the filler gives 1-D tensors 0.1 N(0, 1): the biases, GroupNorm's beta included, keep that), so gamma != 1
and beta != 0 everywhere.  Inputs and cotangents are seeded."""
GAIN = 2.0 ** 0.5

_MOGE = dict(num_features=2, input_feature_dims=[48, 32], dim_proj=64, dim_upsample=[64, 32, 32], num_res_blocks=1, last_conv_channels=32)

# name -> (class, constructor arguments, input shapes, target_output_shape | None)
CASES = {
    # non-square aspect in the UV channels, 24x40 -> 42x70 half-pixel resize, hidden width 64 with GroupNorm G = 2, a residual block
    # without a skip convolution in the output blocks
    "moge_small_p14": ("MoGeConvFeature", dict(_MOGE, patch_size=14, dim_out=[2, 1], last_res_blocks=1, last_conv_size=1),
                       [(2, 48, 3, 5), (2, 32, 3, 5)], (42, 70)),
    # exact x2 resize, G = 1 throughout, a replicate-padded 3x3 final convolution to 3 channels
    "moge_ln_p16": ("MoGeConvFeature", dict(_MOGE, patch_size=16, dim_out=[3], res_block_norm="layer_norm", last_res_blocks=0, last_conv_size=3),
                    [(1, 48, 2, 2), (1, 32, 2, 2)], (32, 32)),
    "resblock_skip": ("ResidualConvBlock", dict(in_channels=32, out_channels=64, hidden_channels=64), [(2, 32, 5, 7)], None),
    "mlpfeature_small": ("MLPFeature", dict(input_feature_dim=32, patch_size=4, output_dim=3), [(2, 32, 3, 5)], None),
    "mlpfeature_p14": ("MLPFeature", dict(input_feature_dim=64, patch_size=14, output_dim=4, mlp_ratio=2), [(1, 64, 2, 3)], None),
}
MODULE_OF = {"MoGeConvFeature": "moge_conv", "ResidualConvBlock": "moge_conv", "MLPFeature": "mlp_feature"}
NSAMP = 192     # samples per parameter gradient
GRAD_FLOOR = 1e-3   # parameter-gradient errors are divided by max(|g_ref|, GRAD_FLOOR x the largest parameter-gradient norm of the case)


def fill(model):
    import torch
    from oracle import dust3r_oracle as O
    O.fill_state_dict_(dict(model.state_dict()), gain=GAIN)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.GroupNorm):
                m.weight.add_(1.0)


def inputs(name):
    import torch
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    return [torch.randn(*s, generator=g) for s in CASES[name][2]]


def cotangent(name, shape):
    import torch
    g = torch.Generator().manual_seed(7 + sum(map(ord, name)))
    return torch.randn(*shape, generator=g)


def run(name, model, xs, head_input, layered_input):
    "call the module of case `name` on the tensors xs; returns the output tensor"
    kind, _, _, target = CASES[name]
    if kind == "ResidualConvBlock":
        return model(xs[0])
    if kind == "MoGeConvFeature":
        return model(layered_input(list_features=list(xs), target_output_shape=target)).decoded_channels
    return model(head_input(last_feature=xs[0])).decoded_channels


def signature(cls):
    "constructor parameters as 'name=default' lines (no default: 'name'; *args / **kwargs with their stars)"
    import inspect
    out = []
    for p in list(inspect.signature(cls.__init__).parameters.values())[1:]:
        star = {p.VAR_POSITIONAL: "*", p.VAR_KEYWORD: "**"}.get(p.kind, "")
        out.append(star + p.name + ("" if p.default is p.empty else f"={p.default!r}"))
    return "\n".join(out)


def keys_of(model):
    return "\n".join(f"{k}:{'x'.join(map(str, v.shape))}" for k, v in model.state_dict().items())


def grad_errors(got, want):
    """{name: |got - want| / max(|want|, GRAD_FLOOR x the largest |want| of the case)} over dicts of 1-D sample vectors: the
    convolution biases in front of a GroupNorm have a true gradient that nearly cancels, against which a plain relative error is noise."""
    import torch
    norms = {k: float(torch.as_tensor(v).double().norm()) for k, v in want.items()}
    floor = GRAD_FLOOR * max(norms.values())
    return {k: float((torch.as_tensor(got[k]).double() - torch.as_tensor(want[k]).double()).norm()) / max(norms[k], floor) for k in want}
