"""Cases of the summary heads (PoseHead, GlobalHead, MLPHead, ResConvBlock), shared by the golden generator
(make_golden_summary_heads.py) and the tests.  Weights come from the oracle's name-keyed filler with a gain of sqrt(2) (every layer
is followed by a ReLU, which halves the second moment: the activations keep their scale down the chain and no output is a sum of
cancelling terms — the generator checks and prints that); inputs and cotangents are seeded."""
GAIN = 2.0 ** 0.5

# name -> (class, constructor arguments, input shape)
CASES = {
    "pose_small": ("PoseHead", dict(patch_size=4, input_feature_dim=48), (3, 48, 5, 7)),
    "pose_default": ("PoseHead", dict(patch_size=16, input_feature_dim=768), (2, 768, 3, 5)),      # hidden 1024: the real GEMM shape on 30 tokens
    "global_small": ("GlobalHead", dict(patch_size=4, input_feature_dim=40, num_resconv_block=1, output_representation_dim=2), (2, 40, 6, 6)),
    "resconv_skip": ("ResConvBlock", dict(in_channels=24, out_channels=64), (2, 24, 4, 4)),
    "mlp_default": ("MLPHead", dict(input_feature_dim=96, output_dim=3), (4, 96, 3)),               # hidden 196: no multiple of 8
    "mlp_small": ("MLPHead", dict(input_feature_dim=64, output_dim=1, num_mlp_layers=1, hidden_dim=32), (2, 64, 1)),
}
MODULE_OF = {"PoseHead": "pose_head", "ResConvBlock": "pose_head", "GlobalHead": "global_head", "MLPHead": "mlp_head"}
NSAMP = 192     # samples per parameter gradient


def fill(model):
    from oracle import dust3r_oracle as O
    O.fill_state_dict_(dict(model.state_dict()), gain=GAIN)


def inputs(name):
    import torch
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    return torch.randn(*CASES[name][2], generator=g)


def cotangent(name, shape):
    import torch
    g = torch.Generator().manual_seed(7 + sum(map(ord, name)))
    return torch.randn(*shape, generator=g)


def run(name, model, x, head_input, token_input):
    "call the module of case `name` on tensor x; returns the output tensor"
    kind = CASES[name][0]
    if kind == "ResConvBlock":
        return model(x)
    return model((token_input if kind == "MLPHead" else head_input)(last_feature=x)).decoded_channels


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
