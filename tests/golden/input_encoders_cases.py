"""Cases of the non-image input encoders (PatchEmbedder, DenseRepresentationEncoder, GlobalRepresentationEncoder), shared by the golden
generator (make_golden_input_encoders.py) and the tests.  Weights come from the oracle's name-keyed filler; `fill` then brings every
term of the tail LN2(LN1(x) + pe) to O(1) so that each of them matters in the output and in the gradients: the position table (the
filler gives the learned [1, N, C] table N(0, 1 / (N C)) and overwrites the sinusoid buffer with N(0, 1 / C)) becomes N(0, 1), and the
LayerNorm parameters become gamma = 1 + 0.5 N(0, 1), beta = 0.5 N(0, 1) (the filler's deviations times five).  Inputs and cotangents
are seeded; the cotangent is random because the gradient of sum() behind a LayerNorm vanishes."""
GAIN = 2.0 ** 0.5
NORM_SPREAD = 5.0          # the filler's 0.1 N(0, 1) deviations of a LayerNorm's gamma (from 1) and beta (from 0), times this

# name -> (class, constructor arguments as a callable (they hold nn classes), input shape)
_PATCH = dict(name="pe", in_chans=3, patch_size=4, enc_embed_dim=64, input_size=20)


def _kw(name):
    from functools import partial
    import torch.nn as nn
    return {
        # 3 x 7 grid on a 5 x 5 table (scale-factor resize, non-square); 40 -> padded to 64; one conv shortcut, one Identity shortcut
        "dense_small": dict(name="d", in_chans=2, patch_size=4, intermediate_dims=[40, 64, 64], enc_embed_dim=64, input_size_for_pe=20),
        # raw-table shortcut; 196 -> 256 columns
        "dense_native_p14": dict(name="d", in_chans=1, patch_size=14, intermediate_dims=[72, 128], enc_embed_dim=128, input_size_for_pe=70),
        # no table, no norm, ReLU
        "dense_plain": dict(name="d", in_chans=2, patch_size=4, intermediate_dims=[40, 64, 64], enc_embed_dim=64, input_size_for_pe=20,
                            apply_pe=False, norm_layer=None, act_layer=nn.ReLU),
        "patch_small": dict(_PATCH),
        # size-form resize, LN in front of the table, none behind it
        "patch_size_form": dict(_PATCH, interpolate_offset=0.0, norm_layer=partial(nn.LayerNorm, eps=1e-6), post_pe_norm_layer=None),
        "patch_native": dict(_PATCH),
        "global_small": dict(name="g", in_chans=9, intermediate_dims=[16, 32], enc_embed_dim=64),
        "global_default": dict(name="g", in_chans=3),
    }[name]


CASES = {
    "dense_small": ("DenseRepresentationEncoder", (2, 2, 12, 28)),
    "dense_native_p14": ("DenseRepresentationEncoder", (2, 1, 70, 70)),
    "dense_plain": ("DenseRepresentationEncoder", (2, 2, 12, 28)),
    "patch_small": ("PatchEmbedder", (2, 3, 12, 28)),
    "patch_size_form": ("PatchEmbedder", (2, 3, 12, 28)),
    "patch_native": ("PatchEmbedder", (2, 3, 20, 20)),
    "global_small": ("GlobalRepresentationEncoder", (4, 9)),
    "global_default": ("GlobalRepresentationEncoder", (3, 3)),
}
MODULE_OF = {"DenseRepresentationEncoder": "dense_rep_encoder", "PatchEmbedder": "patch_embedder",
             "GlobalRepresentationEncoder": "global_rep_encoder"}
NSAMP = 192     # samples per parameter gradient
GRAD_FLOOR = 1e-3   # parameter-gradient errors are divided by max(|g_ref|, GRAD_FLOOR x the largest parameter-gradient norm of the case)


def kwargs(name):
    return _kw(name)


def fill(model):
    import torch
    from oracle import dust3r_oracle as O
    O.fill_state_dict_(dict(model.state_dict()), gain=GAIN)
    with torch.no_grad():
        for key, t in model.state_dict().items():
            if key == "pos_embed":
                t.mul_(float(t[0].numel() if t.dim() == 3 else t.shape[1]) ** 0.5 / GAIN)      # N(0, gain^2 / fan_in) -> N(0, 1)
        for m in model.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.copy_(1.0 + NORM_SPREAD * (m.weight - 1.0))
                m.bias.mul_(NORM_SPREAD)


def inputs(name):
    import torch
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    return [torch.randn(*CASES[name][1], generator=g)]


def cotangent(name, shape):
    import torch
    g = torch.Generator().manual_seed(7 + sum(map(ord, name)))
    return torch.randn(*shape, generator=g)


def run(name, model, xs, non_image_input, global_input):
    "call the module of case `name` on the tensors xs; returns the output tensor"
    if CASES[name][0] == "GlobalRepresentationEncoder":
        return model(global_input(data=xs[0])).features
    return model(non_image_input(data=xs[0])).features


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
    "{name: |got - want| / max(|want|, GRAD_FLOOR x the largest |want| of the case)} over dicts of 1-D sample vectors"
    import torch
    norms = {k: float(torch.as_tensor(v).double().norm()) for k, v in want.items()}
    floor = GRAD_FLOOR * max(norms.values())
    return {k: float((torch.as_tensor(got[k]).double() - torch.as_tensor(want[k]).double()).norm()) / max(norms[k], floor) for k in want}
