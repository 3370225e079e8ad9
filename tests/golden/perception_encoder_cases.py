"""Cases of the Perception Encoder wrappers (PerceptionEncoder, PerceptionEncoderIntermediateFeatureReturner), shared by the golden
generator (make_golden_perception_encoder.py) and the tests.  Every case is a tiny vision tower (width 128, 2 heads: head_dim 64) put
under a PUBLISHED config name, so that the real wrapper code runs around it.  Weights come from the oracle's name-keyed filler; `fill`
then brings the terms the filler leaves small to O(1) so that each of them matters in the output and in the gradients: LayerNorm
parameters become gamma = 1 + 0.5 N(0, 1), beta = 0.5 N(0, 1) (the filler does not know the names ln_*), the position table and the
class embedding N(0, 1), LayerScale 0.5 + 0.1 N(0, 1).  Inputs and cotangents are seeded."""
GAIN = 2.0 ** 0.5
NORM_SPREAD = 5.0
NSAMP = 192         # samples per parameter gradient
ROPE_GRID = (3, 5)  # grid of the rope/ fixture
ROPE_HEADS, ROPE_DIM = 2, 64

_BASE = dict(patch_size=14, width=128, layers=3, heads=2, mlp_ratio=4.0, image_size=56, use_cls_token=True)
# tower configurations (PEConfig fields)
CONFIGS = {
    # grid 5 x 9 on a 4 x 4 table: resampled, 46 tokens (odd); the pooling head's parameters are there and unused
    "core_cls": dict(_BASE, pool_type="attn", output_dim=64),
    # native 4 x 4 grid (17 tokens), LayerScale, no ln_post
    "lang_ls": dict(_BASE, pool_type="none", output_dim=None, ls_init_value=0.1, use_ln_post=False),
    # patch 16 (K = 768), no class token: 9 x 8 = 72 tokens (more than one 64-key tile), positions without the offset
    "nocls_big": dict(patch_size=16, width=128, layers=2, heads=2, mlp_ratio=4.0, image_size=64, use_cls_token=False, pool_type="none",
                      output_dim=None, ls_init_value=0.1),
}

# case -> (wrapper class, tower configuration, (checkpoint_type, size) it stands in for, extra constructor arguments, input shapes)
CASES = {
    "core_cls": ("PerceptionEncoder", "core_cls", ("core", "large"), {}, [(2, 3, 70, 126), (2, 3, 56, 84)]),
    "lang_ls": ("PerceptionEncoder", "lang_ls", ("lang", "large"), {}, [(2, 3, 56, 56)]),
    "nocls_big": ("PerceptionEncoder", "nocls_big", ("core", "base"), dict(patch_size=16), [(2, 3, 144, 128)]),
    "ret_norm": ("PerceptionEncoderIntermediateFeatureReturner", "core_cls", ("core", "large"), dict(indices=[0, 2], norm_intermediate=True),
                 [(2, 3, 70, 126)]),
    "ret_raw": ("PerceptionEncoderIntermediateFeatureReturner", "core_cls", ("core", "large"), dict(indices=[0, 2], norm_intermediate=False),
                [(2, 3, 70, 126)]),
    # truncate(1) of 3 blocks leaves 2; the integer indices = 1 then returns the single layer 2 - 1 = 1
    "ret_trunc": ("PerceptionEncoderIntermediateFeatureReturner", "core_cls", ("core", "large"), dict(keep_first_n_layers=1, indices=1),
                  [(2, 3, 70, 126)]),
}
CONFIG_NAME = {("core", "base"): "PE-Core-B16-224", ("core", "large"): "PE-Core-L14-336", ("lang", "large"): "PE-Lang-L14-448"}


def kwargs(name):
    _, _, (ctype, size), extra, _ = CASES[name]
    return dict(name="pe", size=size, checkpoint_type=ctype, **extra)


def fill(model):
    import torch
    from oracle import dust3r_oracle as O
    O.fill_state_dict_(dict(model.state_dict()), gain=GAIN)
    with torch.no_grad():
        for key, t in model.state_dict().items():
            leaf = key.rsplit(".", 1)[-1]
            if leaf == "positional_embedding":
                t.mul_(float(t.shape[1]) ** 0.5 / GAIN)          # N(0, gain^2 / C) -> N(0, 1)
            elif leaf == "class_embedding":
                t.mul_(10.0)                                     # 0.1 N(0, 1) -> N(0, 1)
            elif leaf == "gamma":
                t.add_(0.5)                                      # LayerScale: 0.5 + 0.1 N(0, 1)
        for m in model.modules():
            if isinstance(m, torch.nn.LayerNorm):                # the filler's 0.1 N(0, 1) for both
                m.weight.copy_(1.0 + NORM_SPREAD * m.weight)
                m.bias.mul_(NORM_SPREAD)


def inputs(name):
    "the case's images: the first is the one every quantity is stored for, further ones only have their output stored"
    import torch
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    return [torch.randn(*shape, generator=g) for shape in CASES[name][4]]


def cotangent(name, i, shape):
    import torch
    g = torch.Generator().manual_seed(7 + 13 * i + sum(map(ord, name)))
    return torch.randn(*shape, generator=g)


def outputs(name, model, image, vit_input):
    "call the wrapper of case `name` on `image`; returns the list of its output feature maps"
    out = model(vit_input(image=image, data_norm_type="perception_encoder"))
    return [o.features for o in out] if isinstance(out, (list, tuple)) else [out.features]


def rope_inputs(with_cls):
    "seeded q, k [1, heads, N, head_dim] of the rope/ fixture at grid ROPE_GRID"
    import torch
    n = ROPE_GRID[0] * ROPE_GRID[1] + int(with_cls)
    g = torch.Generator().manual_seed(101 + int(with_cls))
    return torch.randn(1, ROPE_HEADS, n, ROPE_DIM, generator=g), torch.randn(1, ROPE_HEADS, n, ROPE_DIM, generator=g)
