"""Cases of the Pixio encoder, shared by the golden generator (make_golden_pixio.py) and the tests.  Every case is a tiny PixioEncoder
(patch 16, depth 2, img_size 64: a native 4 x 4 table) at one of the head dims the published sizes have.  Weights, inputs and cotangents
are regenerated from seeds: `fill` walks the state_dict in its order with one generator, so the `blocks.N.*` and `blocks.N.inner.*`
layouts of one architecture receive the same values."""
NSAMP = 192         # samples per parameter gradient
GAIN = 2.0 ** 0.5

# case -> (embed_dim, num_heads, n_cls_tokens, gradient_checkpointing, image shapes: the first has every quantity stored, further ones
# only their output)
CASES = {
    "h80": (160, 2, 8, True, [(2, 3, 64, 64), (2, 3, 48, 80)]),         # head_dim 80; then a resized, non-square grid (3 x 5)
    "h96": (192, 2, 3, True, [(2, 3, 144, 160)]),                       # head_dim 96, 9 x 10 patches + 3: two 64-key tiles, ragged
    "h64": (128, 2, 8, True, [(2, 3, 64, 64)]),                         # the existing head_dim-64 kernels under the same class
    "h80_nockpt": (160, 2, 8, False, [(2, 3, 64, 64), (2, 3, 48, 80)]),  # the other key layout
}


def kwargs(name):
    width, heads, n_cls, ckpt, _ = CASES[name]
    return dict(name="pixio", data_norm_type="pixio", img_size=64, patch_size=16, embed_dim=width, depth=2, num_heads=heads,
                n_cls_tokens=n_cls, gradient_checkpointing=ckpt)


def fill(model, name):
    "seeded O(1) weights: linear / conv weights N(0, 2 / fan_in), biases 0.1 N(0, 1), LayerNorm 1 + 0.5 N | 0.5 N, table and class tokens N(0, 1)"
    import torch
    g = torch.Generator().manual_seed(1000 + sum(map(ord, name.split("_")[0])))
    with torch.no_grad():
        for key, t in model.state_dict().items():
            r = torch.randn(t.shape, generator=g, dtype=torch.float64)
            leaf = key.rsplit(".", 1)[-1]
            if leaf in ("cls_token", "pos_embed"):
                v = r
            elif "norm" in key:
                v = 1.0 + 0.5 * r if leaf == "weight" else 0.5 * r
            elif leaf == "weight":
                v = r * GAIN / float(t[0].numel()) ** 0.5
            else:
                v = 0.1 * r
            t.copy_(v.to(t.dtype))


def inputs(name):
    import torch
    g = torch.Generator().manual_seed(sum(map(ord, name.split("_")[0])))
    return [torch.randn(*shape, generator=g) for shape in CASES[name][4]]


def cotangent(name, shape):
    import torch
    g = torch.Generator().manual_seed(7 + sum(map(ord, name.split("_")[0])))
    return torch.randn(*shape, generator=g)


def plain_key(key):
    "the `blocks.N.*` name of a state_dict key of either layout"
    return key.replace(".inner.", ".")
