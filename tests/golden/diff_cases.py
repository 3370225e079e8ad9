"""Cases of the differential attention layers, blocks and transformer, shared by the golden generator (make_golden_diff_attention.py)
and the tests.  Weights come from the oracle's name-keyed filler; the DiffTransformer-specific parameters (subln.weight and the four
lambda vectors) are then moved away from their initial values by a seeded perturbation so that every gradient is exercised."""
GRID = (8, 6)          # patch grid of the queries (and of both views of the transformer)
KGRID = (5, 6)         # patch grid of the key / value tokens of the layer and block cases (cross shape: 48 queries, 30 keys)
B = 2
DIM = 192

# name -> (kind, constructor arguments); "ROPE_OBJECT": a RoPE2D(100.0) instance of the side that builds the module
CASES = {
    "cross": ("DiffCrossAttention", dict(dim=DIM, depth=1, num_heads=3, qkv_bias=True, custom_positional_encoding="ROPE_OBJECT")),
    "self": ("DiffAttention", dict(dim=DIM, depth=2, num_heads=3, qkv_bias=True, custom_positional_encoding="ROPE_OBJECT")),
    "block": ("DiffCrossAttentionBlock", dict(dim=DIM, depth=1, num_heads=3, qkv_bias=True, custom_positional_encoding="ROPE_OBJECT")),
    "transformer": ("DifferentialMultiViewCrossAttentionTransformer",
                    dict(name="diff", input_embed_dim=128, num_views=2, dim=DIM, num_heads=6, depth=2, custom_positional_encoding="ROPE_OBJECT")),
}
# classes whose state_dict key set / shapes the fixture also records (no forward)
KEY_ONLY = {
    "selfblock": ("DiffSelfAttentionBlock", dict(dim=DIM, depth=3, num_heads=3, qkv_bias=True)),
    "transformer_ifr": ("DifferentialMultiViewCrossAttentionTransformerIFR",
                        dict(name="diff", input_embed_dim=128, num_views=2, dim=DIM, num_heads=6, depth=2, indices=[0])),
}


def resolve(kw, rope_cls):
    e = dict(kw)
    if e.get("custom_positional_encoding") == "ROPE_OBJECT":
        e["custom_positional_encoding"] = rope_cls(100.0)
    return e


def fill(model, name):
    "name-keyed filler, then the seeded perturbation of subln.weight (around 1) and the lambda vectors (std 0.35: lambda_full far from lambda_init)"
    import torch
    from oracle import dust3r_oracle as O
    O.fill_state_dict_(dict(model.state_dict()))
    g = torch.Generator().manual_seed(11 + sum(map(ord, name)))
    with torch.no_grad():
        for k, p in sorted(model.named_parameters()):
            leaf = k.rsplit(".", 1)[-1]
            if k.endswith("subln.weight"):
                p.copy_(1.0 + 0.3 * torch.randn(p.shape, generator=g))
            elif leaf in ("lambda_q1", "lambda_k1", "lambda_q2", "lambda_k2"):
                p.copy_(0.35 * torch.randn(p.shape, generator=g))


def positions(h, w):
    "what PositionGetter returns for a B x h x w grid: [B, h*w, 2] int64 (y, x)"
    import torch
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    return torch.stack([ys.flatten(), xs.flatten()], -1)[None].expand(B, -1, -1).contiguous()


def inputs(name):
    "the case's input tensors (fp32, seeded), in forward-argument order, and its position tensors"
    import torch
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    nq, nk = GRID[0] * GRID[1], KGRID[0] * KGRID[1]
    if name == "cross":
        return [torch.randn(B, nq, DIM, generator=g), torch.randn(B, nk, DIM, generator=g)], [positions(*GRID), positions(*KGRID)]
    if name in ("self", "selfblock"):
        return [torch.randn(B, nq, DIM, generator=g)], [positions(*GRID)]
    if name == "block":
        return [torch.randn(B, nq, DIM, generator=g), torch.randn(B, nk, DIM, generator=g)], [positions(*GRID), positions(*KGRID)]
    if name == "transformer":
        return [torch.randn(B, 128, GRID[0], GRID[1], generator=g) for _ in range(2)], []
    raise KeyError(name)


def run(name, model, ins, pos, wrap_input=None):
    "call the module of case `name`; returns the list of output tensors"
    if name == "cross":
        return [model(ins[0], ins[1], ins[1], pos[0], pos[1])]
    if name in ("self", "selfblock"):
        return [model(ins[0], pos[0])]
    if name == "block":
        return [model(ins[0], ins[1], pos[0], pos[1])]
    return list(model(wrap_input(features=list(ins))).features)


def cotangents(name, shapes):
    import torch
    g = torch.Generator().manual_seed(7 + sum(map(ord, name)))
    return [torch.randn(*s, generator=g) for s in shapes]
