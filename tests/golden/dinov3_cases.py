"""DINOv3 ViT cases pinned to an independent implementation (HuggingFace transformers' DINOv3ViTModel) — shared by the golden generator
(make_golden_dinov3_hf.py), the CPU test and the GPU test.  Tiny configurations that still take every branch: hidden 128, 2 heads
(head_dim 64), 2 layers, 4 register tokens, LayerScale drawn away from 1 (0.1 N(0,1), the name-keyed filler's 1-D rule), no key bias,
the GELU MLP and the gated (SwiGLU) one, and NON-SQUARE token grids — 32x48 -> 2x3 and 48x32 -> 3x2 — so that a swapped axis or a table
shared between the axes shows.  The weights are held under transformers' names; the tests put them through
uniception_amd.tools.convert_checkpoint (--mode dinov3), which exercises the key map."""
import torch

HIDDEN, HEADS, LAYERS, REGISTERS, PATCH = 128, 2, 2, 4, 16
GAINS = {"cls_token": 10.0, "register_tokens": 20.0}
DINOV3_HF_CASES = {
    "mlp_32x48": dict(gated=False, ffn_hidden=512, hw=(32, 48), B=2, seed=31),
    "mlp_48x32": dict(gated=False, ffn_hidden=512, hw=(48, 32), B=2, seed=32),
    "gated_32x48": dict(gated=True, ffn_hidden=256, hw=(32, 48), B=2, seed=33),
    "gated_48x32": dict(gated=True, ffn_hidden=256, hw=(48, 32), B=2, seed=34),
}
# cases that also carry gradients (transformers' autograd, position augmentation off): loss = <features, Wf>, seeded cotangent
DINOV3_HF_GRAD_CASES = ("mlp_32x48", "gated_48x32")


def dinov3_size(c):
    "the `size` dict DINOv3Encoder takes for this configuration"
    return dict(embed_dim=HIDDEN, depth=LAYERS, num_heads=HEADS, ffn="swiglu" if c["gated"] else "mlp", ffn_hidden=c["ffn_hidden"])


def dinov3_hf_config_kwargs(c):
    "keyword arguments of transformers' DINOv3ViTConfig for this configuration"
    return dict(hidden_size=HIDDEN, num_hidden_layers=LAYERS, num_attention_heads=HEADS, intermediate_size=c["ffn_hidden"],
                hidden_act="silu" if c["gated"] else "gelu", use_gated_mlp=c["gated"], num_register_tokens=REGISTERS, patch_size=PATCH,
                image_size=64, num_channels=3, layer_norm_eps=1e-5, rope_theta=100.0, query_bias=True, key_bias=False, value_bias=True,
                proj_bias=True, mlp_bias=True, layerscale_value=1.0, drop_path_rate=0.0, attention_dropout=0.0,
                pos_embed_shift=None, pos_embed_jitter=None, pos_embed_rescale=None)


def dinov3_image(c):
    g = torch.Generator().manual_seed(c["seed"])
    return torch.randn(c["B"], 3, *c["hw"], generator=g)


def dinov3_hf_state_dict(c):
    "Parameters under transformers' DINOv3ViTModel names, filled by the name-keyed filler (mask_token: zeros, unused)."
    from oracle import dust3r_oracle as O
    D, Hf = HIDDEN, c["ffn_hidden"]
    sd = {"embeddings.cls_token": torch.empty(1, 1, D), "embeddings.mask_token": torch.empty(1, 1, D),
          "embeddings.register_tokens": torch.empty(1, REGISTERS, D),
          "embeddings.patch_embeddings.weight": torch.empty(D, 3, PATCH, PATCH), "embeddings.patch_embeddings.bias": torch.empty(D),
          "norm.weight": torch.empty(D), "norm.bias": torch.empty(D)}
    for i in range(LAYERS):
        b = f"model.layer.{i}."
        shapes = [("norm1.weight", (D,)), ("norm1.bias", (D,)), ("norm2.weight", (D,)), ("norm2.bias", (D,)),
                  ("attention.q_proj.weight", (D, D)), ("attention.q_proj.bias", (D,)), ("attention.k_proj.weight", (D, D)),
                  ("attention.v_proj.weight", (D, D)), ("attention.v_proj.bias", (D,)), ("attention.o_proj.weight", (D, D)),
                  ("attention.o_proj.bias", (D,)), ("layer_scale1.lambda1", (D,)), ("layer_scale2.lambda1", (D,)),
                  ("mlp.up_proj.weight", (Hf, D)), ("mlp.up_proj.bias", (Hf,)), ("mlp.down_proj.weight", (D, Hf)), ("mlp.down_proj.bias", (D,))]
        if c["gated"]:
            shapes += [("mlp.gate_proj.weight", (Hf, D)), ("mlp.gate_proj.bias", (Hf,))]
        for n, shp in shapes:
            sd[b + n] = torch.empty(*shp)
    O.fill_state_dict_(sd, gains=GAINS)
    sd["embeddings.mask_token"].zero_()
    return sd


def dinov3_grad_weights(name, f_shape):
    g = torch.Generator().manual_seed(sum(map(ord, name)) + 4111)
    return torch.randn(*f_shape, generator=g)
