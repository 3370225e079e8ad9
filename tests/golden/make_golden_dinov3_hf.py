"""Golden vectors of the DINOv3 ViT encoder from an INDEPENDENT implementation: HuggingFace transformers' DINOv3ViTModel (the reference
takes this network from torch.hub out of a local clone of the DINOv3 repository, which is not part of the reference tree;
transformers ships its own implementation of the same published architecture).  CPU, fp32 weights, the network evaluated in fp64
(its RoPE tables stay fp32, as the implementation forces them).

    PYTHONDONTWRITEBYTECODE=1 python3 -B tests/golden/make_golden_dinov3_hf.py        (from the repository root)

Per case of tests/golden/dinov3_cases.py, in eval(): the final-normed patch map [B, D, h, w] and the patch maps of every block's
output, raw and through the final norm (what the intermediate-feature returner hands out).  For DINOV3_HF_GRAD_CASES also the
gradients (transformers' autograd, position augmentation off) of loss = <patch map, Wf> with respect to every parameter, mapped to
this project's names by the checkpoint converter: 512 strided samples + norm each.  Also the RoPE cos / sin of the 2x3, 3x2 and
14x14 grids (for machines without transformers) and the transformers version.  Data only."""
import os
import sys

import numpy as np
import torch
import transformers
from transformers import DINOv3ViTConfig, DINOv3ViTModel

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden.cases import sample_indices  # noqa: E402
from tests.golden.dinov3_cases import (DINOV3_HF_CASES, DINOV3_HF_GRAD_CASES, HIDDEN, PATCH, REGISTERS, dinov3_grad_weights,  # noqa: E402
                                       dinov3_hf_config_kwargs, dinov3_hf_state_dict, dinov3_image)
from uniception_amd.tools.convert_checkpoint import dinov3_hf_to_uniception  # noqa: E402


def run(model, img):
    "(final-normed tokens, [tokens after block i]) of the transformers model, block by block"
    x = model.embeddings(img)
    pe = model.rope_embeddings(img)
    taken = []
    for layer in model.model.layer:
        x = layer(x, position_embeddings=pe)
        taken.append(x)
    return model.norm(x), taken


def patch_map(tok, B, h, w):
    return tok[:, 1 + REGISTERS:].permute(0, 2, 1).reshape(B, HIDDEN, h, w)


def main():
    store = {"transformers_version": np.array(transformers.__version__)}
    rope = DINOv3ViTModel(DINOv3ViTConfig(**dinov3_hf_config_kwargs(DINOV3_HF_CASES["mlp_32x48"]))).eval().rope_embeddings
    for h, w in ((2, 3), (3, 2), (14, 14)):
        cos, sin = rope(torch.zeros(1, 3, h * PATCH, w * PATCH))
        store[f"rope/{h}x{w}/cos"], store[f"rope/{h}x{w}/sin"] = cos.numpy(), sin.numpy()
    for name, c in DINOV3_HF_CASES.items():
        model = DINOv3ViTModel(DINOv3ViTConfig(**dinov3_hf_config_kwargs(c))).eval()
        print(name, model.load_state_dict(dinov3_hf_state_dict(c), strict=True))
        model = model.double()
        img = dinov3_image(c).double()
        B, (h, w) = c["B"], (c["hw"][0] // PATCH, c["hw"][1] // PATCH)
        with torch.no_grad():
            tok, taken = run(model, img)
            store[f"{name}/features"] = patch_map(tok, B, h, w).numpy()
            for i, t in enumerate(taken):
                store[f"{name}/take{i}_raw"] = patch_map(t, B, h, w).numpy()
                store[f"{name}/take{i}_norm"] = patch_map(model.norm(t), B, h, w).numpy()
        print(name, tuple(store[f"{name}/features"].shape), f"|features| {np.linalg.norm(store[f'{name}/features']):.4f}")
        if name in DINOV3_HF_GRAD_CASES:
            model.train()          # (no dropout anywhere; pos_embed_shift / jitter / rescale are None: the coordinates stay plain)
            tok, _ = run(model, img)
            feats = patch_map(tok, B, h, w)
            loss = (feats * dinov3_grad_weights(name, feats.shape).double()).sum()
            loss.backward()
            grads = dinov3_hf_to_uniception({k: p.grad for k, p in model.named_parameters() if p.grad is not None}, num_heads=2)
            store[f"{name}/loss"] = np.float64(float(loss.detach()))
            n = 0
            for k, gr in grads.items():
                if k.endswith(("bias_mask", "rope_embed.periods")):
                    continue
                store[f"{name}/grad/{k}__samples"] = gr.flatten()[sample_indices(gr.numel(), 512)].double().numpy()
                store[f"{name}/grad/{k}__norm"] = np.float64(gr.double().norm().item())
                n += 1
            print(name, "gradients of", n, "parameters; loss", float(loss.detach()))
    np.savez_compressed(os.path.join(HERE, "dinov3_hf.npz"), **store)
    print("wrote", os.path.join(HERE, "dinov3_hf.npz"), os.path.getsize(os.path.join(HERE, "dinov3_hf.npz")), "bytes")


if __name__ == "__main__":
    main()
