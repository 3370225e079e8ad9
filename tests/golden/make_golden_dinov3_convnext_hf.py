"""Golden vectors of the DINOv3 ConvNeXt encoder from an INDEPENDENT implementation: HuggingFace transformers' DINOv3ConvNextModel (the
reference takes this network from torch.hub out of a local clone of the DINOv3 repository, which is not part of the reference tree;
transformers ships its own implementation of the same published architecture).  CPU, fp32 weights, the network evaluated in fp64.

    PYTHONDONTWRITEBYTECODE=1 python3 -B tests/golden/make_golden_dinov3_convnext_hf.py        (from the repository root)

Per case of tests/golden/dinov3_convnext_cases.py, in eval(): the final-normed last-stage map [B, C, H/32, W/32] (the patch rows of
last_hidden_state; the pooled row is dropped), the four stage outputs raw, and stage 3 through the final norm (what the
intermediate-feature returner hands out).  For DINOV3_CONVNEXT_GRAD_CASES also the gradients (transformers' autograd) of
loss = <features, Wf> with respect to every parameter, renamed by the checkpoint converter: 512 strided samples + norm each.  Also the
transformers version.  Data only.

Everything is evaluated in fp64; maps and gradient samples are STORED as float32 (a relative 6e-8, four orders below the tightest
tolerance any test applies to them) and the stride-4 maps of stage 0, by far the largest arrays, go to a file of their own
(dinov3_convnext_hf_stage0.npz), so that each committed file stays under the repository's size limit for one file."""
import os
import sys

import numpy as np
import torch
import transformers
from transformers.models.dinov3_convnext import DINOv3ConvNextConfig, DINOv3ConvNextModel

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden.cases import sample_indices  # noqa: E402
from tests.golden.dinov3_convnext_cases import (DINOV3_CONVNEXT_CASES, DINOV3_CONVNEXT_GRAD_CASES, convnext_grad_weights,  # noqa: E402
                                                convnext_hf_config_kwargs, convnext_hf_state_dict, convnext_image)
from uniception_amd.tools.convert_checkpoint import dinov3_convnext_hf_to_uniception  # noqa: E402

OUT = os.path.join(HERE, "dinov3_convnext_hf.npz")
OUT_STAGE0 = os.path.join(HERE, "dinov3_convnext_hf_stage0.npz")


def f32(t):
    return t.detach().to(torch.float32).numpy()


def run(model, img):
    "(final-normed last-stage map NCHW, [the four stage outputs NCHW]) of the transformers model"
    out = model(img, output_hidden_states=True)
    stages = list(out.hidden_states[1:])
    B, C, h, w = stages[-1].shape
    feats = out.last_hidden_state[:, 1:].permute(0, 2, 1).reshape(B, C, h, w)
    return feats, stages


def golden_keys(cases=DINOV3_CONVNEXT_CASES, grad_cases=DINOV3_CONVNEXT_GRAD_CASES):
    "every key this generator writes, over both files (the provenance test compares the committed files against it)"
    grads = sorted(dinov3_convnext_hf_to_uniception({k: None for k in convnext_hf_state_dict()}))
    keys = ["transformers_version"]
    for name in cases:
        keys += [f"{name}/features", f"{name}/stage3_norm"] + [f"{name}/stage{i}_raw" for i in range(4)]
        if name in grad_cases:
            keys += [f"{name}/loss"] + [f"{name}/grad/{k}__{s}" for k in grads for s in ("samples", "norm")]
    return sorted(keys)


def main():
    store = {"transformers_version": np.array(transformers.__version__)}
    for name, c in DINOV3_CONVNEXT_CASES.items():
        model = DINOv3ConvNextModel(DINOv3ConvNextConfig(**convnext_hf_config_kwargs())).eval()
        print(name, model.load_state_dict(convnext_hf_state_dict(), strict=True))
        model = model.double()
        img = convnext_image(c).double()
        with torch.no_grad():
            feats, stages = run(model, img)
            store[f"{name}/features"] = f32(feats)
            for i, s in enumerate(stages):
                store[f"{name}/stage{i}_raw"] = f32(s)
            store[f"{name}/stage3_norm"] = f32(model.layer_norm(stages[3].permute(0, 2, 3, 1)).permute(0, 3, 1, 2))
        print(name, tuple(feats.shape), f"|features| {np.linalg.norm(store[f'{name}/features']):.4f}")
        if name in DINOV3_CONVNEXT_GRAD_CASES:
            model.train()          # (drop_path_rate 0: nothing random)
            feats, _ = run(model, img)
            loss = (feats * convnext_grad_weights(name, feats.shape).double()).sum()
            loss.backward()
            grads = dinov3_convnext_hf_to_uniception({k: p.grad for k, p in model.named_parameters()})
            store[f"{name}/loss"] = np.float64(float(loss.detach()))
            for k, gr in grads.items():
                store[f"{name}/grad/{k}__samples"] = f32(gr.flatten()[sample_indices(gr.numel(), 512)])
                store[f"{name}/grad/{k}__norm"] = np.float64(gr.double().norm().item())
            print(name, "gradients of", len(grads), "parameters; loss", float(loss.detach()))
    assert sorted(store) == golden_keys()
    stage0 = {k: store.pop(k) for k in sorted(store) if k.endswith("/stage0_raw")}
    for path, part in ((OUT, store), (OUT_STAGE0, stage0)):
        np.savez_compressed(path, **part)
        print("wrote", path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
