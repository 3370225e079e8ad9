"""Golden vectors of the differential attention layers, blocks and transformer from the REAL reference (recipe of make_golden.py: the
reference is imported from its own tree with the two import stubs of SURVEY.md App. B on PYTHONPATH):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<stubs>:<reference>:<repo> python3 -B tests/golden/make_golden_diff_attention.py

Writes tests/golden/diff_attention.npz; data only.  Per case of tests/golden/diff_cases.py:
  <case>/out<j>                          reference outputs (fp32, CPU) for the seeded inputs of diff_cases.inputs (regenerated, not stored:
                                         the fixture has to stay under the size limit of a committed file)
  <case>/din<i>                          gradient of L = sum_j <out_j, R_j> (seeded R_j) with respect to input i
  <case>/p/<param>__samples, __norm      evenly spaced samples (NSAMP) and the norm of every parameter gradient
  <case>/diffp/<param>                   the perturbed values of subln.weight and the lambda vectors (the rest of the state_dict is the
                                         oracle's name-keyed filler: regenerated, not stored)
  <case>/keys                            "name:shape" of every state_dict entry, one per line
  <case>/bf16/out<j>, /din<i>, /p/<param> the yardstick of the bf16 tests: rel-L2 error of the reference's OWN arithmetic with module and inputs
                                         cast to bfloat16 on the CPU against its fp32 result (parameter gradients: on the stored samples)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
NSAMP = 192     # samples per parameter gradient (the fixture stays well under the 1 MiB limit of a committed file)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden.cases import sample_indices  # noqa: E402
from tests.golden.diff_cases import CASES, KEY_ONLY, cotangents, fill, inputs, resolve, run  # noqa: E402

import uniception.models.utils.transformer_blocks as TB  # noqa: E402
from uniception.models.info_sharing import diff_cross_attention_transformer as DT  # noqa: E402
from uniception.models.info_sharing.base import MultiViewTransformerInput  # noqa: E402
from uniception.models.libs.croco.pos_embed import RoPE2D  # noqa: E402


def build(kind, kw):
    cls = getattr(TB, kind, None) or getattr(DT, kind)
    return cls(**resolve(kw, RoPE2D))


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def keys_of(model):
    return "\n".join(f"{k}:{'x'.join(map(str, v.shape))}" for k, v in model.state_dict().items())


def forward_backward(name, model, dtype):
    ins, pos = inputs(name)
    ins = [t.to(dtype).requires_grad_(True) for t in ins]
    outs = run(name, model, ins, pos, MultiViewTransformerInput)
    ws = cotangents(name, [tuple(o.shape) for o in outs])
    loss = sum((o.float() * w).sum() for o, w in zip(outs, ws))
    loss.backward()
    return ins, outs


def main():
    store = {}
    for name, (kind, kw) in CASES.items():
        model = build(kind, kw).train()
        fill(model, name)
        ins, outs = forward_backward(name, model, torch.float32)
        store[f"{name}/keys"] = np.array(keys_of(model))
        for i, t in enumerate(ins):
            store[f"{name}/din{i}"] = t.grad.numpy()
        for j, o in enumerate(outs):
            store[f"{name}/out{j}"] = o.detach().numpy()
        for k, p in model.named_parameters():
            if k.endswith("subln.weight") or k.rsplit(".", 1)[-1].startswith("lambda_"):
                store[f"{name}/diffp/{k}"] = p.detach().numpy().copy()
            idx = sample_indices(p.numel(), NSAMP)
            store[f"{name}/p/{k}__samples"] = p.grad.flatten()[idx].numpy().copy()
            store[f"{name}/p/{k}__norm"] = np.float64(p.grad.double().norm().item())
        # the yardstick: the same module and inputs in bfloat16 on the CPU
        m16 = build(kind, kw).train()
        fill(m16, name)
        m16 = m16.to(torch.bfloat16)
        ins16, outs16 = forward_backward(name, m16, torch.bfloat16)
        for i, t in enumerate(ins16):
            store[f"{name}/bf16/din{i}"] = np.float64(rel_l2(t.grad.float(), ins[i].grad))
        for j, o in enumerate(outs16):
            store[f"{name}/bf16/out{j}"] = np.float64(rel_l2(o.detach().float(), outs[j].detach()))
        p32 = dict(model.named_parameters())
        for k, p in m16.named_parameters():
            idx = sample_indices(p.numel(), NSAMP)
            store[f"{name}/bf16/p/{k}"] = np.float64(rel_l2(p.grad.float().flatten()[idx], p32[k].grad.flatten()[idx]))
        print(name, "ok:", {k.split("/", 1)[1]: float(v) for k, v in store.items() if k.startswith(f"{name}/bf16/") and "/p/" not in k},
              "worst parameter-gradient bf16 error", max(float(v) for k, v in store.items() if k.startswith(f"{name}/bf16/p/")))
    for name, (kind, kw) in KEY_ONLY.items():
        store[f"{name}/keys"] = np.array(keys_of(build(kind, kw)))
    out = os.path.join(HERE, "diff_attention.npz")
    np.savez_compressed(out, **store)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
