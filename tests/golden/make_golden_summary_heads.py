"""Golden vectors of the summary heads from the REAL reference classes on the CPU (recipe of make_golden_heads.py: the reference is
imported from its own tree with the two import stubs of SURVEY.md App. B on PYTHONPATH):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<stubs>:<reference>:<repo> python3 -B tests/golden/make_golden_summary_heads.py

Writes tests/golden/summary_heads.npz; data only.  Per case of tests/golden/summary_heads_cases.py:
  <case>/keys, <case>/signature          "name:shape" of every state_dict entry / the constructor's "name=default" lines
  <case>/out, /din                       the reference run in FLOAT64 (module and input cast to double): output, and the gradient of
                                         L = <out, R> (seeded R) with respect to the input (stored rounded to fp32)
  <case>/p/<param>__samples, __norm      evenly spaced samples (NSAMP, float64) and the norm of every parameter gradient of that run
  <case>/e32/<q>, <case>/e16/<q>         rel-L2 error against the float64 run of the reference's OWN fp32 / bfloat16-on-CPU arithmetic,
                                         q = out, din, p/<param> (parameter gradients: on the stored samples)
Inputs, weights and cotangents are regenerated from seeds (summary_heads_cases), not stored.
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden.cases import sample_indices  # noqa: E402
from tests.golden.summary_heads_cases import CASES, MODULE_OF, NSAMP, cotangent, fill, inputs, keys_of, run, signature  # noqa: E402

from uniception.models.prediction_heads.base import PredictionHeadInput, PredictionHeadTokenInput  # noqa: E402


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def ref_class(kind):
    return getattr(importlib.import_module(f"uniception.models.prediction_heads.{MODULE_OF[kind]}"), kind)


def forward_backward(name, dtype):
    kind, kw, _ = CASES[name]
    model = ref_class(kind)(**kw).train()
    fill(model)
    model = model.to(dtype)
    x = inputs(name).to(dtype).requires_grad_(True)
    out = run(name, model, x, PredictionHeadInput, PredictionHeadTokenInput)
    (out.double() * cotangent(name, tuple(out.shape)).double()).sum().backward()
    return model, x, out


def cancellation(model, name, out):
    "norm of the output over the norm of the magnitudes of the terms of its last layer: far below 1 means cancelling terms"
    kind = CASES[name][0]
    feats = {}
    last = {"PoseHead": "fc_rot", "GlobalHead": "fc_output", "MLPHead": "output_proj", "ResConvBlock": "res_conv3"}[kind]
    mod = getattr(model, last)
    h = mod.register_forward_hook(lambda m, i, o: feats.setdefault("x", i[0].detach()))
    with torch.no_grad():
        run(name, model, inputs(name).double(), PredictionHeadInput, PredictionHeadTokenInput)
    h.remove()
    xin = feats["x"]
    w = mod.weight.detach().reshape(mod.weight.shape[0], -1)
    xin = xin.movedim(1, -1).reshape(-1, w.shape[1]) if kind == "ResConvBlock" else xin.reshape(-1, w.shape[1])
    terms = (xin.abs() @ w.abs().T + mod.bias.detach().abs()).norm()
    return float(out.detach().norm() / terms), float(out.detach().norm())


def main():
    store = {}
    for name, (kind, kw, _) in CASES.items():
        m64, x64, o64 = forward_backward(name, torch.float64)
        ratio, onorm = cancellation(m64, name, o64)
        assert ratio > 1e-2, f"{name}: output norm {onorm:.3e} is {ratio:.2e} of its terms' scale: cancelling terms, pick other scales"
        store[f"{name}/keys"] = np.array(keys_of(m64))
        store[f"{name}/signature"] = np.array(signature(ref_class(kind)))
        store[f"{name}/out"] = o64.detach().numpy().copy()
        store[f"{name}/din"] = x64.grad.float().numpy().copy()
        idx = {k: sample_indices(p.numel(), NSAMP) for k, p in m64.named_parameters()}
        for k, p in m64.named_parameters():
            store[f"{name}/p/{k}__samples"] = p.grad.flatten()[idx[k]].numpy().copy()
            store[f"{name}/p/{k}__norm"] = np.float64(p.grad.norm().item())
        print(f"{name}: |out| = {onorm:.3e} ({ratio:.2f} of its terms' scale), |din| = {x64.grad.norm():.3e}")
        for tag, dtype in (("e32", torch.float32), ("e16", torch.bfloat16)):
            m, x, o = forward_backward(name, dtype)
            errs = {"out": rel_l2(o.detach(), o64.detach()), "din": rel_l2(x.grad, x64.grad)}
            p64 = dict(m64.named_parameters())
            for k, p in m.named_parameters():
                errs[f"p/{k}"] = rel_l2(p.grad.flatten()[idx[k]], p64[k].grad.flatten()[idx[k]])
            for q, e in errs.items():
                store[f"{name}/{tag}/{q}"] = np.float64(e)
            print(f"  {tag}: out {errs['out']:.3e}  din {errs['din']:.3e}  parameter gradients max {max(v for q, v in errs.items() if q.startswith('p/')):.3e}")
    path = os.path.join(HERE, "summary_heads.npz")
    np.savez_compressed(path, **store)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
