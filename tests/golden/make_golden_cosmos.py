"""Golden vectors of CosmosEncoder, CosmosSingleChannel and CosmosFeature from the REAL reference classes on the CPU (recipe of
make_golden_moge_heads.py: the reference is imported from its own tree with the two import stubs of SURVEY.md App. B on PYTHONPATH;
einops, which the tokenizer's patcher imports, is installed):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<stubs>:<reference>:<repo> python3 -B tests/golden/make_golden_cosmos.py

Writes tests/golden/cosmos.npz; data only.  Per case of tests/golden/cosmos_cases.py:
  <case>/keys, <case>/signature          "name:shape" of every state_dict entry / the constructor's "name=default" lines
  <case>/out<i>, /din                    the reference run in FLOAT64 (module and input cast to double), train mode: the outputs
                                         (CosmosFeature: decoded_channels, then the x_split pieces), and the gradient of
                                         L = <out0, R> (seeded R) with respect to the input (stored rounded to fp32)
  <case>/p_names, /p_samples, /p_norm    per parameter (names joined by newlines, in named_parameters() order): evenly spaced samples
                                         [P, NSAMP] (float64; a parameter with fewer elements repeats its last sample) and the norm of its
                                         gradient in that run — packed per case: one archive member per parameter would put the file
                                         over the size limit of a committed file
  <case>/cancel                          (|out0| / |terms of its last layer|, |out0|, rms of out0): far below 1 means cancelling terms
  <case>/e32/<q>, <case>/e16/<q>         error against the float64 run of the reference's OWN fp32 / bfloat16-on-CPU arithmetic,
                                         q = out<i>, din (rel-L2); <case>/e32/p, /e16/p: [P], per parameter on the stored samples
                                         (cosmos_cases.grad_errors)
Inputs, weights and cotangents are regenerated from seeds (cosmos_cases), not stored.
"""
import importlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden.cases import sample_indices  # noqa: E402
from tests.golden.cosmos_cases import (CASES, MODULE_OF, NSAMP, cotangent, fill, grad_errors, input_of, keys_of, last_conv, run,  # noqa: E402
                                       signature)

from uniception.models.encoders.base import ViTEncoderInput  # noqa: E402
from uniception.models.prediction_heads.base import PredictionHeadInput  # noqa: E402


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def ref_class(kind):
    return getattr(importlib.import_module(f"uniception.models.{MODULE_OF[kind]}"), kind)


def forward_backward(name, dtype):
    kind, kw, _ = CASES[name]
    model = ref_class(kind)(**kw).train()
    fill(model)
    model = model.to(dtype)
    x = input_of(name).to(dtype).requires_grad_(True)
    outs = run(name, model, x, ViTEncoderInput, PredictionHeadInput)
    (outs[0].double() * cotangent(name, tuple(outs[0].shape)).double()).sum().backward()
    return model, x, outs


def padded(v):
    "a parameter's samples as a row of NSAMP values (its last sample repeated when it has fewer elements)"
    a = v.numpy()
    return np.concatenate([a, np.full(NSAMP - a.size, a[-1])]) if a.size < NSAMP else a.copy()


def cancellation(model, name, out):
    "norm of the output over the norm of the magnitudes of the terms of its last layer"
    kind = CASES[name][0]
    mod, feats = last_conv(model, kind), {}
    hook = mod.register_forward_hook(lambda m, inp, o: feats.__setitem__(0, (inp[0].detach(), o.detach())))
    with torch.no_grad():
        run(name, model, input_of(name).double(), ViTEncoderInput, PredictionHeadInput)
    hook.remove()
    xin, o = feats[0]
    t = F.conv2d(xin.abs(), mod.weight.detach().abs(), mod.bias.detach().abs(), padding=mod.padding)
    return float(o.norm() / t.norm()), float(out.detach().norm()), float(out.detach().pow(2).mean().sqrt())


def main():
    store = {}
    for name, (kind, kw, _) in CASES.items():
        m64, x64, o64 = forward_backward(name, torch.float64)
        ratio, onorm, orms = cancellation(m64, name, o64[0])
        assert ratio > 1e-2, f"{name}: the last layer's output is {ratio:.2e} of its terms' scale: cancelling terms, pick other scales"
        assert 0.1 < orms < 10, f"{name}: output rms {orms:.3e} is not of order 1: change GAIN"
        store[f"{name}/keys"] = np.array(keys_of(m64))
        store[f"{name}/signature"] = np.array(signature(ref_class(kind)))
        store[f"{name}/cancel"] = np.array([ratio, onorm, orms])
        for i, o in enumerate(o64):
            store[f"{name}/out{i}"] = o.detach().numpy().copy()
        store[f"{name}/din"] = x64.grad.float().numpy().copy()
        idx = {k: sample_indices(p.numel(), NSAMP) for k, p in m64.named_parameters()}
        names = [k for k, _ in m64.named_parameters()]
        want = {k: p.grad.flatten()[idx[k]].clone() for k, p in m64.named_parameters()}
        store[f"{name}/p_names"] = np.array("\n".join(names))
        store[f"{name}/p_samples"] = np.stack([padded(want[k]) for k in names])
        store[f"{name}/p_norm"] = np.array([p.grad.norm().item() for _, p in m64.named_parameters()])
        print(f"{name}: rms(out) = {orms:.3e} ({ratio:.2f} of its last layer's terms' scale), |din| = {x64.grad.norm():.3e}")
        for tag, dtype in (("e32", torch.float32), ("e16", torch.bfloat16)):
            m, x, outs = forward_backward(name, dtype)
            errs = {f"out{i}": rel_l2(o.detach(), o64[i].detach()) for i, o in enumerate(outs)}
            errs["din"] = rel_l2(x.grad, x64.grad)
            for q, e in errs.items():
                store[f"{name}/{tag}/{q}"] = np.float64(e)
            perr = grad_errors({k: p.grad.flatten()[idx[k]] for k, p in m.named_parameters()}, want)
            store[f"{name}/{tag}/p"] = np.array([perr[k] for k in names])
            worst = max((v, q) for q, v in perr.items())
            print(f"  {tag}: out0 {errs['out0']:.3e}  din {errs['din']:.3e}  parameter gradients max {worst[0]:.3e} ({worst[1]})")
    path = os.path.join(HERE, "cosmos.npz")
    np.savez_compressed(path, **store)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
