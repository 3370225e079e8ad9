"""Golden vectors of the MoGe convolutional head and MLPFeature from the REAL reference classes on the CPU (recipe of
make_golden_summary_heads.py: the reference is imported from its own tree with the two import stubs of SURVEY.md App. B on PYTHONPATH):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<stubs>:<reference>:<repo> python3 -B tests/golden/make_golden_moge_heads.py

Writes tests/golden/moge_heads.npz; data only.  Per case of tests/golden/moge_heads_cases.py:
  <case>/keys, <case>/signature          "name:shape" of every state_dict entry / the constructor's "name=default" lines
  <case>/out, /din<i>                    the reference run in FLOAT64 (module and inputs cast to double), train mode: output, and the
                                         gradient of L = <out, R> (seeded R) with respect to input feature i (stored rounded to fp32)
  <case>/p/<param>__samples, __norm      evenly spaced samples (NSAMP, float64) and the norm of every parameter gradient of that run
  <case>/e32/<q>, <case>/e16/<q>         error against the float64 run of the reference's OWN fp32 / bfloat16-on-CPU arithmetic,
                                         q = out, din<i> (rel-L2), p/<param> (on the stored samples, divided by max(|g_ref|, 1e-3 x the
                                         largest parameter-gradient norm of the case): moge_heads_cases.grad_errors)
Inputs, weights and cotangents are regenerated from seeds (moge_heads_cases), not stored.
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
from tests.golden.moge_heads_cases import CASES, MODULE_OF, NSAMP, cotangent, fill, grad_errors, inputs, keys_of, run, signature  # noqa: E402

from uniception.models.prediction_heads.base import PredictionHeadInput, PredictionHeadLayeredInput  # noqa: E402


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def ref_class(kind):
    return getattr(importlib.import_module(f"uniception.models.prediction_heads.{MODULE_OF[kind]}"), kind)


def forward_backward(name, dtype):
    kind, kw, _, _ = CASES[name]
    model = ref_class(kind)(**kw).train()
    fill(model)
    model = model.to(dtype)
    xs = [x.to(dtype).requires_grad_(True) for x in inputs(name)]
    out = run(name, model, xs, PredictionHeadInput, PredictionHeadLayeredInput)
    (out.double() * cotangent(name, tuple(out.shape)).double()).sum().backward()
    return model, xs, out


def last_convs(model, kind):
    if kind == "MoGeConvFeature":
        return [b[-1] for b in model.output_block]
    return [model.layers[5]] if kind == "ResidualConvBlock" else [model.linear]


def cancellation(model, name, out):
    "norm of the output over the norm of the magnitudes of the terms of its last layer(s): far below 1 means cancelling terms"
    kind = CASES[name][0]
    feats, hooks = {}, []
    for i, mod in enumerate(last_convs(model, kind)):
        def keep(m, inp, o, i=i):
            feats[i] = inp[0].detach()
        hooks.append(mod.register_forward_hook(keep))
    with torch.no_grad():
        run(name, model, [x.double() for x in inputs(name)], PredictionHeadInput, PredictionHeadLayeredInput)
    terms = []
    for i, mod in enumerate(last_convs(model, kind)):
        hooks[i].remove()
        p = mod.kernel_size[0] // 2
        xin = F.pad(feats[i].abs(), (p, p, p, p), mode="replicate") if p else feats[i].abs()
        terms.append(F.conv2d(xin, mod.weight.detach().abs(), mod.bias.detach().abs()))
    t = torch.cat(terms, 1)
    if kind == "MLPFeature":
        t = F.pixel_shuffle(t, model.patch_size)
    return float(out.detach().norm() / t.norm()), float(out.detach().norm())


def main():
    store = {}
    for name, (kind, kw, _, _) in CASES.items():
        m64, x64, o64 = forward_backward(name, torch.float64)
        ratio, onorm = cancellation(m64, name, o64)
        assert ratio > 1e-2, f"{name}: output norm {onorm:.3e} is {ratio:.2e} of its terms' scale: cancelling terms, pick other scales"
        store[f"{name}/keys"] = np.array(keys_of(m64))
        store[f"{name}/signature"] = np.array(signature(ref_class(kind)))
        store[f"{name}/out"] = o64.detach().numpy().copy()
        for i, x in enumerate(x64):
            store[f"{name}/din{i}"] = x.grad.float().numpy().copy()
        idx = {k: sample_indices(p.numel(), NSAMP) for k, p in m64.named_parameters()}
        want = {}
        for k, p in m64.named_parameters():
            want[k] = p.grad.flatten()[idx[k]].clone()
            store[f"{name}/p/{k}__samples"] = want[k].numpy().copy()
            store[f"{name}/p/{k}__norm"] = np.float64(p.grad.norm().item())
        print(f"{name}: |out| = {onorm:.3e} ({ratio:.2f} of its terms' scale), |din0| = {x64[0].grad.norm():.3e}")
        for tag, dtype in (("e32", torch.float32), ("e16", torch.bfloat16)):
            m, xs, o = forward_backward(name, dtype)
            errs = {"out": rel_l2(o.detach(), o64.detach())}
            for i, x in enumerate(xs):
                errs[f"din{i}"] = rel_l2(x.grad, x64[i].grad)
            for k, e in grad_errors({k: p.grad.flatten()[idx[k]] for k, p in m.named_parameters()}, want).items():
                errs[f"p/{k}"] = e
            for q, e in errs.items():
                store[f"{name}/{tag}/{q}"] = np.float64(e)
            worst = max((v, q) for q, v in errs.items() if q.startswith("p/"))
            print(f"  {tag}: out {errs['out']:.3e}  din0 {errs['din0']:.3e}  parameter gradients max {worst[0]:.3e} ({worst[1]})")
            if tag == "e16":
                assert all(v < 0.25 for v in errs.values()), f"{name}: a bfloat16 error of the reference is not below 0.25: change the scales in fill"
    path = os.path.join(HERE, "moge_heads.npz")
    np.savez_compressed(path, **store)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
