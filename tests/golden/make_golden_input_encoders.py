"""Golden vectors of the non-image input encoders from the REAL reference classes on the CPU (recipe of make_golden_moge_heads.py: the
reference is imported from its own tree with the two import stubs of SURVEY.md App. B on PYTHONPATH):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<stubs>:<reference>:<repo> python3 -B tests/golden/make_golden_input_encoders.py

Writes tests/golden/input_encoders.npz; data only.  Per case of tests/golden/input_encoders_cases.py:
  <case>/keys, <case>/signature          "name:shape" of every state_dict entry / the constructor's "name=default" lines
  <case>/pos_embed_init                  (dense cases with a table) the sinusoid buffer as the reference's constructor leaves it
  <case>/out, /din0                      the reference run in FLOAT64 (module and input cast to double), train mode: output, and the
                                         gradient of L = <out, R> (seeded R) with respect to the input (stored rounded to fp32)
  <case>/p/<param>__samples, __norm      evenly spaced samples (NSAMP, float64) and the norm of every parameter gradient of that run
  <case>/e32/<q>, <case>/e16/<q>         error against the float64 run of the reference's OWN fp32 / bfloat16-on-CPU arithmetic,
                                         q = out, din0 (rel-L2), p/<param> (on the stored samples, divided by max(|g_ref|, 1e-3 x the
                                         largest parameter-gradient norm of the case): input_encoders_cases.grad_errors)
Inputs, weights and cotangents are regenerated from seeds (input_encoders_cases), not stored.
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden.cases import sample_indices  # noqa: E402
from tests.golden.input_encoders_cases import CASES, MODULE_OF, NSAMP, cotangent, fill, grad_errors, inputs, keys_of, kwargs, run, signature  # noqa: E402

from uniception.models.encoders.base import EncoderGlobalRepInput, ViTEncoderNonImageInput  # noqa: E402


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def ref_class(kind):
    return getattr(importlib.import_module(f"uniception.models.encoders.{MODULE_OF[kind]}"), kind)


def forward_backward(name, dtype):
    kind = CASES[name][0]
    model = ref_class(kind)(**kwargs(name)).train()
    fill(model)
    model = model.to(dtype)
    xs = [x.to(dtype).requires_grad_(True) for x in inputs(name)]
    out = run(name, model, xs, ViTEncoderNonImageInput, EncoderGlobalRepInput)
    (out.double() * cotangent(name, tuple(out.shape)).double()).sum().backward()
    return model, xs, out


def last_layer(model):
    "the module that writes the output: the last LayerNorm that is applied, else the last Linear / convolution"
    for attr in ("post_pe_norm", "norm_layer", "norm"):
        m = getattr(model, attr, None)
        if isinstance(m, torch.nn.LayerNorm) and (attr != "post_pe_norm" or getattr(model, "apply_pe", True)):
            return m
    return [m for m in model.modules() if isinstance(m, (torch.nn.Linear, torch.nn.Conv2d))][-1]


def cancellation(model, name, out):
    """how much of its operands' magnitude the last layer keeps: for a LayerNorm |z - mean(z)| / |z| over its input rows (a row that is
    almost its own mean loses that many digits in the subtraction), for a Linear / 1x1 convolution |out| / | |x| |W|^T + |b| |"""
    mod, seen = last_layer(model), {}
    hook = mod.register_forward_hook(lambda m, inp, o: seen.update(x=inp[0].detach()))
    with torch.no_grad():
        run(name, model, [x.double() for x in inputs(name)], ViTEncoderNonImageInput, EncoderGlobalRepInput)
    hook.remove()
    z = seen["x"]
    if isinstance(mod, torch.nn.LayerNorm):
        return float((z - z.mean(-1, keepdim=True)).norm() / z.norm()), float(out.detach().norm())
    w = mod.weight.detach().abs().reshape(mod.weight.shape[0], -1)
    zc = z.abs() if z.dim() == 2 else z.abs().permute(0, 2, 3, 1).reshape(-1, z.shape[1])
    return float(out.detach().norm() / (zc @ w.t() + mod.bias.detach().abs()).norm()), float(out.detach().norm())


def main():
    store = {}
    for name, (kind, _) in CASES.items():
        pristine = ref_class(kind)(**kwargs(name))
        if kind == "DenseRepresentationEncoder" and pristine.apply_pe:
            store[f"{name}/pos_embed_init"] = pristine.pos_embed.numpy().copy()
        m64, x64, o64 = forward_backward(name, torch.float64)
        ratio, onorm = cancellation(m64, name, o64)
        assert ratio > 1e-2, f"{name}: the last layer keeps {ratio:.2e} of its operands' magnitude: cancelling terms, pick other scales"
        store[f"{name}/keys"] = np.array(keys_of(m64))
        store[f"{name}/signature"] = np.array(signature(ref_class(kind)))
        store[f"{name}/out"] = o64.detach().numpy().copy()
        store[f"{name}/din0"] = x64[0].grad.float().numpy().copy()
        idx = {k: sample_indices(p.numel(), NSAMP) for k, p in m64.named_parameters()}
        want = {}
        for k, p in m64.named_parameters():
            assert p.grad is not None, f"{name}: {k} received no gradient"
            want[k] = p.grad.flatten()[idx[k]].clone()
            store[f"{name}/p/{k}__samples"] = want[k].numpy().copy()
            store[f"{name}/p/{k}__norm"] = np.float64(p.grad.norm().item())
        print(f"{name}: |out| = {onorm:.3e} (cancellation ratio {ratio:.2f}), |din0| = {x64[0].grad.norm():.3e}")
        for tag, dtype in (("e32", torch.float32), ("e16", torch.bfloat16)):
            m, xs, o = forward_backward(name, dtype)
            errs = {"out": rel_l2(o.detach(), o64.detach()), "din0": rel_l2(xs[0].grad, x64[0].grad)}
            for k, e in grad_errors({k: p.grad.flatten()[idx[k]] for k, p in m.named_parameters()}, want).items():
                errs[f"p/{k}"] = e
            for q, e in errs.items():
                store[f"{name}/{tag}/{q}"] = np.float64(e)
            worst = max((v, q) for q, v in errs.items() if q.startswith("p/"))
            print(f"  {tag}: out {errs['out']:.3e}  din0 {errs['din0']:.3e}  parameter gradients max {worst[0]:.3e} ({worst[1]})")
            if tag == "e16":
                assert all(v < 0.25 for v in errs.values()), f"{name}: a bfloat16 error of the reference is not below 0.25: change the scales in fill"
    path = os.path.join(HERE, "input_encoders.npz")
    np.savez_compressed(path, **store)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
