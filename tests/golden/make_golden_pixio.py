"""Golden vectors of PixioEncoder from the REAL reference class on the CPU (recipe of make_golden_perception_encoder.py: the reference is
imported from its own tree with the two import stubs of SURVEY.md App. B on PYTHONPATH):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<stubs>:<reference>:<repo> python3 -B tests/golden/make_golden_pixio.py

The reference downloads its weights in the constructor (get_pth_file -> hf_hub_download, then torch.load): the maker replaces
`PixioEncoder.get_pth_file` by a function that returns a placeholder and `torch.load`, during construction, by one that returns an empty
state_dict, so nothing is fetched and the real constructor and forward run.

Writes tests/golden/pixio_<case>.npz; data only.  Per case of pixio_cases.py:
  <case>/keys, <case>/signature       "name:shape" of every state_dict entry / the constructor's "name=default" lines
  <case>/out0, /din0                  the reference run in FLOAT64, train mode: the features, and the gradient of L = <out, R> (seeded R) with
                                      respect to the image (rounded to fp32)
  <case>/p/<param>__samples, __norm   evenly spaced samples (NSAMP, float64) and the norm of every parameter gradient of that run
  <case>/e32/<q>, <case>/e16/<q>      error against the float64 run of the reference's OWN fp32 / bfloat16-on-CPU arithmetic, q = out0, din0
                                      (rel-L2), p/<param> (input_encoders_cases.grad_errors)
  <case>/second/out0, second/e32|e16  (cases with a second image: another grid) its features, and their errors
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden.cases import sample_indices  # noqa: E402
from tests.golden.input_encoders_cases import grad_errors, keys_of, signature  # noqa: E402
from tests.golden.pixio_cases import CASES, NSAMP, cotangent, fill, inputs, kwargs  # noqa: E402

import uniception.models.encoders.pixio as ref  # noqa: E402
from uniception.models.encoders.base import ViTEncoderInput  # noqa: E402

ref.PixioEncoder.get_pth_file = lambda self, repo_id: "nothing-is-fetched"


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def build(name, dtype):
    real_load = torch.load
    torch.load = lambda *a, **k: {}
    try:
        model = ref.PixioEncoder(**kwargs(name)).train()
    finally:
        torch.load = real_load
    fill(model, name)
    return model.to(dtype)


def run(model, image):
    return model(ViTEncoderInput(image=image, data_norm_type="pixio")).features


def forward_backward(name, dtype):
    model = build(name, dtype)
    x = inputs(name)[0].to(dtype).requires_grad_(True)
    out = run(model, x)
    (out.double() * cotangent(name, tuple(out.shape)).double()).sum().backward()
    return model, x, out


def main():
    for name in CASES:
        store = {}
        m64, x64, o64 = forward_backward(name, torch.float64)
        store[f"{name}/keys"] = np.array(keys_of(m64))
        store[f"{name}/signature"] = np.array(signature(ref.PixioEncoder))
        store[f"{name}/out0"] = o64.detach().numpy().copy()
        store[f"{name}/din0"] = x64.grad.float().numpy().copy()
        grads = {k: p.grad for k, p in m64.named_parameters()}
        assert all(g is not None for g in grads.values())
        idx = {k: sample_indices(g.numel(), NSAMP) for k, g in grads.items()}
        want = {}
        for k, g in grads.items():
            want[k] = g.flatten()[idx[k]].clone()
            store[f"{name}/p/{k}__samples"] = want[k].numpy().copy()
            store[f"{name}/p/{k}__norm"] = np.float64(g.norm().item())
        print(f"{name}: out {tuple(o64.shape)}, |out0| = {o64.detach().norm():.3e}, |din0| = {x64.grad.norm():.3e}, {len(grads)} parameter gradients")
        second64 = None
        if len(CASES[name][4]) > 1:
            with torch.no_grad():
                second64 = run(m64, inputs(name)[1].double())
            store[f"{name}/second/out0"] = second64.numpy().copy()
        for tag, dtype in (("e32", torch.float32), ("e16", torch.bfloat16)):
            m, x, out = forward_backward(name, dtype)
            errs = {"out0": rel_l2(out.detach(), o64.detach()), "din0": rel_l2(x.grad, x64.grad)}
            for k, e in grad_errors({k: p.grad.flatten()[idx[k]] for k, p in m.named_parameters()}, want).items():
                errs[f"p/{k}"] = e
            for q, e in errs.items():
                store[f"{name}/{tag}/{q}"] = np.float64(e)
            worst = max((v, q) for q, v in errs.items() if q.startswith("p/"))
            print(f"  {tag}: out0 {errs['out0']:.3e}  din0 {errs['din0']:.3e}  parameter gradients max {worst[0]:.3e} ({worst[1]})")
            if second64 is not None:
                with torch.no_grad():
                    e2 = rel_l2(run(m, inputs(name)[1].to(dtype)), second64)
                store[f"{name}/second/{tag}/out0"] = np.float64(e2)
                print(f"  {tag}: second image out0 {e2:.3e}")
            if tag == "e16":
                assert all(float(v) < 0.25 for v in errs.values()), f"{name}: a bfloat16 error of the reference is not below 0.25"
        path = os.path.join(HERE, f"pixio_{name}.npz")
        np.savez_compressed(path, **store)
        print(f"wrote {path}: {os.path.getsize(path)} bytes")
        assert os.path.getsize(path) < (1 << 20), path


if __name__ == "__main__":
    main()
