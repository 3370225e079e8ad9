"""Golden vectors of the Perception Encoder wrappers from the REAL reference classes on the CPU (recipe of
make_golden_input_encoders.py: the reference is imported from its own tree with the two import stubs of SURVEY.md App. B on PYTHONPATH):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<stubs>:<reference>:<repo> python3 -B tests/golden/make_golden_perception_encoder.py

The reference wrapper downloads its weights in the constructor, so it cannot be built offline as it is: the maker replaces
`pe.VisionTransformer.from_config` by a function that returns a tiny reference `VisionTransformer(**config of the case)` and runs the
real `PerceptionEncoder` / `PerceptionEncoderIntermediateFeatureReturner` constructor and forward around it.

Writes tests/golden/perception_encoder_<case>.npz (one file per case: each stays under the 1 MiB limit of a committed file),
perception_encoder_rope.npz and pe_configs.json; data only.  Per case of perception_encoder_cases.py:
  <case>/keys, <case>/signature          "name:shape" of every state_dict entry / the constructor's "name=default" lines
  <case>/out<i>, /din0                   the reference run in FLOAT64 (module and input cast to double), train mode: every output, and
                                         the gradient of L = sum_i <out_i, R_i> (seeded R_i) with respect to the image (rounded to fp32)
  <case>/p/<param>__samples, __norm      evenly spaced samples (NSAMP, float64) and the norm of every parameter gradient of that run
  <case>/nograd                          the parameters that received no gradient (the unused pooling head, `proj`, ...)
  <case>/e32/<q>, <case>/e16/<q>         error against the float64 run of the reference's OWN fp32 / bfloat16-on-CPU arithmetic on
                                         fresh leaf tensors, q = out<i>, din0 (rel-L2), p/<param> (input_encoders_cases.grad_errors)
  <case>/second/out<i>, second/e32|e16   (cases with a second image: another grid) the outputs for it, and their errors
perception_encoder_rope.npz:
  rope/{cls,nocls}/{q,k}                 the reference's Rope2D on perception_encoder_cases.rope_inputs at grid 3 x 5
pe_configs.json: asdict of every PE_VISION_CONFIG entry and the wrapper's (checkpoint_type, size) -> name table.
Inputs, weights and cotangents are regenerated from seeds (perception_encoder_cases), not stored.
"""
import inspect
import json
import os
import re
import sys
from dataclasses import asdict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden.cases import sample_indices  # noqa: E402
from tests.golden.input_encoders_cases import grad_errors, keys_of, signature  # noqa: E402
from tests.golden.perception_encoder_cases import CASES, CONFIGS, NSAMP, ROPE_DIM, ROPE_GRID, cotangent, fill, inputs, kwargs, outputs, rope_inputs  # noqa: E402

import uniception.models.encoders.perception_encoder as ref_enc  # noqa: E402
import uniception.models.libs.perception_encoder.vision_encoder.pe as ref_pe  # noqa: E402
from uniception.models.encoders.base import ViTEncoderInput  # noqa: E402
from uniception.models.libs.perception_encoder.vision_encoder.config import PE_VISION_CONFIG  # noqa: E402
from uniception.models.libs.perception_encoder.vision_encoder.rope import Rope2D  # noqa: E402

_TOWER = {}


def _tiny_from_config(cls, name, pretrained=False, checkpoint_path=None, **kw):
    return cls(**_TOWER["config"])


ref_pe.VisionTransformer.from_config = classmethod(_tiny_from_config)


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def build(name, dtype):
    kind, cfg = CASES[name][:2]
    _TOWER["config"] = CONFIGS[cfg]
    model = getattr(ref_enc, kind)(**kwargs(name)).train()
    fill(model)
    return model.to(dtype)


def forward_backward(name, dtype):
    model = build(name, dtype)
    x = inputs(name)[0].to(dtype).requires_grad_(True)
    outs = outputs(name, model, x, ViTEncoderInput)
    sum((o.double() * cotangent(name, i, tuple(o.shape)).double()).sum() for i, o in enumerate(outs)).backward()
    return model, x, outs


def wrapper_table():
    "the (checkpoint_type, size) -> config name table, read out of the reference constructor's source (it is a local there)"
    src = inspect.getsource(ref_enc.PerceptionEncoder.__init__)
    return {f"{a}/{b}": c for a, b, c in re.findall(r'\("(\w+)",\s*"(\w+)"\):\s*"([\w-]+)"', src)}


def save(tag, store):
    path = os.path.join(HERE, f"perception_encoder_{tag}.npz")
    np.savez_compressed(path, **store)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < (1 << 20), path


def main():
    for name, (kind, _, _, _, shapes) in CASES.items():
        store = {}
        m64, x64, o64 = forward_backward(name, torch.float64)
        store[f"{name}/keys"] = np.array(keys_of(m64))
        store[f"{name}/signature"] = np.array(signature(getattr(ref_enc, kind)))
        for i, o in enumerate(o64):
            store[f"{name}/out{i}"] = o.detach().numpy().copy()
        store[f"{name}/din0"] = x64.grad.float().numpy().copy()
        with_grad = {k: p for k, p in m64.named_parameters() if p.grad is not None}
        nograd = [k for k, p in m64.named_parameters() if p.grad is None]
        assert all(re.search(r"attn_pool|\.proj$|ln_post", k) for k in nograd), nograd
        store[f"{name}/nograd"] = np.array("\n".join(nograd))
        idx = {k: sample_indices(p.numel(), NSAMP) for k, p in with_grad.items()}
        want = {}
        for k, p in with_grad.items():
            want[k] = p.grad.flatten()[idx[k]].clone()
            store[f"{name}/p/{k}__samples"] = want[k].numpy().copy()
            store[f"{name}/p/{k}__norm"] = np.float64(p.grad.norm().item())
        print(f"{name}: {len(o64)} outputs, |out0| = {o64[0].detach().norm():.3e}, |din0| = {x64.grad.norm():.3e}, "
              f"{len(with_grad)} parameter gradients, {len(nograd)} parameters without one")
        second = {}
        if len(shapes) > 1:
            with torch.no_grad():
                second[torch.float64] = outputs(name, m64, inputs(name)[1].double(), ViTEncoderInput)
            for i, o in enumerate(second[torch.float64]):
                store[f"{name}/second/out{i}"] = o.numpy().copy()
        for tag, dtype in (("e32", torch.float32), ("e16", torch.bfloat16)):
            m, x, outs = forward_backward(name, dtype)
            errs = {f"out{i}": rel_l2(o.detach(), r.detach()) for i, (o, r) in enumerate(zip(outs, o64))}
            errs["din0"] = rel_l2(x.grad, x64.grad)
            assert [k for k, p in m.named_parameters() if p.grad is None] == nograd
            for k, e in grad_errors({k: p.grad.flatten()[idx[k]] for k, p in m.named_parameters() if p.grad is not None}, want).items():
                errs[f"p/{k}"] = e
            for q, e in errs.items():
                store[f"{name}/{tag}/{q}"] = np.float64(e)
            worst = max((v, q) for q, v in errs.items() if q.startswith("p/"))
            print(f"  {tag}: out0 {errs['out0']:.3e}  din0 {errs['din0']:.3e}  parameter gradients max {worst[0]:.3e} ({worst[1]})")
            if second:
                with torch.no_grad():
                    o2 = outputs(name, m, inputs(name)[1].to(dtype), ViTEncoderInput)
                for i, (o, r) in enumerate(zip(o2, second[torch.float64])):
                    errs[f"second/out{i}"] = store[f"{name}/second/{tag}/out{i}"] = np.float64(rel_l2(o, r))
                print(f"  {tag}: second image out0 {float(errs['second/out0']):.3e}")
            if tag == "e16":
                assert all(float(v) < 0.25 for v in errs.values()), f"{name}: a bfloat16 error of the reference is not below 0.25: change the scales in fill"
        for q in ["keys", "signature", "out0", "din0", "nograd", "e32/out0", "e16/out0", "e32/din0", "e16/din0"]:
            assert f"{name}/{q}" in store, (name, q)
        assert all(f"{name}/{t}/p/{k}" in store for t in ("e32", "e16") for k in with_grad)
        save(name, store)

    store = {}
    for tag, with_cls in (("cls", True), ("nocls", False)):
        rope = Rope2D(dim=ROPE_DIM, use_cls_token=with_cls)
        rope.init_tensors()
        rope.update_grid(torch.device("cpu"), *ROPE_GRID)
        q, k = rope(*rope_inputs(with_cls))
        store[f"rope/{tag}/q"], store[f"rope/{tag}/k"] = q.numpy().copy(), k.numpy().copy()
    assert all(f"rope/{t}/{x}" in store for t in ("cls", "nocls") for x in "qk")

    save("rope", store)
    table = wrapper_table()
    assert len(table) == 7, table
    path = os.path.join(HERE, "pe_configs.json")
    with open(path, "w") as f:
        json.dump({"configs": {k: asdict(v) for k, v in PE_VISION_CONFIG.items()}, "wrapper": table}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
