"""GPU: PerceptionEncoder / PerceptionEncoderIntermediateFeatureReturner against the float64 run of the REAL reference wrappers
(tests/golden/perception_encoder_<case>.npz), every output and every gradient, in train mode, in engine.precision("fp32") and "bf16".

Tolerances (the rule of tests/test_input_encoders_gpu.py): fp32: outputs within max(2e-6, 8 e32) (rel-L2), gradients within 1e-3;
bf16: every quantity within 2 x e16 — e32 / e16: the reference's own fp32 / bfloat16-on-CPU error against float64, from the fixture.
Parameter-gradient errors are divided by max(|g_ref|, 1e-3 x the largest parameter-gradient norm of the case), in the fixture and here
(input_encoders_cases.grad_errors).  Parameters the reference leaves without a gradient (the pooling head, `proj`, ln_post where it is
not applied) have none here either.  Gradient checkpointing: the same output bits, gradients within 1e-5 (the rule of
tests/test_checkpointing_gpu.py)."""
import os

import numpy as np
import pytest
import torch

from tests.golden.cases import sample_indices
from tests.golden.input_encoders_cases import grad_errors
from tests.golden.perception_encoder_cases import CASES, CONFIG_NAME, CONFIGS, NSAMP, cotangent, fill, inputs, kwargs, outputs
from tests.helpers import GOLDEN_DIR, rel_l2

pytestmark = pytest.mark.gpu
_GOLD = {}


def gold(name):
    if name not in _GOLD:
        _GOLD[name] = np.load(os.path.join(GOLDEN_DIR, f"perception_encoder_{name}.npz"))
    return _GOLD[name]


def _model(name, gpu, monkeypatch, **extra):
    from uniception_amd.models import encoders as E
    from uniception_amd.models.libs.perception_encoder.vision_encoder import config
    kind, cfg, key = CASES[name][:3]
    monkeypatch.setitem(config.PE_VISION_CONFIG, CONFIG_NAME[key], config.PEConfig(**CONFIGS[cfg]))
    model = getattr(E, kind)(**kwargs(name), **extra)
    fill(model)                                # the reference's state_dict, rebuilt from the case's seeds (name-keyed filler)
    return model.to(gpu)


def _run(name, model, image):
    from uniception_amd.models.encoders import ViTEncoderInput
    return outputs(name, model, image, ViTEncoderInput)


def _forward_backward(name, model, gpu, mode):
    from uniception_amd import engine
    x = inputs(name)[0].to(gpu).requires_grad_(True)
    with engine.precision(mode):
        outs = _run(name, model, x)
        sum((o.float() * cotangent(name, i, tuple(o.shape)).to(gpu)).sum() for i, o in enumerate(outs)).backward()
    torch.cuda.synchronize()
    return x, outs


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_forward_and_backward_against_the_reference_in_fp64(gpu, monkeypatch, name, mode):
    from uniception_amd import engine
    G = gold(name)
    model = _model(name, gpu, monkeypatch).train()
    x, outs = _forward_backward(name, model, gpu, mode)
    fp32 = mode == "fp32"
    tag = "e32" if fp32 else "e16"
    errs = {}
    for i, o in enumerate(outs):
        assert o.dtype == torch.float32 and tuple(o.shape) == G[f"{name}/out{i}"].shape
        errs[f"out{i}"] = rel_l2(o.detach().cpu(), torch.from_numpy(G[f"{name}/out{i}"]))
    assert f"{name}/out{len(outs)}" not in G.files
    assert x.grad is not None
    errs["din0"] = rel_l2(x.grad.cpu(), torch.from_numpy(G[f"{name}/din0"]))
    nograd = [k for k in str(G[f"{name}/nograd"]).split("\n") if k]
    got, want = {}, {}
    for k, p in model.named_parameters():
        if k in nograd:
            assert p.grad is None, f"{k} is unused by the reference's feature path and must receive no gradient"
            continue
        assert p.grad is not None, f"{k} received no gradient"
        idx = torch.from_numpy(sample_indices(p.numel(), NSAMP))
        got[k], want[k] = p.grad.flatten().cpu()[idx], torch.from_numpy(G[f"{name}/p/{k}__samples"])
    errs.update({f"p/{k}": e for k, e in grad_errors(got, want).items()})
    stored = {q[len(name) + len(tag) + 2:] for q in G.files if q.startswith(f"{name}/{tag}/")}
    assert set(errs) == stored, (set(errs) ^ stored)               # no quantity is skipped
    bad = []
    for q, err in errs.items():
        if fp32:
            bound = max(2e-6, 8.0 * float(G[f"{name}/e32/{q}"])) if q.startswith("out") else 1e-3
        else:
            bound = 2.0 * float(G[f"{name}/e16/{q}"])
        print(f"{name} {mode} {q}: {err:.3e} (bound {bound:.3e})")
        if not err < bound:
            bad.append((q, err, bound))
    assert not bad, bad
    # eval mode, no graph: the inference pipeline (cached permuted in_proj rows, cached position table, folded LayerScale)
    with torch.no_grad(), engine.precision(mode):
        again = _run(name, model.eval(), x.detach())
        cached = _run(name, model, x.detach())
    for i, (a, c_, o) in enumerate(zip(again, cached, outs)):
        assert a.grad_fn is None and not a.requires_grad and torch.equal(a, c_)
        err = rel_l2(a.cpu(), torch.from_numpy(G[f"{name}/out{i}"]))
        bound = max(2e-6, 8.0 * float(G[f"{name}/e32/out{i}"])) if fp32 else 2.0 * float(G[f"{name}/e16/out{i}"])
        print(f"{name} {mode} inference out{i}: {err:.3e} (bound {bound:.3e})")
        assert err < bound


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_second_forward_at_another_grid(gpu, monkeypatch, mode):
    "position-table and RoPE-position caches are per grid: a 5 x 9 forward first, then the fixture's second image (4 x 6), then the first again"
    from uniception_amd import engine
    name = "core_cls"
    G = gold(name)
    model = _model(name, gpu, monkeypatch).eval()
    first, second = (t.to(gpu) for t in inputs(name))
    tag = "e32" if mode == "fp32" else "e16"
    with torch.no_grad(), engine.precision(mode):
        a = _run(name, model, first)[0]
        b = _run(name, model, second)[0]
        a2 = _run(name, model, first)[0]
    for label, got, key, ekey in (("first", a, "out0", f"{tag}/out0"), ("second", b, "second/out0", f"second/{tag}/out0")):
        e = float(G[f"{name}/{ekey}"])
        bound = max(2e-6, 8.0 * e) if mode == "fp32" else 2.0 * e
        err = rel_l2(got.cpu(), torch.from_numpy(G[f"{name}/{key}"]))
        print(f"{name} {mode} {label} image: {err:.3e} (bound {bound:.3e})")
        assert tuple(got.shape) == G[f"{name}/{key}"].shape and err < bound
    assert torch.equal(a, a2)
    # in training the table is resampled differentiably on every call: the second grid's output is within the same bound
    model.train()
    with engine.precision(mode):
        bt = _run(name, model, second)[0]
    e = float(G[f"{name}/second/{tag}/out0"])
    assert rel_l2(bt.detach().cpu(), torch.from_numpy(G[f"{name}/second/out0"])) < (max(2e-6, 8.0 * e) if mode == "fp32" else 2.0 * e)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["lang_ls", "ret_norm"])
def test_gradient_checkpointing_equals_the_plain_run(gpu, monkeypatch, name, mode):
    plain, ckpt = _model(name, gpu, monkeypatch).train(), _model(name, gpu, monkeypatch, gradient_checkpointing=True).train()
    assert all(type(b).__name__.startswith("Checkpointed") for b in ckpt.model.transformer.resblocks)
    x0, out0 = _forward_backward(name, plain, gpu, mode)
    x1, out1 = _forward_backward(name, ckpt, gpu, mode)
    assert len(out0) == len(out1) and all(torch.equal(a, b) for a, b in zip(out0, out1))          # the same kernels on the same inputs
    assert rel_l2(x1.grad.double().cpu(), x0.grad.double().cpu()) < 1e-5
    for (k, p), (_, q) in zip(plain.named_parameters(), ckpt.named_parameters()):
        assert (p.grad is None) == (q.grad is None), k
        if p.grad is not None:
            assert rel_l2(q.grad.double().cpu(), p.grad.double().cpu()) < 1e-5, k


def test_an_updated_parameter_reaches_the_inference_caches(gpu, monkeypatch):
    "the permuted in_proj copy, the resampled table and the folded LayerScale are keyed on the parameters' versions"
    from uniception_amd import engine
    name = "lang_ls"
    model = _model(name, gpu, monkeypatch).eval()
    x = inputs(name)[0].to(gpu)
    with torch.no_grad(), engine.precision("bf16"):
        a = _run(name, model, x)[0]
        blk = model.model.transformer.resblocks[0]
        blk.attn.in_proj_weight.mul_(0.5)
        model.model.positional_embedding.add_(0.25)
        blk.ls_2.gamma.mul_(2.0)
        b = _run(name, model, x)[0]
        fresh = _model(name, gpu, monkeypatch).eval()
        fresh.load_state_dict(model.state_dict())
        c = _run(name, fresh, x)[0]
    assert not torch.equal(a, b) and torch.equal(b, c)
