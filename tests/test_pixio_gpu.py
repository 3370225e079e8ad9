"""GPU: PixioEncoder against the float64 run of the REAL reference class (tests/golden/pixio_<case>.npz): the features and every gradient,
in train mode, in engine.precision("fp32") and "bf16"; then inference, the second grid, gradient checkpointing, and a checkpoint file
with `blocks.N.*` keys.

Tolerances (the rule of tests/test_perception_encoder_gpu.py): fp32: output within max(2e-6, 8 e32) (rel-L2),
gradients within 1e-3; bf16: every quantity within 2 x e16 — e32 / e16: the reference's own fp32 / bfloat16-on-CPU error against float64,
from the fixture.  Gradient checkpointing: the same output bits, gradients within 1e-5.  The attention route is asserted: head_dim 64
takes an existing fused route, head_dim 80 / 96 the "wide" one."""
import os

import numpy as np
import pytest
import torch

from tests.golden.cases import sample_indices
from tests.golden.input_encoders_cases import grad_errors
from tests.golden.pixio_cases import CASES, NSAMP, cotangent, fill, inputs, kwargs, plain_key
from tests.helpers import GOLDEN_DIR, rel_l2

pytestmark = pytest.mark.gpu
_GOLD = {}


def gold(name):
    if name not in _GOLD:
        _GOLD[name] = np.load(os.path.join(GOLDEN_DIR, f"pixio_{name}.npz"))
    return _GOLD[name]


def _model(name, gpu, **extra):
    from uniception_amd.models.encoders import PixioEncoder
    model = PixioEncoder(**{**kwargs(name), **extra})
    fill(model, name)
    return model.to(gpu)


def _run(model, image):
    from uniception_amd.models.encoders import ViTEncoderInput
    return model(ViTEncoderInput(image=image, data_norm_type="pixio")).features


def _forward_backward(name, model, gpu, mode):
    from uniception_amd import engine
    x = inputs(name)[0].to(gpu).requires_grad_(True)
    with engine.precision(mode):
        out = _run(model, x)
        (out.float() * cotangent(name, tuple(out.shape)).to(gpu)).sum().backward()
    torch.cuda.synchronize()
    return x, out


def _bound_second(G, name, mode):
    "the bound of the second image's output"
    e = float(G[f"{name}/second/{'e32' if mode == 'fp32' else 'e16'}/out0"])
    return max(2e-6, 8.0 * e) if mode == "fp32" else 2.0 * e


def _bound(G, name, mode, q):
    if mode == "fp32":
        return max(2e-6, 8.0 * float(G[f"{name}/e32/{q}"])) if q.endswith("out0") else 1e-3
    return 2.0 * float(G[f"{name}/e16/{q}"])


class _Routes:
    "records what engine.attention_route returns while a model runs"

    def __init__(self, monkeypatch):
        from uniception_amd import engine
        self.seen, real = [], engine.attention_route

        def spy(*a, **k):
            r = real(*a, **k)
            self.seen.append(r)
            return r
        monkeypatch.setattr(engine, "attention_route", spy)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_forward_and_backward_against_the_reference_in_fp64(gpu, monkeypatch, name, mode):
    from uniception_amd import engine
    G = gold(name)
    model = _model(name, gpu).train()
    x, out = _forward_backward(name, model, gpu, mode)
    tag = "e32" if mode == "fp32" else "e16"
    assert out.dtype == torch.float32 and tuple(out.shape) == G[f"{name}/out0"].shape
    errs = {"out0": rel_l2(out.detach().cpu(), torch.from_numpy(G[f"{name}/out0"])), "din0": rel_l2(x.grad.cpu(), torch.from_numpy(G[f"{name}/din0"]))}
    got, want = {}, {}
    for k, p in model.named_parameters():
        assert p.grad is not None, f"{k} received no gradient"
        idx = torch.from_numpy(sample_indices(p.numel(), NSAMP))
        got[k], want[k] = p.grad.flatten().cpu()[idx], torch.from_numpy(G[f"{name}/p/{k}__samples"])
    errs.update({f"p/{k}": e for k, e in grad_errors(got, want).items()})
    stored = {q[len(name) + len(tag) + 2:] for q in G.files if q.startswith(f"{name}/{tag}/")}
    assert set(errs) == stored, (set(errs) ^ stored)               # no quantity is skipped
    bad = []
    for q, err in errs.items():
        bound = _bound(G, name, mode, q)
        print(f"{name} {mode} {q}: {err:.3e} (bound {bound:.3e})")
        if not err < bound:
            bad.append((q, err, bound))
    assert not bad, bad
    # eval mode, no graph: the inference pipeline; its attention route is the one the head_dim calls for
    routes = _Routes(monkeypatch)
    with torch.no_grad(), engine.precision(mode):
        again = _run(model.eval(), x.detach())
        cached = _run(model, x.detach())
    assert again.grad_fn is None and torch.equal(again, cached)
    err, bound = rel_l2(again.cpu(), torch.from_numpy(G[f"{name}/out0"])), _bound(G, name, mode, "out0")
    print(f"{name} {mode} inference out0: {err:.3e} (bound {bound:.3e}) routes {sorted(set(routes.seen))}")
    assert err < bound
    hd = CASES[name][0] // CASES[name][1]
    want_routes = {"unfused"} if mode == "fp32" else ({"wide"} if hd in (80, 96) else {"vt_epilogue", "vt_pack"})
    assert routes.seen and set(routes.seen) <= want_routes, (routes.seen, want_routes)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["h80", "h80_nockpt"])
def test_second_forward_at_another_grid(gpu, name, mode):
    "the resized table is cached per grid: the native 4 x 4 forward first, then the fixture's second image (3 x 5), then the first again"
    from uniception_amd import engine
    G = gold(name)
    model = _model(name, gpu).eval()
    first, second = (t.to(gpu) for t in inputs(name))
    with torch.no_grad(), engine.precision(mode):
        a, b, a2 = _run(model, first), _run(model, second), _run(model, first)
    for label, got, key in (("first", a, "out0"), ("second", b, "second/out0")):
        err, bound = rel_l2(got.cpu(), torch.from_numpy(G[f"{name}/{key}"])), (_bound(G, name, mode, "out0") if key == "out0" else _bound_second(G, name, mode))
        print(f"{name} {mode} {label} image: {err:.3e} (bound {bound:.3e})")
        assert tuple(got.shape) == G[f"{name}/{key}"].shape and err < bound
    assert torch.equal(a, a2)
    model.train()      # in training the table is resampled differentiably on every call
    with engine.precision(mode):
        bt = _run(model, second)
    assert bt.requires_grad
    assert rel_l2(bt.detach().cpu(), torch.from_numpy(G[f"{name}/second/out0"])) < _bound_second(G, name, mode)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_gradient_checkpointing_equals_the_plain_run(gpu, mode):
    plain, ckpt = _model("h80_nockpt", gpu).train(), _model("h80", gpu).train()
    assert all(type(b).__name__ == "_CheckpointingWrapper" for b in ckpt.blocks) and not any(hasattr(b, "inner") for b in plain.blocks)
    x0, out0 = _forward_backward("h80_nockpt", plain, gpu, mode)
    x1, out1 = _forward_backward("h80", ckpt, gpu, mode)
    assert torch.equal(out0, out1)                                     # the same kernels on the same inputs
    assert rel_l2(x1.grad.double().cpu(), x0.grad.double().cpu()) < 1e-5
    pg = dict(plain.named_parameters())
    for k, q in ckpt.named_parameters():
        assert rel_l2(q.grad.double().cpu(), pg[plain_key(k)].grad.double().cpu()) < 1e-5, k


def test_a_checkpoint_file_with_plain_block_keys_loads_before_the_blocks_are_wrapped(gpu, tmp_path):
    from uniception_amd import engine
    src = _model("h80_nockpt", gpu)
    path = os.path.join(str(tmp_path), "pixio.pth")
    torch.save({k: v.cpu() for k, v in src.state_dict().items()}, path)
    assert not any(".inner." in k for k in src.state_dict())
    from uniception_amd.models.encoders import PixioEncoder
    loaded = PixioEncoder(**kwargs("h80"), pretrained_checkpoint_path=path).to(gpu).eval()
    assert all(torch.equal(v, src.state_dict()[plain_key(k)]) for k, v in loaded.state_dict().items())
    x = inputs("h80")[0].to(gpu)
    with torch.no_grad(), engine.precision("bf16"):
        assert torch.equal(_run(loaded, x), _run(src.eval(), x))
