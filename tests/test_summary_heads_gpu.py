"""GPU: the token-pooling kernels against float64, and the summary heads (PoseHead, GlobalHead, ResConvBlock, MLPHead) against the
float64 run of the REAL reference (tests/golden/summary_heads.npz), outputs and every gradient, in train mode.

Tolerances.
  uc_token_pool: rel-L2 < 1e-6 against the float64 mean of the values the kernel reads (bf16 inputs: of the rounded inputs) — a mean
    of at most a few thousand fp32 terms accumulated in fp32, unit roundoff 6e-8.  The inputs are N(0.5, 1): a mean of zero-mean
    samples is a cancelling sum, against which no relative bound means anything.  Two calls give the same bits.
  uc_token_pool_bwd: exact in fp32 (one correctly rounded division); bf16: one rounding, 2^-8 relative per element; gated-off elements exactly 0.
  modules, fp32: outputs within max(2e-6, 8 e32), e32 = the reference's own fp32 error against float64 from the fixture (the exact
    kernels sum K = 1024 in one ascending chain where the CPU sums in blocks; 2e-6 is the project's fp32 head gate); gradients
    rel-L2 < 1e-3 per tensor and their norms within 1e-3 (the gates of the sibling head and transformer tests).
  modules, bf16: every quantity within 2 x e16, the reference's own bfloat16-on-CPU error against float64 from the fixture."""
import importlib
import os

import numpy as np
import pytest
import torch

from tests.golden.cases import sample_indices
from tests.golden.summary_heads_cases import CASES, MODULE_OF, NSAMP, cotangent, fill, inputs, run
from tests.helpers import GOLDEN_DIR, rel_l2

pytestmark = pytest.mark.gpu

CHUNK = 64      # rows of T one workgroup of uc_token_pool's first stage sums (csrc/pool.hip: POOL_CHUNK)
# (B, T, C, ld): one row; odd T and C % 8 != 0 with padded rows; the PoseHead shape (several chunks, 4 = 196 - 3 * 64 rows in the
# last); 4133 = 64 * CHUNK + 37: 65 chunks, a partial last one
POOL_SHAPES = [(3, 1, 8, 8), (2, 77, 20, 24), (2, 196, 1024, 1024), (1, 64 * CHUNK + 37, 64, 64)]
_GOLD = []


def OFF(T):
    return slice(1, None, max(2, T // 2))


def gold():
    if not _GOLD:
        _GOLD.append(np.load(os.path.join(GOLDEN_DIR, "summary_heads.npz")))
    return _GOLD[0]


def _rows(B, T, C, ld, dtype, seed, gpu, mean=0.5):
    "a [B T, C] view of a [B T, ld] buffer whose padding columns are NaN (nothing may read them)"
    buf = (torch.randn(B * T, ld, generator=torch.Generator().manual_seed(seed)) + mean).to(dtype)
    buf[:, C:] = float("nan")
    return buf.to(gpu)[:, :C]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,T,C,ld", POOL_SHAPES)
def test_token_pool_against_fp64_and_bitwise_reproducible(gpu, dtype, B, T, C, ld):
    from uniception_amd import ops
    x = _rows(B, T, C, ld, dtype, 100 + T + C, gpu)
    want = x.double().view(B, T, C).mean(1).cpu()
    got, again = ops.token_pool(x, B, T), ops.token_pool(x, B, T)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and got.shape == (B, C)
    err = rel_l2(got.cpu(), want)
    print(f"token_pool {dtype} B {B} T {T} C {C} ld {ld}: rel-L2 {err:.3e} (bound 1e-6)")
    assert err < 1e-6
    assert torch.equal(got, again)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("B,T,C,ld", POOL_SHAPES)
def test_token_pool_bwd_is_the_gated_broadcast(gpu, dtype, gated, B, T, C, ld):
    from uniception_amd import ops
    g = torch.randn(B, C, generator=torch.Generator().manual_seed(7 + T)).to(gpu)
    gate = None
    if gated:
        gate = _rows(B, T, C, ld, dtype, 300 + T + C, gpu, mean=0.0)
        gate[::3, ::2] = 0.0                 # exact zeros are gated off like negatives
        gate[OFF(T)] = -1.0                  # whole rows gated off
    out = ops.token_pool_bwd(g, T, dtype, gate)
    torch.cuda.synchronize()
    assert out.dtype == dtype and out.shape == (B * T, C)
    # the correctly rounded fp32 quotient, as the kernel's one IEEE division gives it (a float64 quotient of fp32 operands rounds to
    # the same fp32 value; `g / T` in PyTorch multiplies by the rounded reciprocal instead)
    exact = (g.double() / T).float().view(B, 1, C).expand(B, T, C).reshape(B * T, C)
    if gated:
        on = gate > 0
        assert on.any() and not on.all()
        assert bool((out[~on] == 0).all()) and bool((out[OFF(T)] == 0).all())
        exact = torch.where(on, exact, torch.zeros_like(exact))
    if dtype == torch.float32:
        assert torch.equal(out, exact)
    else:
        worst = float(((out.float() - exact).abs() / exact.abs().clamp_min(1e-30)).max())
        print(f"token_pool_bwd bf16 B {B} T {T} C {C} gated {gated}: worst relative error {worst:.3e} (bound {2.0 ** -8:.3e})")
        assert worst <= 2.0 ** -8


def test_token_pool_and_its_backward_fp16(gpu):
    """fp16 rows (the heads' default operand type) at B 2, T 15, C 16: two column groups.  Forward: the bound of the other dtypes
    (the float64 mean of the stored values).  Backward: one rounding of the exact quotient, 2^-11 relative, or half a subnormal
    step (2^-25) below fp16's normal range; gated-off elements exactly 0."""
    from uniception_amd import ops
    B, T, C = 2, 15, 16
    x = _rows(B, T, C, 24, torch.float16, 131, gpu)
    assert rel_l2(ops.token_pool(x, B, T).cpu(), x.double().view(B, T, C).mean(1).cpu()) < 1e-6
    g = torch.randn(B, C, generator=torch.Generator().manual_seed(22)).to(gpu)
    gate = _rows(B, T, C, 24, torch.float16, 315, gpu, mean=0.0)
    gate[::3, ::2] = 0.0
    out = ops.token_pool_bwd(g, T, torch.float16, gate)
    exact = torch.where(gate > 0, (g.double() / T).view(B, 1, C).expand(B, T, C).reshape(B * T, C), torch.zeros((), dtype=torch.float64, device=gpu))
    assert out.dtype == torch.float16 and bool((out[~(gate > 0)] == 0).all())
    assert bool(((out.double() - exact).abs() <= torch.clamp(exact.abs() * 2.0 ** -11, min=2.0 ** -25)).all())


def _model(name, gpu):
    kind, kw, _ = CASES[name]
    model = getattr(importlib.import_module(f"uniception_amd.models.prediction_heads.{MODULE_OF[kind]}"), kind)(**kw)
    fill(model)
    return model.to(gpu)


def _run(name, model, x):
    from uniception_amd.models.prediction_heads.base import PredictionHeadInput, PredictionHeadTokenInput
    return run(name, model, x, PredictionHeadInput, PredictionHeadTokenInput)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_module_forward_and_backward_against_the_reference_in_fp64(gpu, name, mode):
    from uniception_amd import engine
    G = gold()
    model = _model(name, gpu).train()
    x = inputs(name).to(gpu).requires_grad_(True)
    with engine.precision(mode):
        out = _run(name, model, x)
        (out.float() * cotangent(name, tuple(out.shape)).to(gpu)).sum().backward()
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and tuple(out.shape) == G[f"{name}/out"].shape
    fp32 = mode == "fp32"
    tag = "e32" if fp32 else "e16"
    checks = [("out", out.detach().cpu(), torch.from_numpy(G[f"{name}/out"]), max(2e-6, 8.0 * float(G[f"{name}/e32/out"])) if fp32 else None),
              ("din", x.grad.cpu(), torch.from_numpy(G[f"{name}/din"]), 1e-3 if fp32 else None)]
    norms = []
    for k, p in model.named_parameters():
        assert p.grad is not None, f"{k} received no gradient"
        idx = torch.from_numpy(sample_indices(p.numel(), NSAMP))
        checks.append((f"p/{k}", p.grad.flatten().cpu()[idx], torch.from_numpy(G[f"{name}/p/{k}__samples"]), 1e-3 if fp32 else None))
        norms.append((k, float(p.grad.double().norm()), float(G[f"{name}/p/{k}__norm"])))
    bad = []
    for q, got, want, bound in checks:
        bound = 2.0 * float(G[f"{name}/{tag}/{q}"]) if bound is None else bound
        err = rel_l2(got, want)
        print(f"{name} {mode} {q}: rel-L2 {err:.3e} (bound {bound:.3e})")
        if not err < bound:
            bad.append((q, err, bound))
    if fp32:
        for k, got, want in norms:
            err = abs(got - want) / want
            print(f"{name} {mode} |p/{k}|: relative difference {err:.3e} (bound 1e-3)")
            if not err < 1e-3:
                bad.append((f"|p/{k}|", err, 1e-3))
    assert not bad, bad


def test_inference_under_the_default_head_policy_stays_within_the_bf16_bound(gpu):
    """pose_default in eval mode without autograd next to a bf16 transformer: the default head policy runs fp16 MFMA operands (more
    mantissa than bf16), so the bf16 bound of the fixture holds; no autograd graph is built."""
    from uniception_amd import engine
    name = "pose_default"
    model = _model(name, gpu).eval()
    want = torch.from_numpy(gold()[f"{name}/out"])
    bound = 2.0 * float(gold()[f"{name}/e16/out"])
    with torch.no_grad(), engine.precision("bf16"):
        assert engine.head_dtype_name() != "fp16" or engine.head_dtype() == torch.float16
        out = _run(name, model, inputs(name).to(gpu))
    torch.cuda.synchronize()
    assert out.grad_fn is None and not out.requires_grad and out.dtype == torch.float32
    err = rel_l2(out.cpu(), want)
    print(f"{name} inference, head policy {engine.head_dtype_name()}: rel-L2 {err:.3e} (bound {bound:.3e})")
    assert err < bound
    with engine.precision("bf16"):       # with the parameters requiring a gradient and autograd on, the same call records a graph
        assert _run(name, model, inputs(name).to(gpu)).grad_fn is not None
