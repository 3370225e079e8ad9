"""GPU: the channels-last kernels of the MoGe head against float64 on the CPU, and MoGeConvFeature / ResidualConvBlock / MLPFeature
against the float64 run of the REAL reference (tests/golden/moge_heads.npz), outputs and every gradient, in train mode.

Tolerances.
  fp32 kernels: rel-L2 <= 1e-5 against float64 (GroupNorm: y, dx, dgamma, dbeta, mean, rstd; replicate 3x3 convolution: y, dx, dW,
    db), 1e-6 for the resize and the inner-product identities of the adjoints; pad, crop (+ residual) and embed are exact.
  bf16 kernels: <= 2 x the error of the same formula evaluated by PyTorch in bfloat16 on the CPU, computed here on the same rounded
    inputs (the statistics of a bf16 map are fp32 and keep the fp32 bound).
  GroupNorm inputs are 0.5 + N(0, 1): the mean of zero-mean samples is a cancelling sum against which no relative bound means
    anything.  x = 100 + N(0, 1) in fp32 must give rstd within 1e-4 of float64 (E[x^2] - E[x]^2 does not).
  modules, fp32: outputs within max(2e-6, 8 e32), gradients within 1e-3; bf16: every quantity within 2 x e16 (e32 / e16: the
    reference's own fp32 / bfloat16-on-CPU error against float64 from the fixture).  Parameter-gradient errors are divided by
    max(|g_ref|, 1e-3 x the largest parameter-gradient norm of the case), in the fixture and here (moge_heads_cases.grad_errors)."""
import importlib
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.golden.cases import sample_indices
from tests.golden.moge_heads_cases import CASES, MODULE_OF, NSAMP, cotangent, fill, grad_errors, inputs, run
from tests.helpers import GOLDEN_DIR, rel_l2

pytestmark = pytest.mark.gpu

# (B, H, W, C, G); the last: C = 32 gives chunks of 512 pixels (csrc/groupnorm.hip: 256 / (C / 8) rows x 8), 23 x 29 = 667 = 512 + 155
GN_SHAPES = [(2, 5, 7, 32, 1), (2, 5, 7, 64, 2), (1, 37, 37, 64, 1), (3, 1, 1, 96, 3), (1, 23, 29, 32, 1)]
MAPS = [(1, 1), (1, 5), (3, 5), (6, 4)]
_GOLD = []


def gold():
    if not _GOLD:
        _GOLD.append(np.load(os.path.join(GOLDEN_DIR, "moge_heads.npz")))
    return _GOLD[0]


def _rand(shape, seed, dtype, mean=0.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) + mean).to(dtype)


def _gn_cpu(x, dy, gamma, beta, G, eps, relu, dtype):
    "F.group_norm (+ ReLU) and its gradients on the CPU in `dtype`, from NHWC x / dy: (y, dx, dgamma, dbeta) as float64 NHWC"
    xc = x.to(dtype).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    g, b = gamma.to(dtype).requires_grad_(True), beta.to(dtype).requires_grad_(True)
    y = F.group_norm(xc, G, g, b, eps)
    y = F.relu(y) if relu else y
    y.backward(dy.to(dtype).permute(0, 3, 1, 2).contiguous())
    return y.detach().permute(0, 2, 3, 1).double(), xc.grad.permute(0, 2, 3, 1).double(), g.grad.double(), b.grad.double()


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,H,W,C,G", GN_SHAPES)
def test_group_norm_forward_and_backward_against_fp64(gpu, B, H, W, C, G, dtype, relu):
    from uniception_amd import ops
    eps = 1e-5
    x = _rand((B, H, W, C), 10 + H + C, dtype, 0.5)
    dy = _rand((B, H, W, C), 20 + H + C, dtype, 0.25)
    gamma = 1.0 + 0.1 * _rand((C,), 30 + C, torch.float32)
    beta = 0.1 * _rand((C,), 40 + C, torch.float32)
    want = _gn_cpu(x.double(), dy.double(), gamma.double(), beta.double(), G, eps, relu, torch.float64)
    xg = x.double().view(B, H * W, G, C // G)
    mean64 = xg.mean(dim=(1, 3))
    rstd64 = 1.0 / torch.sqrt(xg.var(dim=(1, 3), unbiased=False) + eps)
    xd, dyd, gd, bd = x.to(gpu), dy.to(gpu), gamma.to(gpu), beta.to(gpu)
    y, mean, rstd = ops.group_norm_nhwc(xd, gd, bd, G, eps, relu)
    dx, dg, db = ops.group_norm_nhwc_bwd(dyd, xd, mean, rstd, gd, gate=y if relu else None)
    y2, mean2, rstd2 = ops.group_norm_nhwc(xd, gd, bd, G, eps, relu)
    dx2, dg2, db2 = ops.group_norm_nhwc_bwd(dyd, xd, mean2, rstd2, gd, gate=y2 if relu else None)
    torch.cuda.synchronize()
    assert y.dtype == dtype and dx.dtype == dtype and dg.dtype == db.dtype == mean.dtype == rstd.dtype == torch.float32
    for a, b in ((y, y2), (mean, mean2), (rstd, rstd2), (dx, dx2), (dg, dg2), (db, db2)):
        assert torch.equal(a, b)                    # fixed-order reductions: two calls give the same bits
    got = dict(y=y, dx=dx, dgamma=dg, dbeta=db, mean=mean, rstd=rstd)
    ref = dict(y=want[0], dx=want[1], dgamma=want[2], dbeta=want[3], mean=mean64, rstd=rstd64)
    bounds = dict.fromkeys(got, 1e-5)
    if dtype == torch.bfloat16:
        twin = _gn_cpu(x, dy, gamma, beta, G, eps, relu, torch.bfloat16)
        for k, t in zip(("y", "dx", "dgamma", "dbeta"), twin):
            bounds[k] = 2.0 * rel_l2(t, ref[k])
    bad = []
    for k in got:
        err = rel_l2(got[k].cpu().double(), ref[k])
        print(f"group_norm {dtype} {(B, H, W, C, G)} relu {relu} {k}: rel-L2 {err:.3e} (bound {bounds[k]:.3e})")
        if not err <= bounds[k]:
            bad.append((k, err, bounds[k]))
    assert not bad, bad


def test_group_norm_statistics_do_not_cancel_at_an_offset(gpu):
    from uniception_amd import ops
    B, H, W, C, G = 2, 37, 37, 64, 2
    x = 100.0 + _rand((B, H, W, C), 5, torch.float32)
    xg = x.double().view(B, H * W, G, C // G)
    rstd64 = 1.0 / torch.sqrt(xg.var(dim=(1, 3), unbiased=False) + 1e-5)
    _, mean, rstd = ops.group_norm_nhwc(x.to(gpu), torch.ones(C, device=gpu), torch.zeros(C, device=gpu), G, 1e-5)
    worst = float(((rstd.cpu().double() - rstd64).abs() / rstd64).max())
    print(f"rstd at offset 100: worst relative error {worst:.3e} (bound 1e-4)")
    assert worst <= 1e-4
    assert float(((mean.cpu().double() - xg.mean(dim=(1, 3))).abs() / 100.0).max()) <= 1e-6


def test_group_norm_rejects_a_group_size_off_the_vector_width(gpu):
    from uniception_amd import ops
    from uniception_amd._lib import UcHipError
    with pytest.raises(UcHipError, match="channels per group .12. must be a multiple of 8"):
        ops.group_norm_nhwc(torch.zeros(1, 2, 2, 48, device=gpu), torch.ones(48, device=gpu), torch.zeros(48, device=gpu), 4, 1e-5)


@pytest.mark.parametrize("C", [8, 40])
@pytest.mark.parametrize("H,W", MAPS)
def test_replicate_pad_is_exact_and_its_adjoint_is_the_adjoint(gpu, H, W, C):
    from uniception_amd import ops
    B = 2
    x = _rand((B, H, W, C), 50 + H + W + C, torch.float32)
    g = _rand((B, H + 2, W + 2, C), 60 + H + W + C, torch.float32)
    want = F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="replicate").permute(0, 2, 3, 1)
    for dtype in (torch.float32, torch.bfloat16):
        got = ops.replicate_pad_nhwc(x.to(dtype).to(gpu))
        assert got.shape == (B, H + 2, W + 2, C) and torch.equal(got.cpu(), want.to(dtype))
    gt = ops.replicate_pad_nhwc_bwd(g.to(gpu)).cpu().double()
    lhs, rhs = float((want.double() * g.double()).sum()), float((x.double() * gt).sum())
    err = abs(lhs - rhs) / float(want.double().norm() * g.double().norm())
    print(f"pad adjoint {H}x{W} C {C}: <pad x, g> - <x, pad^T g> = {err:.3e} (bound 1e-6)")
    assert err <= 1e-6
    assert torch.equal(ops.replicate_pad_nhwc_bwd(g.to(gpu)), ops.replicate_pad_nhwc_bwd(g.to(gpu)))


@pytest.mark.parametrize("C", [8, 40])
@pytest.mark.parametrize("H,W", MAPS)
def test_crop_add_and_embed_are_exact(gpu, H, W, C):
    from uniception_amd import ops
    B = 2
    xp = _rand((B, H + 2, W + 2, C), 70 + H + W + C, torch.float32)
    r = _rand((B, H, W, C), 80 + H + W + C, torch.float32)
    inner = xp[:, 1:-1, 1:-1]
    assert torch.equal(ops.crop_add_nhwc(xp.to(gpu)).cpu(), inner)
    assert torch.equal(ops.crop_add_nhwc(xp.to(gpu), r.to(gpu)).cpu(), inner + r)
    assert torch.equal(ops.crop_add_nhwc(xp.to(gpu), r.to(gpu), relu=True).cpu(), F.relu(inner + r))
    emb = ops.crop_embed_nhwc(r.to(gpu)).cpu()
    assert emb.shape == xp.shape and torch.equal(emb, F.pad(r, (0, 0, 1, 1, 1, 1)))


def _conv_cpu(x, dy, w, b, dtype):
    "replicate-padded 3x3 convolution and its gradients on the CPU in `dtype` from NHWC x / dy: (y, dx NHWC, dW, db) as float64"
    xc = x.to(dtype).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wc, bc = w.to(dtype).requires_grad_(True), b.to(dtype).requires_grad_(True)
    y = F.conv2d(F.pad(xc, (1, 1, 1, 1), mode="replicate"), wc, bc)
    y.backward(dy.to(dtype).permute(0, 3, 1, 2).contiguous())
    return y.detach().permute(0, 2, 3, 1).double(), xc.grad.permute(0, 2, 3, 1).double(), wc.grad.double(), bc.grad.double()


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("Cin,Cout,H,W", [(32, 64, 5, 7), (64, 32, 1, 3)])
def test_replicate_conv3x3_against_fp64(gpu, Cin, Cout, H, W, mode):
    from uniception_amd import autograd, engine
    B = 2
    dtype = torch.float32 if mode == "fp32" else torch.bfloat16
    conv = nn.Conv2d(Cin, Cout, 3, padding=1, padding_mode="replicate")
    with torch.no_grad():
        conv.weight.copy_(_rand(tuple(conv.weight.shape), 90 + Cin, torch.float32) * (2.0 / (9 * Cin)) ** 0.5)
        conv.bias.copy_(0.1 * _rand((Cout,), 91 + Cin, torch.float32))
    x = _rand((B, H, W, Cin), 92 + Cin, dtype)
    dy = _rand((B, H, W, Cout), 93 + Cin, dtype)
    w, b = conv.weight.detach().clone(), conv.bias.detach().clone()
    wq = w.to(dtype)              # the kernel multiplies the weights rounded to the operand dtype
    want = _conv_cpu(x.double(), dy.double(), wq.double(), b.double(), torch.float64)
    conv = conv.to(gpu)
    xd = x.to(gpu).requires_grad_(True)
    with engine.precision(mode):
        y = autograd.conv3x3_replicate(xd, conv)
        y.backward(dy.to(gpu))
    torch.cuda.synchronize()
    assert y.dtype == dtype and tuple(y.shape) == (B, H, W, Cout)
    got = dict(y=y.detach(), dx=xd.grad, dW=conv.weight.grad, db=conv.bias.grad)
    ref = dict(zip(("y", "dx", "dW", "db"), want))
    bounds = dict.fromkeys(got, 1e-5)
    if mode == "bf16":
        for k, t in zip(("y", "dx", "dW", "db"), _conv_cpu(x, dy, w, b, torch.bfloat16)):
            bounds[k] = 2.0 * rel_l2(t, ref[k])
    bad = []
    for k in got:
        err = rel_l2(got[k].cpu().double(), ref[k])
        print(f"conv3x3_replicate {mode} {Cin}->{Cout} {H}x{W} {k}: rel-L2 {err:.3e} (bound {bounds[k]:.3e})")
        if not err <= bounds[k]:
            bad.append((k, err, bounds[k]))
    assert not bad, bad


@pytest.mark.parametrize("C", [64, 8])
@pytest.mark.parametrize("Hi,Wi,Ho,Wo", [(24, 40, 42, 70), (16, 16, 32, 32), (5, 7, 5, 7)])
def test_half_pixel_resize_and_its_adjoint(gpu, Hi, Wi, Ho, Wo, C):
    from uniception_amd import ops
    B = 2
    x = _rand((B, Hi, Wi, C), 100 + Hi + C, torch.float32)
    g = _rand((B, Ho, Wo, C), 101 + Hi + C, torch.float32)
    want = F.interpolate(x.double().permute(0, 3, 1, 2), (Ho, Wo), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    got = ops.resize_bilinear_nhwc(x.to(gpu), Ho, Wo, False)
    err = rel_l2(got.cpu().double(), want)
    print(f"resize {Hi}x{Wi} -> {Ho}x{Wo} C {C}: rel-L2 {err:.3e} (bound 1e-6)")
    assert got.shape == (B, Ho, Wo, C) and err <= 1e-6
    gt = ops.resize_bilinear_nhwc_bwd(g.to(gpu), Hi, Wi, False)
    assert gt.shape == x.shape and torch.equal(gt, ops.resize_bilinear_nhwc_bwd(g.to(gpu), Hi, Wi, False))
    lhs, rhs = float((want * g.double()).sum()), float((x.double() * gt.cpu().double()).sum())
    aerr = abs(lhs - rhs) / float(want.norm() * g.double().norm())
    print(f"resize adjoint: <R x, g> - <x, R^T g> = {aerr:.3e} (bound 1e-6)")
    assert aerr <= 1e-6
    # align_corners=True is uc_bilinear_nhwc, bit for bit
    for dtype in (torch.float32, torch.bfloat16):
        xd = x.to(dtype).to(gpu)
        assert torch.equal(ops.resize_bilinear_nhwc(xd, Ho, Wo, True), ops.bilinear_nhwc(xd, Ho, Wo))
        gd = g.to(dtype).to(gpu)
        assert torch.equal(ops.resize_bilinear_nhwc_bwd(gd, Hi, Wi, True), ops.bilinear_nhwc_bwd(gd, Hi, Wi, Ho, Wo))


def _model(name, gpu):
    kind, kw, _, _ = CASES[name]
    cls = getattr(importlib.import_module(f"uniception_amd.models.prediction_heads.{MODULE_OF[kind]}"), kind)
    src = cls(**kw)
    fill(src)                                  # the reference's state_dict, rebuilt from the case's seeds (name-keyed filler)
    model = cls(**kw)
    res = model.load_state_dict(src.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return model.to(gpu)


def _run(name, model, xs):
    from uniception_amd.models.prediction_heads.base import PredictionHeadInput, PredictionHeadLayeredInput
    return run(name, model, xs, PredictionHeadInput, PredictionHeadLayeredInput)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_module_forward_and_backward_against_the_reference_in_fp64(gpu, name, mode):
    from uniception_amd import engine
    G = gold()
    model = _model(name, gpu).train()
    xs = [x.to(gpu).requires_grad_(True) for x in inputs(name)]
    with engine.precision(mode):
        out = _run(name, model, xs)
        (out.float() * cotangent(name, tuple(out.shape)).to(gpu)).sum().backward()
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and tuple(out.shape) == G[f"{name}/out"].shape
    fp32 = mode == "fp32"
    tag = "e32" if fp32 else "e16"
    errs = {"out": rel_l2(out.detach().cpu(), torch.from_numpy(G[f"{name}/out"]))}
    for i, x in enumerate(xs):
        assert x.grad is not None
        errs[f"din{i}"] = rel_l2(x.grad.cpu(), torch.from_numpy(G[f"{name}/din{i}"]))
    got, want = {}, {}
    for k, p in model.named_parameters():
        assert p.grad is not None, f"{k} received no gradient"
        idx = torch.from_numpy(sample_indices(p.numel(), NSAMP))
        got[k], want[k] = p.grad.flatten().cpu()[idx], torch.from_numpy(G[f"{name}/p/{k}__samples"])
    errs.update({f"p/{k}": e for k, e in grad_errors(got, want).items()})
    assert set(errs) == {q[len(name) + len(tag) + 2:] for q in G.files if q.startswith(f"{name}/{tag}/")}      # no quantity is skipped
    bad = []
    for q, err in errs.items():
        if fp32:
            bound = max(2e-6, 8.0 * float(G[f"{name}/e32/out"])) if q == "out" else 1e-3
        else:
            bound = 2.0 * float(G[f"{name}/e16/{q}"])
        print(f"{name} {mode} {q}: {err:.3e} (bound {bound:.3e})")
        if not err < bound:
            bad.append((q, err, bound))
    assert not bad, bad
    # inference: no graph, the same kernels, the same bits ("follow": the head dtype of training, not the fp16 inference policy)
    with torch.no_grad(), engine.precision(mode), engine.head_precision("follow"):
        again = _run(name, model.eval(), [x.detach() for x in xs])
    assert again.grad_fn is None and not again.requires_grad
    assert torch.equal(again, out.detach())


def test_inference_under_the_default_head_policy_stays_within_the_bf16_bound(gpu):
    from uniception_amd import engine
    name = "moge_small_p14"
    model = _model(name, gpu).eval()
    with torch.no_grad(), engine.precision("bf16"):
        out = _run(name, model, [x.to(gpu) for x in inputs(name)])
    torch.cuda.synchronize()
    err, bound = rel_l2(out.cpu(), torch.from_numpy(gold()[f"{name}/out"])), 2.0 * float(gold()[f"{name}/e16/out"])
    print(f"{name} inference, head policy {engine.head_dtype_name()}: rel-L2 {err:.3e} (bound {bound:.3e})")
    assert out.grad_fn is None and out.dtype == torch.float32 and err < bound


def test_mlpfeature_dropout_applies_the_drawn_masks_with_their_scale(gpu):
    """drop = 0.5 in train mode, exact-fp32 kernels: the masks autograd.make_drops draws (drop2 on the Mlp's output first, then drop1 on
    the hidden activation, uint8 bernoulli(keep) from the device generator) are drawn again from the same seed, and the output and the
    input gradient must equal the float64 recomputation with those masks and the scale 1 / keep — to 1e-5 rel-L2 (fp32 chains of at
    most 256 terms against float64).  Eval mode drops nothing."""
    from uniception_amd import engine
    from uniception_amd.models.prediction_heads import MLPFeature, PredictionHeadInput
    B, C, h, w, P, O, p = 2, 64, 3, 5, 2, 2, 0.5
    torch.manual_seed(3)
    m = MLPFeature(C, patch_size=P, output_dim=O, drop=p).to(gpu).train()
    x = torch.randn(B, C, h, w, device=gpu, requires_grad=True)
    cot = torch.randn(B, O, P * h, P * w, device=gpu)
    torch.manual_seed(11)
    with engine.precision("fp32"):
        out = m(PredictionHeadInput(last_feature=x)).decoded_channels
        (out * cot).sum().backward()
        other = m(PredictionHeadInput(last_feature=x)).decoded_channels
    torch.manual_seed(11)
    keep_out = torch.empty((B * h * w, C), dtype=torch.uint8, device=gpu).bernoulli_(1.0 - p).cpu().double()
    keep_mid = torch.empty((B * h * w, 4 * C), dtype=torch.uint8, device=gpu).bernoulli_(1.0 - p).cpu().double()
    assert 0.3 < float(keep_out.mean()) < 0.7 and 0.3 < float(keep_mid.mean()) < 0.7
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    x64 = x.detach().cpu().double().requires_grad_(True)
    tok = x64.permute(0, 2, 3, 1).reshape(B * h * w, C)
    a = F.gelu(F.linear(tok, sd["mlp.fc1.weight"], sd["mlp.fc1.bias"])) * keep_mid / (1.0 - p)
    t = F.linear(a, sd["mlp.fc2.weight"], sd["mlp.fc2.bias"]) * keep_out / (1.0 - p)
    y = F.linear(t, sd["linear.weight"].reshape(O * P * P, C), sd["linear.bias"])
    want = F.pixel_shuffle(y.view(B, h, w, O * P * P).permute(0, 3, 1, 2), P)
    (want * cot.cpu().double()).sum().backward()
    e_out, e_dx = rel_l2(out.detach().cpu(), want.detach()), rel_l2(x.grad.cpu(), x64.grad)
    print(f"MLPFeature drop 0.5, fp32: out {e_out:.3e}, dx {e_dx:.3e} (bound 1e-5)")
    assert e_out <= 1e-5 and e_dx <= 1e-5
    assert not torch.equal(out, other)                       # the next call draws new masks
    with engine.precision("fp32"), torch.no_grad():
        c, d = m.eval()(PredictionHeadInput(last_feature=x)).decoded_channels, m(PredictionHeadInput(last_feature=x)).decoded_channels
    plain = F.linear(F.linear(F.gelu(F.linear(tok, sd["mlp.fc1.weight"], sd["mlp.fc1.bias"])), sd["mlp.fc2.weight"], sd["mlp.fc2.bias"]),
                     sd["linear.weight"].reshape(O * P * P, C), sd["linear.bias"])
    plain = F.pixel_shuffle(plain.view(B, h, w, O * P * P).permute(0, 3, 1, 2), P)
    assert torch.equal(c, d) and rel_l2(c.cpu(), plain.detach()) <= 1e-5


def test_head_is_captured_into_a_hip_graph(gpu):
    "one capture-and-replay of moge_small_p14 the way graphs.GraphedTwoView captures: the replay gives the eager output bit for bit"
    from uniception_amd import engine, ops
    name = "moge_small_p14"
    model = _model(name, gpu).eval()
    static = [x.to(gpu) for x in inputs(name)]

    def forward():
        with torch.no_grad(), engine.precision("bf16"):
            return _run(name, model, static)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            eager = forward().clone()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    token = 0x4D6F4765
    ops.fuse_ws_reserve(4)
    graph = torch.cuda.CUDAGraph()
    try:
        with ops.capture_scope(token), torch.cuda.graph(graph):
            out = forward()
        keep = [x.clone() for x in static]
        for x in static:
            x.add_(1.0)
        graph.replay()                      # other inputs: the graph really recomputes
        torch.cuda.synchronize()
        assert not torch.equal(out, eager)
        for x, k in zip(static, keep):
            x.copy_(k)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    finally:
        torch.cuda.synchronize()
        del graph
        ops.fuse_ws_release(token)
