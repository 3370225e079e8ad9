"""GPU: the streaming kernels of the non-image input encoders against float64 on the CPU, and PatchEmbedder /
DenseRepresentationEncoder / GlobalRepresentationEncoder against the float64 run of the REAL reference
(tests/golden/input_encoders.npz), outputs and every gradient, in train mode.

Tolerances.
  uc_unshuffle_rows and its adjoint move values: exact after the rounding to the output dtype; <R, A x> = <A^T R, x> to 1e-6.
  uc_act, fp32: rel-L2 <= 1e-6 against float64 (libm erff is good to an ulp or two of the result, fp32 eps = 6e-8).
  uc_ln_pe_ln, fp32: y and mid within 1e-5 (two fp32 reductions over at most 1024 terms per norm), 1e-4 at x = 100 + N(0, 1)
    (the two-pass variance loses the log2(100^2) bits of the mean to the subtraction, E[x^2] - E[x]^2 would lose all of them).
  bf16 kernels: <= 2 x the error of the same formula evaluated by PyTorch in bfloat16 on the CPU on the same rounded inputs.
  Inputs of the norms are 0.5 + N(0, 1): the mean of zero-mean samples is a cancelling sum against which no relative bound means anything.
  composed backward (uc_layernorm_bwd, uc_colsum, uc_layernorm_bwd; dgamma / dbeta from uc_ln_param_grads), fp32: dx, both
    dgamma / dbeta and dpe within 1e-5; uc_ln_param_grads alone within 1e-5 and the same bits on every call.
  modules, fp32: outputs within max(2e-6, 8 e32), gradients within 1e-3; bf16: every quantity within 2 x e16 (e32 / e16: the
    reference's own fp32 / bfloat16-on-CPU error against float64 from the fixture).  Parameter-gradient errors are divided by
    max(|g_ref|, 1e-3 x the largest parameter-gradient norm of the case), in the fixture and here (input_encoders_cases.grad_errors)."""
import importlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.golden.cases import sample_indices
from tests.golden.input_encoders_cases import CASES, MODULE_OF, NSAMP, cotangent, fill, grad_errors, inputs, kwargs, run
from tests.helpers import GOLDEN_DIR, rel_l2

pytestmark = pytest.mark.gpu

UNSHUFFLE = [(2, 4, 3, 7, 64), (1, 14, 5, 5, 256), (3, 2, 1, 1, 16), (1, 3, 2, 5, 16)]          # (C, P, h, w, ld)
ACT_N = [8, 4104, 37 * 37 * 40]
LN_C = [64, 1000, 1024]
LN_BN = [(2, 21), (1, 1), (3, 37)]
COMBOS = [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1) if a or b or c]              # (LN1, pe, LN2)
EPS1, EPS2 = 1e-6, 1e-5
_GOLD = []


def gold():
    if not _GOLD:
        _GOLD.append(np.load(os.path.join(GOLDEN_DIR, "input_encoders.npz")))
    return _GOLD[0]


def _rand(shape, seed, dtype=torch.float32, mean=0.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) + mean).to(dtype)


# ---- uc_unshuffle_rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dst_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("src_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C,P,h,w,ld", UNSHUFFLE)
def test_unshuffle_rows_is_exact_and_pads_with_zeros(gpu, C, P, h, w, ld, src_dtype, dst_dtype):
    from uniception_amd import _lib, ops
    B = 2
    x = _rand((B, C, h * P, w * P), 3 + C + P, src_dtype)
    want = F.pixel_unshuffle(x.float(), P).permute(0, 2, 3, 1).reshape(B * h * w, C * P * P).to(dst_dtype)
    xd = x.to(gpu)
    got = torch.full((B * h * w, ld), float("nan"), dtype=dst_dtype, device=gpu)          # the pad columns are WRITTEN as zeros
    _lib.check(_lib.load().uc_unshuffle_rows(xd.data_ptr(), ops._dt(src_dtype), got.data_ptr(), ops._dt(dst_dtype), B, C, h, w, P, ld,
                                             torch.cuda.current_stream().cuda_stream), "uc_unshuffle_rows")
    torch.cuda.synchronize()
    assert torch.equal(got[:, :C * P * P].cpu(), want)
    assert torch.equal(got[:, C * P * P:].cpu(), torch.zeros(B * h * w, ld - C * P * P, dtype=dst_dtype))
    assert torch.equal(ops.unshuffle_rows(xd, P, ld, dst_dtype), got)


@pytest.mark.parametrize("C,P,h,w,ld", UNSHUFFLE)
def test_unshuffle_rows_adjoint_is_exact_and_is_the_adjoint(gpu, C, P, h, w, ld):
    from uniception_amd import ops
    B = 2
    x = _rand((B, C, h * P, w * P), 5 + C + P)
    r = _rand((B * h * w, ld), 6 + C + P)
    want = F.pixel_shuffle(r[:, :C * P * P].view(B, h, w, C * P * P).permute(0, 3, 1, 2), P)
    for dtype in (torch.float32, torch.bfloat16):
        got = ops.unshuffle_rows_bwd(r.to(dtype).to(gpu), B, C, h, w, P)
        assert got.dtype == torch.float32 and torch.equal(got.cpu(), F.pixel_shuffle(
            r.to(dtype).float()[:, :C * P * P].view(B, h, w, C * P * P).permute(0, 3, 1, 2), P))
    ax = ops.unshuffle_rows(x.to(gpu), P, ld, torch.float32).cpu().double()
    atr = ops.unshuffle_rows_bwd(r.to(gpu), B, C, h, w, P).cpu().double()
    assert torch.equal(atr, want.double())
    lhs, rhs = float((r.double() * ax).sum()), float((atr * x.double()).sum())
    err = abs(lhs - rhs) / float(r.double().norm() * ax.norm())
    print(f"unshuffle adjoint {(C, P, h, w, ld)}: <R, A x> - <A^T R, x> = {err:.3e} (bound 1e-6)")
    assert err <= 1e-6


def test_unshuffle_rows_function_gives_the_input_gradient(gpu):
    from uniception_amd import autograd
    x = _rand((2, 2, 12, 28), 9).to(gpu).requires_grad_(True)
    r = _rand((2 * 3 * 7, 64), 10).to(gpu)
    (autograd.unshuffle_rows(x, 4, 64, torch.bfloat16).float() * r).sum().backward()
    want = F.pixel_shuffle(r.bfloat16().float()[:, :32].view(2, 3, 7, 32).permute(0, 3, 1, 2), 4)
    assert torch.equal(x.grad, want)


# ---- uc_act --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("act", ["gelu", "relu"])
@pytest.mark.parametrize("n", ACT_N)
def test_act_against_fp64_in_place_and_out_of_place(gpu, n, act, dtype):
    from uniception_amd import ops
    x = (2.0 * _rand((n,), 11 + n)).to(dtype)
    f = F.gelu if act == "gelu" else F.relu
    want = f(x.double())
    xd = x.to(gpu)
    y = ops.act(xd, act)
    assert y.data_ptr() != xd.data_ptr() and torch.equal(xd.cpu(), x)            # out of place leaves x alone
    z = xd.clone()
    assert ops.act(z, act, out=z).data_ptr() == z.data_ptr() and torch.equal(z, y)
    # a pointer off the 16-byte grid takes the scalar form: the same values
    if n > 8:
        buf = xd.clone()
        assert torch.equal(ops.act(buf[1:].contiguous(), act), y[1:]) and torch.equal(ops.act(buf[1:], act, out=buf[1:]), y[1:])
    err = rel_l2(y.cpu(), want)
    bound = 1e-6 if dtype == torch.float32 else 2.0 * rel_l2(f(x), want)
    print(f"act {act} {dtype} n {n}: rel-L2 {err:.3e} (bound {bound:.3e})")
    assert y.dtype == dtype and err <= bound


def test_act_function_backward_is_act_bwd_on_the_saved_input(gpu):
    from uniception_amd import autograd
    u = _rand((37, 40), 13).to(gpu).requires_grad_(True)
    g = _rand((37, 40), 14).to(gpu)
    autograd.act(u, "gelu").backward(g)
    u64 = u.detach().cpu().double().requires_grad_(True)
    F.gelu(u64).backward(g.cpu().double())
    assert rel_l2(u.grad.cpu(), u64.grad) <= 1e-6


# ---- uc_ln_pe_ln ---------------------------------------------------------------------------------------------------------------
def _ln_params(C, seed):
    return (1.0 + 0.5 * _rand((C,), seed), 0.5 * _rand((C,), seed + 1))


def _formula(x, ln1, pe, ln2, dtype):
    "LN2(LN1(x) + pe) by PyTorch on the CPU in `dtype`: (y, mid)"
    t = x.to(dtype)
    C = t.shape[-1]
    if ln1 is not None:
        t = F.layer_norm(t, (C,), ln1[0].to(dtype), ln1[1].to(dtype), EPS1)
    if pe is not None:
        t = t + pe.to(dtype)
    mid = t
    if ln2 is not None:
        t = F.layer_norm(t, (C,), ln2[0].to(dtype), ln2[1].to(dtype), EPS2)
    return t, mid


def _case(B, N, C, dtype, offset=0.5):
    x = _rand((B, N, C), 17 + B + N + C, torch.float32, offset).to(dtype)
    return x, _ln_params(C, 19 + C), _rand((N, C), 23 + N + C), _ln_params(C, 29 + C)


def _launch(gpu, x, ln1, pe, ln2, out_dtype, want_mid=True):
    from uniception_amd import ops
    B, N, C = x.shape
    dev = lambda n: None if n is None else (n[0].to(gpu), n[1].to(gpu), n[2])      # noqa: E731
    return ops.ln_pe_ln(x.to(gpu).view(B * N, C), B, N, dev(ln1), None if pe is None else pe.to(gpu), dev(ln2), out_dtype, want_mid=want_mid)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,N", LN_BN)
@pytest.mark.parametrize("C", LN_C)
def test_ln_pe_ln_every_combination_against_fp64(gpu, C, B, N, dtype):
    x, p1, pe, p2 = _case(B, N, C, dtype)
    bad = []
    for use1, usepe, use2 in COMBOS:
        ln1, t, ln2 = (p1 if use1 else None), (pe if usepe else None), (p2 if use2 else None)
        want_y, want_mid = _formula(x.double(), ln1, t, ln2, torch.float64)
        y, mid = _launch(gpu, x, ln1 and (*ln1, EPS1), t, ln2 and (*ln2, EPS2), dtype)
        y2, mid2 = _launch(gpu, x, ln1 and (*ln1, EPS1), t, ln2 and (*ln2, EPS2), dtype)
        torch.cuda.synchronize()
        assert y.dtype == dtype and mid.dtype == torch.float32 and tuple(y.shape) == tuple(mid.shape) == (B * N, C)
        assert torch.equal(y, y2) and torch.equal(mid, mid2)                     # fixed-order reductions: two calls give the same bits
        if usepe or (use1 and use2):         # (a lone norm without mid is uc_layernorm itself: another kernel, its own last bits)
            assert torch.equal(_launch(gpu, x, ln1 and (*ln1, EPS1), t, ln2 and (*ln2, EPS2), dtype, want_mid=False), y)
        bounds = {"y": 1e-5, "mid": 1e-5}
        if dtype == torch.bfloat16:
            ty, tmid = _formula(x, ln1, t, ln2, torch.bfloat16)
            bounds = {"y": 2.0 * rel_l2(ty, want_y), "mid": 2.0 * rel_l2(tmid, want_mid)}
        for k, got, want in (("y", y, want_y), ("mid", mid, want_mid)):
            err = rel_l2(got.cpu().view(B, N, C), want)
            print(f"ln_pe_ln {dtype} C {C} (B, N) {(B, N)} LN1/pe/LN2 {(use1, usepe, use2)} {k}: rel-L2 {err:.3e} (bound {bounds[k]:.3e})")
            if not err <= bounds[k]:
                bad.append(((use1, usepe, use2), k, err, bounds[k]))
    assert not bad, bad


@pytest.mark.parametrize("combo", [(1, 0, 0), (1, 1, 1)])
def test_ln_pe_ln_statistics_do_not_cancel_at_an_offset(gpu, combo):
    B, N, C = 3, 37, 1000
    x, p1, pe, p2 = _case(B, N, C, torch.float32, offset=100.0)
    ln1, t, ln2 = p1, (pe if combo[1] else None), (p2 if combo[2] else None)
    want_y, want_mid = _formula(x.double(), ln1, t, ln2, torch.float64)
    y, mid = _launch(gpu, x, (*ln1, EPS1), t, ln2 and (*ln2, EPS2), torch.float32)
    ey, em = rel_l2(y.cpu().view(B, N, C), want_y), rel_l2(mid.cpu().view(B, N, C), want_mid)
    print(f"ln_pe_ln at offset 100, LN1/pe/LN2 {combo}: y {ey:.3e}, mid {em:.3e} (bound 1e-4)")
    assert ey <= 1e-4 and em <= 1e-4


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", LN_C + [768, 1001])
def test_ln_pe_ln_with_ln1_alone_equals_layernorm_bit_for_bit(gpu, C, dtype):
    "every kernel form of uc_layernorm: predicated (64, 1000), exact width (768, 1024), scalar (1001); LN2 alone is a LayerNorm too"
    from uniception_amd import ops
    B, N = 3, 37
    x, p1, _, _ = _case(B, N, C, dtype)
    for out_dtype in (torch.float32, torch.bfloat16):
        want = ops.layernorm(x.to(gpu).view(B * N, C), p1[0].to(gpu), p1[1].to(gpu), EPS1, out_dtype)
        got = _launch(gpu, x, (*p1, EPS1), None, None, out_dtype, want_mid=False)
        assert torch.equal(got, want), (C, dtype, out_dtype, rel_l2(got.float().cpu(), want.float().cpu()))


def test_ln_pe_ln_scalar_form_against_fp64(gpu):
    "C % 4 != 0 takes the scalar kernel, which re-evaluates the LN2 input instead of holding it"
    B, N, C = 2, 21, 1001
    x, p1, pe, p2 = _case(B, N, C, torch.float32)
    want_y, want_mid = _formula(x.double(), p1, pe, p2, torch.float64)
    y, mid = _launch(gpu, x, (*p1, EPS1), pe, (*p2, EPS2), torch.float32)
    assert rel_l2(y.cpu().view(B, N, C), want_y) <= 1e-5 and rel_l2(mid.cpu().view(B, N, C), want_mid) <= 1e-5


@pytest.mark.parametrize("combo", COMBOS)
@pytest.mark.parametrize("B,N,C", [(2, 21, 64), (3, 37, 1000)])
def test_composed_backward_against_fp64(gpu, B, N, C, combo):
    from uniception_amd import autograd
    x, p1, pe, p2 = _case(B, N, C, torch.float32)
    dy = _rand((B, N, C), 31 + C)
    use1, usepe, use2 = combo
    leaves64 = [t.double().requires_grad_(True) for t in (x, p1[0], p1[1], pe, p2[0], p2[1])]
    x64, g1, b1, pe64, g2, b2 = leaves64
    want_y, _ = _formula(x64, (g1, b1) if use1 else None, pe64 if usepe else None, (g2, b2) if use2 else None, torch.float64)
    want_y.backward(dy.double())
    ln1 = torch.nn.LayerNorm(C, eps=EPS1).to(gpu) if use1 else None
    ln2 = torch.nn.LayerNorm(C, eps=EPS2).to(gpu) if use2 else None
    with torch.no_grad():
        for ln, p in ((ln1, p1), (ln2, p2)):
            if ln is not None:
                ln.weight.copy_(p[0])
                ln.bias.copy_(p[1])
    xd = x.to(gpu).view(B * N, C).requires_grad_(True)
    ped = pe.to(gpu).requires_grad_(True) if usepe else None
    y = autograd.ln_pe_ln(xd, B, N, ln1, ped, ln2, torch.float32)
    y.backward(dy.to(gpu).view(B * N, C))
    torch.cuda.synchronize()
    got = {"y": y.detach().view(B, N, C), "dx": xd.grad.view(B, N, C)}
    want = {"y": want_y.detach(), "dx": x64.grad}
    if use1:
        got.update(dgamma1=ln1.weight.grad, dbeta1=ln1.bias.grad)
        want.update(dgamma1=g1.grad, dbeta1=b1.grad)
    if usepe:
        got.update(dpe=ped.grad)
        want.update(dpe=pe64.grad)
    if use2:
        got.update(dgamma2=ln2.weight.grad, dbeta2=ln2.bias.grad)
        want.update(dgamma2=g2.grad, dbeta2=b2.grad)
    bad = []
    for k in got:
        err = rel_l2(got[k].cpu(), want[k])
        print(f"ln_pe_ln backward {(B, N, C)} LN1/pe/LN2 {combo} {k}: rel-L2 {err:.3e} (bound 1e-5)")
        if not err <= 1e-5:
            bad.append((k, err))
    assert not bad, bad


# ---- modules -------------------------------------------------------------------------------------------------------------------
def _model(name, gpu, **extra):
    kind = CASES[name][0]
    cls = getattr(importlib.import_module(f"uniception_amd.models.encoders.{MODULE_OF[kind]}"), kind)
    src = cls(**kwargs(name))
    fill(src)                                  # the reference's state_dict, rebuilt from the case's seeds (name-keyed filler)
    model = cls(**kwargs(name), **extra)
    res = model.load_state_dict(src.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return model.to(gpu)


def _run(name, model, xs):
    from uniception_amd.models.encoders import EncoderGlobalRepInput, ViTEncoderNonImageInput
    return run(name, model, xs, ViTEncoderNonImageInput, EncoderGlobalRepInput)


def _forward_backward(name, model, gpu, mode):
    from uniception_amd import engine
    xs = [x.to(gpu).requires_grad_(True) for x in inputs(name)]
    with engine.precision(mode):
        out = _run(name, model, xs)
        (out.float() * cotangent(name, tuple(out.shape)).to(gpu)).sum().backward()
    torch.cuda.synchronize()
    return xs, out


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_module_forward_and_backward_against_the_reference_in_fp64(gpu, name, mode):
    from uniception_amd import engine
    G = gold()
    model = _model(name, gpu).train()
    xs, out = _forward_backward(name, model, gpu, mode)
    assert out.dtype == torch.float32 and tuple(out.shape) == G[f"{name}/out"].shape
    fp32 = mode == "fp32"
    tag = "e32" if fp32 else "e16"
    errs = {"out": rel_l2(out.detach().cpu(), torch.from_numpy(G[f"{name}/out"]))}
    assert xs[0].grad is not None
    errs["din0"] = rel_l2(xs[0].grad.cpu(), torch.from_numpy(G[f"{name}/din0"]))
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
    # eval mode, no graph: the same kernels (the resized position table now comes from the cache), the same bits
    with torch.no_grad(), engine.precision(mode):
        again = _run(name, model.eval(), [x.detach() for x in xs])
        cached = _run(name, model, [x.detach() for x in xs])
    assert again.grad_fn is None and not again.requires_grad
    assert torch.equal(again, out.detach()) and torch.equal(cached, again)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows,C", [(42, 64), (1, 64), (111, 1000), (130, 1001)])
def test_ln_param_grads_against_fp64_and_the_same_bits_twice(gpu, rows, C, dtype):
    "rows: below one 64-row slab, one row, a ragged second slab, three slabs; 1001: a column block that is not full"
    from uniception_amd import ops
    x = _rand((rows, C), 41 + rows + C, torch.float32, 0.5).to(dtype)
    dy = _rand((rows, C), 43 + rows + C).to(dtype)
    xh = F.layer_norm(x.double(), (C,), None, None, EPS1)
    want = {"dgamma": (dy.double() * xh).sum(0), "dbeta": dy.double().sum(0)}
    got = dict(zip(("dgamma", "dbeta"), ops.ln_param_grads(x.to(gpu), dy.to(gpu), EPS1)))
    again = ops.ln_param_grads(x.to(gpu), dy.to(gpu), EPS1)
    assert torch.equal(got["dgamma"], again[0]) and torch.equal(got["dbeta"], again[1])
    for k in got:
        err = rel_l2(got[k].cpu(), want[k])
        print(f"ln_param_grads {dtype} {(rows, C)} {k}: rel-L2 {err:.3e} (bound 1e-5)")
        assert got[k].dtype == torch.float32 and err <= 1e-5      # (fp32 sums of the given, already rounded, values in both dtypes)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_gradient_checkpointing_gives_the_same_gradients_bit_for_bit(gpu, mode):
    """Every gradient of the checkpointed encoder equals the plain encoder's bit for bit — the LayerNorm parameters' too, which sit
    behind the wrapped blocks: their sums run in a fixed order (uc_ln_param_grads), not through uc_layernorm_bwd's atomics."""
    name = "dense_small"
    plain, ckpt = _model(name, gpu).train(), _model(name, gpu, gradient_checkpointing=True).train()
    xs0, out0 = _forward_backward(name, plain, gpu, mode)
    xs1, out1 = _forward_backward(name, ckpt, gpu, mode)
    assert torch.equal(out0, out1) and torch.equal(xs0[0].grad, xs1[0].grad)
    for (k, p), (_, q) in zip(plain.named_parameters(), ckpt.named_parameters()):
        assert p.grad is not None and q.grad is not None and torch.equal(p.grad, q.grad), k


def test_residual_block_alone_matches_fp64(gpu):
    "ResidualBlock is callable on its own on an NCHW map, like the reference's: channel counts off the 64 granule, a conv shortcut"
    from uniception_amd import engine
    from uniception_amd.models.encoders import ResidualBlock
    torch.manual_seed(5)
    blk = ResidualBlock(40, 72)
    x = _rand((2, 40, 3, 7), 37)
    sd = {k: v.detach().double() for k, v in blk.state_dict().items()}
    x64 = x.double()
    idn = F.conv2d(x64, sd["shortcut.weight"], sd["shortcut.bias"])
    want = F.gelu(F.conv2d(F.gelu(F.conv2d(x64, sd["conv1.weight"], sd["conv1.bias"], padding=1)), sd["conv2.weight"], sd["conv2.bias"], padding=1) + idn)
    with torch.no_grad(), engine.precision("fp32"):
        got = blk.to(gpu)(x.to(gpu))
    err = rel_l2(got.cpu(), want)
    print(f"ResidualBlock 40 -> 72 fp32: rel-L2 {err:.3e} (bound 1e-5)")
    assert tuple(got.shape) == (2, 72, 3, 7) and got.dtype == torch.float32 and err <= 1e-5
